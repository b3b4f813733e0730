/*
 * aes_xts.hip -- XTS-AES (IEEE 1619 / SP 800-38E) sector kernels for gfx950,
 * on the LDS T-table rounds of aes_tt.hip (aes_tt_dev.h).
 *
 * Per block j of data unit u:  T = E_K2(LE128(tweak0 + u)) * x^j in GF(2^128)
 * (x^128 + x^7 + x^2 + x + 1, T a little-endian integer), C = E_K1(P ^ T) ^ T
 * (decryption: D_K1).  Both expanded keys arrive by value; K2 is always an
 * encryption schedule.
 *
 * Layout.  A wave takes a RUN of 2048 consecutive blocks as 8 passes of 256
 * (4 blocks per lane, block = pass base + 64 b + lane: every access a
 * coalesced 1 KiB wave access, as the ECB kernel's); a 1024-thread workgroup
 * takes a chunk of 16 runs (512 KiB) per grid step.
 *  * Tweak encryption.  One single-block pass under K2 encrypts the tweak
 *    numbers of 64 consecutive units, lane l that of unit (first + l), and
 *    stays in the lane's registers; a block's lane fetches its unit's
 *    E_K2(..) from there with a cross-lane read (ds_bpermute: no LDS memory,
 *    the decryption image fills all 160 KiB).  A pass refills the set only
 *    when its last block's unit lies past it, so units of >= 32 blocks cost
 *    one single-block tweak pass per run of 8 four-block data passes (1/32
 *    more block encryptions), 16 blocks two, 8 blocks four.  A pass of 256
 *    blocks must fit one set of 64 units: true from 5-block units on
 *    wherever the pass starts.  Units of 1..4 blocks take the SMALL form:
 *    every lane encrypts its own block's tweak number (one K2 pass per data
 *    pass, which a 16-byte unit needs anyway).
 *  * The encryption kernel's tweak passes use the LDS image; the decryption
 *    kernel's LDS holds the inverse tables only, so its tweak passes look up
 *    g_tab.te0 / sb in global memory (1.25 KiB, L1 resident).
 *  * Stepping.  T * x^k = (T << k) ^ f(T >> (128 - k)), f(v) = v ^ v<<1 ^
 *    v<<2 ^ v<<7, in closed form for k <= 63; x^64 moves the low qword up and
 *    folds f(high qword) in.  A lane's consecutive blocks are 64 apart, so
 *    inside a unit its tweak steps by x^64; at a block whose position in the
 *    unit is below 64 (the lane entered a new unit) it is E_K2(..) * x^j with
 *    one variable step.  Only a lane's first block of a run can sit deep in
 *    a unit: j >> 6 steps of x^64, then the variable one.  That is <= 64
 *    steps per 32 blocks for units up to 64 KiB, the sizes this kernel is
 *    tuned for; larger units (to the 2^20-block limit) are correct but pay
 *    up to 16384 steps per run and are slower.
 *  * Ciphertext stealing (a single unit of 16 m + r bytes): the bulk kernel
 *    does blocks 0 .. m-2, k_aes_xts_cts behind it the last 16 + r bytes on
 *    one lane; it reads both input pieces before it writes (in place exact).
 * Loads and stores are the streaming (non-temporal) form; every block is read
 * and written by the same lane, so in place is allowed in both directions.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "otc_device.h"
#include "otc_kernels.h"
#include "aes_tt_dev.h"

using namespace otc_dev;

namespace {

constexpr int XTS_THREADS = 1024;
constexpr int XTS_B = 4;                                          /* blocks per lane and pass */
constexpr uint32_t XTS_PASS = 64u * XTS_B;                        /* blocks per wave pass */
constexpr uint32_t XTS_PASSES = 8;
constexpr uint32_t XTS_RUN = XTS_PASS * XTS_PASSES;               /* 2048 blocks per wave */
constexpr uint64_t XTS_CHUNK = (uint64_t)(XTS_THREADS / 64) * XTS_RUN; /* 32768 blocks per workgroup step */
constexpr uint32_t XTS_SMALL_MAX = 4;                             /* units up to here: the SMALL form */
/* a pass of the cached form starts anywhere in a unit of XTS_SMALL_MAX + 1 blocks or more */
static_assert((XTS_SMALL_MAX + XTS_PASS - 1) / (XTS_SMALL_MAX + 1) + 1 <= 64, "a pass must fit one 64-unit tweak set");

struct XtsParams {
    const uint8_t *in;
    uint8_t *out;
    uint64_t nblocks;
    uint64_t tw_lo, tw_hi; /* tweak0 as a little-endian 128-bit number */
    uint64_t magic;        /* 2^42 / ub + 1: off / ub = off * magic >> 42 for off < 2^21 */
    uint32_t ub;           /* blocks per unit, 1 .. 2^20 */
    uint32_t pad;
};

/* a tweak: the little-endian integer's qwords */
struct T128 {
    uint64_t lo, hi;
};
/* v * (x^7 + x^2 + x + 1): what v, shifted out at the top, folds back in */
__device__ __forceinline__ T128 fold(uint64_t v)
{
    return {v ^ (v << 1) ^ (v << 2) ^ (v << 7), (v >> 63) ^ (v >> 62) ^ (v >> 57)};
}
__device__ __forceinline__ T128 mul_x64(T128 t)
{
    const T128 f = fold(t.hi);
    return {f.lo, t.lo ^ f.hi};
}
/* T * x^k, 0 <= k <= 63 */
__device__ __forceinline__ T128 mul_xk(T128 t, uint32_t k)
{
    const uint32_t n = 63u - k;
    const T128 f = fold((t.hi >> 1) >> n);
    return {(t.lo << k) ^ f.lo, ((t.hi << k) | ((t.lo >> 1) >> n)) ^ f.hi};
}
__device__ __forceinline__ T128 mul_xj(T128 t, uint32_t j)
{
    for (uint32_t q = j >> 6; q; --q) t = mul_x64(t);
    return mul_xk(t, j & 63u);
}
__device__ __forceinline__ void t_words(T128 t, uint32_t (&w)[4])
{
    w[0] = (uint32_t)t.lo; w[1] = (uint32_t)(t.lo >> 32); w[2] = (uint32_t)t.hi; w[3] = (uint32_t)(t.hi >> 32);
}
__device__ __forceinline__ T128 t_shfl(T128 t, uint32_t src)
{
    uint32_t w[4];
    t_words(t, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (uint32_t)__shfl((int)w[k], (int)src);
    return {(uint64_t)w[1] << 32 | w[0], (uint64_t)w[3] << 32 | w[2]};
}
/* the cipher input of unit u's tweak: tweak0 + u, 128-bit little-endian */
__device__ __forceinline__ void tweak_number(const XtsParams &P, uint64_t u, uint32_t (&s)[4])
{
    const uint64_t lo = P.tw_lo + u;
    t_words({lo, P.tw_hi + (lo < P.tw_lo ? 1u : 0u)}, s);
}

/* The forward cipher on the constant tables in global memory (the
 * decryption kernel's tweak passes, the stealing kernel); state ^ rk[0..3]
 * already applied, as enc_rounds4_from<1, ..>. */
__device__ __forceinline__ uint32_t b0(uint32_t w) { return w & 0xFFu; }
__device__ __forceinline__ uint32_t b1(uint32_t w) { return (w >> 8) & 0xFFu; }
__device__ __forceinline__ uint32_t b2(uint32_t w) { return (w >> 16) & 0xFFu; }
__device__ __forceinline__ uint32_t b3(uint32_t w) { return w >> 24; }
template <int NR, int B>
__device__ __forceinline__ void enc_rounds_global(const otc_aes_key &K, uint32_t (&s)[B][4])
{
    const uint32_t *te = g_tab.te0;
    const uint8_t *sb = g_tab.sb;
    uint32_t t[B][4];
#pragma unroll
    for (int r = 1; r < NR; ++r) {
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                t[b][j] = te[b0(s[b][j])] ^ rotl8(te[b1(s[b][(j + 1) & 3])]) ^ rotl16(te[b2(s[b][(j + 2) & 3])]) ^
                          rotl24(te[b3(s[b][(j + 3) & 3])]) ^ K.rk[4 * r + j];
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[b][j] = t[b][j];
    }
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            t[b][j] = ((uint32_t)sb[b0(s[b][j])] | (uint32_t)sb[b1(s[b][(j + 1) & 3])] << 8 |
                       (uint32_t)sb[b2(s[b][(j + 2) & 3])] << 16 | (uint32_t)sb[b3(s[b][(j + 3) & 3])] << 24) ^
                      K.rk[4 * NR + j];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[b][j] = t[b][j];
}
/* the inverse cipher likewise (equivalent-inverse schedule, as dec_rounds4) */
template <int NR>
__device__ __forceinline__ void dec_rounds_global(const otc_aes_key &K, uint32_t (&s)[4])
{
    const uint32_t *td = g_tab.td0;
    const uint8_t *isb = g_tab.isb;
    uint32_t t[4];
#pragma unroll
    for (int r = 1; r < NR; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            t[j] = td[b0(s[j])] ^ rotl8(td[b1(s[(j + 3) & 3])]) ^ rotl16(td[b2(s[(j + 2) & 3])]) ^
                   rotl24(td[b3(s[(j + 1) & 3])]) ^ K.rk[4 * r + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = t[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        t[j] = ((uint32_t)isb[b0(s[j])] | (uint32_t)isb[b1(s[(j + 3) & 3])] << 8 |
                (uint32_t)isb[b2(s[(j + 2) & 3])] << 16 | (uint32_t)isb[b3(s[(j + 1) & 3])] << 24) ^
               K.rk[4 * NR + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = t[j];
}

/* E_K2 of B tweak numbers per lane: the LDS image (encryption kernel) or the
 * global tables (decryption kernel, whose LDS holds the inverse image) */
template <int NR, bool DEC, int B>
__device__ __forceinline__ void tweak_encrypt(const uint32_t *tbl, const uint32_t (&lk)[4], const otc_aes_key &K2,
                                              uint32_t (&s)[B][4])
{
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[b][j] ^= K2.rk[j];
    if constexpr (DEC)
        enc_rounds_global<NR, B>(K2, s);
    else
        enc_rounds4_from<1, NR, B>(tbl, lk, K2, s);
}

/* One wave's run: the blocks [r0, r0 + XTS_RUN) below P.nblocks (r0 wave-uniform) */
template <int NR, bool DEC, bool SMALL>
__device__ __forceinline__ void xts_run(const XtsParams &P, const otc_aes_key &K1, const otc_aes_key &K2,
                                        const uint32_t *tbl, const uint32_t (&lk)[4], uint32_t lk_is2,
                                        uint32_t lane, uint64_t r0)
{
    constexpr int B = XTS_B;
    /* where a pass starts: block ra of unit ua (both wave-uniform) */
    uint64_t ua = r0 / P.ub;
    uint32_t ra = (uint32_t)(r0 - ua * P.ub);
    auto div_ub = [&](uint32_t off) { return (uint32_t)(((uint64_t)off * P.magic) >> 42); };

    T128 set = {0, 0};   /* E_K2 of unit (set0 + lane)'s tweak number */
    uint64_t set0 = 0, set_end = 0;
    T128 cur = {0, 0};   /* the tweak of the lane's previous block */

#pragma unroll 1
    for (uint32_t p = 0; p < XTS_PASSES; ++p) {
        const uint64_t p0 = r0 + (uint64_t)p * XTS_PASS;
        if (p0 >= P.nblocks) break;
        const bool full = p0 + XTS_PASS <= P.nblocks;
        uint32_t T[B][4];

        if constexpr (SMALL) {
            uint32_t s[B][4];
            uint32_t jj[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const uint32_t off = ra + 64u * b + lane, du = div_ub(off);
                jj[b] = off - du * P.ub;
                tweak_number(P, ua + du, s[b]);
            }
            tweak_encrypt<NR, DEC, B>(tbl, lk, K2, s);
#pragma unroll
            for (int b = 0; b < B; ++b)
                t_words(mul_xk({(uint64_t)s[b][1] << 32 | s[b][0], (uint64_t)s[b][3] << 32 | s[b][2]}, jj[b]), T[b]);
        } else {
            /* the pass's last block inside the call decides whether the set still covers it */
            const uint32_t last = ra + (full ? XTS_PASS - 1u : (uint32_t)(P.nblocks - 1u - p0));
            if (ua + div_ub(last) >= set_end) {
                uint32_t s[1][4];
                tweak_number(P, ua + lane, s[0]);
                tweak_encrypt<NR, DEC, 1>(tbl, lk, K2, s);
                set = {(uint64_t)s[0][1] << 32 | s[0][0], (uint64_t)s[0][3] << 32 | s[0][2]};
                set0 = ua;
                set_end = ua + 64u;
            }
            const uint32_t ahead = (uint32_t)(ua - set0);
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const uint32_t off = ra + 64u * b + lane, du = div_ub(off);
                const uint32_t j = off - du * P.ub;
                const bool first = b == 0 && p == 0; /* no previous block in this run */
                const bool fetch = first || j < 64u;
                const T128 step = mul_x64(cur);
                if (__any(fetch)) { /* wave-uniform: every lane takes part in the cross-lane read */
                    T128 f = t_shfl(set, (ahead + du) & 63u);
                    if (first) f = mul_xj(f, j);
                    else f = mul_xk(f, j & 63u);
                    cur = fetch ? f : step;
                } else {
                    cur = step;
                }
                t_words(cur, T[b]);
            }
        }

        uint32_t s[B][4];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const uint64_t i = p0 + 64u * b + lane;
            const uint4 v = (full || i < P.nblocks) ? ld16<M_STREAM>(P.in, i) : make_uint4(0, 0, 0, 0);
            s[b][0] = v.x ^ T[b][0] ^ K1.rk[0]; s[b][1] = v.y ^ T[b][1] ^ K1.rk[1];
            s[b][2] = v.z ^ T[b][2] ^ K1.rk[2]; s[b][3] = v.w ^ T[b][3] ^ K1.rk[3];
        }
        if constexpr (DEC)
            dec_rounds4<NR, B>(tbl, lk, lk_is2, K1, s);
        else
            enc_rounds4_from<1, NR, B>(tbl, lk, K1, s);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const uint64_t i = p0 + 64u * b + lane;
            if (full || i < P.nblocks)
                st16<M_STREAM>(P.out, i, make_uint4(s[b][0] ^ T[b][0], s[b][1] ^ T[b][1], s[b][2] ^ T[b][2],
                                                    s[b][3] ^ T[b][3]));
        }

        /* the next pass starts XTS_PASS blocks on */
        ra += XTS_PASS;
        const uint32_t d = div_ub(ra);
        ua += d;
        ra -= d * P.ub;
    }
}

template <int NR, bool DEC, bool SMALL>
__global__ __launch_bounds__(XTS_THREADS) void k_aes_xts(XtsParams P, otc_aes_key K1, otc_aes_key K2)
{
    /* encryption: Te0..Te3 (128 KiB); decryption: Td0..Td3 + inverse S-box (160 KiB) */
    __shared__ __attribute__((aligned(16))) uint32_t tbl[DEC ? 2 * 256 * 64 + 256 * 32 : 2 * 256 * 64];
    uint32_t lk[4];
    uint32_t lane;
    if constexpr (DEC) {
        fill_dtbl4<XTS_THREADS>(tbl, g_tab.td0, g_tab.is4);
        __syncthreads();
        lane = threadIdx.x & 63u;
        tbl4_lane_consts(lane, lk);
    } else {
        lane = tt_open<XTS_THREADS>(tbl, lk).lane;
    }
    const uint32_t lk_is2 = 0x40000u | ((lane & 31u) << 3);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t base = (uint64_t)blockIdx.x * XTS_CHUNK; base < P.nblocks; base += (uint64_t)gridDim.x * XTS_CHUNK) {
        const uint64_t r0 = base + (uint64_t)wave * XTS_RUN;
        if (r0 < P.nblocks) xts_run<NR, DEC, SMALL>(P, K1, K2, tbl, lk, lk_is2, lane, r0);
    }
}

/* Ciphertext stealing: the last 16 + r bytes of a single unit of 16 m + r
 * bytes (m >= 1, 0 < r < 16), on one lane with the tables in global memory.
 *   encryption: CC = Enc(P_{m-1}, T_{m-1}); C_m = CC[:r]; C_{m-1} = Enc(P_m || CC[r:], T_m)
 *   decryption: PP = Dec(C_{m-1}, T_m);     P_m = PP[:r]; P_{m-1} = Dec(C_m || PP[r:], T_{m-1})
 * Both input pieces are read before anything is written. */
struct XtsCtsParams {
    const uint8_t *in;
    uint8_t *out;
    uint64_t tw_lo, tw_hi;
    uint32_t m, r;
};
template <int NR, bool DEC>
__device__ __forceinline__ void cts_block(const otc_aes_key &K1, T128 t, uint32_t (&s)[4])
{
    uint32_t w[4];
    t_words(t, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] ^= w[j] ^ K1.rk[j];
    if constexpr (DEC) {
        dec_rounds_global<NR>(K1, s);
    } else {
        uint32_t s1[1][4] = {{s[0], s[1], s[2], s[3]}};
        enc_rounds_global<NR, 1>(K1, s1);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = s1[0][j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] ^= w[j];
}
template <int NR, bool DEC>
__global__ __launch_bounds__(64) void k_aes_xts_cts(XtsCtsParams P, otc_aes_key K1, otc_aes_key K2)
{
    if (threadIdx.x != 0) return;
    uint32_t tn[1][4];
    t_words({P.tw_lo, P.tw_hi}, tn[0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) tn[0][j] ^= K2.rk[j];
    enc_rounds_global<NR, 1>(K2, tn);
    const T128 t_full = mul_xj({(uint64_t)tn[0][1] << 32 | tn[0][0], (uint64_t)tn[0][3] << 32 | tn[0][2]}, P.m - 1u);
    const T128 t_part = mul_xk(t_full, 1u); /* T_m */

    const uint4 v = ld16(P.in, P.m - 1u);
    uint8_t part[16];
    for (uint32_t n = 0; n < 16; ++n) part[n] = n < P.r ? P.in[16ull * P.m + n] : 0;

    uint32_t cc[4] = {v.x, v.y, v.z, v.w};
    cts_block<NR, DEC>(K1, DEC ? t_part : t_full, cc);
    uint32_t last[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t n = 4u * j + q;
            w |= (n < P.r ? (uint32_t)part[n] : (cc[j] >> (8 * q)) & 0xFFu) << (8 * q);
        }
        last[j] = w;
    }
    cts_block<NR, DEC>(K1, DEC ? t_full : t_part, last);
    for (uint32_t n = 0; n < P.r; ++n) P.out[16ull * P.m + n] = (uint8_t)(cc[n >> 2] >> (8 * (n & 3u)));
    st16(P.out, P.m - 1u, make_uint4(last[0], last[1], last[2], last[3]));
}

void le128(const uint8_t t[16], uint64_t &lo, uint64_t &hi)
{
    lo = hi = 0;
    for (int i = 7; i >= 0; --i) {
        lo = lo << 8 | t[i];
        hi = hi << 8 | t[8 + i];
    }
}

} // namespace

/* ---- host entry points (otc_kernels.h) ------------------------------------- */
namespace otc_impl {

hipError_t xts_bulk(const void *in, void *out, uint64_t nblocks, uint32_t unit_blocks, const otc_aes_key &K1,
                    const otc_aes_key &K2, const uint8_t tweak0[16], hipStream_t st)
{
    if (nblocks == 0) return hipSuccess;
    if (unit_blocks < 1 || unit_blocks > (1u << 20) || K1.nr != K2.nr) return hipErrorInvalidValue;
    XtsParams P{};
    P.in = (const uint8_t *)in;
    P.out = (uint8_t *)out;
    P.nblocks = nblocks;
    le128(tweak0, P.tw_lo, P.tw_hi);
    P.ub = unit_blocks;
    P.magic = (1ull << 42) / unit_blocks + 1u;
    /* one workgroup per CU (the 128 / 160 KiB table image), grid-stride over the chunks */
    const uint64_t need = (nblocks + XTS_CHUNK - 1) / XTS_CHUNK, cus = (uint64_t)device_cus();
    const dim3 grid((unsigned)(need < cus ? need : cus)), wg(XTS_THREADS);
    const bool dec = K1.dir == OTC_DIR_DECRYPT, small = unit_blocks <= XTS_SMALL_MAX;
    return with_rounds(K1.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        if (dec && small) hipLaunchKernelGGL((k_aes_xts<NR, true, true>), grid, wg, 0, st, P, K1, K2);
        else if (dec) hipLaunchKernelGGL((k_aes_xts<NR, true, false>), grid, wg, 0, st, P, K1, K2);
        else if (small) hipLaunchKernelGGL((k_aes_xts<NR, false, true>), grid, wg, 0, st, P, K1, K2);
        else hipLaunchKernelGGL((k_aes_xts<NR, false, false>), grid, wg, 0, st, P, K1, K2);
        return hipGetLastError();
    });
}

hipError_t xts_steal(const void *in, void *out, uint32_t m, uint32_t r, const otc_aes_key &K1, const otc_aes_key &K2,
                     const uint8_t tweak0[16], hipStream_t st)
{
    if (m < 1 || m > (1u << 20) || r < 1 || r > 15 || K1.nr != K2.nr) return hipErrorInvalidValue;
    XtsCtsParams P{};
    P.in = (const uint8_t *)in;
    P.out = (uint8_t *)out;
    le128(tweak0, P.tw_lo, P.tw_hi);
    P.m = m;
    P.r = r;
    const bool dec = K1.dir == OTC_DIR_DECRYPT;
    return with_rounds(K1.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        if (dec) hipLaunchKernelGGL((k_aes_xts_cts<NR, true>), dim3(1), dim3(64), 0, st, P, K1, K2);
        else hipLaunchKernelGGL((k_aes_xts_cts<NR, false>), dim3(1), dim3(64), 0, st, P, K1, K2);
        return hipGetLastError();
    });
}

} // namespace otc_impl
