/*
 * aes_gcm_siv.hip -- AES-GCM-SIV (RFC 8452) on gfx950: POLYVAL over the whole
 * chip, the finisher that turns the hash into the tag, and a T-table counter
 * mode whose initial counter block is read from DEVICE memory.
 *
 * POLYVAL is Y_i = dot(Y_{i-1} ^ X_i, H), dot(a, b) = a . b . x^-128 in
 * GF(2^128) mod x^128 + x^127 + x^126 + x^121 + 1, blocks little-endian.  It
 * has GHASH's shape, so it runs GHASH's decomposition (aes_gcm.hip's header)
 * with GHASH's level kernel, k_ghash_level of ghash_levels_dev.h, unchanged: that
 * kernel multiplies by positional byte tables and XORs, and dot is as linear
 * in its argument as GHASH's product.
 *
 * Of the two ways to feed it, this file builds the tables directly in
 * POLYVAL's convention (k_polyval_tables, doubling pv_mulx of polyval_dev.h)
 * and does NOT go through rev(GHASH(mulX(rev H), rev X)):
 *   - the hot loop stays gh_mul as it is: no byte reversal per loaded block
 *     (four v_perm_b32 per 16 lookups) and none of the partials between
 *     levels, and k_ghash_level needs no template parameter, so GHASH's own
 *     instantiation is the code it was;
 *   - four little-endian words as loaded ARE a POLYVAL element, so the
 *     builder and the finisher need no swaps at all (GHASH's need two each);
 *   - what differs sits where it is cheap: 16 x 256 table entries per
 *     constant, once per call.
 * T[p][b] = dot(byte b at position p, C) = sum over the bits k of b of
 * C . x^(8 p + k - 128): doublings of the SEED dot(C, 1) = C . x^-128, which
 * the host computes with the powers C = H^(2048^l) and C^64 (aes.h
 * aes_polyval_dot), as it does GHASH's.
 *
 * The finisher k_gcmsiv_final, one lane: Y = dot(S, H) by the bit loop; for
 * the AEAD then S_s = dot(Y ^ lenblock, H) ^ nonce with bit 127 cleared and
 * tag = E(S_s) under the derived encryption key, the cipher on the constant
 * tables in global memory (ocb_dev.h enc_block_global); lanes 0..3 store one
 * word each.
 *
 * k_aes_ctr_le32: the counter block of block i is the tag with word 0
 * replaced by (tag word 0 + i) mod 2^32 and bit 31 of word 3 forced on
 * (polyval_dev.h siv_ctr_block).  The tag is computed on the device from the
 * data, so the kernel takes a POINTER to it and every wave reads the 16 bytes
 * once, a uniform load, before its first block; nothing goes back to the
 * host.  A message has at most 2^32 blocks, so the 32-bit counter never
 * repeats within one and the wrap needs no second launch.  Layout:
 * aes_xts.hip's and aes_ocb.hip's -- a wave takes a RUN of 2048 consecutive
 * blocks as 8 passes of 256 (4 blocks per lane, block = pass base + 64 b +
 * lane: every access a coalesced 1 KiB wave access), a 1024-thread workgroup
 * a chunk of 16 runs (512 KiB) per grid step, one workgroup per CU; loads and
 * stores are the streaming (non-temporal) form.  Every block is read and
 * written by the same lane, so in place is allowed.  All ten (fourteen) rounds
 * go through the LDS tables: the round-1 sharing that ctr_cache of aes_tt.hip
 * exploits (only the counter's low byte varies between the lanes of an
 * aligned group) would need the runs aligned to a counter the host does not
 * know; it was not built and so not measured.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "aes.h"
#include "otc_device.h"
#include "otc_kernels.h"
#include "aes_tt_dev.h"
#include "ocb_dev.h"
#include "ghash_levels_dev.h"
#include "polyval_dev.h"

using namespace otc_dev;

namespace otc_impl {

namespace {

/* ---- POLYVAL: the tables and the finisher ----------------------------------- */
/* tab[t] = the table of the constant whose seed is K.c[t]: one workgroup per
 * (table, byte position), one thread per byte value, as k_gf128_tables */
template <int N>
__global__ __launch_bounds__(256) void k_polyval_tables(GfConsts<N> K, uint4 *tab)
{
    const uint32_t t = blockIdx.x >> 4, pos = blockIdx.x & 15u, b = threadIdx.x;
    const uint32_t seed[4] = {K.c[t].x, K.c[t].y, K.c[t].z, K.c[t].w};
    uint32_t e[4];
    pv_table_entry(e, seed, pos, b);
    tab[(size_t)t * GF_TAB + pos * 256 + b] = make_uint4(e[0], e[1], e[2], e[3]);
}

struct SivFinal {
    const uint4 *s;      /* the last level's one partial; null: no data, Y = y0 */
    uint32_t y0[4];
    uint32_t hseed[4];   /* dot(H, 1) */
    uint32_t lenblock[4];
    uint32_t nonce[3];
    uint32_t *out;       /* 16 bytes */
};

/* NR == 0: write Y (POLYVAL); else the GCM-SIV tag under K */
template <int NR>
__global__ __launch_bounds__(64) void k_gcmsiv_final(SivFinal F, otc_aes_key K)
{
    uint32_t y[4];
    if (F.s) {
        const uint4 s = *F.s;
        const uint32_t x[4] = {s.x, s.y, s.z, s.w};
        pv_dot(y, x, F.hseed);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = F.y0[j];
    }
    if constexpr (NR != 0) {
        uint32_t x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = y[j] ^ F.lenblock[j];
        pv_dot(y, x, F.hseed);
#pragma unroll
        for (int j = 0; j < 3; ++j) y[j] ^= F.nonce[j];
        y[3] &= 0x7FFFFFFFu;
        enc_block_global<NR>(K, y);
    }
    const uint32_t l = threadIdx.x;
    /* lanes 0..3 store one word each */
    if (l < 4) F.out[l] = l == 0 ? y[0] : l == 1 ? y[1] : l == 2 ? y[2] : y[3];
}

/* ---- the counter mode -------------------------------------------------------- */
constexpr int SIV_THREADS = 1024;
constexpr int SIV_B = 4;                                             /* blocks per lane and pass */
constexpr uint32_t SIV_PASS = 64u * SIV_B;                           /* blocks per wave pass */
constexpr uint32_t SIV_PASSES = 8;
constexpr uint32_t SIV_RUN = SIV_PASS * SIV_PASSES;                  /* 2048 blocks per wave */
constexpr uint64_t SIV_CHUNK = (uint64_t)(SIV_THREADS / 64) * SIV_RUN; /* 32768 blocks per workgroup step */

struct SivCtrParams {
    const uint8_t *in;
    uint8_t *out;
    uint64_t nfull;       /* full blocks, <= 2^32 */
    uint32_t tail;        /* trailing partial block bytes */
    const uint32_t *ctr0; /* the initial counter block: 16 bytes of device memory, 4-byte aligned */
};

template <int NR>
__global__ __launch_bounds__(SIV_THREADS) void k_aes_ctr_le32(SivCtrParams P, otc_aes_key K)
{
    constexpr int B = SIV_B;
    __shared__ __attribute__((aligned(16))) uint32_t tbl[2 * 256 * 64];
    uint32_t lk[4];
    const uint32_t lane = tt_open<SIV_THREADS>(tbl, lk).lane;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    /* once per wave, the same address in every lane */
    const uint32_t t[4] = {P.ctr0[0], P.ctr0[1], P.ctr0[2], P.ctr0[3]};
    const uint64_t total = P.nfull + (P.tail ? 1u : 0u);
    for (uint64_t base = (uint64_t)blockIdx.x * SIV_CHUNK; base < total; base += (uint64_t)gridDim.x * SIV_CHUNK) {
        const uint64_t r0 = base + (uint64_t)wave * SIV_RUN;
#pragma unroll 1
        for (uint32_t p = 0; p < SIV_PASSES; ++p) {
            const uint64_t W = r0 + (uint64_t)p * SIV_PASS; /* wave-uniform */
            if (W >= total) break;
            const bool full = W + SIV_PASS <= P.nfull;
            uint32_t s[B][4];
            uint4 x[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const uint64_t i = W + 64u * b + lane;
                const bool ok = full || i < P.nfull;
                x[b] = ok ? ld16<M_STREAM>(P.in, i) : make_uint4(0, 0, 0, 0);
                uint32_t c[4];
                siv_ctr_block(c, t, (uint32_t)i);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[b][j] = c[j] ^ K.rk[j];
            }
            enc_rounds4_from<1, NR, B>(tbl, lk, K, s);
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const uint64_t i = W + 64u * b + lane;
                if (full || i < P.nfull) {
                    st16<M_STREAM>(P.out, i,
                                   make_uint4(x[b].x ^ s[b][0], x[b].y ^ s[b][1], x[b].z ^ s[b][2], x[b].w ^ s[b][3]));
                } else if (i == P.nfull && P.tail) {
                    /* the partial last block, as in ctr_cached_iter of aes_tt.hip */
                    const uint32_t ks[4] = {s[b][0], s[b][1], s[b][2], s[b][3]};
                    for (uint32_t n = 0; n < P.tail; ++n)
                        P.out[16 * i + n] = P.in[16 * i + n] ^ (uint8_t)(ks[n >> 2] >> (8 * (n & 3)));
                }
            }
        }
    }
}

} // namespace

/* ---- host entry points (otc_kernels.h) ------------------------------------- */
int polyval_spans(uint64_t *spans, int max) { return otc_dev::hash_spans(GH_SHAPE, spans, max); }

hipError_t polyval_ws_alloc(uint64_t nbytes, hipStream_t st, void **ws) { return otc_dev::hash_ws_alloc(GH_SHAPE, nbytes, st, ws); }

hipError_t polyval_run(const void *data, uint64_t nbytes, const uint8_t h[16], const uint8_t y0[16], const SivTag *siv,
                       void *out16, void *ws, hipStream_t st)
{
    otc_dev::HashLevels pl;
    if (!otc_dev::hash_levels(GH_SHAPE, nbytes, pl) || (pl.nlevels && !ws) || (siv && !siv->enc)) {
        if (ws) (void)otc_dev::ws_free(ws, st);
        return hipErrorInvalidValue;
    }
    static const uint8_t one[16] = {1};
    uint8_t seed[16];
    SivFinal F{};
    F.s = nullptr;
    words(F.y0, y0);
    aes_polyval_dot(seed, h, one);
    words(F.hseed, seed);
    if (siv) {
        words(F.lenblock, siv->lenblock);
        memcpy(F.nonce, siv->nonce, 12);
    }
    F.out = (uint32_t *)out16;
    hipError_t e = hipSuccess;
    if (pl.nlevels) {
        GfConsts<2 * GH_MAX_LEVELS> K{}; /* per level: the seeds of C^64, then C */
        uint8_t k[2 * GH_MAX_LEVELS][16];
        gh_level_consts(k, pl.nlevels, h, aes_polyval_dot);
        for (int i = 0; i < 2 * pl.nlevels; ++i) {
            aes_polyval_dot(seed, k[i], one);
            K.c[i] = u4_of(seed);
        }
        uint4 *tab = (uint4 *)ws;
        hipLaunchKernelGGL(k_polyval_tables<2 * GH_MAX_LEVELS>, dim3((unsigned)pl.nlevels * 2 * 16), dim3(256), 0, st, K, tab);
        e = hipGetLastError();
        if (e == hipSuccess) e = gh_run_levels(pl, data, nbytes, u4_of(y0), tab, st, &F.s);
    }
    if (e == hipSuccess) {
        if (siv) {
            e = with_rounds(siv->enc->nr, [&](auto nr) {
                constexpr int NR = decltype(nr)::value;
                hipLaunchKernelGGL((k_gcmsiv_final<NR>), dim3(1), dim3(64), 0, st, F, *siv->enc);
                return hipGetLastError();
            });
        } else {
            hipLaunchKernelGGL((k_gcmsiv_final<0>), dim3(1), dim3(64), 0, st, F, otc_aes_key{});
            e = hipGetLastError();
        }
    }
    if (ws) {
        const hipError_t f = otc_dev::ws_free(ws, st);
        if (e == hipSuccess) e = f;
    }
    return e;
}

int ctr_le32_spans(uint64_t *spans, int max)
{
    const uint64_t s[] = {16,                  /* a lane's block */
                          64 * 16,             /* one load of a wave */
                          SIV_PASS * 16,       /* a pass */
                          SIV_RUN * 16,        /* a wave's run */
                          SIV_CHUNK * 16,      /* a workgroup's chunk */
                          (uint64_t)device_cus() * SIV_CHUNK * 16}; /* the full grid's first step: past it a second begins */
    const int n = (int)(sizeof s / sizeof s[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = s[i];
    return n;
}

hipError_t ctr_le32_run(const void *in, void *out, uint64_t nbytes, const otc_aes_key &K, const void *ctr0_dev,
                        hipStream_t st)
{
    if (nbytes == 0) return hipSuccess;
    if (nbytes > ((uint64_t)1 << 36) || K.dir != OTC_DIR_ENCRYPT) return hipErrorInvalidValue;
    SivCtrParams P{};
    P.in = (const uint8_t *)in;
    P.out = (uint8_t *)out;
    P.nfull = nbytes / 16;
    P.tail = (uint32_t)(nbytes % 16);
    P.ctr0 = (const uint32_t *)ctr0_dev;
    /* one workgroup per CU (the 128 KiB table image), grid-stride over the chunks */
    const uint64_t total = P.nfull + (P.tail ? 1 : 0);
    const uint64_t need = (total + SIV_CHUNK - 1) / SIV_CHUNK, cus = (uint64_t)device_cus();
    const dim3 grid((unsigned)(need < cus ? need : cus)), wg(SIV_THREADS);
    return with_rounds(K.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        hipLaunchKernelGGL((k_aes_ctr_le32<NR>), grid, wg, 0, st, P, K);
        return hipGetLastError();
    });
}

} // namespace otc_impl
