/*
 * chacha.hip -- ChaCha20 and Poly1305 (RFC 8439) on gfx950.
 *
 * ChaCha20.  One lane computes whole 64-byte blocks with the 16 state words
 * in VGPRs.  Constants, key and nonce are kernel arguments by value (SGPRs);
 * only the counter word differs per lane.  No tables, no LDS, no
 * secret-dependent addresses or branches.
 *
 *   pass    64 blocks (4 KiB), one per lane.
 *   wave    CC_RUN consecutive passes; a workgroup is CC_WAVES waves, the
 *           grid one workgroup per CC_WAVES * CC_RUN passes (no stride loop).
 *   bulk    whole passes of 16-byte aligned buffers: 16-byte non-temporal
 *           loads and stores, the plaintext of a pass loaded before its
 *           keystream is computed (so in place is safe: a lane stores only
 *           over addresses it loaded).
 *   edge    everything past the last whole pass, and the whole call when a
 *           buffer is not 16-byte aligned: one block per lane, byte loads and
 *           stores, every byte guarded by the length.
 *
 * Store layout of the bulk kernel: transposed.  Lane 4g + q computes block
 * 16q + g of the pass and the four lanes of a quad exchange quarters (two DPP
 * quad_perm butterflies, a 4x4 transpose of 16-byte pieces), after which load
 * and store j of lane l cover bytes (64 j + l) * 16 ..: every load and store
 * instruction of a wave covers 1 KiB contiguously.  The direct layout -- lane l
 * owns block l, so the lanes of one 16-byte access are 64 bytes apart -- needs
 * no exchange and measured 2.4-3.1 times SLOWER (633-691 against 1639-1967
 * GB/s, docs/PERF.md "ChaCha20-Poly1305") and was removed.
 *
 * Poly1305.  tag = ((sum_{i=1..n} c_i r^(n-i+1)) mod p + s) mod 2^128 with
 * p = 2^130 - 5 -- polynomial evaluation, the shape of GHASH (aes_gcm.hip),
 * and the same tree:
 *
 *   pass        64 consecutive blocks, one per lane: a coalesced 1 KiB load.
 *   batch       PL_BATCH = 4 passes: A = A C^4 + X0 C^3 + X1 C^2 + X2 C + X3
 *               with C = r^64, the products accumulated in 64 bits and
 *               carried once per batch.
 *   wave span   m = PL_SPAN = 64 * PL_RUN = 2048 blocks (32 KiB).  Lane j
 *               runs Horner under r^64 over blocks j, j + 64, ...
 *   fold        lane j multiplies its accumulator by r^(63-j); the wave sums
 *               the 64 products limb by limb: P = sum c_i r^(m-1-i), the
 *               span's partial, its last block unmultiplied.
 *   level       the partials are the blocks of the next level under
 *               G = r^m: the SAME kernel runs over them (32-byte entries of
 *               five limbs) until one is left.  Spans are aligned to the END
 *               of the data; zero blocks in front change nothing.
 *   finish      one wave: h = S r, for the AEAD h = (h + lengths) r, the full
 *               reduction mod p, a constant-time conditional subtract, + s.
 *
 * Arithmetic: five 26-bit limbs, 2^130 = 5 (mod p).  A product limb is five
 * 32x32->64 multiply-adds (v_mad_u64_u32) with precomputed 5 r_i.  Carry
 * bound: operand limbs a_i < 2^28 (a carried value is < 2^26 + 2^13, a raw
 * block limb < 2^26, block 0 adds the incoming state), multiplier limbs
 * b_j < 2^27, 5 b_j < 2^29.33: one term < 2^57.33, the five of one
 * multiplication < 2^59.66, so a 64-bit limb could overflow after 20
 * accumulated multiplications.  The code carries after PL_BATCH = 4 (plus one
 * added block): < 2^61.7.  The wave sum adds 64 carried limbs: < 2^33 in 64
 * bits.  The multipliers of a Horner step are wave-uniform (SGPRs); the powers
 * of r are computed on the host, which knows r, and travel by value: no
 * setup kernel, no host synchronisation.
 *
 * The block function, the quad transpose and the field arithmetic live in
 * chacha_dev.h, shared with chacha_batch.hip (many records per launch).
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "chacha_dev.h"
#include "otc_device.h"
#include "otc_kernels.h"

namespace otc_impl {

using otc_dev::lane_id;
using otc_dev::ld_u4;
using otc_dev::st_u4;

namespace {

/* ======================= ChaCha20 ========================================= */

constexpr uint32_t CC_WAVES = 4;        /* waves of a workgroup */
constexpr uint32_t CC_RUN = 4;          /* passes of a wave */
constexpr uint32_t CC_PASS = 64 * 64;   /* bytes of a pass */

struct CcParams {
    uint32_t key[8], nonce[3], ctr0;
    const uint8_t *in;
    uint8_t *out;
    uint64_t npass;  /* bulk: whole passes from byte 0 */
    uint64_t off;    /* edge: its first byte (a multiple of 64) */
    uint64_t nbytes; /* edge: bytes of the whole call */
};

__global__ __launch_bounds__(64 * CC_WAVES) void k_chacha20_bulk(CcParams P)
{
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * CC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    /* lane 4g + q computes block 16q + g of the pass; its 16-byte piece j is at (64 j + lane) * 16 */
    const uint32_t lb = (lane & 3u) << 4 | lane >> 2;
    for (uint32_t k = 0; k < CC_RUN; ++k) {
        const uint64_t pass = wave * CC_RUN + k;
        if (pass >= P.npass) break; /* wave-uniform */
        const uint8_t *src = P.in + pass * CC_PASS + lane * 16;
        uint8_t *dst = P.out + pass * CC_PASS + lane * 16;
        uint4 m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = ld_u4<true, true>(src + j * 1024);
        uint32_t x[16];
        /* the host refuses a call whose last counter passes 2^32 - 1: no wrap */
        cc_block(P.key, P.nonce, P.ctr0 + (uint32_t)(pass * 64) + lb, x);
        /* quarter j of this lane's block goes to lane 4g + j, which stores it as its piece q */
        cc_xchg<1>(x, (lane & 1u) != 0);
        cc_xchg<2>(x, (lane & 2u) != 0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            st_u4<true, true>(dst + j * 1024, make_uint4(m[j].x ^ x[4 * j], m[j].y ^ x[4 * j + 1], m[j].z ^ x[4 * j + 2],
                                                         m[j].w ^ x[4 * j + 3]));
    }
}

/* one block per lane from byte P.off, byte by byte; touches nothing outside
 * [in, in + nbytes) and [out, out + nbytes) */
__global__ __launch_bounds__(256) void k_chacha20_edge(CcParams P)
{
    const uint64_t at = P.off + ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 64;
    if (at >= P.nbytes) return;
    const uint64_t left = P.nbytes - at;
    const uint32_t m = left < 64 ? (uint32_t)left : 64u;
    uint32_t x[16];
    cc_block(P.key, P.nonce, P.ctr0 + (uint32_t)(at / 64), x);
    auto src = (__attribute__((address_space(1))) const uint8_t *)(P.in + at);
    auto dst = (__attribute__((address_space(1))) uint8_t *)(P.out + at);
#pragma unroll
    for (uint32_t i = 0; i < 64; ++i)
        if (i < m) dst[i] = (uint8_t)(src[i] ^ (x[i >> 2] >> (8 * (i & 3))));
}

/* ======================= Poly1305 ========================================= */

constexpr uint32_t PL_RUN = 32;              /* blocks per lane in a wave span */
constexpr uint32_t PL_SPAN = 64 * PL_RUN;    /* blocks of a wave span */
constexpr uint32_t PL_WAVES = 4;             /* wave spans of a workgroup */
constexpr int PL_MAX_LEVELS = 4;             /* 2048^4 blocks: more than any call has */
constexpr uint32_t PL_ENTRY = 32;            /* bytes of a partial: five limbs, padded */
static_assert(PL_RUN % PL_BATCH == 0, "a wave span is whole batches");

struct PlLevel {
    const uint8_t *in;  /* level 0: the message, 16-byte aligned; above: PL_ENTRY-byte partials */
    uint64_t nbytes;    /* level 0: bytes of the message */
    uint64_t nblocks;   /* blocks (entries) of this level, >= 1 */
    uint64_t nspans;    /* ceil(nblocks / PL_SPAN) */
    uint64_t pad;       /* nspans * PL_SPAN - nblocks zero blocks in front */
    uint32_t *out;      /* nspans partials */
    Fe y0;              /* level 0: the incoming state, added to block 0 */
    uint32_t pad16;     /* level 0: a short last block is zero-padded to a full one (the AEAD's pad16),
                           else it gets the 0x01 byte */
    Mul m[PL_BATCH];    /* C^64, C^128, C^192, C^256 for this level's C */
    Fe pw[64];          /* C^0 .. C^63 */
};

/* block i of the level; never reads at or past in + nbytes */
template <bool RAW>
__device__ __forceinline__ Fe pl_load(const PlLevel &P, uint64_t i)
{
    if constexpr (!RAW) {
        const uint4 a = ld_u4<false, true>(P.in + i * PL_ENTRY), b = ld_u4<false, true>(P.in + i * PL_ENTRY + 16);
        Fe f;
        f.l[0] = a.x, f.l[1] = a.y, f.l[2] = a.z, f.l[3] = a.w, f.l[4] = b.x;
        return f;
    } else {
        const uint64_t off = i * 16;
        uint32_t w[4] = {0, 0, 0, 0}, hibit = 1;
        if (off + 16 <= P.nbytes) {
            const uint4 x = ld_u4<true, true>(P.in + off);
            w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
        } else {
            /* the short last block: a branch on the length, never on the data */
            const uint32_t n = (uint32_t)(P.nbytes - off);
            auto src = (__attribute__((address_space(1))) const uint8_t *)(P.in + off);
#pragma unroll
            for (uint32_t b = 0; b < 15; ++b)
                if (b < n) w[b >> 2] |= (uint32_t)src[b] << (8 * (b & 3));
            if (!P.pad16) {
                hibit = 0;
#pragma unroll
                for (uint32_t b = 1; b < 16; ++b)
                    if (b == n) w[b >> 2] |= 1u << (8 * (b & 3));
            }
        }
        Fe f = fe_of_words(w[0], w[1], w[2], w[3], hibit);
        if (i == 0)
            for (int k = 0; k < 5; ++k) f.l[k] += P.y0.l[k];
        return f;
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool RAW>
__global__ __launch_bounds__(64 * PL_WAVES) void k_poly1305_level(PlLevel P)
{
    const uint32_t lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t ngroups = (P.nspans + PL_WAVES - 1) / PL_WAVES;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t s = g * PL_WAVES + wave;
        if (s >= P.nspans) break; /* wave-uniform; nothing in this kernel synchronises waves */
        const uint64_t v0 = s * PL_SPAN; /* index among the zero-extended blocks */
        /* the first span skips the batches that are all padding */
        const uint32_t k0 = v0 < P.pad ? (uint32_t)((P.pad - v0) / 64) & ~(PL_BATCH - 1) : 0u;
        Fe A = {{0, 0, 0, 0, 0}};
        for (uint32_t kb = k0; kb < PL_RUN; kb += PL_BATCH) {
            Fe X[PL_BATCH];
#pragma unroll
            for (uint32_t i = 0; i < PL_BATCH; ++i) {
                const uint64_t v = v0 + (uint64_t)(kb + i) * 64 + lane;
                if (v >= P.pad)
                    X[i] = pl_load<RAW>(P, v - P.pad);
                else
                    X[i] = Fe{{0, 0, 0, 0, 0}};
            }
            uint64_t d[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) d[k] = X[PL_BATCH - 1].l[k];
            fe_mac(d, A, P.m[PL_BATCH - 1]);
#pragma unroll
            for (uint32_t i = 0; i + 1 < PL_BATCH; ++i) fe_mac(d, X[i], P.m[PL_BATCH - 2 - i]);
            A = fe_carry(d);
        }
        /* fold: lane j's blocks are 63 - j short of the span's last */
        uint64_t d[5] = {0, 0, 0, 0, 0};
        fe_mac(d, A, mul_of(P.pw[63 - lane]));
        A = fe_carry(d);
#pragma unroll
        for (int k = 0; k < 5; ++k) d[k] = wave_sum(A.l[k]);
        A = fe_carry(d);
        if (lane == 0) {
            st_u4<false, true>(P.out + s * (PL_ENTRY / 4), make_uint4(A.l[0], A.l[1], A.l[2], A.l[3]));
            st_u4<false, true>(P.out + s * (PL_ENTRY / 4) + 4, make_uint4(A.l[4], 0, 0, 0));
        }
    }
}

struct PlFinal {
    const uint32_t *s; /* the last level's one partial; null: no data, h = y0 */
    Fe y0;
    Mul r;
    Fe len;            /* the AEAD's length block with its 2^128 bit */
    uint32_t aead;     /* 1: h = (h + len) r before the reduction */
    uint32_t skey[4];  /* s, little-endian words */
    uint32_t *out;     /* 16 bytes */
};

__global__ __launch_bounds__(64) void k_poly1305_final(PlFinal F)
{
    Fe h = F.y0;
    if (F.s) { /* on the call's shape, not on data */
        Fe p;
        for (int k = 0; k < 5; ++k) p.l[k] = F.s[k];
        h = fe_mul(p, F.r);
    }
    if (F.aead) {
        for (int k = 0; k < 5; ++k) h.l[k] += F.len.l[k];
        h = fe_mul(h, F.r);
    }
    uint32_t t[4];
    fe_tag(h, F.skey, t);
    const uint32_t l = threadIdx.x;
    /* lanes 0..3 store one word each */
    if (l < 4) F.out[l] = l == 0 ? t[0] : l == 1 ? t[1] : l == 2 ? t[2] : t[3];
}

uint32_t ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* the workspace: every level's partials */
constexpr otc_dev::HashShape PL_SHAPE{PL_SPAN, PL_BATCH, PL_WAVES, PL_MAX_LEVELS, PL_ENTRY, 0};

} // namespace

/* ---- host entry points ---------------------------------------------------- */

hipError_t chacha20_run(const void *in, void *out, uint64_t nbytes, const uint8_t key[32], const uint8_t nonce[12],
                        uint32_t counter, hipStream_t st)
{
    if (nbytes == 0) return hipSuccess;
    CcParams P{};
    for (int i = 0; i < 8; ++i) P.key[i] = ld32(key + 4 * i);
    for (int i = 0; i < 3; ++i) P.nonce[i] = ld32(nonce + 4 * i);
    P.ctr0 = counter;
    P.in = (const uint8_t *)in;
    P.out = (uint8_t *)out;
    P.nbytes = nbytes;
    const bool aligned = !(((uintptr_t)in | (uintptr_t)out) & 15u);
    P.npass = aligned ? nbytes / CC_PASS : 0;
    P.off = P.npass * CC_PASS;
    if (P.npass) {
        const uint64_t per = (uint64_t)CC_WAVES * CC_RUN, wgs = (P.npass + per - 1) / per;
        if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_chacha20_bulk, dim3((unsigned)wgs), dim3(64 * CC_WAVES), 0, st, P);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (P.off < nbytes) {
        const uint64_t blocks = (nbytes - P.off + 63) / 64, wgs = (blocks + 255) / 256;
        if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_chacha20_edge, dim3((unsigned)wgs), dim3(256), 0, st, P);
        return hipGetLastError();
    }
    return hipSuccess;
}

int poly1305_spans(uint64_t *spans, int max) { return otc_dev::hash_spans(PL_SHAPE, spans, max); }

hipError_t poly1305_ws_alloc(uint64_t nbytes, hipStream_t st, void **ws) { return otc_dev::hash_ws_alloc(PL_SHAPE, nbytes, st, ws); }

hipError_t poly1305_run(const void *data, uint64_t nbytes, const uint32_t r[5], const uint32_t h0[5],
                        const uint8_t s[16], const uint8_t *lenblock, bool pad16, void *out16, void *ws,
                        hipStream_t st)
{
    otc_dev::HashLevels pl;
    if (!otc_dev::hash_levels(PL_SHAPE, nbytes, pl) || (pl.nlevels && !ws)) {
        if (ws) (void)otc_dev::ws_free(ws, st);
        return hipErrorInvalidValue;
    }
    Fe R, Y0;
    for (int k = 0; k < 5; ++k) R.l[k] = r[k], Y0.l[k] = h0[k];
    PlFinal F{};
    F.s = nullptr;
    F.y0 = Y0;
    F.r = mul_of(R);
    F.aead = lenblock ? 1u : 0u;
    if (lenblock) F.len = fe_of_words(ld32(lenblock), ld32(lenblock + 4), ld32(lenblock + 8), ld32(lenblock + 12), 1);
    for (int i = 0; i < 4; ++i) F.skey[i] = ld32(s + 4 * i);
    F.out = (uint32_t *)out16;
    hipError_t e = hipSuccess;
    const uint8_t *in = (const uint8_t *)data;
    uint32_t *part = (uint32_t *)ws;
    Fe C = R; /* level l works under C = r^(PL_SPAN^l) */
    for (int l = 0; l < pl.nlevels && e == hipSuccess; ++l) {
        PlLevel P{};
        P.in = in;
        P.nbytes = l == 0 ? nbytes : 0;
        P.nblocks = pl.nblocks[l];
        P.nspans = pl.nspans[l];
        P.pad = P.nspans * PL_SPAN - P.nblocks;
        P.out = part;
        P.y0 = l == 0 ? Y0 : Fe{{0, 0, 0, 0, 0}};
        P.pad16 = pad16 ? 1u : 0u;
        const Mul mc = mul_of(C);
        P.pw[0] = Fe{{1, 0, 0, 0, 0}};
        for (int j = 1; j < 64; ++j) P.pw[j] = fe_mul(P.pw[j - 1], mc);
        const Fe c64 = fe_mul(P.pw[63], mc);
        const Mul m64 = mul_of(c64);
        Fe p = c64;
        for (uint32_t k = 0; k < PL_BATCH; ++k) {
            P.m[k] = mul_of(p);
            if (k + 1 < PL_BATCH) p = fe_mul(p, m64);
        }
        /* C^(64 PL_BATCH), squared on to C^PL_SPAN */
        for (uint32_t q = 64 * PL_BATCH; q < PL_SPAN; q *= 2) p = fe_mul(p, mul_of(p));
        C = p;
        const uint64_t ngroups = (P.nspans + PL_WAVES - 1) / PL_WAVES, cap = (uint64_t)otc_dev::device_cus() * 16;
        const dim3 g((unsigned)(ngroups < cap ? ngroups : cap)), b(64 * PL_WAVES);
        if (l == 0)
            hipLaunchKernelGGL(k_poly1305_level<true>, g, b, 0, st, P); /* the data streams once */
        else
            hipLaunchKernelGGL(k_poly1305_level<false>, g, b, 0, st, P); /* partials come back from L2 */
        e = hipGetLastError();
        in = (const uint8_t *)part;
        F.s = part;
        part += P.nspans * (PL_ENTRY / 4);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_poly1305_final, dim3(1), dim3(64), 0, st, F);
        e = hipGetLastError();
    }
    if (ws) {
        const hipError_t f = otc_dev::ws_free(ws, st);
        if (e == hipSuccess) e = f;
    }
    return e;
}

} // namespace otc_impl
