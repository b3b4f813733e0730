/*
 * aes_gcm.hip -- GHASH (NIST SP 800-38D) on gfx950, parallel over the whole
 * chip, and the finishing step of AES-GCM.  GCM's counter mode is the CTR
 * kernels' (engine.cpp otc_aes_ctr32); this file is the hash.
 *
 * GHASH is Y_i = (Y_{i-1} ^ X_i) . H in GF(2^128) -- serial as written.  With
 * n blocks, Y_n = S . H where S = sum X_i . H^(n-1-i) (X_0 carries the
 * incoming state y0).  The decomposition, smallest piece first:
 *
 *   pass        64 consecutive blocks, one per lane: a coalesced 1 KiB load.
 *   batch       GH_BATCH = 8 passes loaded ahead of the multiplications.
 *   wave span   m = GH_SPAN = 64 * GH_RUN = 2048 blocks (32 KiB).  Lane j
 *               runs Horner under H^64 over blocks j, j + 64, ...:
 *               A_j = sum_k X_{j+64k} . (H^64)^(GH_RUN-1-k).
 *   workgroup   GH_WAVES = 16 wave spans (512 KiB).  The waves leave their 64
 *               accumulators in LDS; then lane w of wave 0 folds wave w's:
 *               P = sum_j A_j . H^(63-j), 63 multiplications under H -- one
 *               serial chain for the 16 wave spans at once instead of one per
 *               wave (a wave instruction costs the same for 16 lanes as for
 *               one).  P is the wave span's partial, its last block
 *               unmultiplied.
 *   level       S = sum_l P_l . G^(L-1-l) with G = H^m is the same sum over
 *               the L partials under G, so the SAME kernel runs again over
 *               the partials with tables for G^64 and G, and again under
 *               G^m, until one block is left: 3 levels reach 2^33 blocks,
 *               more than a GCM message has.  The spans are aligned to the
 *               END of the data: the first one is the short one (zero blocks
 *               in front of the data change nothing), every later one full.
 *   finish      one tiny kernel: Y = S . H, and for GCM
 *               tag = ((Y ^ lenblock) . H) ^ E_K(J0).
 *
 * Multiplication by a constant C is 16 table lookups and no reduction:
 * T[p][b] = (byte b at byte position p, the rest zero) . C, 16 x 256 entries
 * of 16 B = 64 KiB per constant, one ds_read_b128 each.  A level needs two
 * constants (C^64 and C): 128 KiB of the CU's 160 KiB LDS, filled per
 * workgroup from a per-call global image that a prologue kernel builds from
 * the products C . x^i (successive doublings).  The constants themselves --
 * H^64, H^2048, ... by repeated squaring -- are computed on the host, which
 * knows H, and travel by value.
 *
 * The multiplication, the doubling, the table builder and the bit order they
 * keep are in ghash_dev.h, shared with aes_gcm_batch.hip; the end-aligned
 * levels and their workspace in otc_device.h, shared with chacha.hip.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "aes.h"
#include "ghash_dev.h"
#include "otc_device.h"
#include "otc_kernels.h"

namespace otc_impl {

using otc_dev::ld_u4;

namespace {

constexpr uint32_t GH_RUN = 32;                 /* blocks per lane in a wave span */
constexpr uint32_t GH_BATCH = 8;                /* passes loaded ahead */
constexpr uint32_t GH_SPAN = 64 * GH_RUN;       /* blocks of a wave span */
constexpr uint32_t GH_WAVES = 16;               /* wave spans of a workgroup */
constexpr uint32_t GH_ACC_STRIDE = 65;          /* accumulators of a wave, padded off one bank */
constexpr uint32_t GH_LDS = (2 * GF_TAB + GH_WAVES * GH_ACC_STRIDE) * 16;
constexpr int GH_MAX_LEVELS = 3;
static_assert(GH_RUN % GH_BATCH == 0, "a wave span is whole batches");
static_assert(GH_LDS <= 160 * 1024, "two tables and the accumulators must fit the CU's LDS");

struct GhLevel {
    const uint8_t *in;  /* nblocks blocks, 16-byte aligned; the last one may be short */
    uint64_t nbytes;
    uint64_t nblocks;   /* ceil(nbytes / 16), >= 1 */
    uint64_t nspans;    /* ceil(nblocks / GH_SPAN) */
    uint64_t pad;       /* nspans * GH_SPAN - nblocks zero blocks in front */
    const uint4 *tab;   /* [2][GF_TAB]: this level's C^64, then C */
    uint4 *out;         /* nspans partials */
    uint4 y0;           /* XORed into block 0 */
};

/* block i of the level's input; never reads at or past in + nbytes */
template <bool NT>
__device__ __forceinline__ uint4 gh_load(const GhLevel &P, uint64_t i)
{
    uint4 x;
    const uint64_t off = i * 16;
    if (off + 16 <= P.nbytes) {
        x = ld_u4<NT, true>(P.in + off);
    } else {
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint64_t b = off; b < P.nbytes; ++b) w[(b - off) >> 2] |= (uint32_t)P.in[b] << (8 * ((b - off) & 3));
        x = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return i == 0 ? xor4(x, P.y0) : x;
}

template <bool NT>
__global__ __launch_bounds__(64 * GH_WAVES) void k_ghash_level(GhLevel P)
{
    extern __shared__ __attribute__((aligned(16))) uint4 gh_lds[];
    uint4 *const T64 = gh_lds, *const T1 = gh_lds + GF_TAB, *const acc = gh_lds + 2 * GF_TAB;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    for (uint32_t i = tid; i < 2 * GF_TAB; i += 64 * GH_WAVES) gh_lds[i] = ld_u4<false, true>(P.tab + i);
    __syncthreads();
    const uint64_t ngroups = (P.nspans + GH_WAVES - 1) / GH_WAVES;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t s = g * GH_WAVES + wave;
        uint4 A = make_uint4(0, 0, 0, 0);
        if (s < P.nspans) {
            const uint64_t v0 = s * GH_SPAN; /* index among the zero-extended blocks */
            /* the first span skips the batches that are all padding */
            const uint32_t k0 = v0 < P.pad ? (uint32_t)((P.pad - v0) / 64) & ~(GH_BATCH - 1) : 0u;
            for (uint32_t kb = k0; kb < GH_RUN; kb += GH_BATCH) {
                uint4 X[GH_BATCH];
#pragma unroll
                for (uint32_t i = 0; i < GH_BATCH; ++i) {
                    const uint64_t v = v0 + (uint64_t)(kb + i) * 64 + lane;
                    X[i] = v >= P.pad ? gh_load<NT>(P, v - P.pad) : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (uint32_t i = 0; i < GH_BATCH; ++i) A = xor4(gh_mul(T64, A), X[i]);
            }
        }
        acc[wave * GH_ACC_STRIDE + lane] = A;
        __syncthreads();
        const uint64_t fs = g * GH_WAVES + lane; /* the span whose accumulators this lane folds */
        if (wave == 0 && lane < GH_WAVES && fs < P.nspans) {
            const uint4 *a = acc + lane * GH_ACC_STRIDE;
            uint4 Y = a[0];
            for (uint32_t j = 1; j < 64; ++j) Y = xor4(gh_mul(T1, Y), a[j]);
            P.out[fs] = Y;
        }
        __syncthreads();
    }
}

/* x . y by the bit loop (the finishing kernel only); memory-order words */
__device__ uint4 gh_mul_bits(uint4 xm, uint4 ym)
{
    const uint4 x = gh_swap(xm);
    uint4 v = gh_swap(ym), z = make_uint4(0, 0, 0, 0);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    for (int i = 0; i < 128; ++i) {
        if ((w[i >> 5] >> (31 - (i & 31))) & 1u) z = xor4(z, v);
        v = gh_mulx(v);
    }
    return gh_swap(z);
}

struct GhFinal {
    const uint4 *s;  /* the last level's one partial; null: no data, Y = y0 */
    uint4 y0, h, lenblock, ekj0;
    int tag;         /* 0: write Y (GHASH); 1: write ((Y ^ lenblock) . H) ^ ekj0 (the GCM tag) */
    uint32_t *out;   /* 16 bytes */
};

__global__ __launch_bounds__(64) void k_ghash_final(GhFinal F)
{
    uint4 y = F.s ? gh_mul_bits(*F.s, F.h) : F.y0;
    if (F.tag) y = xor4(gh_mul_bits(xor4(y, F.lenblock), F.h), F.ekj0);
    const uint32_t l = threadIdx.x;
    /* lanes 0..3 store one word each */
    if (l < 4) F.out[l] = l == 0 ? y.x : l == 1 ? y.y : l == 2 ? y.z : y.w;
}

uint4 u4_of(const uint8_t b[16])
{
    uint4 v;
    memcpy(&v, b, 16);
    return v;
}

/* the workspace: every level's two tables, then every level's partials */
constexpr otc_dev::HashShape GH_SHAPE{GH_SPAN, GH_BATCH, GH_WAVES, GH_MAX_LEVELS, 16, 2 * GF_TAB * 16};

hipError_t gh_launch_level(bool nt, const GhLevel &P, hipStream_t st)
{
    const hipError_t e = otc_dev::lds_opt_in<k_ghash_level<true>, k_ghash_level<false>>(GH_LDS);
    if (e != hipSuccess) return e;
    const uint64_t ngroups = (P.nspans + GH_WAVES - 1) / GH_WAVES, cus = (uint64_t)otc_dev::device_cus();
    const dim3 g((unsigned)(ngroups < cus ? ngroups : cus)), b(64 * GH_WAVES);
    if (nt)
        hipLaunchKernelGGL(k_ghash_level<true>, g, b, GH_LDS, st, P);
    else
        hipLaunchKernelGGL(k_ghash_level<false>, g, b, GH_LDS, st, P);
    return hipGetLastError();
}

} // namespace

int ghash_spans(uint64_t *spans, int max) { return otc_dev::hash_spans(GH_SHAPE, spans, max); }

bool ghash_fits(uint64_t nbytes)
{
    otc_dev::HashLevels pl;
    return otc_dev::hash_levels(GH_SHAPE, nbytes, pl);
}

hipError_t ghash_ws_alloc(uint64_t nbytes, hipStream_t st, void **ws) { return otc_dev::hash_ws_alloc(GH_SHAPE, nbytes, st, ws); }

hipError_t ghash_run(const void *data, uint64_t nbytes, const uint8_t h[16], const uint8_t y0[16],
                     const uint8_t *lenblock, const uint8_t *ekj0, void *out16, void *ws, hipStream_t st)
{
    otc_dev::HashLevels pl;
    if (!otc_dev::hash_levels(GH_SHAPE, nbytes, pl) || (pl.nlevels && !ws)) {
        if (ws) (void)otc_dev::ws_free(ws, st);
        return hipErrorInvalidValue;
    }
    GhFinal F{};
    F.s = nullptr;
    F.y0 = u4_of(y0);
    F.h = u4_of(h);
    F.tag = lenblock ? 1 : 0;
    if (lenblock) {
        F.lenblock = u4_of(lenblock);
        F.ekj0 = u4_of(ekj0);
    }
    F.out = (uint32_t *)out16;
    hipError_t e = hipSuccess;
    if (pl.nlevels) {
        /* level l multiplies by C_l = H^(GH_SPAN^l) and, across lanes, C_l^64 */
        GfConsts<2 * GH_MAX_LEVELS> K{}; /* per level: C^64, then C */
        uint8_t c[16], c64[16];
        memcpy(c, h, 16);
        for (int l = 0; l < pl.nlevels; ++l) {
            memcpy(c64, c, 16);
            for (int i = 0; i < 6; ++i) aes_gf128_mul(c64, c64, c64);
            K.c[2 * l] = u4_of(c64);
            K.c[2 * l + 1] = u4_of(c);
            memcpy(c, c64, 16); /* C^64, squared on to C^GH_SPAN */
            for (uint32_t p = 64; p < GH_SPAN; p *= 2) aes_gf128_mul(c, c, c);
        }
        uint4 *tab = (uint4 *)ws, *part = tab + (size_t)pl.nlevels * 2 * GF_TAB;
        hipLaunchKernelGGL(k_gf128_tables<2 * GH_MAX_LEVELS>, dim3((unsigned)pl.nlevels * 2 * 16), dim3(256), 0, st, K, tab);
        e = hipGetLastError();
        const uint8_t *in = (const uint8_t *)data;
        uint64_t in_bytes = nbytes;
        for (int l = 0; l < pl.nlevels && e == hipSuccess; ++l) {
            GhLevel P{};
            P.in = in;
            P.nbytes = in_bytes;
            P.nblocks = pl.nblocks[l];
            P.nspans = pl.nspans[l];
            P.pad = P.nspans * GH_SPAN - P.nblocks;
            P.tab = tab + (size_t)l * 2 * GF_TAB;
            P.out = part;
            P.y0 = l == 0 ? u4_of(y0) : make_uint4(0, 0, 0, 0);
            e = gh_launch_level(l == 0, P, st); /* the data streams once; partials are read back from L2 */
            in = (const uint8_t *)part;
            in_bytes = P.nspans * 16;
            F.s = part;
            part += P.nspans;
        }
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_ghash_final, dim3(1), dim3(64), 0, st, F);
        e = hipGetLastError();
    }
    if (ws) {
        const hipError_t f = otc_dev::ws_free(ws, st);
        if (e == hipSuccess) e = f;
    }
    return e;
}

} // namespace otc_impl
