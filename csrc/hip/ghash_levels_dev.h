/*
 * ghash_levels_dev.h -- the chip-wide level kernel of the two GF(2^128) hashes
 * and its host driver, in one copy: GHASH (aes_gcm.hip) and POLYVAL
 * (aes_gcm_siv.hip) both run it.  The kernel only multiplies by positional
 * tables (ghash_dev.h gh_mul) and XORs, so whose field and bit order the
 * tables are in is nothing to it; what differs between the hashes -- the
 * table builder, the host product behind the constants, the finisher -- stays
 * with each.  The decomposition: aes_gcm.hip's header.  A header of its own
 * because the batched GHASH (aes_gcm_batch.hip) shares ghash_dev.h and has no
 * levels: included there, the launcher would instantiate these kernels into
 * its code object.  Everything is file-local (an unnamed namespace).
 */
#ifndef OTC_GHASH_LEVELS_DEV_H
#define OTC_GHASH_LEVELS_DEV_H

#include <hip/hip_runtime.h>

#include <cstring>

#include "ghash_dev.h"
#include "otc_device.h"

namespace otc_impl {
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
        x = otc_dev::ld_u4<NT, true>(P.in + off);
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
    for (uint32_t i = tid; i < 2 * GF_TAB; i += 64 * GH_WAVES) gh_lds[i] = otc_dev::ld_u4<false, true>(P.tab + i);
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

inline uint4 u4_of(const uint8_t b[16])
{
    uint4 v;
    memcpy(&v, b, 16);
    return v;
}

/* the workspace: every level's two tables, then every level's partials */
constexpr otc_dev::HashShape GH_SHAPE{GH_SPAN, GH_BATCH, GH_WAVES, GH_MAX_LEVELS, 16, 2 * GF_TAB * 16};

inline hipError_t gh_launch_level(bool nt, const GhLevel &P, hipStream_t st)
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

/* Per level the constants C^64, then C: level l multiplies by C_l =
 * H^(GH_SPAN^l) and, across lanes, C_l^64.  mul(z, x, y) is the hash's product
 * on the host (z may be x and y). */
template <class Mul>
inline void gh_level_consts(uint8_t (*k)[16], int nlevels, const uint8_t h[16], Mul mul)
{
    uint8_t c[16], c64[16];
    memcpy(c, h, 16);
    for (int l = 0; l < nlevels; ++l) {
        memcpy(c64, c, 16);
        for (int i = 0; i < 6; ++i) mul(c64, c64, c64);
        memcpy(k[2 * l], c64, 16);
        memcpy(k[2 * l + 1], c, 16);
        memcpy(c, c64, 16); /* C^64, squared on to C^GH_SPAN */
        for (uint32_t p = 64; p < GH_SPAN; p *= 2) mul(c, c, c);
    }
}

/* the levels of pl over the data, their tables already queued into tab; the
 * partials follow the tables in the workspace.  *s: the last level's one partial */
inline hipError_t gh_run_levels(const otc_dev::HashLevels &pl, const void *data, uint64_t nbytes, uint4 y0, uint4 *tab,
                                hipStream_t st, const uint4 **s)
{
    uint4 *part = tab + (size_t)pl.nlevels * 2 * GF_TAB;
    const uint8_t *in = (const uint8_t *)data;
    uint64_t in_bytes = nbytes;
    hipError_t e = hipSuccess;
    for (int l = 0; l < pl.nlevels && e == hipSuccess; ++l) {
        GhLevel P{};
        P.in = in;
        P.nbytes = in_bytes;
        P.nblocks = pl.nblocks[l];
        P.nspans = pl.nspans[l];
        P.pad = P.nspans * GH_SPAN - P.nblocks;
        P.tab = tab + (size_t)l * 2 * GF_TAB;
        P.out = part;
        P.y0 = l == 0 ? y0 : make_uint4(0, 0, 0, 0);
        e = gh_launch_level(l == 0, P, st); /* the data streams once; partials are read back from L2 */
        in = (const uint8_t *)part;
        in_bytes = P.nspans * 16;
        *s = part;
        part += P.nspans;
    }
    return e;
}

} // namespace
} // namespace otc_impl

#endif
