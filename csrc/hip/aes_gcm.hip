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
 * keep are in ghash_dev.h, shared with aes_gcm_batch.hip; the level kernel and
 * its driver in ghash_levels_dev.h, which POLYVAL (aes_gcm_siv.hip) runs over
 * tables of its own; the end-aligned levels and their workspace are in otc_device.h,
 * shared with chacha.hip.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "aes.h"
#include "ghash_levels_dev.h"
#include "otc_device.h"
#include "otc_kernels.h"

namespace otc_impl {

namespace {

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
        GfConsts<2 * GH_MAX_LEVELS> K{}; /* per level: C^64, then C */
        uint8_t k[2 * GH_MAX_LEVELS][16];
        gh_level_consts(k, pl.nlevels, h, aes_gf128_mul);
        for (int i = 0; i < 2 * pl.nlevels; ++i) K.c[i] = u4_of(k[i]);
        uint4 *tab = (uint4 *)ws;
        hipLaunchKernelGGL(k_gf128_tables<2 * GH_MAX_LEVELS>, dim3((unsigned)pl.nlevels * 2 * 16), dim3(256), 0, st, K, tab);
        e = hipGetLastError();
        if (e == hipSuccess) e = gh_run_levels(pl, data, nbytes, u4_of(y0), tab, st, &F.s);
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
