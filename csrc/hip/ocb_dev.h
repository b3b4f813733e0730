/*
 * ocb_dev.h -- what the two OCB3 kernel files (aes_ocb.hip, aes_ocb_batch.hip)
 * share, in two parts.
 *
 * The first part is plain C, callable on the host and on the device: the closed
 * forms of the offsets.  csrc/cpu/ocb_batch_selftest.c includes this file for
 * them and runs the batched kernels' decomposition against aes.c.  A block, an
 * offset and an L_j are four little-endian words as loaded; XOR does not care
 * about byte order, so only Offset_0's stretch-and-shift swaps bytes.
 *
 *   Offset_i = Offset_0 ^ XOR{ L_j : bit j of i ^ (i >> 1) }      (1-based i)
 *
 * The second part is device code: the forward cipher on the constant tables in
 * global memory (include aes_tt_dev.h first: g_tab is that file's).
 */
#ifndef OTC_OCB_DEV_H
#define OTC_OCB_DEV_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define OCB_HD __host__ __device__ __forceinline__
#else
#define OCB_HD static inline
#endif

OCB_HD uint32_t ocb_gray(uint32_t i) { return i ^ (i >> 1); }

/* o ^= XOR{ L_j : bit j of g }: one table entry per set bit */
OCB_HD void ocb_xor_gray(uint32_t o[4], const uint32_t (*l)[4], uint32_t g)
{
    for (; g; g &= g - 1) {
        const int q = __builtin_ctz(g);
        for (int j = 0; j < 4; ++j) o[j] ^= l[q][j];
    }
}

/* Offset_i from Offset_0 (i <= 2^16 needs L_0 .. L_16): a slot's start S with
 * i = W, the finisher's Offset_m with i = the record's whole blocks */
OCB_HD void ocb_offset_at(uint32_t out[4], const uint32_t off0[4], const uint32_t (*l)[4], uint32_t i)
{
    for (int j = 0; j < 4; ++j) out[j] = off0[j];
    ocb_xor_gray(out, l, ocb_gray(i));
}

/* low = XOR{ L_q : bit q of gl }, q <= 5: the part of an offset that depends on
 * the lane alone, computed once per lane.  Lane v - 1 (v = 1 .. 63) of a run of
 * 64 blocks from W (a multiple of 64) holds index W + v with offset
 * S ^ low(gray(v)). */
OCB_HD void ocb_low(uint32_t low[4], const uint32_t (*l)[4], uint32_t gl)
{
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) low[j] ^= (gl >> q) & 1u ? l[q][j] : 0u;
}

/* The batched kernel's lane mask: gray(v) below bit 6.  v = 64 (lane 63, index
 * W + 64) gives L_5 alone: Offset_{W+64} = Offset_{W+63} ^ L_ntz(W+64) and
 * Offset_{W+63} = S ^ L_5, so lane 63 adds L_ocb_carry_ntz(W) to S ^ low. */
OCB_HD uint32_t ocb_lane_mask(uint32_t v) { return ocb_gray(v) & 63u; }
OCB_HD int ocb_carry_ntz(uint32_t W) { return __builtin_ctz(W + 64u); } /* 6 .. 16 for W < 2^16 */

/* The nonce block of a 12-byte nonce (three words as loaded) with TAGLEN 128:
 * 0^7 || 0^24 || 1 || N with the last six bits cleared; returns those bits */
OCB_HD uint32_t ocb_nonce_block12(uint32_t nb[4], const uint32_t n[3])
{
    nb[0] = 0x01000000u; /* byte 3 = 1: (128 mod 128) << 1 is zero */
    nb[1] = n[0];
    nb[2] = n[1];
    nb[3] = n[2] & 0xC0FFFFFFu;
    return (n[2] >> 24) & 63u;
}

/* Offset_0 = (Stretch << bottom)[0 .. 127], Stretch = Ktop || (Ktop[0..63] ^ Ktop[8..71]) */
OCB_HD void ocb_offset0_from_ktop(uint32_t out[4], const uint32_t kt[4], uint32_t bottom)
{
    const uint64_t hi = (uint64_t)__builtin_bswap32(kt[0]) << 32 | __builtin_bswap32(kt[1]);
    const uint64_t lo = (uint64_t)__builtin_bswap32(kt[2]) << 32 | __builtin_bswap32(kt[3]);
    const uint64_t ext = hi ^ (hi << 8 | lo >> 56);
    const uint64_t oh = bottom ? hi << bottom | lo >> (64 - bottom) : hi;
    const uint64_t ol = bottom ? lo << bottom | ext >> (64 - bottom) : lo;
    out[0] = __builtin_bswap32((uint32_t)(oh >> 32));
    out[1] = __builtin_bswap32((uint32_t)oh);
    out[2] = __builtin_bswap32((uint32_t)(ol >> 32));
    out[3] = __builtin_bswap32((uint32_t)ol);
}

#if defined(__HIPCC__)

namespace {

using namespace otc_dev;

/* The forward cipher of one block on the constant tables in global memory
 * (1.25 KiB, L1 resident), for the finisher's two blocks */
template <int NR>
__device__ __forceinline__ void enc_block_global(const otc_aes_key &K, uint32_t (&s)[4])
{
    const uint32_t *te = g_tab.te0;
    const uint8_t *sb = g_tab.sb;
    uint32_t t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] ^= K.rk[j];
#pragma unroll
    for (int r = 1; r < NR; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            t[j] = te[s[j] & 0xFFu] ^ rotl8(te[(s[(j + 1) & 3] >> 8) & 0xFFu]) ^
                   rotl16(te[(s[(j + 2) & 3] >> 16) & 0xFFu]) ^ rotl24(te[s[(j + 3) & 3] >> 24]) ^ K.rk[4 * r + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = t[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        t[j] = ((uint32_t)sb[s[j] & 0xFFu] | (uint32_t)sb[(s[(j + 1) & 3] >> 8) & 0xFFu] << 8 |
                (uint32_t)sb[(s[(j + 2) & 3] >> 16) & 0xFFu] << 16 | (uint32_t)sb[s[(j + 3) & 3] >> 24] << 24) ^
               K.rk[4 * NR + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = t[j];
}

/* 16 host bytes as the four words the kernels take by value */
inline void words(uint32_t (&w)[4], const uint8_t b[16]) { memcpy(w, b, 16); }

} // namespace

#endif /* __HIPCC__ */

#endif
