/*
 * ccm_dev.h -- everything of the batched AES-CCM kernel (aes_ccm_batch.hip) that
 * is not the cipher call, in plain C, callable on the host and on the device:
 * the blocks B0 and A_i as words, the j-th MAC block of the encoded AAD from any
 * alignment, the mask of the last partial block, the lane's bursts and the
 * planner's order.  csrc/cpu/ccm_batch_selftest.c includes this file and replays
 * the lane's decomposition with it against aes.c.
 *
 * A block is four little-endian words as loaded: byte i of the block is byte
 * i & 3 of word i >> 2.  SP 800-38C appendix A (the same as RFC 3610):
 *
 *   B0  = flags || N || [len]_L,  flags = 64 (aad_len > 0) + 8 ((M - 2) / 2) + (L - 1)
 *   A_i = (L - 1) || N || [i]_L
 *
 * with L = 15 - nonce_len.  Both fields are big-endian in the block's last L
 * bytes.  A record has at most 2^20 bytes here and the planner refuses a length
 * of 2^(8 L) or more, so len and every i fit both the field and 32 bits: the
 * field is the byte-swapped value ORed into word 3 (and the low bytes of word 2
 * stay zero), and a carry across the field's bytes is the swap's.
 */
#ifndef OTC_CCM_DEV_H
#define OTC_CCM_DEV_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CCM_HD __host__ __device__ __forceinline__
#else
#define CCM_HD static inline
#endif

#define CCM_BURST 8u /* blocks a lane loads, and stores, back to back */

CCM_HD uint32_t ccm_flags_b0(int has_aad, uint32_t tag_len, uint32_t nonce_len)
{
    return (has_aad ? 64u : 0u) + 8u * ((tag_len - 2u) / 2u) + (14u - nonce_len);
}
CCM_HD uint32_t ccm_flags_ctr(uint32_t nonce_len) { return 14u - nonce_len; }

/* 0 || N || 0^L from the nonce's bytes as four words n (bytes past nonce_len
 * zero): the nonce moves up by one byte */
CCM_HD void ccm_base(uint32_t base[4], const uint32_t n[4])
{
    base[0] = n[0] << 8;
    for (int j = 1; j < 4; ++j) base[j] = n[j] << 8 | n[j - 1] >> 24;
}

/* flags || N || [v]_L from the base block */
CCM_HD void ccm_block(uint32_t b[4], const uint32_t base[4], uint32_t flags, uint32_t v)
{
    b[0] = base[0] | flags;
    b[1] = base[1];
    b[2] = base[2];
    b[3] = base[3] | __builtin_bswap32(v);
}

/* bytes of the AAD length's encoding in front of the AAD: 2 below 0xFF00, FF FE
 * and four bytes from there up; no AAD, no encoding */
CCM_HD uint32_t ccm_aad_hdr(uint32_t aad_len) { return aad_len == 0 ? 0u : aad_len < 0xFF00u ? 2u : 6u; }
/* MAC blocks of the encoded AAD, zero-padded */
CCM_HD uint32_t ccm_aad_blocks(uint32_t aad_len) { return (ccm_aad_hdr(aad_len) + aad_len + 15u) >> 4; }

/* byte p (< hdr) of the length's encoding */
CCM_HD uint32_t ccm_aad_hdr_byte(uint32_t aad_len, uint32_t hdr, uint32_t p)
{
    if (hdr == 2u) return (aad_len >> (8u * (1u - p))) & 0xFFu;
    return p == 0 ? 0xFFu : p == 1 ? 0xFEu : (aad_len >> (8u * (5u - p))) & 0xFFu;
}

/* MAC block j (< ccm_aad_blocks) of the encoded AAD: the encoding's bytes, the
 * AAD's, then zeros; reads aad[0 .. aad_len) only, by bytes, at any alignment */
CCM_HD void ccm_aad_block(uint32_t w[4], const uint8_t *aad, uint32_t aad_len, uint32_t j)
{
    const uint32_t hdr = ccm_aad_hdr(aad_len);
    for (int q = 0; q < 4; ++q) w[q] = 0;
    for (uint32_t t = 0; t < 16; ++t) {
        const uint32_t p = 16u * j + t; /* < 2^16 + 22 */
        uint32_t v = 0;
        if (p < hdr) v = ccm_aad_hdr_byte(aad_len, hdr, p);
        else if (p - hdr < aad_len) v = aad[p - hdr];
        w[t >> 2] |= v << (8u * (t & 3u));
    }
}

/* the words' mask of a block's first r bytes (r = 1 .. 16) */
CCM_HD uint32_t ccm_mask_word(uint32_t r, int q)
{
    const uint32_t k = r > 4u * (uint32_t)q ? r - 4u * (uint32_t)q : 0u;
    return k >= 4u ? 0xFFFFFFFFu : (1u << (8u * k)) - 1u;
}

/* cipher steps of a record's data: its blocks, the last partial one counted */
CCM_HD uint32_t ccm_data_blocks(uint64_t nbytes) { return (uint32_t)((nbytes + 15u) >> 4); }

/* The counter of the SECOND cipher call of data step j (0-based) of n steps.
 * Encryption: A_{j+1}, whose output S_{j+1} makes C_j in the same step.
 * Decryption runs one block ahead -- the MAC takes the plaintext C_j ^ S_{j+1},
 * so S_{j+1} comes from the step before (S_1 from the MAC's first step) -- and
 * step j makes S_{j+2}; the last step has no block to prepare and makes S_0, the
 * tag's pad.  The same with j = -1 for the call beside B0: ccm_ctr_first. */
CCM_HD uint32_t ccm_ctr_of_step(int dec, uint32_t j, uint32_t n) { return !dec ? j + 1u : j + 1u < n ? j + 2u : 0u; }
CCM_HD uint32_t ccm_ctr_first(int dec, uint32_t n) { return dec && n ? 1u : 0u; }

/* ---- host only: the planner's order ------------------------------------------
 * Lane t takes record order[t].  The records of a wave run in lock step for as
 * long as the longest of them, so the planner sorts them by their data's block
 * count, longest first (records of one count keep their order: a counting sort).
 * nbytes: the first record's length, `stride` 64-bit words from one record's to
 * the next; every length is at most 2^20.  Returns 0, or -1 without memory. */
#include <stdlib.h>
static inline int ccm_order_fill(uint32_t *order, const uint64_t *nbytes, size_t stride, size_t n)
{
    const size_t nb = (1u << 16) + 2u;
    size_t *at = (size_t *)calloc(nb, sizeof *at);
    if (!at) return -1;
    for (size_t m = 0; m < n; ++m) ++at[65536u - ccm_data_blocks(nbytes[m * stride]) + 1u];
    for (size_t b = 1; b < nb; ++b) at[b] += at[b - 1]; /* at[k]: where the records of 65536 - k blocks start */
    for (size_t m = 0; m < n; ++m) order[at[65536u - ccm_data_blocks(nbytes[m * stride])]++] = (uint32_t)m;
    free(at);
    return 0;
}

#endif
