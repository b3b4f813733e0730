/*
 * polyval_dev.h -- POLYVAL's field arithmetic (RFC 8452) as the device code of
 * aes_gcm_siv.hip uses it, in plain C callable on the host and on the device:
 * csrc/cpu/gcmsiv_selftest.c includes this file and runs the kernels'
 * decomposition with it against aes.c.
 *
 * A block is four little-endian words as loaded, which IS POLYVAL's order:
 * bit k of word j is the coefficient of x^(32 j + k).  "Times x" is a one-bit
 * left shift of the 128-bit number; a bit shifted out of the top is folded
 * back as x^127 + x^126 + x^121 + 1.  The hash's product is
 * dot(a, b) = a . b . x^-128, so everything here starts from a constant's
 * SEED, dot(C, 1) = C . x^-128 (the host computes it: aes.h aes_polyval_dot),
 * and reaches dot(x^i, C) by i doublings -- no division on the device.
 */
#ifndef OTC_POLYVAL_DEV_H
#define OTC_POLYVAL_DEV_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PV_HD __host__ __device__ __forceinline__
#else
#define PV_HD static inline
#endif

/* v . x */
PV_HD void pv_mulx(uint32_t v[4])
{
    const uint32_t carry = v[3] >> 31;
    v[3] = v[3] << 1 | v[2] >> 31;
    v[2] = v[2] << 1 | v[1] >> 31;
    v[1] = v[1] << 1 | v[0] >> 31;
    v[0] = v[0] << 1;
    if (carry) {
        v[3] ^= 0xC2000000u;
        v[0] ^= 1u;
    }
}

/* e = dot(byte b at byte position pos, C): entry [pos][b] of C's positional
 * table (ghash_dev.h gh_mul reads it).  The byte's LOWEST bit is the lowest power. */
PV_HD void pv_table_entry(uint32_t e[4], const uint32_t seed[4], uint32_t pos, uint32_t b)
{
    uint32_t v[4] = {seed[0], seed[1], seed[2], seed[3]};
    for (uint32_t i = 0; i < 8 * pos; ++i) pv_mulx(v);
    e[0] = e[1] = e[2] = e[3] = 0;
    for (uint32_t k = 0; k < 8; ++k) {
        if ((b >> k) & 1u)
            for (int j = 0; j < 4; ++j) e[j] ^= v[j];
        pv_mulx(v);
    }
}

/* z = dot(x, C) by the bit loop (the finishing kernel only) */
PV_HD void pv_dot(uint32_t z[4], const uint32_t x[4], const uint32_t seed[4])
{
    uint32_t v[4] = {seed[0], seed[1], seed[2], seed[3]};
    z[0] = z[1] = z[2] = z[3] = 0;
    for (int i = 0; i < 128; ++i) {
        if ((x[i >> 5] >> (i & 31)) & 1u)
            for (int j = 0; j < 4; ++j) z[j] ^= v[j];
        pv_mulx(v);
    }
}

/* GCM-SIV's counter block for block i of a message whose tag is t: word 0
 * counts modulo 2^32, words 1..2 stay, word 3 stays with its top bit forced on */
PV_HD void siv_ctr_block(uint32_t c[4], const uint32_t t[4], uint32_t i)
{
    c[0] = t[0] + i;
    c[1] = t[1];
    c[2] = t[2];
    c[3] = t[3] | 0x80000000u;
}

#endif
