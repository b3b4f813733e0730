/*
 * polyval_dev.h -- POLYVAL's field arithmetic (RFC 8452) as the device code of
 * aes_gcm_siv.hip, aes_gcm_siv_batch.hip and aes_gcm_mk_batch.hip (GHASH through
 * POLYVAL) uses it, in plain C callable on the host and on the device:
 * csrc/cpu/gcmsiv_selftest.c, csrc/cpu/gcmsiv_batch_selftest.c and
 * csrc/cpu/gcm_mk_batch_selftest.c include this file and run the kernels'
 * decompositions with it against aes.c.
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

/* ---- what the batched kernels add (aes_gcm_siv_batch.hip) --------------------
 * A hash key per record rules the positional byte tables out (64 KiB per
 * constant).  dot(a, C) = a . C . x^-128 needs no seed when it is taken as a
 * Horner rule over a's 32 nibbles n_k, LOWEST first, that divides by x^4 at
 * every step:  z = (z ^ n_k(x) . C) . x^-4,  k = 0 .. 31  -- n_0 is divided
 * 32 times (x^-128), n_31 once (x^(124 - 128)).  The 16 products n(x) . C are
 * the record's NIBBLE TABLE of C, 256 bytes.  Dividing is the clean direction
 * in this field: x^-1 = x^127 + x^126 + x^125 + x^120 (aes.c aes_polyval_dot),
 * so the four bits o that a right shift by 4 drops come back as
 * clmul(o, 0xE1) << 117, which lies in word 3 alone (written as shifts of the
 * nibble: as o . constant hipcc made it a quarter-rate v_mul_lo_u32 per step). */

/* e = n(x) . C, n < 16: entry n of C's nibble table.  The nibble's lowest bit is the lowest power. */
PV_HD void pv4_entry(uint32_t e[4], const uint32_t c[4], uint32_t n)
{
    uint32_t v[4] = {c[0], c[1], c[2], c[3]};
    e[0] = e[1] = e[2] = e[3] = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t on = 0u - ((n >> k) & 1u);
        for (int j = 0; j < 4; ++j) e[j] ^= v[j] & on;
        pv_mulx(v);
    }
}

/* nibble k (0 .. 31) of a */
PV_HD uint32_t pv4_nibble(const uint32_t a[4], int k) { return (a[k >> 3] >> (4 * (k & 7))) & 15u; }

/* one Horner step: z = (z ^ t) . x^-4, t the table entry of the step's nibble */
PV_HD void pv4_step(uint32_t z[4], const uint32_t t[4])
{
    const uint32_t w0 = z[0] ^ t[0], w1 = z[1] ^ t[1], w2 = z[2] ^ t[2], w3 = z[3] ^ t[3];
    const uint32_t o = w0 << 28; /* the dropped nibble at bits 28 .. 31: o . 0xE1 << 21 in shifts alone */
    z[0] = w0 >> 4 | w1 << 28;
    z[1] = w1 >> 4 | w2 << 28;
    z[2] = w2 >> 4 | w3 << 28;
    z[3] = (w3 >> 4) ^ o ^ (o >> 1) ^ (o >> 2) ^ (o >> 7);
}

/* z = dot(a, C) over C's nibble table (the host's form; the kernel reads the entries as uint4 from LDS) */
PV_HD void pv4_dot(uint32_t z[4], const uint32_t a[4], const uint32_t (*tab)[4])
{
    uint32_t r[4] = {0, 0, 0, 0};
    for (int k = 0; k < 32; ++k) pv4_step(r, tab[pv4_nibble(a, k)]);
    for (int j = 0; j < 4; ++j) z[j] = r[j];
}

/* ---- what the many-key batched GCM adds (aes_gcm_mk_batch.hip) ------------------
 * RFC 8452 appendix A: GHASH(H, X_1 .. X_n) = ByteReverse(POLYVAL(mulX_POLYVAL(
 * ByteReverse(H)), ByteReverse(X_1), .., ByteReverse(X_n))).  So GHASH under a key
 * per record runs on the nibble tables above: the hash key enters as gmk_key,
 * every block enters through pv_rev, and the result leaves through pv_rev. */
#define GMK_NTAB 7 /* a key's table image: the nibble tables of C^(2^s), s = 0 .. 6, 256 bytes each */

PV_HD uint32_t pv_bswap32(uint32_t w) { return w >> 24 | (w >> 8 & 0xFF00u) | (w << 8 & 0xFF0000u) | w << 24; }

/* r = the 16 bytes of x in reverse order (r and x may be the same array) */
PV_HD void pv_rev(uint32_t r[4], const uint32_t x[4])
{
    const uint32_t a = pv_bswap32(x[3]), b = pv_bswap32(x[2]), c = pv_bswap32(x[1]), d = pv_bswap32(x[0]);
    r[0] = a;
    r[1] = b;
    r[2] = c;
    r[3] = d;
}

/* the POLYVAL key that stands for the GHASH key h = E_K(0^128) (four words as loaded) */
PV_HD void gmk_key(uint32_t c[4], const uint32_t h[4])
{
    pv_rev(c, h);
    pv_mulx(c);
}

/* GCM's length block [8 aad]_64 [8 n]_64, big-endian, already byte-reversed */
PV_HD void gmk_len_block(uint32_t x[4], uint64_t aad_bytes, uint64_t nbytes)
{
    const uint64_t ab = aad_bytes * 8, db = nbytes * 8;
    x[0] = (uint32_t)db;
    x[1] = (uint32_t)(db >> 32);
    x[2] = (uint32_t)ab;
    x[3] = (uint32_t)(ab >> 32);
}

/* RFC 8452 section 4: derivation block i of a nonce (three words as loaded) is le32(i) || nonce */
PV_HD void siv_derive_block(uint32_t b[4], const uint32_t n[3], uint32_t i)
{
    b[0] = i;
    b[1] = n[0];
    b[2] = n[1];
    b[3] = n[2];
}

PV_HD uint32_t siv_subword(uint32_t w, const uint8_t *sb)
{
    return (uint32_t)sb[w & 0xFFu] | (uint32_t)sb[(w >> 8) & 0xFFu] << 8 | (uint32_t)sb[(w >> 16) & 0xFFu] << 16 |
           (uint32_t)sb[w >> 24] << 24;
}

/* FIPS-197 key expansion in otc_aes_key's convention (round key words as
 * loaded little-endian, aes.c's): rk[0 .. nk) hold the key, nk = 4 or 8; fills
 * rk[nk .. 4 (nk + 7)).  sb: the S-box.  The kernel calls it with a constant nk
 * and the loop unrolls: the schedule stays in registers. */
PV_HD void siv_expand_key(uint32_t *rk, const uint8_t *sb, const int nk)
{
    uint32_t rcon = 1;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = nk; i < 4 * (nk + 7); ++i) {
        uint32_t t = rk[i - 1];
        if (i % nk == 0) {
            t = siv_subword(t >> 8 | t << 24, sb) ^ rcon;
            rcon = (rcon << 1) ^ ((rcon & 0x80u) ? 0x11Bu : 0u);
        } else if (nk == 8 && i % 8 == 4) {
            t = siv_subword(t, sb);
        }
        rk[i] = rk[i - nk] ^ t;
    }
}

#endif
