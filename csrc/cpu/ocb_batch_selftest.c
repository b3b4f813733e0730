/*
 * ocb_batch_selftest.c -- the batched OCB3 kernels' decomposition
 * (csrc/hip/aes_ocb_batch.hip) on the host, with the kernels' own closed forms
 * (csrc/hip/ocb_dev.h), against aes_crypt_ocb of aes.c:
 *
 *   prep      Offset_0 from a 12-byte nonce's block, Ktop and the stretch;
 *             HASH(K, A) by 16 lanes that stride over the AAD's blocks, block i
 *             under XOR{ L_j : bit j of i ^ (i >> 1) }
 *   bulk      tile k of 64 blocks from W = 64 k: the slot start S, lane v - 1
 *             under S ^ low(v), lane 63 under S ^ L_5 ^ L_ntz(W + 64); the
 *             checksum slot by slot; both directions
 *   finish    Offset_m by the closed form, the trailing bytes, the tag
 *
 * for every record length 0 .. 4200 bytes, at 65535 / 65536 blocks around the
 * cap (1 MiB - 16, 1 MiB - 1, 1 MiB: the last reaches index 2^16 and L_16) and
 * for all three key sizes.  Prints one line per key size; exits non-zero on
 * the first mismatch.  tests/test_ocb_batch_cpu.py builds it plain and with
 * -fsanitize=address,undefined.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aes.h"
#include "ocb_dev.h"

#define MAX_BYTES (1u << 20)

typedef struct {
    aes_context enc, dec;
    uint32_t l[17][4], l_star[4], l_dollar[4];
} host_key;

/* a block as the kernels hold it: four words as loaded (the host is little-endian like the device) */
static void enc_words(host_key *k, uint32_t w[4])
{
    unsigned char b[16];
    memcpy(b, w, 16);
    aes_crypt_ecb(&k->enc, AES_ENCRYPT, b, b);
    memcpy(w, b, 16);
}

static void dec_words(host_key *k, uint32_t w[4])
{
    unsigned char b[16];
    memcpy(b, w, 16);
    aes_crypt_ecb(&k->dec, AES_DECRYPT, b, b);
    memcpy(w, b, 16);
}

/* the 16 bytes at p + off as four words, those at or past end as zero */
static void bytes_words(uint32_t w[4], const unsigned char *p, size_t off, size_t end)
{
    unsigned char b[16] = {0};
    if (off < end) memcpy(b, p + off, end - off < 16 ? end - off : 16);
    memcpy(w, b, 16);
}

/* prep's first half */
static void prep_offset0(host_key *k, const unsigned char nonce[12], uint32_t off0[4])
{
    uint32_t n[3], nb[4];
    memcpy(n, nonce, 12);
    const uint32_t bottom = ocb_nonce_block12(nb, n);
    enc_words(k, nb); /* Ktop */
    ocb_offset0_from_ktop(off0, nb, bottom);
}

/* prep's second half: 16 lanes stride over the blocks, then the fold */
static void prep_hash(host_key *k, const unsigned char *aad, size_t abytes, uint32_t hash[4])
{
    const size_t nfull = abytes / 16;
    uint32_t sum[16][4];
    memset(sum, 0, sizeof sum);
    for (unsigned j = 0; j < 16; ++j) {
        for (size_t i = j; i < nfull; i += 16) {
            uint32_t x[4], o[4] = {0, 0, 0, 0};
            bytes_words(x, aad, i * 16, abytes);
            ocb_xor_gray(o, (const uint32_t(*)[4])k->l, ocb_gray((uint32_t)i + 1u));
            for (int q = 0; q < 4; ++q) x[q] ^= o[q];
            enc_words(k, x);
            for (int q = 0; q < 4; ++q) sum[j][q] ^= x[q];
        }
        if ((abytes & 15u) && j == (nfull & 15u)) {
            uint32_t x[4], o[4];
            const uint32_t r = (uint32_t)abytes & 15u;
            bytes_words(x, aad, nfull * 16, abytes);
            x[r >> 2] |= 0x80u << (8 * (r & 3u));
            for (int q = 0; q < 4; ++q) o[q] = k->l_star[q];
            ocb_xor_gray(o, (const uint32_t(*)[4])k->l, ocb_gray((uint32_t)nfull));
            for (int q = 0; q < 4; ++q) x[q] ^= o[q];
            enc_words(k, x);
            for (int q = 0; q < 4; ++q) sum[j][q] ^= x[q];
        }
    }
    for (unsigned d = 8; d; d >>= 1)
        for (unsigned j = 0; j < 16; ++j)
            if (!(j & d))
                for (int q = 0; q < 4; ++q) sum[j][q] ^= sum[j ^ d][q];
    memcpy(hash, sum[0], 16);
}

/* the bulk kernel's tiles over the whole blocks of in -> out; the plaintexts' XOR into cs */
static void bulk(host_key *k, int dec, const uint32_t off0[4], const unsigned char *in, unsigned char *out, size_t nblk,
                 uint32_t cs[4])
{
    const uint32_t(*l)[4] = (const uint32_t(*)[4])k->l;
    for (uint32_t W = 0; W < nblk; W += 64) { /* tile W / 64 */
        uint32_t S[4];
        ocb_offset_at(S, off0, l, W);
        const int z = ocb_carry_ntz(W);
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const size_t a = (size_t)W + lane;
            if (a >= nblk) continue; /* lanes past the record's whole blocks do nothing */
            uint32_t low[4] = {0, 0, 0, 0}, T[4], s[4], v[4];
            ocb_low(low, l, ocb_lane_mask(lane + 1u));
            for (int j = 0; j < 4; ++j) T[j] = low[j] ^ S[j] ^ (lane == 63u ? l[z][j] : 0u);
            memcpy(v, in + 16 * a, 16);
            for (int j = 0; j < 4; ++j) s[j] = v[j] ^ T[j];
            if (dec) dec_words(k, s);
            else enc_words(k, s);
            for (int j = 0; j < 4; ++j) s[j] ^= T[j];
            memcpy(out + 16 * a, s, 16);
            for (int j = 0; j < 4; ++j) cs[j] ^= dec ? s[j] : v[j];
        }
    }
}

/* the finisher: the trailing bytes and the tag */
static void finish(host_key *k, int dec, const uint32_t off0[4], const unsigned char *in, unsigned char *out, size_t nbytes,
                   uint32_t cs[4], const uint32_t hash[4], unsigned char tag[16])
{
    const uint32_t nblk = (uint32_t)(nbytes / 16), r = (uint32_t)nbytes & 15u;
    uint32_t off[4], t[4];
    ocb_offset_at(off, off0, (const uint32_t(*)[4])k->l, nblk);
    if (r) {
        uint32_t pad[4], x[4], y[4];
        unsigned char yb[16];
        for (int j = 0; j < 4; ++j) pad[j] = off[j] ^= k->l_star[j];
        enc_words(k, pad);
        bytes_words(x, in + 16 * (size_t)nblk, 0, r);
        for (int j = 0; j < 4; ++j) {
            const uint32_t n = r > 4u * j ? r - 4u * j : 0u;
            y[j] = (x[j] ^ pad[j]) & (n >= 4 ? 0xFFFFFFFFu : (1u << (8 * n)) - 1u);
        }
        memcpy(yb, y, 16);
        memcpy(out + 16 * (size_t)nblk, yb, r);
        for (int j = 0; j < 4; ++j) cs[j] ^= dec ? y[j] : x[j];
        cs[r >> 2] ^= 0x80u << (8 * (r & 3u));
    }
    for (int j = 0; j < 4; ++j) t[j] = cs[j] ^ off[j] ^ k->l_dollar[j];
    enc_words(k, t);
    for (int j = 0; j < 4; ++j) t[j] ^= hash[j];
    memcpy(tag, t, 16);
}

static unsigned char *g_p, *g_c, *g_d, *g_ref, *g_aad;

/* one record: both directions through the decomposition, against the oracle */
static int record(const aes_ocb_context *ctx, host_key *k, size_t n, size_t alen, unsigned seed)
{
    unsigned char nonce[12], tag[16], tag2[16], rtag[16], o0[16];
    for (int i = 0; i < 12; ++i) nonce[i] = (unsigned char)(seed * 29u + 7u * (unsigned)i + (unsigned)n);
    uint32_t off0[4], hash[4], cs[4] = {0, 0, 0, 0};
    prep_offset0(k, nonce, off0);
    if (aes_ocb_offset0(ctx, nonce, 12, 16, o0) || memcmp(o0, off0, 16)) return printf("FAIL Offset_0 n=%zu\n", n), 1;
    prep_hash(k, g_aad, alen, hash);
    aes_ocb_hash(ctx, g_aad, alen, o0);
    if (memcmp(o0, hash, 16)) return printf("FAIL HASH alen=%zu\n", alen), 1;
    if (aes_crypt_ocb(ctx, AES_ENCRYPT, n, nonce, 12, g_aad, alen, g_p, g_ref, rtag, 16)) return printf("FAIL oracle\n"), 1;
    bulk(k, 0, off0, g_p, g_c, n / 16, cs);
    finish(k, 0, off0, g_p, g_c, n, cs, hash, tag);
    if (memcmp(g_c, g_ref, n) || memcmp(tag, rtag, 16)) return printf("FAIL encrypt n=%zu alen=%zu\n", n, alen), 1;
    memset(cs, 0, sizeof cs);
    bulk(k, 1, off0, g_c, g_d, n / 16, cs);
    finish(k, 1, off0, g_c, g_d, n, cs, hash, tag2);
    if (memcmp(g_d, g_p, n) || memcmp(tag2, rtag, 16)) return printf("FAIL decrypt n=%zu alen=%zu\n", n, alen), 1;
    return 0;
}

int main(void)
{
    static const size_t edge[3] = {MAX_BYTES - 16, MAX_BYTES - 1, MAX_BYTES};
    static const size_t alens[8] = {0, 1, 15, 16, 17, 255, 4096, 65536};
    unsigned char key[32];
    g_p = malloc(MAX_BYTES), g_c = malloc(MAX_BYTES), g_d = malloc(MAX_BYTES), g_ref = malloc(MAX_BYTES);
    g_aad = malloc(65536);
    if (!g_p || !g_c || !g_d || !g_ref || !g_aad) return 2;
    uint32_t x = 0x9E3779B9u;
    for (size_t i = 0; i < MAX_BYTES; ++i) g_p[i] = (unsigned char)((x = x * 1664525u + 1013904223u) >> 24);
    for (size_t i = 0; i < 65536; ++i) g_aad[i] = (unsigned char)((x = x * 1664525u + 1013904223u) >> 24);
    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)(0xA0 + 3 * i);
    int bad = 0;
    for (int keybits = 128; keybits <= 256 && !bad; keybits += 64) {
        aes_ocb_context ctx;
        host_key k;
        if (aes_ocb_setkey(&ctx, key, (unsigned)keybits)) return printf("FAIL setkey\n"), 1;
        if (aes_setkey_enc(&k.enc, key, (unsigned)keybits) || aes_setkey_dec(&k.dec, key, (unsigned)keybits))
            return printf("FAIL setkey\n"), 1;
        memcpy(k.l, ctx.l, sizeof k.l); /* L_0 .. L_16 of the oracle's 33 */
        memcpy(k.l_star, ctx.l_star, 16);
        memcpy(k.l_dollar, ctx.l_dollar, 16);
        size_t nrec = 0;
        for (size_t n = 0; n <= 4200 && !bad; ++n, ++nrec) bad = record(&ctx, &k, n, n % 41, (unsigned)keybits);
        for (int e = 0; e < 3 && !bad; ++e, ++nrec) bad = record(&ctx, &k, edge[e], 13, (unsigned)keybits + (unsigned)e);
        for (int a = 0; a < 8 && !bad; ++a, ++nrec) bad = record(&ctx, &k, 100, alens[a], (unsigned)keybits + (unsigned)a);
        if (!bad) printf("OK AES-%d %zu records\n", keybits, nrec);
    }
    free(g_p), free(g_c), free(g_d), free(g_ref), free(g_aad);
    return bad;
}
