/*
 * gcmsiv_selftest.c -- the AES-GCM-SIV oracle (aes.c) as a stand-alone program:
 * RFC 8452's POLYVAL example, derivation and sealed vectors, the little-endian
 * counter across its wrap, an authenticated round trip with each kind of
 * tampering, and the decomposition the device uses (csrc/hip/polyval_dev.h,
 * csrc/hip/aes_gcm_siv.hip: positional byte tables from a constant's seed,
 * end-aligned wave spans, Horner under C^64 per lane and under C across the
 * lanes, level after level, the bit-loop finish) against aes_polyval.  Prints
 * every result; exits non-zero if a check fails.
 * tests/test_gcm_siv_selftest_cpu.py builds it with
 * -fsanitize=address,undefined and compares the output.
 *
 *   POLYVAL <result>
 *   DERIVE <auth key> <enc key>
 *   V <keybits> <alen> <plen> <ciphertext || tag>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aes.h"
#include "../hip/polyval_dev.h"

static int g_fail;

static void hex(const unsigned char *p, size_t n)
{
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

static void fail(const char *what)
{
    printf("FAIL %s\n", what);
    g_fail = 1;
}

static size_t unhex(const char *s, unsigned char *out)
{
    size_t n = 0;
    for (; s[0] && s[1]; s += 2) {
        unsigned v;
        sscanf(s, "%2x", &v);
        out[n++] = (unsigned char)v;
    }
    return n;
}

static void seal(const char *keyhex, const char *noncehex, const unsigned char *aad, size_t al, const unsigned char *pt,
                 size_t n)
{
    unsigned char key[32], nonce[12], out[80], back[80], tag[16];
    aes_context kgk;
    const size_t kl = unhex(keyhex, key);
    unhex(noncehex, nonce);
    if (aes_setkey_enc(&kgk, key, (unsigned)(kl * 8))) fail("setkey");
    if (aes_crypt_gcmsiv(&kgk, AES_ENCRYPT, n, nonce, aad, al, pt, out, NULL, tag)) fail("encrypt");
    printf("V %zu %zu %zu ", kl * 8, al, n);
    hex(out, n);
    hex(tag, 16);
    printf("\n");
    memset(back, 0xA5, sizeof back);
    if (aes_gcmsiv_auth_decrypt(&kgk, n, nonce, aad, al, tag, out, back) || (n && memcmp(back, pt, n))) fail("round trip");
}

static void vectors(void)
{
    static const char *K128 = "01000000000000000000000000000000";
    static const char *K256 = "0100000000000000000000000000000000000000000000000000000000000000";
    static const char *N3 = "030000000000000000000000", *NA = "a0a1a2a3a4a5a6a7a8a9aaab";
    static const unsigned char one[8] = {1}, two[8] = {2}, a1[1] = {1};
    unsigned char h[16], x[32], y[16] = {0}, key[16], nonce[12], ak[16], ek[32], aad[21], pt[49];
    aes_context kgk;

    unhex("25629347589242761d31f826ba4b757b", h);
    unhex("4f4f95668c83dfb6401762bb2d01a262d1a24ddd2721d006bbe45f20d3c9f362", x);
    aes_polyval(h, y, x, 32);
    printf("POLYVAL ");
    hex(y, 16);
    printf("\n");

    unhex("ee8e1ed9ff2540ae8f2ba9f50bc2f27c", key);
    unhex("752abad3e0afb5f434dc4310", nonce);
    aes_setkey_enc(&kgk, key, 128);
    if (aes_gcmsiv_derive(&kgk, nonce, ak, ek) != 16) fail("derive");
    printf("DERIVE ");
    hex(ak, 16);
    printf(" ");
    hex(ek, 16);
    printf("\n");
    aes_setkey_enc(&kgk, ek, 192); /* any 24 bytes: a 192-bit schedule derives nothing */
    if (aes_gcmsiv_derive(&kgk, nonce, ak, ek) >= 0) fail("192-bit key accepted");

    seal(K128, N3, NULL, 0, NULL, 0);
    seal(K128, N3, NULL, 0, one, 8);
    seal(K128, N3, a1, 1, two, 8);
    seal(K256, N3, NULL, 0, NULL, 0);
    seal(K256, N3, NULL, 0, one, 8);
    for (int i = 0; i < 21; ++i) aad[i] = (unsigned char)(100 + i);
    for (int i = 0; i < 49; ++i) pt[i] = (unsigned char)(1 + i);
    seal("000102030405060708090a0b0c0d0e0f", NA, aad, 21, pt, 49);
    seal("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f", NA, aad, 21, pt, 49);
    if (aes_gcmsiv_self_test(0)) fail("aes_gcmsiv_self_test");
}

/* the counter across 2^32: bytes 0..3 wrap, bytes 4..15 stay, and every block
 * is E(counter block) as polyval_dev.h's siv_ctr_block builds it */
static void wrap(void)
{
    static const uint32_t starts[2] = {0xFFFFFFFEu, 0xFFFFFFFFu};
    unsigned char key[32], zero[5 * 16 + 7] = {0}, ks[sizeof zero], blk[16], want[16];
    aes_context enc;
    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)(0x40 + i);
    for (int bits = 128; bits <= 256; bits += 128) {
        aes_setkey_enc(&enc, key, (unsigned)bits);
        for (int s = 0; s < 2; ++s) {
            unsigned char ctr[16];
            uint32_t t[4] = {starts[s], 0x11223344u, 0x55667788u, 0x99AABBCCu | 0x80000000u};
            memcpy(ctr, t, 16);
            aes_crypt_ctr_le32(&enc, sizeof zero, ctr, zero, ks);
            for (uint32_t i = 0; i < 6; ++i) {
                uint32_t c[4];
                siv_ctr_block(c, t, i);
                memcpy(blk, c, 16);
                aes_crypt_ecb(&enc, AES_ENCRYPT, blk, want);
                if (memcmp(ks + 16 * i, want, i < 5 ? 16 : 7)) fail("ctr_le32 block");
            }
            uint32_t after[4];
            memcpy(after, ctr, 16);
            if (after[0] != (uint32_t)(starts[s] + 6u) || memcmp(after + 1, t + 1, 12)) fail("ctr_le32 counter after the wrap");
        }
    }
    if (!g_fail) printf("WRAP ok\n");
}

static void tamper(void)
{
    unsigned char key[32], nonce[12], aad[13], pt[100], ct[100], out[100], tag[16], zero[100] = {0};
    aes_context kgk;
    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)(3 * i + 1);
    for (int i = 0; i < 12; ++i) nonce[i] = (unsigned char)(0xB0 + i);
    for (int i = 0; i < 13; ++i) aad[i] = (unsigned char)i;
    for (int i = 0; i < 100; ++i) pt[i] = (unsigned char)(7 * i);
    aes_setkey_enc(&kgk, key, 256);
    aes_crypt_gcmsiv(&kgk, AES_ENCRYPT, 100, nonce, aad, 13, pt, ct, NULL, tag);
    int bad = 0;
    for (int what = 0; what < 3; ++what) {
        unsigned char c2[100], t2[16], a2[13];
        memcpy(c2, ct, 100);
        memcpy(t2, tag, 16);
        memcpy(a2, aad, 13);
        if (what == 0) t2[15] ^= 1;
        if (what == 1) c2[50] ^= 0x80;
        if (what == 2) a2[0] ^= 1;
        memset(out, 0xA5, sizeof out);
        if (aes_gcmsiv_auth_decrypt(&kgk, 100, nonce, a2, 13, t2, c2, out) != POLARSSL_ERR_GCM_AUTH_FAILED) bad = 1;
        if (memcmp(out, zero, 100)) bad = 1;
    }
    /* the same nonce, another plaintext: another tag, another keystream */
    unsigned char ct2[100], tag2[16];
    pt[99] ^= 1;
    aes_crypt_gcmsiv(&kgk, AES_ENCRYPT, 100, nonce, aad, 13, pt, ct2, NULL, tag2);
    if (!memcmp(tag, tag2, 16) || !memcmp(ct, ct2, 16)) bad = 1;
    if (bad) fail("tamper");
    else printf("TAMPER ok\n");
}

/* ---- the device's decomposition, on the host -------------------------------- */
enum { SPAN_RUN = 32, SPAN = 64 * SPAN_RUN }; /* GH_RUN, GH_SPAN of ghash_levels_dev.h */

typedef struct {
    uint32_t t[16][256][4];
} pv_table;

static void table_of(pv_table *T, const unsigned char c[16])
{
    static const unsigned char one[16] = {1};
    unsigned char s[16];
    uint32_t seed[4];
    aes_polyval_dot(s, c, one);
    memcpy(seed, s, 16);
    for (uint32_t pos = 0; pos < 16; ++pos)
        for (uint32_t b = 0; b < 256; ++b) pv_table_entry(T->t[pos][b], seed, pos, b);
}

static void table_mul(const pv_table *T, uint32_t x[4])
{
    uint32_t r[4] = {0, 0, 0, 0};
    for (int p = 0; p < 16; ++p) {
        const uint32_t *e = T->t[p][(x[p >> 2] >> (8 * (p & 3))) & 0xFFu];
        for (int j = 0; j < 4; ++j) r[j] ^= e[j];
    }
    memcpy(x, r, 16);
}

static void decomposition(void)
{
    static const size_t lens[] = {1, 16, 17, 1024 + 1, 16 * SPAN - 1, 16 * SPAN, 16 * SPAN + 1, 16 * (2 * SPAN + 3) + 5};
    pv_table *T64 = malloc(sizeof *T64), *T1 = malloc(sizeof *T1);
    unsigned char h[16], y0[16], *data = malloc(16 * (2 * SPAN + 4));
    if (!T64 || !T1 || !data) {
        fail("no memory");
        return;
    }
    unhex("25629347589242761d31f826ba4b757b", h);
    h[0] |= 1;
    h[15] |= 0x80; /* both end bits set */
    for (int i = 0; i < 16; ++i) y0[i] = (unsigned char)(0xC0 + i);
    for (size_t i = 0; i < 16 * (2 * SPAN + 4); ++i) data[i] = (unsigned char)(i * 131 + (i >> 8));
    int bad = 0;
    for (size_t li = 0; li < sizeof lens / sizeof lens[0]; ++li) {
        const size_t len = lens[li];
        unsigned char want[16], c[16], c64[16];
        memcpy(want, y0, 16);
        aes_polyval(h, want, data, len);

        /* level 0 reads the data (block 0 carries y0), level l the partials of level l - 1 */
        size_t n = (len + 15) / 16;
        uint32_t(*x)[4] = calloc(n, 16);
        memcpy(x, data, len);
        uint32_t y0w[4];
        memcpy(y0w, y0, 16);
        for (int j = 0; j < 4; ++j) x[0][j] ^= y0w[j];
        memcpy(c, h, 16);
        for (;;) {
            memcpy(c64, c, 16);
            for (int i = 0; i < 6; ++i) aes_polyval_dot(c64, c64, c64);
            table_of(T64, c64);
            table_of(T1, c);
            const size_t nspans = (n + SPAN - 1) / SPAN, pad = nspans * SPAN - n;
            uint32_t(*part)[4] = calloc(nspans, 16);
            for (size_t s = 0; s < nspans; ++s) {
                uint32_t A[64][4];
                memset(A, 0, sizeof A);
                for (size_t lane = 0; lane < 64; ++lane)
                    for (size_t k = 0; k < SPAN_RUN; ++k) {
                        const size_t v = s * SPAN + k * 64 + lane;
                        table_mul(T64, A[lane]);
                        if (v >= pad)
                            for (int j = 0; j < 4; ++j) A[lane][j] ^= x[v - pad][j];
                    }
                uint32_t Y[4];
                memcpy(Y, A[0], 16);
                for (int j = 1; j < 64; ++j) {
                    table_mul(T1, Y);
                    for (int w = 0; w < 4; ++w) Y[w] ^= A[j][w];
                }
                memcpy(part[s], Y, 16);
            }
            free(x);
            x = part;
            n = nspans;
            memcpy(c, c64, 16); /* C^64, squared on to C^SPAN */
            for (unsigned p = 64; p < SPAN; p *= 2) aes_polyval_dot(c, c, c);
            if (nspans == 1) break;
        }
        /* the finish: Y = dot(S, H) by the bit loop from H's seed */
        static const unsigned char one[16] = {1};
        unsigned char sd[16];
        uint32_t seed[4], got[4];
        aes_polyval_dot(sd, h, one);
        memcpy(seed, sd, 16);
        pv_dot(got, x[0], seed);
        free(x);
        if (memcmp(got, want, 16)) {
            printf("FAIL decomposition at %zu bytes\n", len);
            bad = g_fail = 1;
        }
    }
    free(T64);
    free(T1);
    free(data);
    if (!bad) printf("DECOMP ok\n");
}

int main(void)
{
    vectors();
    wrap();
    tamper();
    decomposition();
    return g_fail;
}
