/*
 * ocb_selftest.c -- the AES-OCB3 oracle (aes.c) as a stand-alone program: the
 * inputs of tests/golden/ocb_vectors.json (RFC 7253 Appendix A's pattern, the
 * extra nonce and tag lengths), the RFC's iterated check for every key size
 * and tag length, an authenticated round trip with each kind of tampering, and
 * pieces chained through aes_crypt_ocb_blocks.  Prints every result; exits
 * non-zero if a round trip or a tamper check fails.  tests/test_ocb_selftest_cpu.py
 * builds it with -fsanitize=address,undefined and compares the output.
 *
 *   V <keybits> <nonce> <alen> <plen> <taglen bytes> <ciphertext or -> <tag>
 *   ITER <keybits> <taglen bits> <result>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aes.h"

static int g_fail;

static void hex(const unsigned char *p, size_t n)
{
    if (!n) printf("-");
    for (size_t i = 0; i < n; ++i) printf("%02X", p[i]);
}

static void fail(const char *what)
{
    printf("FAIL %s\n", what);
    g_fail = 1;
}

/* one vector: encrypt, print, decrypt again through the authenticated call */
static void vector(const aes_ocb_context *ctx, int keybits, const unsigned char *nonce, size_t nl, size_t alen,
                   size_t plen, size_t tl)
{
    unsigned char a[64], p[64], c[64], d[64], tag[16];
    for (size_t i = 0; i < 64; ++i) a[i] = p[i] = (unsigned char)i;
    if (aes_crypt_ocb(ctx, AES_ENCRYPT, plen, nonce, nl, a, alen, p, c, tag, tl)) fail("encrypt");
    printf("V %d ", keybits);
    hex(nonce, nl);
    printf(" %zu %zu %zu ", alen, plen, tl);
    hex(c, plen);
    printf(" ");
    hex(tag, tl);
    printf("\n");
    memset(d, 0xA5, sizeof d);
    if (aes_ocb_auth_decrypt(ctx, plen, nonce, nl, a, alen, tag, tl, c, d) || memcmp(d, p, plen)) fail("round trip");
}

static void vectors(void)
{
    static const int lens[16][2] = {{0, 0},   {8, 8},   {8, 0},   {0, 8},   {16, 16}, {16, 0}, {0, 16}, {24, 24},
                                    {24, 0},  {0, 24},  {32, 32}, {32, 0},  {0, 32},  {40, 40}, {40, 0}, {0, 40}};
    static const size_t extra_nl[3] = {1, 8, 15}, extra_tl[3] = {8, 12, 16};
    unsigned char key[32], nonce[15];
    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)i;
    for (int keybits = 128; keybits <= 256; keybits += 64) {
        aes_ocb_context ctx;
        if (aes_ocb_setkey(&ctx, key, (unsigned)keybits)) fail("setkey");
        for (int v = 0; v < 16; ++v) {
            static const unsigned char n0[11] = {0xBB, 0xAA, 0x99, 0x88, 0x77, 0x66, 0x55, 0x44, 0x33, 0x22, 0x11};
            memcpy(nonce, n0, 11);
            nonce[11] = (unsigned char)v;
            vector(&ctx, keybits, nonce, 12, (size_t)lens[v][0], (size_t)lens[v][1], 16);
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                for (size_t i = 0; i < extra_nl[a]; ++i) nonce[i] = (unsigned char)(0xF0 - i);
                vector(&ctx, keybits, nonce, extra_nl[a], 24, 40, extra_tl[b]);
            }
    }
}

static void put96(unsigned char n[12], unsigned v)
{
    memset(n, 0, 12);
    n[8] = (unsigned char)(v >> 24);
    n[9] = (unsigned char)(v >> 16);
    n[10] = (unsigned char)(v >> 8);
    n[11] = (unsigned char)v;
}

static void iterated(int keybits, int tagbits)
{
    unsigned char key[32] = {0}, n[12], s[128] = {0}, tag[16];
    const size_t tl = (size_t)tagbits / 8;
    unsigned char *c = (unsigned char *)malloc(128 * (3 * 128 + 3 * 16));
    size_t at = 0;
    aes_ocb_context ctx;
    if (!c) exit(2);
    key[keybits / 8 - 1] = (unsigned char)tagbits;
    aes_ocb_setkey(&ctx, key, (unsigned)keybits);
    for (unsigned i = 0; i < 128; ++i) {
        put96(n, 3 * i + 1);
        aes_crypt_ocb(&ctx, AES_ENCRYPT, i, n, 12, s, i, s, c + at, tag, tl);
        memcpy(c + at + i, tag, tl);
        at += i + tl;
        put96(n, 3 * i + 2);
        aes_crypt_ocb(&ctx, AES_ENCRYPT, i, n, 12, NULL, 0, s, c + at, tag, tl);
        memcpy(c + at + i, tag, tl);
        at += i + tl;
        put96(n, 3 * i + 3);
        aes_crypt_ocb(&ctx, AES_ENCRYPT, 0, n, 12, s, i, s, c + at, tag, tl);
        memcpy(c + at, tag, tl);
        at += tl;
    }
    put96(n, 385);
    aes_crypt_ocb(&ctx, AES_ENCRYPT, 0, n, 12, c, at, s, s, tag, tl);
    printf("ITER %d %d ", keybits, tagbits);
    hex(tag, tl);
    printf("\n");
    free(c);
}

/* a flipped bit anywhere must zero the output */
static void tamper(void)
{
    enum { N = 4111 };
    unsigned char key[16], nonce[12], aad[13], tag[16];
    unsigned char *p = (unsigned char *)malloc(N), *c = (unsigned char *)malloc(N), *d = (unsigned char *)malloc(N);
    aes_ocb_context ctx;
    if (!p || !c || !d) exit(2);
    for (int i = 0; i < 16; ++i) key[i] = (unsigned char)(3 * i + 1);
    for (int i = 0; i < 12; ++i) nonce[i] = (unsigned char)(0x40 + i);
    for (int i = 0; i < 13; ++i) aad[i] = (unsigned char)(0x80 + i);
    for (int i = 0; i < N; ++i) p[i] = (unsigned char)(i * 7 + (i >> 8));
    aes_ocb_setkey(&ctx, key, 128);
    aes_crypt_ocb(&ctx, AES_ENCRYPT, N, nonce, 12, aad, 13, p, c, tag, 16);
    if (aes_ocb_auth_decrypt(&ctx, N, nonce, 12, aad, 13, tag, 16, c, d) || memcmp(d, p, N)) fail("tamper: clean");
    for (int which = 0; which < 4; ++which) {
        unsigned char *t = which == 0 ? c + 2000 : which == 1 ? tag + 5 : which == 2 ? aad + 3 : nonce + 7;
        *t ^= 0x10;
        memset(d, 0xA5, N);
        int zero = 1;
        const int r = aes_ocb_auth_decrypt(&ctx, N, nonce, 12, aad, 13, tag, 16, c, d);
        for (int i = 0; i < N; ++i) zero &= d[i] == 0;
        if (r != POLARSSL_ERR_OCB_AUTH_FAILED || !zero) fail("tamper: accepted or not zeroed");
        *t ^= 0x10;
    }
    /* the message in three pieces through the primitive, in place */
    unsigned char off0[16], cs[16] = {0}, cs1[16] = {0};
    aes_ocb_offset0(&ctx, nonce, 12, 16, off0);
    memcpy(d, p, N);
    aes_crypt_ocb_blocks(&ctx, AES_ENCRYPT, off0, 0, 100, d, d, cs);
    aes_crypt_ocb_blocks(&ctx, AES_ENCRYPT, off0, 100, 1, d + 1600, d + 1600, cs);
    aes_crypt_ocb_blocks(&ctx, AES_ENCRYPT, off0, 101, 155, d + 1616, d + 1616, cs);
    aes_crypt_ocb_blocks(&ctx, AES_ENCRYPT, off0, 0, 256, p, p, cs1);
    if (memcmp(d, c, 4096) || memcmp(p, c, 4096) || memcmp(cs, cs1, 16)) fail("pieces");
    printf("TAMPER %s\n", g_fail ? "failed" : "ok");
    free(p);
    free(c);
    free(d);
}

int main(void)
{
    vectors();
    for (int keybits = 128; keybits <= 256; keybits += 64)
        for (int tagbits = 128; tagbits >= 64; tagbits -= 32) iterated(keybits, tagbits);
    tamper();
    return g_fail;
}
