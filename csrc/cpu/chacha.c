/*
 * chacha.c -- ChaCha20, Poly1305 and ChaCha20-Poly1305 (RFC 8439) on the CPU:
 * the oracle the device kernels are checked against.  Written from the RFC's
 * sections 2.1-2.8; plain C, no tables, no secret-dependent branches or
 * addresses.
 */
#include "chacha.h"

#include <string.h>

static uint32_t ld32(const unsigned char *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static void st32(unsigned char *p, uint32_t v)
{
    p[0] = (unsigned char)v;
    p[1] = (unsigned char)(v >> 8);
    p[2] = (unsigned char)(v >> 16);
    p[3] = (unsigned char)(v >> 24);
}
static void st64(unsigned char *p, uint64_t v)
{
    st32(p, (uint32_t)v);
    st32(p + 4, (uint32_t)(v >> 32));
}

#define ROTL(v, n) (((v) << (n)) | ((v) >> (32 - (n))))
#define QR(a, b, c, d)                                                                                       \
    do {                                                                                                     \
        a += b; d ^= a; d = ROTL(d, 16);                                                                     \
        c += d; b ^= c; b = ROTL(b, 12);                                                                     \
        a += b; d ^= a; d = ROTL(d, 8);                                                                      \
        c += d; b ^= c; b = ROTL(b, 7);                                                                      \
    } while (0)

void chacha20_block(const unsigned char key[32], const unsigned char nonce[12], uint32_t counter,
                    unsigned char out[64])
{
    uint32_t s[16], x[16];
    s[0] = 0x61707865u; /* "expand 32-byte k" */
    s[1] = 0x3320646eu;
    s[2] = 0x79622d32u;
    s[3] = 0x6b206574u;
    for (int i = 0; i < 8; ++i) s[4 + i] = ld32(key + 4 * i);
    s[12] = counter;
    for (int i = 0; i < 3; ++i) s[13 + i] = ld32(nonce + 4 * i);
    memcpy(x, s, sizeof x);
    for (int i = 0; i < 10; ++i) {
        QR(x[0], x[4], x[8], x[12]);
        QR(x[1], x[5], x[9], x[13]);
        QR(x[2], x[6], x[10], x[14]);
        QR(x[3], x[7], x[11], x[15]);
        QR(x[0], x[5], x[10], x[15]);
        QR(x[1], x[6], x[11], x[12]);
        QR(x[2], x[7], x[8], x[13]);
        QR(x[3], x[4], x[9], x[14]);
    }
    for (int i = 0; i < 16; ++i) st32(out + 4 * i, x[i] + s[i]);
}

int chacha20_crypt(const unsigned char key[32], const unsigned char nonce[12], uint32_t counter,
                   const unsigned char *in, unsigned char *out, size_t n)
{
    /* blocks counter .. counter + ceil(n / 64) - 1 must stay below 2^32 */
    const uint64_t nblk = (uint64_t)(n / 64) + (n % 64 ? 1 : 0);
    if ((uint64_t)counter + nblk > ((uint64_t)1 << 32)) return CHACHA_ERR_COUNTER;
    unsigned char ks[64];
    for (size_t off = 0; off < n; off += 64, ++counter) {
        const size_t m = n - off < 64 ? n - off : 64;
        chacha20_block(key, nonce, counter, ks);
        for (size_t i = 0; i < m; ++i) out[off + i] = (unsigned char)(in[off + i] ^ ks[i]);
    }
    return 0;
}

/* ---- Poly1305: five 26-bit limbs -------------------------------------------
 * h and r as sum of limb_i * 2^(26 i).  r is clamped: r < 2^124, limbs < 2^26.
 * h's limbs stay < 2^27 between blocks.  One step is h = (h + c) * r mod p with
 * 2^130 = 5 (mod p): a product limb is five 32x32->64 terms, each below
 * 2^28 * 5 * 2^26 < 2^57, so their sum is below 2^60. */
#define M26 0x3FFFFFFu

void poly1305_init(poly1305_state *st, const unsigned char key[32])
{
    /* the clamp of section 2.5, folded into the limb split */
    st->r[0] = ld32(key + 0) & 0x3FFFFFFu;
    st->r[1] = (ld32(key + 3) >> 2) & 0x3FFFF03u;
    st->r[2] = (ld32(key + 6) >> 4) & 0x3FFC0FFu;
    st->r[3] = (ld32(key + 9) >> 6) & 0x3F03FFFu;
    st->r[4] = (ld32(key + 12) >> 8) & 0x00FFFFFu;
    memset(st->h, 0, sizeof st->h);
    memcpy(st->s, key + 16, 16);
}

/* h = (h + block + hibit * 2^128) * r */
static void poly1305_step(poly1305_state *st, const unsigned char b[16], uint32_t hibit)
{
    const uint32_t r0 = st->r[0], r1 = st->r[1], r2 = st->r[2], r3 = st->r[3], r4 = st->r[4];
    const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
    const uint64_t h0 = (uint64_t)st->h[0] + (ld32(b + 0) & M26);
    const uint64_t h1 = (uint64_t)st->h[1] + ((ld32(b + 3) >> 2) & M26);
    const uint64_t h2 = (uint64_t)st->h[2] + ((ld32(b + 6) >> 4) & M26);
    const uint64_t h3 = (uint64_t)st->h[3] + ((ld32(b + 9) >> 6) & M26);
    const uint64_t h4 = (uint64_t)st->h[4] + ((ld32(b + 12) >> 8) | (hibit << 24));
    uint64_t d0 = h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1;
    uint64_t d1 = h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2;
    uint64_t d2 = h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3;
    uint64_t d3 = h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4;
    uint64_t d4 = h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0;
    d1 += d0 >> 26;
    d2 += d1 >> 26;
    d3 += d2 >> 26;
    d4 += d3 >> 26;
    d0 = (d0 & M26) + (d4 >> 26) * 5; /* 2^130 = 5 */
    d1 = (d1 & M26) + (d0 >> 26);
    st->h[0] = (uint32_t)d0 & M26;
    st->h[1] = (uint32_t)d1;
    st->h[2] = (uint32_t)d2 & M26;
    st->h[3] = (uint32_t)d3 & M26;
    st->h[4] = (uint32_t)d4 & M26;
}

void poly1305_blocks(poly1305_state *st, const unsigned char *data, size_t nblocks)
{
    for (size_t i = 0; i < nblocks; ++i) poly1305_step(st, data + 16 * i, 1);
}

void poly1305_last(poly1305_state *st, const unsigned char *data, size_t n)
{
    unsigned char b[16] = {0};
    if (n == 0 || n > 15) return;
    memcpy(b, data, n);
    b[n] = 1;
    poly1305_step(st, b, 0);
}

void poly1305_pad16(poly1305_state *st, const unsigned char *data, size_t n)
{
    poly1305_blocks(st, data, n / 16);
    if (n % 16) {
        unsigned char b[16] = {0};
        memcpy(b, data + (n - n % 16), n % 16);
        poly1305_step(st, b, 1);
    }
}

void poly1305_finish(poly1305_state *st, unsigned char tag[16])
{
    uint32_t h0 = st->h[0], h1 = st->h[1], h2 = st->h[2], h3 = st->h[3], h4 = st->h[4], c;
    /* full carry: every limb below 2^26, the value below 2^130 + small */
    c = h1 >> 26; h1 &= M26; h2 += c;
    c = h2 >> 26; h2 &= M26; h3 += c;
    c = h3 >> 26; h3 &= M26; h4 += c;
    c = h4 >> 26; h4 &= M26; h0 += c * 5;
    c = h0 >> 26; h0 &= M26; h1 += c;
    c = h1 >> 26; h1 &= M26; h2 += c;
    c = h2 >> 26; h2 &= M26; h3 += c;
    c = h3 >> 26; h3 &= M26; h4 += c;
    c = h4 >> 26; h4 &= M26; h0 += c * 5;
    c = h0 >> 26; h0 &= M26; h1 += c;
    /* g = h - p = h + 5 - 2^130; take g where it did not borrow (h >= p) */
    uint32_t g0 = h0 + 5;
    c = g0 >> 26; g0 &= M26;
    uint32_t g1 = h1 + c;
    c = g1 >> 26; g1 &= M26;
    uint32_t g2 = h2 + c;
    c = g2 >> 26; g2 &= M26;
    uint32_t g3 = h3 + c;
    c = g3 >> 26; g3 &= M26;
    const uint32_t g4 = h4 + c - (1u << 26);
    const uint32_t take_g = (g4 >> 31) - 1; /* all ones when g4 did not go negative */
    h0 = (h0 & ~take_g) | (g0 & take_g);
    h1 = (h1 & ~take_g) | (g1 & take_g);
    h2 = (h2 & ~take_g) | (g2 & take_g);
    h3 = (h3 & ~take_g) | (g3 & take_g);
    h4 = (h4 & ~take_g) | (g4 & take_g);
    /* h mod 2^128 as four words, plus s mod 2^128 */
    const uint32_t w0 = h0 | h1 << 26, w1 = h1 >> 6 | h2 << 20, w2 = h2 >> 12 | h3 << 14, w3 = h3 >> 18 | h4 << 8;
    uint64_t f = (uint64_t)w0 + ld32(st->s + 0);
    st32(tag + 0, (uint32_t)f);
    f = (uint64_t)w1 + ld32(st->s + 4) + (f >> 32);
    st32(tag + 4, (uint32_t)f);
    f = (uint64_t)w2 + ld32(st->s + 8) + (f >> 32);
    st32(tag + 8, (uint32_t)f);
    f = (uint64_t)w3 + ld32(st->s + 12) + (f >> 32);
    st32(tag + 12, (uint32_t)f);
}

void poly1305_mac(const unsigned char key[32], const unsigned char *data, size_t n, unsigned char tag[16])
{
    poly1305_state st;
    poly1305_init(&st, key);
    poly1305_blocks(&st, data, n / 16);
    if (n % 16) poly1305_last(&st, data + (n - n % 16), n % 16);
    poly1305_finish(&st, tag);
}

/* ---- the AEAD (section 2.8) ------------------------------------------------ */
int chacha20_poly1305_tag(const unsigned char key[32], const unsigned char nonce[12], const unsigned char *aad,
                          size_t aad_len, const unsigned char *ct, size_t n, unsigned char tag[16])
{
    if ((uint64_t)n > CHACHA20_POLY1305_MAX_BYTES) return CHACHA_ERR_COUNTER;
    unsigned char b0[64], len[16];
    poly1305_state st;
    chacha20_block(key, nonce, 0, b0); /* the one-time key: bytes 0..31 of block 0 */
    poly1305_init(&st, b0);
    poly1305_pad16(&st, aad, aad_len);
    poly1305_pad16(&st, ct, n);
    st64(len, (uint64_t)aad_len);
    st64(len + 8, (uint64_t)n);
    poly1305_blocks(&st, len, 1);
    poly1305_finish(&st, tag);
    return 0;
}

int chacha20_poly1305_encrypt(const unsigned char key[32], const unsigned char nonce[12], const unsigned char *aad,
                              size_t aad_len, const unsigned char *in, unsigned char *out, size_t n,
                              unsigned char tag[16])
{
    if ((uint64_t)n > CHACHA20_POLY1305_MAX_BYTES) return CHACHA_ERR_COUNTER;
    const int r = chacha20_crypt(key, nonce, 1, in, out, n);
    if (r) return r;
    return chacha20_poly1305_tag(key, nonce, aad, aad_len, out, n, tag);
}

int chacha20_poly1305_auth_decrypt(const unsigned char key[32], const unsigned char nonce[12],
                                   const unsigned char *aad, size_t aad_len, const unsigned char tag[16],
                                   const unsigned char *in, unsigned char *out, size_t n)
{
    unsigned char t[16];
    int r = chacha20_poly1305_tag(key, nonce, aad, aad_len, in, n, t);
    if (r) return r;
    unsigned diff = 0;
    for (int i = 0; i < 16; ++i) diff |= (unsigned)(t[i] ^ tag[i]);
    if (diff) {
        memset(out, 0, n);
        return CHACHA_ERR_AUTH_FAILED;
    }
    return chacha20_crypt(key, nonce, 1, in, out, n);
}
