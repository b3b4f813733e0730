/*
 * ccm_batch_selftest.c -- the batched CCM kernel's lane (csrc/hip/aes_ccm_batch.hip
 * ccm_record) on the host, with the kernel's own block formatting
 * (csrc/hip/ccm_dev.h), against aes_crypt_ccm of aes.c:
 *
 *   MAC start   B0 and the base block from the nonce's words, the encoded AAD's
 *               blocks from any alignment, beside them the first pad
 *               (ccm_ctr_first)
 *   data        bursts of CCM_BURST blocks through a ring of registers, read
 *               whole before any of it is written (the records run IN PLACE
 *               here); encryption's and the pipelined decryption's second call
 *               (ccm_ctr_of_step); the partial block by bytes, masked for the MAC
 *   tag         X ^ S_0, its first tag_len bytes
 *   order       ccm_order_fill: a permutation, block counts never rising, equal
 *               counts in their own order
 *
 * for all key sizes, nonce lengths 7 .. 13 and tag lengths 4 .. 16, the edge
 * lengths 0, 1, 15, 16, 17, 31, 32, 127, 128, 129, 4096, 4097, 4113 (the counter's
 * first carry: block 256), 65535 under a 13-byte nonce, 1 MiB, every length
 * 0 .. 300, and the AAD lengths either side of its encodings' switch at every
 * misalignment.  Guard bytes around every buffer are checked.  Prints one line
 * per key size; exits non-zero on the first mismatch.
 * tests/test_ccm_batch_selftest_cpu.py builds it plain and with
 * -fsanitize=address,undefined.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aes.h"
#include "ccm_dev.h"

#define MAX_BYTES (1u << 20)
#define MAX_AAD (1u << 16)
#define GUARD 32

typedef struct {
    uint32_t w[4];
} blk;

/* the two cipher calls of a step: the kernel's enc_rounds4_from<.., B = 2> */
static void enc2(aes_context *enc, uint32_t a[4], uint32_t b[4])
{
    unsigned char t[16];
    memcpy(t, a, 16);
    aes_crypt_ecb(enc, AES_ENCRYPT, t, t);
    memcpy(a, t, 16);
    memcpy(t, b, 16);
    aes_crypt_ecb(enc, AES_ENCRYPT, t, t);
    memcpy(b, t, 16);
}

/* ccm_record, line by line: in -> out (may be the same), the computed tag */
static void lane(aes_context *enc, int dec, const unsigned char *nonce, uint32_t nonce_len, uint32_t tag_len,
                 const unsigned char *aad, uint32_t alen, const unsigned char *in, unsigned char *out, uint32_t nbytes,
                 unsigned char tag[16])
{
    const uint32_t nfull = nbytes >> 4, r = nbytes & 15u, n = ccm_data_blocks(nbytes), nab = ccm_aad_blocks(alen);
    uint32_t nw[4] = {0, 0, 0, 0}, base[4], X[4], S[4], A[4];
    for (uint32_t i = 0; i < 13; ++i)
        if (i < nonce_len) nw[i >> 2] |= (uint32_t)nonce[i] << (8 * (i & 3u));
    ccm_base(base, nw);
    const uint32_t fl = ccm_flags_ctr(nonce_len);
    ccm_block(X, base, ccm_flags_b0(alen != 0, tag_len, nonce_len), nbytes);
    ccm_block(A, base, fl, ccm_ctr_first(dec, n));
    for (uint32_t k = 0; k <= nab; ++k) {
        uint32_t s1[4];
        if (k) {
            uint32_t w[4];
            ccm_aad_block(w, aad, alen, k - 1u);
            for (int q = 0; q < 4; ++q) X[q] ^= w[q];
        }
        memcpy(s1, A, 16);
        enc2(enc, X, s1);
        memcpy(S, s1, 16);
    }
    uint32_t mask[4];
    for (int q = 0; q < 4; ++q) mask[q] = ccm_mask_word(r, q);
    for (uint32_t g0 = 0; g0 < n; g0 += CCM_BURST) {
        blk cur[CCM_BURST];
        memset(cur, 0, sizeof cur);
        for (uint32_t u = 0; u < CCM_BURST; ++u)
            if (g0 + u < nfull) memcpy(cur[u].w, in + 16 * (size_t)(g0 + u), 16);
        const int tail = r && nfull - g0 < CCM_BURST;
        if (tail) {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < 15; ++b)
                if (b < r) w[b >> 2] |= (uint32_t)in[16 * (size_t)nfull + b] << (8 * (b & 3u));
            memcpy(cur[nfull - g0].w, w, 16);
        }
        const uint32_t cnt = n - g0 < CCM_BURST ? n - g0 : CCM_BURST;
        for (uint32_t u = 0; u < CCM_BURST; ++u) {
            blk res;
            memset(&res, 0, sizeof res);
            if (u < cnt) {
                const uint32_t j = g0 + u;
                uint32_t p[4], s1[4];
                memcpy(p, cur[0].w, 16);
                if (dec)
                    for (int q = 0; q < 4; ++q) p[q] = (p[q] ^ S[q]) & (j == nfull ? mask[q] : 0xFFFFFFFFu);
                ccm_block(s1, base, fl, ccm_ctr_of_step(dec, j, n));
                for (int q = 0; q < 4; ++q) X[q] ^= p[q];
                enc2(enc, X, s1);
                if (dec) {
                    memcpy(S, s1, 16);
                    memcpy(res.w, p, 16);
                } else {
                    for (int q = 0; q < 4; ++q) res.w[q] = p[q] ^ s1[q];
                }
            }
            for (uint32_t v = 0; v + 1 < CCM_BURST; ++v) cur[v] = cur[v + 1];
            cur[CCM_BURST - 1] = res;
        }
        for (uint32_t u = 0; u < CCM_BURST; ++u)
            if (g0 + u < nfull) memcpy(out + 16 * (size_t)(g0 + u), cur[u].w, 16);
        if (tail)
            for (uint32_t b = 0; b < 15; ++b)
                if (b < r) out[16 * (size_t)nfull + b] = (unsigned char)(cur[nfull - g0].w[b >> 2] >> (8 * (b & 3u)));
    }
    memset(tag, 0, 16);
    for (uint32_t b = 0; b < 16; ++b)
        if (b < tag_len) tag[b] = (unsigned char)((X[b >> 2] ^ S[b >> 2]) >> (8 * (b & 3u)));
}

static unsigned char *g_p, *g_buf, *g_ref, *g_aad;

static int guards_ok(const unsigned char *b, size_t n)
{
    for (size_t i = 0; i < GUARD; ++i)
        if (b[i] != 0xC3 || b[GUARD + n + i] != 0xC3) return 0;
    return 1;
}

/* one record: both directions through the lane, in place, against the oracle; the AAD at aad_off */
static int record(aes_context *enc, uint32_t n, uint32_t alen, uint32_t aad_off, uint32_t nl, uint32_t tl, unsigned seed)
{
    unsigned char nonce[13], tag[16], tag2[16], rtag[16];
    for (uint32_t i = 0; i < 13; ++i) nonce[i] = (unsigned char)(seed * 29u + 7u * i + n);
    const unsigned char *aad = g_aad + aad_off;
    if (aes_crypt_ccm(enc, AES_ENCRYPT, n, nonce, nl, aad, alen, g_p, g_ref, rtag, tl)) return printf("FAIL oracle\n"), 1;
    unsigned char *d = g_buf + GUARD;
    memset(g_buf, 0xC3, (size_t)n + 2 * GUARD);
    memcpy(d, g_p, n);
    lane(enc, 0, nonce, nl, tl, aad, alen, d, d, n, tag);
    if (memcmp(d, g_ref, n) || memcmp(tag, rtag, 16) || !guards_ok(g_buf, n))
        return printf("FAIL encrypt n=%u alen=%u+%u nonce=%u tag=%u\n", n, alen, aad_off, nl, tl), 1;
    lane(enc, 1, nonce, nl, tl, aad, alen, d, d, n, tag2);
    if (memcmp(d, g_p, n) || memcmp(tag2, rtag, 16) || !guards_ok(g_buf, n))
        return printf("FAIL decrypt n=%u alen=%u+%u nonce=%u tag=%u\n", n, alen, aad_off, nl, tl), 1;
    return 0;
}

/* the planner's order over descriptors of six words, the length in word 2 */
static int order_check(void)
{
    enum { N = 1000 };
    static uint64_t desc[N][6];
    static uint32_t order[N];
    static unsigned char seen[N];
    uint32_t x = 12345u;
    for (int m = 0; m < N; ++m) {
        x = x * 1664525u + 1013904223u;
        desc[m][2] = m % 7 == 0 ? MAX_BYTES - (x >> 28) : m % 5 == 0 ? 0 : (x >> 16) % 3000u;
    }
    if (ccm_order_fill(order, &desc[0][2], 6, N)) return printf("FAIL order: no memory\n"), 1;
    memset(seen, 0, sizeof seen);
    for (int t = 0; t < N; ++t) {
        if (order[t] >= N || seen[order[t]]++) return printf("FAIL order: not a permutation\n"), 1;
        if (!t) continue;
        const uint32_t a = ccm_data_blocks(desc[order[t - 1]][2]), b = ccm_data_blocks(desc[order[t]][2]);
        if (a < b || (a == b && order[t - 1] > order[t])) return printf("FAIL order at %d\n", t), 1;
    }
    return 0;
}

int main(void)
{
    static const uint32_t edge[] = {0, 1, 15, 16, 17, 31, 32, 127, 128, 129, 4096, 4097, 4113};
    static const uint32_t alens[] = {0, 1, 13, 14, 15, 16, 29, 30, 31, 65279, 65280, 65536};
    unsigned char key[32];
    g_p = malloc(MAX_BYTES), g_buf = malloc(MAX_BYTES + 2 * GUARD), g_ref = malloc(MAX_BYTES);
    g_aad = malloc(MAX_AAD + 4);
    if (!g_p || !g_buf || !g_ref || !g_aad) return 2;
    uint32_t x = 0x9E3779B9u;
    for (size_t i = 0; i < MAX_BYTES; ++i) g_p[i] = (unsigned char)((x = x * 1664525u + 1013904223u) >> 24);
    for (size_t i = 0; i < MAX_AAD + 4; ++i) g_aad[i] = (unsigned char)((x = x * 1664525u + 1013904223u) >> 24);
    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)(0xA0 + 3 * i);
    int bad = order_check();
    for (int keybits = 128; keybits <= 256 && !bad; keybits += 64) {
        aes_context enc;
        if (aes_setkey_enc(&enc, key, (unsigned)keybits)) return printf("FAIL setkey\n"), 1;
        size_t nrec = 0;
        for (uint32_t nl = 7; nl <= 13 && !bad; ++nl)
            for (uint32_t tl = 4; tl <= 16 && !bad; tl += 2)
                for (size_t e = 0; e < sizeof edge / sizeof edge[0] && !bad; ++e, ++nrec)
                    bad = record(&enc, edge[e], (uint32_t)(e * 5 % 23), (uint32_t)e & 3u, nl, tl, (unsigned)keybits);
        for (uint32_t n = 0; n <= 300 && !bad; ++n, ++nrec)
            bad = record(&enc, n, n % 41, n & 3u, 7 + n % 7, 4 + 2 * (n % 7), (unsigned)keybits + n);
        for (size_t a = 0; a < sizeof alens / sizeof alens[0] && !bad; ++a)
            for (uint32_t off = 0; off < 4 && !bad; ++off, ++nrec) {
                bad = record(&enc, 17, alens[a], off, 12, 16, (unsigned)keybits + off);
                if (!bad) bad = record(&enc, 0, alens[a], off, 13, 8, (unsigned)keybits + off); /* AAD only */
            }
        if (!bad) bad = record(&enc, 65535, 13, 1, 13, 16, (unsigned)keybits), ++nrec;
        if (!bad) bad = record(&enc, MAX_BYTES, 20, 0, 12, 4, (unsigned)keybits), ++nrec;
        if (!bad) bad = record(&enc, MAX_BYTES - 1, 0, 0, 7, 16, (unsigned)keybits), ++nrec;
        if (!bad) printf("OK AES-%d %zu records\n", keybits, nrec);
    }
    free(g_p), free(g_buf), free(g_ref), free(g_aad);
    return bad;
}
