/*
 * gcmsiv_batch_selftest.c -- the host-callable arithmetic of the batched
 * AES-GCM-SIV kernels (csrc/hip/aes_gcm_siv_batch.hip) as a stand-alone program,
 * with the kernels' own functions from csrc/hip/polyval_dev.h, against aes.c:
 *
 *   MUL      the per-record product: a nibble table of C (pv4_entry) and Horner
 *            over the multiplicand's nibbles (pv4_dot) against aes_polyval_dot
 *   EXPAND   siv_expand_key against aes_setkey_enc, both key sizes
 *   WRAP     siv_ctr_block across 2^32 against aes_crypt_ctr_le32
 *   OK ...   whole records the way the four kernels cut them: the derivation
 *            blocks, the expanded key, the powers of H by squaring, L lanes of
 *            Horner under H^L aligned to the record's end, the fold of log2 L
 *            steps, the finisher and the counter blocks -- for L = 16 and L = 64,
 *            over RFC 8452's vectors and over the lengths of the GPU tests --
 *            against aes_crypt_gcmsiv, ciphertext and tag.
 *
 * Prints every result; exits non-zero if a check fails.
 * tests/test_gcm_siv_batch_selftest_cpu.py builds it plain and with
 * -fsanitize=address,undefined and compares the output.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aes.h"
#include "../hip/polyval_dev.h"

static int g_fail;
static uint8_t g_sb[256];

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

/* the S-box from its definition (the kernels read the device's constant table) */
static void make_sbox(void)
{
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ (p << 1) ^ ((p & 0x80) ? 0x1B : 0));
        q ^= (uint8_t)(q << 1);
        q ^= (uint8_t)(q << 2);
        q ^= (uint8_t)(q << 4);
        if (q & 0x80) q ^= 0x09;
        const uint8_t x = (uint8_t)(q ^ (q << 1 | q >> 7) ^ (q << 2 | q >> 6) ^ (q << 3 | q >> 5) ^ (q << 4 | q >> 4));
        g_sb[p] = (uint8_t)(x ^ 0x63);
    } while (p != 1);
    g_sb[0] = 0x63;
}

static uint32_t g_rng = 0x9E3779B9u;
static uint32_t rnd(void)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

typedef uint32_t nibtab[16][4];

static void table_of(nibtab T, const uint32_t c[4])
{
    for (uint32_t n = 0; n < 16; ++n) pv4_entry(T[n], c, n);
}

/* ---- MUL ---------------------------------------------------------------------- */
static void mul(void)
{
    uint32_t cases[8][4] = {
        {1u, 0, 0, 0x80000000u},                /* only bits 0 and 127 */
        {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
        {0, 0, 0, 0},
        {1u, 0, 0, 0},
        {0, 0, 0, 0x80000000u},
        {0x0000000Fu, 0, 0, 0xF0000000u},
    };
    unhex("25629347589242761d31f826ba4b757b", (unsigned char *)cases[6]); /* RFC 8452 A: H */
    unhex("4f4f95668c83dfb6401762bb2d01a262", (unsigned char *)cases[7]); /* and X_1 */
    int bad = 0, n = 0;
    for (int ci = 0; ci < 8 + 200; ++ci) {
        uint32_t c[4];
        for (int j = 0; j < 4; ++j) c[j] = ci < 8 ? cases[ci][j] : rnd();
        nibtab T;
        table_of(T, c);
        for (int ai = 0; ai < 8 + 24; ++ai, ++n) {
            uint32_t a[4], got[4];
            unsigned char want[16];
            for (int j = 0; j < 4; ++j) a[j] = ai < 8 ? cases[ai][j] : rnd();
            pv4_dot(got, a, (const uint32_t(*)[4])T);
            aes_polyval_dot(want, (const unsigned char *)a, (const unsigned char *)c);
            if (memcmp(got, want, 16)) bad = 1;
        }
    }
    if (bad) fail("pv4_dot against aes_polyval_dot");
    else printf("MUL ok %d products\n", n);
}

/* ---- EXPAND ------------------------------------------------------------------- */
static void expand(void)
{
    int bad = 0;
    for (int t = 0; t < 64; ++t)
        for (int nk = 4; nk <= 8; nk += 4) {
            unsigned char key[32];
            uint32_t rk[60], want[60];
            aes_context ctx;
            for (int i = 0; i < 32; ++i) key[i] = t == 0 ? 0 : t == 1 ? 0xFF : (unsigned char)rnd();
            memcpy(rk, key, 4 * (size_t)nk);
            siv_expand_key(rk, g_sb, nk);
            aes_setkey_enc(&ctx, key, 32u * (unsigned)nk);
            if (aes_export_rk32(&ctx, want) != 4 * (nk + 7) || memcmp(rk, want, 16 * ((size_t)nk + 7))) bad = 1;
        }
    if (bad) fail("siv_expand_key against aes_setkey_enc");
    else printf("EXPAND ok\n");
}

/* ---- WRAP --------------------------------------------------------------------- */
static void wrap(void)
{
    /* 3, 70 and 256 + 100 blocks before 2^32; byte 4 is 0xff, byte 15 below 0x80 */
    static const uint32_t before[3] = {3, 70, 356};
    enum { NBLK = 400 };
    unsigned char key[32], *zero = calloc(NBLK, 16), *ks = malloc(NBLK * 16), blk[16], want[16];
    aes_context enc;
    int bad = !zero || !ks;
    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)(0x40 + i);
    for (int bits = 128; bits <= 256 && !bad; bits += 128) {
        aes_setkey_enc(&enc, key, (unsigned)bits);
        for (int s = 0; s < 3; ++s) {
            const uint32_t t[4] = {0u - before[s], 0x112233FFu, 0x55667788u, 0x19AABBCCu};
            unsigned char ctr[16];
            memcpy(ctr, t, 16);
            ctr[15] |= 0x80;
            aes_crypt_ctr_le32(&enc, NBLK * 16, ctr, zero, ks);
            for (uint32_t i = 0; i < NBLK; ++i) {
                uint32_t c[4];
                siv_ctr_block(c, t, i);
                if (c[1] != t[1] || c[2] != t[2] || c[3] != (t[3] | 0x80000000u)) bad = 1;
                memcpy(blk, c, 16);
                aes_crypt_ecb(&enc, AES_ENCRYPT, blk, want);
                if (memcmp(ks + 16 * i, want, 16)) bad = 1;
            }
        }
    }
    free(zero);
    free(ks);
    if (bad) fail("siv_ctr_block across the wrap");
    else printf("WRAP ok\n");
}

/* ---- whole records ------------------------------------------------------------ */
/* block i of pad16(aad) || pad16(data) || le64(8 al) le64(8 n), as the kernel's sb_block forms it */
static void hashed_block(uint32_t x[4], const unsigned char *aad, size_t al, const unsigned char *data, size_t n, size_t i)
{
    const size_t na = (al + 15) / 16, nd = (n + 15) / 16;
    unsigned char b[16] = {0};
    if (i < na) {
        memcpy(b, aad + 16 * i, al - 16 * i < 16 ? al - 16 * i : 16);
    } else if (i < na + nd) {
        const size_t off = 16 * (i - na);
        memcpy(b, data + off, n - off < 16 ? n - off : 16);
    } else {
        const uint64_t ab = (uint64_t)al * 8, db = (uint64_t)n * 8;
        const uint32_t w[4] = {(uint32_t)ab, (uint32_t)(ab >> 32), (uint32_t)db, (uint32_t)(db >> 32)};
        memcpy(b, w, 16);
    }
    memcpy(x, b, 16);
}

/* S = POLYVAL_H of the record with L lanes: k_polyval_batch's steps */
static void hash_lanes(uint32_t S[4], const uint32_t H[4], unsigned L, const unsigned char *aad, size_t al,
                       const unsigned char *data, size_t n)
{
    const unsigned LOG = L == 16 ? 4 : 6;
    nibtab T[7];
    uint32_t C[4] = {H[0], H[1], H[2], H[3]};
    for (unsigned s = 0; s <= LOG; ++s) { /* the tables of H^(2^s), by squaring */
        table_of(T[s], C);
        if (s < LOG) pv4_dot(C, C, (const uint32_t(*)[4])T[s]);
    }
    const size_t nb = (al + 15) / 16 + (n + 15) / 16 + 1, npass = (nb + L - 1) / L, pad = npass * L - nb;
    uint32_t A[64][4];
    memset(A, 0, sizeof A);
    for (unsigned l = 0; l < L; ++l)
        for (size_t k = 0; k < npass; ++k) {
            const size_t v = k * L + l;
            uint32_t x[4] = {0, 0, 0, 0};
            if (v >= pad) hashed_block(x, aad, al, data, n, v - pad);
            pv4_dot(A[l], A[l], (const uint32_t(*)[4])T[LOG]);
            for (int j = 0; j < 4; ++j) A[l][j] ^= x[j];
        }
    for (unsigned s = 0; s < LOG; ++s) { /* every lane takes the step; lanes past L - d get zero, as a shuffle's own value is unused */
        const unsigned d = 1u << s;
        uint32_t N[64][4];
        for (unsigned l = 0; l < L; ++l) {
            pv4_dot(N[l], A[l], (const uint32_t(*)[4])T[s]);
            if (l + d < L)
                for (int j = 0; j < 4; ++j) N[l][j] ^= A[l + d][j];
        }
        memcpy(A, N, sizeof N);
    }
    pv4_dot(S, A[0], (const uint32_t(*)[4])T[0]);
}

/* one record through the four kernels' arithmetic; 0 if ciphertext and tag equal the oracle's */
static int record(const unsigned char *key, int bits, const unsigned char nonce[12], const unsigned char *aad, size_t al,
                  const unsigned char *pt, size_t n, unsigned L)
{
    aes_context kgk, enc;
    unsigned char *want = malloc(n + 1), *got = malloc(n + 1), wtag[16], blk[16];
    int bad = !want || !got;
    aes_setkey_enc(&kgk, key, (unsigned)bits);
    if (!bad && aes_crypt_gcmsiv(&kgk, AES_ENCRYPT, n, nonce, aad, al, pt, want, NULL, wtag)) bad = 1;

    /* derive */
    const int nk = bits / 32, nblk = 2 + nk / 2;
    uint32_t nw[3], lo[6][2], H[4], rk[60];
    memcpy(nw, nonce, 12);
    for (int i = 0; i < nblk; ++i) {
        uint32_t b[4];
        siv_derive_block(b, nw, (uint32_t)i);
        memcpy(blk, b, 16);
        aes_crypt_ecb(&kgk, AES_ENCRYPT, blk, blk);
        memcpy(lo[i], blk, 8);
    }
    H[0] = lo[0][0], H[1] = lo[0][1], H[2] = lo[1][0], H[3] = lo[1][1];
    for (int j = 0; j < nk; ++j) rk[j] = lo[2 + j / 2][j & 1];
    siv_expand_key(rk, g_sb, nk);
    unsigned char ak[16], ek[32];
    if (aes_gcmsiv_derive(&kgk, nonce, ak, ek) != 4 * nk || memcmp(ak, H, 16) || memcmp(ek, rk, 4 * (size_t)nk)) bad = 1;
    if (aes_import_rk32(&enc, rk, nk + 6)) bad = 1;

    /* hash, finisher */
    uint32_t S[4], tag[4];
    hash_lanes(S, H, L, aad, al, pt, n);
    for (int j = 0; j < 3; ++j) S[j] ^= nw[j];
    S[3] &= 0x7FFFFFFFu;
    memcpy(blk, S, 16);
    aes_crypt_ecb(&enc, AES_ENCRYPT, blk, blk);
    memcpy(tag, blk, 16);
    if (memcmp(tag, wtag, 16)) bad = 1;

    /* the counter mode from the tag */
    for (size_t i = 0; !bad && 16 * i < n; ++i) {
        uint32_t c[4];
        unsigned char ks[16];
        siv_ctr_block(c, tag, (uint32_t)i);
        memcpy(blk, c, 16);
        aes_crypt_ecb(&enc, AES_ENCRYPT, blk, ks);
        for (size_t b = 0; b < 16 && 16 * i + b < n; ++b) got[16 * i + b] = (unsigned char)(pt[16 * i + b] ^ ks[b]);
    }
    if (!bad && n && memcmp(got, want, n)) bad = 1;
    free(want);
    free(got);
    return bad;
}

static void records(void)
{
    /* RFC 8452 appendix C.1 / C.2 shapes and the appendix A nonce, then the lengths of the GPU tests: 0, 1,
     * 15 .. 17, around the hash kernel's spans (16, 64, 256 hashed blocks; the AAD's blocks and the length
     * block count), around the counter kernel's 4 KiB tile */
    static const size_t lens[] = {0,    1,    15,   16,   17,   14 * 16,      15 * 16 - 1, 15 * 16, 15 * 16 + 1, 16 * 16,
                                  62 * 16,    63 * 16 - 1,  63 * 16,      63 * 16 + 1, 64 * 16, 254 * 16,    255 * 16 - 1,
                                  255 * 16,   255 * 16 + 1, 256 * 16,     4096 - 16,   4095,    4097,        4096 + 16,
                                  3 * 4096 + 17};
    static const size_t aads[] = {0, 13, 16, 4096};
    enum { MAXN = 3 * 4096 + 17, MAXA = 4096 };
    unsigned char *pt = malloc(MAXN + 1), *aad = malloc(MAXA + 1), key[32], nonce[12];
    if (!pt || !aad) {
        fail("no memory");
        return;
    }
    for (size_t i = 0; i < MAXN; ++i) pt[i] = (unsigned char)(i * 131 + (i >> 8) + 1);
    for (size_t i = 0; i < MAXA; ++i) aad[i] = (unsigned char)(i * 29 + 7);
    for (int bits = 128; bits <= 256; bits += 128) {
        int bad = 0, n = 0;
        for (unsigned L = 16; L <= 64; L += 48) {
            /* RFC 8452's vectors' inputs: key 01 00.., nonce 03 00.., plaintext 0 .. 64 bytes of counters, AAD 0 / 1 / 12 / 18 / 20 */
            static const size_t vp[] = {0, 8, 12, 16, 32, 48, 64, 4, 20, 18}, va[] = {0, 0, 0, 0, 0, 0, 0, 12, 18, 20};
            unsigned char vk[32] = {1}, vn[12] = {3}, vpt[64] = {0}, vaad[20] = {1};
            for (size_t v = 0; v < sizeof vp / sizeof vp[0]; ++v, ++n) {
                memset(vpt, 0, sizeof vpt);
                for (size_t b = 0; 16 * b < vp[v]; ++b) vpt[16 * b] = (unsigned char)(2 + b - (va[v] ? 0 : 1));
                bad |= record(vk, bits, vn, vaad, va[v], vpt, vp[v], L);
            }
            for (size_t li = 0; li < sizeof lens / sizeof lens[0]; ++li)
                for (size_t ai = 0; ai < sizeof aads / sizeof aads[0]; ++ai, ++n) {
                    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)rnd();
                    for (int i = 0; i < 12; ++i) nonce[i] = (unsigned char)rnd();
                    if (record(key, bits, nonce, aad, aads[ai], pt, lens[li], L)) {
                        printf("FAIL AES-%d L=%u n=%zu aad=%zu\n", bits, L, lens[li], aads[ai]);
                        bad = 1;
                    }
                }
        }
        if (bad) g_fail = 1;
        else printf("OK AES-%d %d records\n", bits, n);
    }
    free(pt);
    free(aad);
}

int main(void)
{
    make_sbox();
    if (aes_gcmsiv_self_test(0)) fail("aes_gcmsiv_self_test"); /* RFC 8452's vectors hold for the oracle itself */
    mul();
    expand();
    wrap();
    records();
    return g_fail;
}
