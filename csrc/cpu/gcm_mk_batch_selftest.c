/*
 * gcm_mk_batch_selftest.c -- the host-callable arithmetic of the many-key
 * batched AES-GCM kernels (csrc/hip/aes_gcm_mk_batch.hip) as a stand-alone
 * program, with the kernels' own functions from csrc/hip/polyval_dev.h, against
 * aes.c:
 *
 *   APPENDIX-A   RFC 8452 appendix A: GHASH under H = 25629347..757b of X_1, X_2
 *                through gmk_key, pv_rev and the nibble tables; prints the value
 *   OK ...       whole records the way the kernels cut them: a key's seven
 *                nibble tables from E_K(0^128) by squaring (k_gmk_tables), L lanes
 *                of Horner under C^L over byte-reversed blocks aligned to the
 *                record's end, the fold of log2 L steps, the last product and the
 *                reversal (k_ghash_mk_batch), tag = hash ^ E_K(J0) (k_gmk_final)
 *                -- for every key size and for L = 16 and L = 64, hashed-block
 *                counts 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257 and 1025 with
 *                AADs of 0, 1, 16 and 17 bytes -- against aes_ghash and
 *                aes_crypt_gcm.
 *
 * Prints every result; exits non-zero if a check fails.
 * tests/test_gcm_mk_batch_selftest_cpu.py builds it plain and with
 * -fsanitize=address,undefined and compares the output.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aes.h"
#include "../hip/polyval_dev.h"

static int g_fail;

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

static uint32_t g_rng = 0x2545F491u;
static uint32_t rnd(void)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

typedef uint32_t nibtab[16][4];

/* a key's table image from its GHASH key h (16 bytes): k_gmk_tables' steps */
static void image_of(nibtab T[GMK_NTAB], const unsigned char h[16])
{
    uint32_t hw[4], C[4];
    memcpy(hw, h, 16);
    gmk_key(C, hw);
    for (unsigned s = 0; s < GMK_NTAB; ++s) { /* the tables of C^(2^s), by squaring */
        for (uint32_t n = 0; n < 16; ++n) pv4_entry(T[s][n], C, n);
        if (s + 1 < GMK_NTAB) pv4_dot(C, C, (const uint32_t(*)[4])T[s]);
    }
}

/* block i of pad16(aad) || pad16(data) || [8 al]_64 [8 n]_64, byte-reversed, as the kernel's gmk_block forms it */
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
        gmk_len_block(x, al, n);
        return;
    }
    memcpy(x, b, 16);
    pv_rev(x, x);
}

/* S = GHASH of the record with L lanes on the image T: k_ghash_mk_batch's steps */
static void hash_lanes(unsigned char S[16], nibtab T[GMK_NTAB], unsigned L, const unsigned char *aad, size_t al,
                       const unsigned char *data, size_t n)
{
    const unsigned LOG = L == 16 ? 4 : 6;
    const size_t nb = (al + 15) / 16 + (n + 15) / 16 + 1, npass = (nb + L - 1) / L, pad = npass * L - nb;
    uint32_t A[64][4], Y[4];
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
        memset(N, 0, sizeof N);
        for (unsigned l = 0; l < L; ++l) {
            pv4_dot(N[l], A[l], (const uint32_t(*)[4])T[s]);
            if (l + d < L)
                for (int j = 0; j < 4; ++j) N[l][j] ^= A[l + d][j];
        }
        memcpy(A, N, sizeof N);
    }
    pv4_dot(Y, A[0], (const uint32_t(*)[4])T[0]);
    pv_rev(Y, Y);
    memcpy(S, Y, 16);
}

/* ---- APPENDIX-A ----------------------------------------------------------------- */
static void appendix_a(void)
{
    unsigned char h[16], x[32], want[16], got[16], y[16] = {0};
    aes_gcm_context g;
    nibtab T[GMK_NTAB];
    unhex("25629347589242761d31f826ba4b757b", h);
    unhex("4f4f95668c83dfb6401762bb2d01a262", x);      /* X_1 */
    unhex("d1a24ddd2721d006bbe45f20d3c9f362", x + 16); /* X_2 */
    unhex("bd9b3997046731fb96251b91f9c99d7a", want);
    memset(&g, 0, sizeof g);
    aes_gcm_set_h(&g, h);
    aes_ghash(&g, y, x, 32);
    image_of(T, h);
    /* the two blocks alone, no length block: Horner on the table of C itself */
    uint32_t A[4] = {0, 0, 0, 0}, b[4];
    for (int i = 0; i < 2; ++i) {
        memcpy(b, x + 16 * i, 16);
        pv_rev(b, b);
        for (int j = 0; j < 4; ++j) A[j] ^= b[j];
        pv4_dot(A, A, (const uint32_t(*)[4])T[0]);
    }
    pv_rev(A, A);
    memcpy(got, A, 16);
    printf("APPENDIX-A ");
    for (int i = 0; i < 16; ++i) printf("%02x", got[i]);
    printf("\n");
    if (memcmp(got, want, 16)) fail("appendix A: not RFC 8452's value");
    if (memcmp(y, want, 16)) fail("appendix A: aes_ghash disagrees with RFC 8452");
}

/* ---- whole records -------------------------------------------------------------- */
static int record(aes_gcm_context *g, nibtab T[GMK_NTAB], const unsigned char iv[12], const unsigned char *aad, size_t al,
                  const unsigned char *pt, size_t n, unsigned L)
{
    unsigned char *ct = malloc(n + 1), wtag[16], y[16] = {0}, S[16], lenb[16], j0[16], tag[16];
    int bad = !ct;
    if (!bad && aes_crypt_gcm(g, AES_ENCRYPT, n, iv, 12, aad, al, pt, ct, wtag)) bad = 1;
    if (!bad) {
        /* the oracle's hash of the same string, block by block as SP 800-38D pads it */
        aes_ghash(g, y, aad, al);
        aes_ghash(g, y, ct, n);
        const uint64_t ab = (uint64_t)al * 8, db = (uint64_t)n * 8;
        for (int i = 0; i < 8; ++i) {
            lenb[i] = (unsigned char)(ab >> (56 - 8 * i));
            lenb[8 + i] = (unsigned char)(db >> (56 - 8 * i));
        }
        aes_ghash(g, y, lenb, 16);
        hash_lanes(S, T, L, aad, al, ct, n);
        if (memcmp(S, y, 16)) bad = 1;
        /* the finisher */
        memcpy(j0, iv, 12);
        j0[12] = j0[13] = j0[14] = 0;
        j0[15] = 1;
        aes_crypt_ecb(&g->enc, AES_ENCRYPT, j0, tag);
        for (int i = 0; i < 16; ++i) tag[i] ^= S[i];
        if (memcmp(tag, wtag, 16)) bad = 1;
    }
    free(ct);
    return bad;
}

static void records(void)
{
    static const size_t blocks[] = {1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025}; /* hashed blocks */
    static const size_t aads[] = {0, 1, 16, 17};
    enum { MAXN = 1025 * 16, MAXA = 17 };
    unsigned char *pt = malloc(MAXN + 1), aad[MAXA + 1], key[32], iv[12], zero[16] = {0}, h[16];
    if (!pt) {
        fail("no memory");
        return;
    }
    for (size_t i = 0; i < MAXN; ++i) pt[i] = (unsigned char)(i * 131 + (i >> 8) + 1);
    for (size_t i = 0; i < MAXA; ++i) aad[i] = (unsigned char)(i * 29 + 7);
    for (int bits = 128; bits <= 256; bits += 64) {
        int bad = 0, cnt = 0;
        for (unsigned L = 16; L <= 64; L += 48)
            for (size_t bi = 0; bi < sizeof blocks / sizeof blocks[0]; ++bi)
                for (size_t ai = 0; ai < sizeof aads / sizeof aads[0]; ++ai) {
                    const size_t al = aads[ai], na = (al + 15) / 16;
                    if (blocks[bi] < na + 1) continue; /* the AAD's blocks and the length block count */
                    /* the data fills the rest; an odd tail where there is data, so the last data block is partial */
                    const size_t nd = blocks[bi] - na - 1, n = nd ? 16 * nd - (bi & 1 ? 3 : 0) : 0;
                    aes_gcm_context g;
                    nibtab T[GMK_NTAB];
                    for (int i = 0; i < 32; ++i) key[i] = (unsigned char)rnd();
                    for (int i = 0; i < 12; ++i) iv[i] = (unsigned char)rnd();
                    if (aes_gcm_setkey(&g, key, (unsigned)bits)) bad = 1;
                    aes_crypt_ecb(&g.enc, AES_ENCRYPT, zero, h); /* as the table kernel: H = E_K(0^128) */
                    image_of(T, h);
                    ++cnt;
                    if (record(&g, T, iv, aad, al, pt, n, L)) {
                        printf("FAIL AES-%d L=%u blocks=%zu n=%zu aad=%zu\n", bits, L, blocks[bi], n, al);
                        bad = 1;
                    }
                }
        if (bad) g_fail = 1;
        else printf("OK AES-%d %d records\n", bits, cnt);
    }
    free(pt);
}

int main(void)
{
    appendix_a();
    records();
    return g_fail;
}
