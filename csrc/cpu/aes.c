/*
 * aes.c -- CPU reference implementation of AES-128/192/256 (FIPS-197) with
 * ECB / CBC / CFB128 / CTR modes (SP 800-38A).
 *
 * Role in this framework: the correctness oracle for the gfx950 HIP kernels
 * (csrc/hip/ kernels) and the CPU baseline for the harnesses.  API parity with
 * /root/reference/aes-modes/aes.h:62-161 (see include/aes.h).
 *
 * Design notes (new code, not derived from the reference's aes.c):
 *   - all tables (S-box, inverse S-box, Te0, Td0) are computed once from the
 *     GF(2^8) definition under pthread_once (thread safe; the reference's
 *     aes_gen_tables, aes.c:361-435, was guarded by a racy flag);
 *   - the other three T tables are byte rotations of T0 (the same trick the
 *     GPU kernel uses to fit one 64 KiB replicated table in LDS);
 *   - CFB128 and the self test are always built (reference: compiled out).
 */
#include "aes.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>

/* ---------------------------------------------------------------------------
 * Table generation
 * ------------------------------------------------------------------------- */
static uint8_t  g_sbox[256];
static uint8_t  g_isbox[256];
static uint32_t g_te0[256];
static uint32_t g_td0[256];
static uint32_t g_rcon[10];
static pthread_once_t g_once = PTHREAD_ONCE_INIT;

static inline uint32_t rotl32(uint32_t x, int n) { return (x << (n & 31)) | (x >> ((32 - n) & 31)); }
static inline uint8_t xt(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0x00)); }

static uint8_t gf_mul(uint8_t a, uint8_t b)
{
    uint8_t r = 0;
    while (b) {
        if (b & 1) r ^= a;
        a = xt(a);
        b >>= 1;
    }
    return r;
}

static void build_tables(void)
{
    uint8_t ex[256], lg[256];
    uint8_t v = 1;
    for (int i = 0; i < 255; ++i) {      /* generator 0x03 */
        ex[i] = v;
        lg[v] = (uint8_t)i;
        v = (uint8_t)(v ^ xt(v));
    }
    for (int a = 0; a < 256; ++a) {
        uint8_t inv = a ? ex[(255 - lg[a]) % 255] : 0;
        uint8_t s = inv;
        uint8_t r = inv;
        for (int k = 0; k < 4; ++k) {    /* affine map: b ^ rotl1..4(b) ^ 0x63 */
            r = (uint8_t)((r << 1) | (r >> 7));
            s ^= r;
        }
        s ^= 0x63;
        g_sbox[a] = s;
        g_isbox[s] = (uint8_t)a;
    }
    for (int a = 0; a < 256; ++a) {
        uint8_t s = g_sbox[a];
        g_te0[a] = (uint32_t)gf_mul(s, 2) | ((uint32_t)s << 8) | ((uint32_t)s << 16) |
                   ((uint32_t)gf_mul(s, 3) << 24);
        uint8_t t = g_isbox[a];
        g_td0[a] = (uint32_t)gf_mul(t, 14) | ((uint32_t)gf_mul(t, 9) << 8) |
                   ((uint32_t)gf_mul(t, 13) << 16) | ((uint32_t)gf_mul(t, 11) << 24);
    }
    uint8_t rc = 1;
    for (int i = 0; i < 10; ++i) {
        g_rcon[i] = rc;
        rc = xt(rc);
    }
}

static inline void ensure_tables(void) { pthread_once(&g_once, build_tables); }

const uint8_t *aes_sbox(void) { ensure_tables(); return g_sbox; }
const uint8_t *aes_inv_sbox(void) { ensure_tables(); return g_isbox; }
const uint32_t *aes_te0(void) { ensure_tables(); return g_te0; }
const uint32_t *aes_td0(void) { ensure_tables(); return g_td0; }

#define B0(x) ((x) & 0xff)
#define B1(x) (((x) >> 8) & 0xff)
#define B2(x) (((x) >> 16) & 0xff)
#define B3(x) ((x) >> 24)
#define TE(r, x) rotl32(g_te0[x], 8 * (r))
#define TD(r, x) rotl32(g_td0[x], 8 * (r))

static inline uint32_t load_le32(const unsigned char *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static inline void store_le32(unsigned char *p, uint32_t v)
{
    p[0] = (unsigned char)v;
    p[1] = (unsigned char)(v >> 8);
    p[2] = (unsigned char)(v >> 16);
    p[3] = (unsigned char)(v >> 24);
}

/* ---------------------------------------------------------------------------
 * Key schedule
 * ------------------------------------------------------------------------- */
static int expand_key(uint32_t *w, const unsigned char *key, unsigned int keysize, int *nr)
{
    int nk;
    switch (keysize) {
    case 128: nk = 4; *nr = 10; break;
    case 192: nk = 6; *nr = 12; break;
    case 256: nk = 8; *nr = 14; break;
    default: return POLARSSL_ERR_AES_INVALID_KEY_LENGTH;
    }
    int total = 4 * (*nr + 1);
    for (int i = 0; i < nk; ++i) w[i] = load_le32(key + 4 * i);
    for (int i = nk; i < total; ++i) {
        uint32_t t = w[i - 1];
        if (i % nk == 0) {
            t = (t >> 8) | (t << 24); /* RotWord on LE words */
            t = (uint32_t)g_sbox[B0(t)] | ((uint32_t)g_sbox[B1(t)] << 8) |
                ((uint32_t)g_sbox[B2(t)] << 16) | ((uint32_t)g_sbox[B3(t)] << 24);
            t ^= g_rcon[i / nk - 1];
        } else if (nk > 6 && i % nk == 4) {
            t = (uint32_t)g_sbox[B0(t)] | ((uint32_t)g_sbox[B1(t)] << 8) |
                ((uint32_t)g_sbox[B2(t)] << 16) | ((uint32_t)g_sbox[B3(t)] << 24);
        }
        w[i] = w[i - nk] ^ t;
    }
    return 0;
}

int aes_setkey_enc(aes_context *ctx, const unsigned char *key, unsigned int keysize)
{
    uint32_t w[60];
    ensure_tables();
    int ret = expand_key(w, key, keysize, &ctx->nr);
    if (ret) return ret;
    ctx->rk = ctx->buf;
    for (int i = 0; i < 4 * (ctx->nr + 1); ++i) ctx->buf[i] = w[i];
    return 0;
}

static inline uint32_t inv_mix_word(uint32_t x)
{
    /* Td includes the inverse S-box, so feed S-box(x) to cancel it. */
    return TD(0, g_sbox[B0(x)]) ^ TD(1, g_sbox[B1(x)]) ^ TD(2, g_sbox[B2(x)]) ^ TD(3, g_sbox[B3(x)]);
}

int aes_setkey_dec(aes_context *ctx, const unsigned char *key, unsigned int keysize)
{
    uint32_t w[60];
    ensure_tables();
    int nr;
    int ret = expand_key(w, key, keysize, &nr);
    if (ret) return ret;
    ctx->nr = nr;
    ctx->rk = ctx->buf;
    /* equivalent inverse cipher: reversed round keys, InvMixColumns on the
     * inner ones */
    for (int r = 0; r <= nr; ++r) {
        for (int c = 0; c < 4; ++c) {
            uint32_t k = w[4 * (nr - r) + c];
            ctx->buf[4 * r + c] = (r == 0 || r == nr) ? k : inv_mix_word(k);
        }
    }
    return 0;
}

int aes_export_rk32(const aes_context *ctx, uint32_t *out)
{
    int n = 4 * (ctx->nr + 1);
    for (int i = 0; i < n; ++i) out[i] = (uint32_t)ctx->rk[i];
    return n;
}

int aes_import_rk32(aes_context *ctx, const uint32_t *rk, int nr)
{
    if (nr != 10 && nr != 12 && nr != 14) return POLARSSL_ERR_AES_INVALID_KEY_LENGTH;
    ensure_tables();
    ctx->nr = nr;
    ctx->rk = ctx->buf;
    for (int i = 0; i < 4 * (nr + 1); ++i) ctx->buf[i] = rk[i];
    return 0;
}

/* ---------------------------------------------------------------------------
 * Block functions
 * ------------------------------------------------------------------------- */
static void encrypt_block(const aes_context *ctx, const unsigned char in[16], unsigned char out[16])
{
    const unsigned long *rk = ctx->rk;
    uint32_t s0 = load_le32(in) ^ (uint32_t)rk[0];
    uint32_t s1 = load_le32(in + 4) ^ (uint32_t)rk[1];
    uint32_t s2 = load_le32(in + 8) ^ (uint32_t)rk[2];
    uint32_t s3 = load_le32(in + 12) ^ (uint32_t)rk[3];
    for (int r = 1; r < ctx->nr; ++r) {
        rk += 4;
        uint32_t t0 = TE(0, B0(s0)) ^ TE(1, B1(s1)) ^ TE(2, B2(s2)) ^ TE(3, B3(s3)) ^ (uint32_t)rk[0];
        uint32_t t1 = TE(0, B0(s1)) ^ TE(1, B1(s2)) ^ TE(2, B2(s3)) ^ TE(3, B3(s0)) ^ (uint32_t)rk[1];
        uint32_t t2 = TE(0, B0(s2)) ^ TE(1, B1(s3)) ^ TE(2, B2(s0)) ^ TE(3, B3(s1)) ^ (uint32_t)rk[2];
        uint32_t t3 = TE(0, B0(s3)) ^ TE(1, B1(s0)) ^ TE(2, B2(s1)) ^ TE(3, B3(s2)) ^ (uint32_t)rk[3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    rk += 4;
#define FINAL_E(a, b, c, d) ((uint32_t)g_sbox[B0(a)] | ((uint32_t)g_sbox[B1(b)] << 8) | \
                             ((uint32_t)g_sbox[B2(c)] << 16) | ((uint32_t)g_sbox[B3(d)] << 24))
    store_le32(out, FINAL_E(s0, s1, s2, s3) ^ (uint32_t)rk[0]);
    store_le32(out + 4, FINAL_E(s1, s2, s3, s0) ^ (uint32_t)rk[1]);
    store_le32(out + 8, FINAL_E(s2, s3, s0, s1) ^ (uint32_t)rk[2]);
    store_le32(out + 12, FINAL_E(s3, s0, s1, s2) ^ (uint32_t)rk[3]);
#undef FINAL_E
}

static void decrypt_block(const aes_context *ctx, const unsigned char in[16], unsigned char out[16])
{
    const unsigned long *rk = ctx->rk;
    uint32_t s0 = load_le32(in) ^ (uint32_t)rk[0];
    uint32_t s1 = load_le32(in + 4) ^ (uint32_t)rk[1];
    uint32_t s2 = load_le32(in + 8) ^ (uint32_t)rk[2];
    uint32_t s3 = load_le32(in + 12) ^ (uint32_t)rk[3];
    for (int r = 1; r < ctx->nr; ++r) {
        rk += 4;
        uint32_t t0 = TD(0, B0(s0)) ^ TD(1, B1(s3)) ^ TD(2, B2(s2)) ^ TD(3, B3(s1)) ^ (uint32_t)rk[0];
        uint32_t t1 = TD(0, B0(s1)) ^ TD(1, B1(s0)) ^ TD(2, B2(s3)) ^ TD(3, B3(s2)) ^ (uint32_t)rk[1];
        uint32_t t2 = TD(0, B0(s2)) ^ TD(1, B1(s1)) ^ TD(2, B2(s0)) ^ TD(3, B3(s3)) ^ (uint32_t)rk[2];
        uint32_t t3 = TD(0, B0(s3)) ^ TD(1, B1(s2)) ^ TD(2, B2(s1)) ^ TD(3, B3(s0)) ^ (uint32_t)rk[3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    rk += 4;
#define FINAL_D(a, b, c, d) ((uint32_t)g_isbox[B0(a)] | ((uint32_t)g_isbox[B1(b)] << 8) | \
                             ((uint32_t)g_isbox[B2(c)] << 16) | ((uint32_t)g_isbox[B3(d)] << 24))
    store_le32(out, FINAL_D(s0, s3, s2, s1) ^ (uint32_t)rk[0]);
    store_le32(out + 4, FINAL_D(s1, s0, s3, s2) ^ (uint32_t)rk[1]);
    store_le32(out + 8, FINAL_D(s2, s1, s0, s3) ^ (uint32_t)rk[2]);
    store_le32(out + 12, FINAL_D(s3, s2, s1, s0) ^ (uint32_t)rk[3]);
#undef FINAL_D
}

int aes_crypt_ecb(aes_context *ctx, int mode, const unsigned char input[16], unsigned char output[16])
{
    if (mode == AES_ENCRYPT)
        encrypt_block(ctx, input, output);
    else
        decrypt_block(ctx, input, output);
    return 0;
}

/* ---------------------------------------------------------------------------
 * Modes of operation
 * ------------------------------------------------------------------------- */
int aes_crypt_cbc(aes_context *ctx, int mode, size_t length, unsigned char iv[16],
                  const unsigned char *input, unsigned char *output)
{
    if (length % 16) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    unsigned char tmp[16];
    if (mode == AES_DECRYPT) {
        for (; length; length -= 16, input += 16, output += 16) {
            memcpy(tmp, input, 16);
            decrypt_block(ctx, input, output);
            for (int i = 0; i < 16; ++i) output[i] ^= iv[i];
            memcpy(iv, tmp, 16);
        }
    } else {
        for (; length; length -= 16, input += 16, output += 16) {
            for (int i = 0; i < 16; ++i) tmp[i] = input[i] ^ iv[i];
            encrypt_block(ctx, tmp, output);
            memcpy(iv, output, 16);
        }
    }
    return 0;
}

int aes_crypt_cfb128(aes_context *ctx, int mode, size_t length, int *iv_off,
                     unsigned char iv[16], const unsigned char *input, unsigned char *output)
{
    int n = *iv_off & 15;
    for (size_t i = 0; i < length; ++i) {
        if (n == 0) encrypt_block(ctx, iv, iv);
        unsigned char c;
        if (mode == AES_DECRYPT) {
            c = input[i];
            output[i] = (unsigned char)(c ^ iv[n]);
            iv[n] = c;
        } else {
            c = (unsigned char)(input[i] ^ iv[n]);
            output[i] = c;
            iv[n] = c;
        }
        n = (n + 1) & 15;
    }
    *iv_off = n;
    return 0;
}

void aes_ctr128_add(unsigned char ctr[16], uint64_t blocks)
{
    uint64_t carry = blocks;
    for (int i = 15; i >= 0 && carry; --i) {
        uint64_t v = (uint64_t)ctr[i] + (carry & 0xff);
        ctr[i] = (unsigned char)v;
        carry = (carry >> 8) + (v >> 8);
    }
}

int aes_crypt_ctr(aes_context *ctx, int length, int *nc_off, unsigned char nonce_counter[16],
                  unsigned char stream_block[16], const unsigned char *input, unsigned char *output)
{
    int n = *nc_off & 15;
    for (int i = 0; i < length; ++i) {
        if (n == 0) {
            encrypt_block(ctx, nonce_counter, stream_block);
            aes_ctr128_add(nonce_counter, 1);
        }
        output[i] = (unsigned char)(input[i] ^ stream_block[n]);
        n = (n + 1) & 15;
    }
    *nc_off = n;
    return 0;
}

/* ---------------------------------------------------------------------------
 * Multi-threaded bulk helpers (CPU baseline; remainders are NOT dropped and
 * every shard gets its own counter offset -- the reference's harness reused
 * one keystream across threads, aes-modes/test.c:282)
 * ------------------------------------------------------------------------- */
typedef struct {
    const aes_context *ctx;
    int mode;              /* AES_ENCRYPT / AES_DECRYPT for ECB, 2 for CTR */
    unsigned char ctr[16];
    const unsigned char *in;
    unsigned char *out;
    size_t len;
} bulk_job;

static void *bulk_worker(void *arg)
{
    bulk_job *j = (bulk_job *)arg;
    if (j->mode == 2) {
        unsigned char ks[16];
        size_t off = 0;
        while (off < j->len) {
            encrypt_block(j->ctx, j->ctr, ks);
            aes_ctr128_add(j->ctr, 1);
            size_t n = j->len - off < 16 ? j->len - off : 16;
            for (size_t i = 0; i < n; ++i) j->out[off + i] = (unsigned char)(j->in[off + i] ^ ks[i]);
            off += n;
        }
    } else {
        for (size_t off = 0; off + 16 <= j->len; off += 16) {
            if (j->mode == AES_ENCRYPT)
                encrypt_block(j->ctx, j->in + off, j->out + off);
            else
                decrypt_block(j->ctx, j->in + off, j->out + off);
        }
    }
    return NULL;
}

static int run_bulk(const aes_context *ctx, int mode, const unsigned char *nc,
                    const unsigned char *in, unsigned char *out, size_t len, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    size_t nblocks = (len + 15) / 16;
    if ((size_t)nthreads > nblocks && nblocks > 0) nthreads = (int)nblocks;
    bulk_job jobs[256];
    pthread_t th[256];
    size_t per = nblocks / (size_t)nthreads, extra = nblocks % (size_t)nthreads;
    size_t blk = 0;
    for (int t = 0; t < nthreads; ++t) {
        size_t nb = per + ((size_t)t < extra ? 1 : 0);
        bulk_job *j = &jobs[t];
        j->ctx = ctx;
        j->mode = mode;
        if (nc) {
            memcpy(j->ctr, nc, 16);
            aes_ctr128_add(j->ctr, blk);
        }
        size_t start = blk * 16;
        size_t end = (blk + nb) * 16;
        if (end > len) end = len;
        j->in = in + start;
        j->out = out + start;
        j->len = end > start ? end - start : 0;
        blk += nb;
    }
    if (nthreads == 1) {
        bulk_worker(&jobs[0]);
        return 0;
    }
    for (int t = 0; t < nthreads; ++t) pthread_create(&th[t], NULL, bulk_worker, &jobs[t]);
    for (int t = 0; t < nthreads; ++t) pthread_join(th[t], NULL);
    return 0;
}

int aes_ctr_bulk(const aes_context *ctx, const unsigned char nonce_counter[16],
                 const unsigned char *input, unsigned char *output, size_t length, int nthreads)
{
    return run_bulk(ctx, 2, nonce_counter, input, output, length, nthreads);
}

int aes_ecb_bulk(const aes_context *ctx, int mode, const unsigned char *input,
                 unsigned char *output, size_t length, int nthreads)
{
    if (length % 16) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    return run_bulk(ctx, mode, NULL, input, output, length, nthreads);
}

/* ---------------------------------------------------------------------------
 * XTS-AES (IEEE 1619 / SP 800-38E), written from the standard's definition:
 * T_0 = E_K2(data unit number as a 128-bit little-endian block), T_{j+1} =
 * T_j * alpha in GF(2^128) (x^128 + x^7 + x^2 + x + 1, T read as a
 * little-endian integer), C_j = E_K1(P_j ^ T_j) ^ T_j, ciphertext stealing
 * for a last block of 1..15 bytes.  In place (input == output) is exact:
 * every block is read before it is written.
 * ------------------------------------------------------------------------- */
int aes_xts_setkey_enc(aes_xts_context *ctx, const unsigned char *key, unsigned int keybits)
{
    if (keybits != 256 && keybits != 512) return POLARSSL_ERR_AES_INVALID_KEY_LENGTH;
    int r = aes_setkey_enc(&ctx->crypt, key, keybits / 2);
    return r ? r : aes_setkey_enc(&ctx->tweak, key + keybits / 16, keybits / 2);
}

int aes_xts_setkey_dec(aes_xts_context *ctx, const unsigned char *key, unsigned int keybits)
{
    if (keybits != 256 && keybits != 512) return POLARSSL_ERR_AES_INVALID_KEY_LENGTH;
    int r = aes_setkey_dec(&ctx->crypt, key, keybits / 2);
    return r ? r : aes_setkey_enc(&ctx->tweak, key + keybits / 16, keybits / 2); /* always encrypts */
}

/* T *= alpha: shift the little-endian integer left one bit, fold the carry */
static void xts_mul_alpha(unsigned char t[16])
{
    unsigned carry = 0;
    for (int i = 0; i < 16; ++i) {
        const unsigned v = ((unsigned)t[i] << 1) | carry;
        carry = t[i] >> 7;
        t[i] = (unsigned char)v;
    }
    if (carry) t[0] ^= 0x87;
}

static void xts_block(const aes_context *k1, int mode, const unsigned char t[16], const unsigned char in[16],
                      unsigned char out[16])
{
    unsigned char x[16];
    for (int i = 0; i < 16; ++i) x[i] = (unsigned char)(in[i] ^ t[i]);
    if (mode == AES_ENCRYPT)
        encrypt_block(k1, x, x);
    else
        decrypt_block(k1, x, x);
    for (int i = 0; i < 16; ++i) out[i] = (unsigned char)(x[i] ^ t[i]);
}

int aes_crypt_xts(aes_xts_context *ctx, int mode, size_t length, const unsigned char data_unit[16],
                  const unsigned char *input, unsigned char *output)
{
    if (length < 16 || length > ((size_t)1 << 24)) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    const size_t m = length / 16, r = length % 16;
    unsigned char t[16];
    encrypt_block(&ctx->tweak, data_unit, t);
    const size_t plain = r ? m - 1 : m; /* blocks before the stolen pair */
    for (size_t j = 0; j < plain; ++j) {
        xts_block(&ctx->crypt, mode, t, input + 16 * j, output + 16 * j);
        xts_mul_alpha(t);
    }
    if (r) {
        /* t = T_{m-1}, t1 = T_m; decryption uses them in the other order */
        unsigned char t1[16], cc[16], last[16];
        memcpy(t1, t, 16);
        xts_mul_alpha(t1);
        const unsigned char *in_full = input + 16 * (m - 1), *in_part = input + 16 * m;
        xts_block(&ctx->crypt, mode, mode == AES_ENCRYPT ? t : t1, in_full, cc);
        memcpy(last, in_part, r);
        memcpy(last + r, cc + r, 16 - r);
        xts_block(&ctx->crypt, mode, mode == AES_ENCRYPT ? t1 : t, last, last);
        memcpy(output + 16 * m, cc, r);
        memcpy(output + 16 * (m - 1), last, 16);
    }
    return 0;
}

/* tweak number + n as a 128-bit little-endian integer (wraps at 2^128) */
static void xts_tweak_add(unsigned char t[16], uint64_t n)
{
    uint64_t carry = n;
    for (int i = 0; i < 16 && carry; ++i) {
        const uint64_t v = (uint64_t)t[i] + (carry & 0xff);
        t[i] = (unsigned char)v;
        carry = (carry >> 8) + (v >> 8);
    }
}

typedef struct {
    aes_xts_context *ctx;
    int mode;
    size_t unit_bytes, first, count;
    const unsigned char *tweak0, *in;
    unsigned char *out;
} xts_job;

static void *xts_worker(void *arg)
{
    xts_job *j = (xts_job *)arg;
    for (size_t u = j->first; u < j->first + j->count; ++u) {
        unsigned char du[16];
        memcpy(du, j->tweak0, 16);
        xts_tweak_add(du, (uint64_t)u);
        aes_crypt_xts(j->ctx, j->mode, j->unit_bytes, du, j->in + u * j->unit_bytes, j->out + u * j->unit_bytes);
    }
    return NULL;
}

int aes_crypt_xts_units(aes_xts_context *ctx, int mode, size_t unit_bytes, size_t nunits,
                        const unsigned char tweak0[16], const unsigned char *input, unsigned char *output)
{
    if (unit_bytes < 16 || unit_bytes > ((size_t)1 << 24)) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    if (nunits > 1 && unit_bytes % 16) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    /* units are independent: large calls (the device tests' oracle) run on
     * up to 8 threads */
    enum { MAXT = 8 };
    size_t nt = unit_bytes * nunits >= ((size_t)4 << 20) ? MAXT : 1;
    if (nt > nunits) nt = nunits ? nunits : 1;
    xts_job jobs[MAXT];
    pthread_t th[MAXT];
    size_t first = 0;
    for (size_t t = 0; t < nt; ++t) {
        const size_t count = nunits / nt + (t < nunits % nt ? 1 : 0);
        jobs[t] = (xts_job){ctx, mode, unit_bytes, first, count, tweak0, input, output};
        first += count;
    }
    for (size_t t = 1; t < nt; ++t) pthread_create(&th[t], NULL, xts_worker, &jobs[t]);
    xts_worker(&jobs[0]);
    for (size_t t = 1; t < nt; ++t) pthread_join(th[t], NULL);
    return 0;
}

/* ---------------------------------------------------------------------------
 * AES-GCM (NIST SP 800-38D), written from the standard.  A block is an
 * element of GF(2^128) with its LEFTMOST bit (bit 7 of byte 0) the coefficient
 * of x^0, so "times x" is a one-bit right shift of the 16-byte string, and a
 * bit shifted out of byte 15 is folded back as R = 0xE1 || 0^120.
 * GHASH's multiplications by H go through positional tables: tab[p][n] is
 * (nibble n at nibble position p, everything else zero) . H, each a sum of the
 * products H . x^i, and X . H the sum of 32 entries with no reduction step.
 * The device tables (csrc/hip/aes_gcm.hip) are the byte form of the same.
 * ------------------------------------------------------------------------- */
static void gf128_mulx(unsigned char v[16])
{
    const unsigned carry = v[15] & 1u;
    for (int i = 15; i > 0; --i) v[i] = (unsigned char)((v[i] >> 1) | (v[i - 1] << 7));
    v[0] >>= 1;
    if (carry) v[0] ^= 0xE1;
}

void aes_gf128_mul(unsigned char z[16], const unsigned char x[16], const unsigned char y[16])
{
    unsigned char v[16], acc[16] = {0};
    memcpy(v, y, 16);
    for (int i = 0; i < 128; ++i) {
        if (x[i / 8] & (0x80u >> (i % 8)))
            for (int j = 0; j < 16; ++j) acc[j] ^= v[j];
        gf128_mulx(v);
    }
    memcpy(z, acc, 16);
}

void aes_gcm_set_h(aes_gcm_context *ctx, const unsigned char h[16])
{
    unsigned char p[128][16]; /* H . x^i */
    memcpy(ctx->h, h, 16);
    memcpy(p[0], h, 16);
    for (int i = 1; i < 128; ++i) {
        memcpy(p[i], p[i - 1], 16);
        gf128_mulx(p[i]);
    }
    for (int pos = 0; pos < 32; ++pos)
        for (int n = 0; n < 16; ++n) {
            unsigned char e[16] = {0};
            for (int k = 0; k < 4; ++k) /* the nibble's leftmost bit is the lowest power */
                if (n & (8 >> k))
                    for (int j = 0; j < 16; ++j) e[j] ^= p[4 * pos + k][j];
            memcpy(ctx->tab[pos][n], e, 16);
        }
}

int aes_gcm_setkey(aes_gcm_context *ctx, const unsigned char *key, unsigned int keybits)
{
    const int r = aes_setkey_enc(&ctx->enc, key, keybits);
    if (r) return r;
    unsigned char h[16] = {0};
    /* this copy's tables: in a process that holds two copies of this file
     * (libotc.so loaded globally, then libotc_cpu.so) the call above may have
     * run in the other one, and encrypt_block is this one's */
    ensure_tables();
    encrypt_block(&ctx->enc, h, h);
    aes_gcm_set_h(ctx, h);
    return 0;
}

/* y = y . H */
static void ghash_mul_h(const aes_gcm_context *ctx, unsigned char y[16])
{
    uint64_t a = 0, b = 0;
    for (int i = 0; i < 16; ++i) {
        const uint64_t *hi = ctx->tab[2 * i][y[i] >> 4], *lo = ctx->tab[2 * i + 1][y[i] & 15];
        a ^= hi[0] ^ lo[0];
        b ^= hi[1] ^ lo[1];
    }
    memcpy(y, &a, 8);
    memcpy(y + 8, &b, 8);
}

static void ghash_serial(const aes_gcm_context *ctx, unsigned char y[16], const unsigned char *data, size_t len)
{
    while (len) {
        const size_t n = len < 16 ? len : 16;
        for (size_t i = 0; i < n; ++i) y[i] ^= data[i];
        ghash_mul_h(ctx, y);
        data += n;
        len -= n;
    }
}

typedef struct {
    const aes_gcm_context *ctx;
    const unsigned char *data;
    size_t len;
    unsigned char y[16];
} ghash_job;

static void *ghash_worker(void *arg)
{
    ghash_job *j = (ghash_job *)arg;
    ghash_serial(j->ctx, j->y, j->data, j->len);
    return NULL;
}

/* Large calls (the device tests' oracle) hash T pieces of whole blocks on T
 * threads, piece 0 from y and the others from 0, and join them as
 * Y = sum P_t . H^(blocks after piece t).  mul is the product that ctx's
 * tables are of: GHASH's, or POLYVAL's dot. */
typedef void (*hash_mul_fn)(unsigned char z[16], const unsigned char x[16], const unsigned char y[16]);

static void hash_threaded(const aes_gcm_context *ctx, hash_mul_fn mul, unsigned char y[16], const unsigned char *data,
                          size_t len)
{
    enum { MAXT = 8 };
    if (len < ((size_t)4 << 20)) {
        ghash_serial(ctx, y, data, len);
        return;
    }
    const size_t nblocks = (len + 15) / 16, per = nblocks / MAXT;
    ghash_job jobs[MAXT];
    pthread_t th[MAXT];
    for (size_t t = 0; t < MAXT; ++t) {
        const size_t first = t * per, end = t + 1 == MAXT ? nblocks : first + per;
        jobs[t].ctx = ctx;
        jobs[t].data = data + 16 * first;
        jobs[t].len = t + 1 == MAXT ? len - 16 * first : 16 * (end - first);
        memset(jobs[t].y, 0, 16);
    }
    memcpy(jobs[0].y, y, 16);
    for (size_t t = 1; t < MAXT; ++t) pthread_create(&th[t], NULL, ghash_worker, &jobs[t]);
    ghash_worker(&jobs[0]);
    for (size_t t = 1; t < MAXT; ++t) pthread_join(th[t], NULL);
    memset(y, 0, 16);
    for (size_t t = 0; t < MAXT; ++t) {
        /* H^after by square and multiply; after == 0 leaves the piece as it is */
        size_t after = t + 1 == MAXT ? 0 : nblocks - (t + 1) * per;
        unsigned char p[16], sq[16];
        memcpy(p, jobs[t].y, 16);
        memcpy(sq, ctx->h, 16);
        for (; after; after >>= 1) {
            if (after & 1) mul(p, p, sq);
            mul(sq, sq, sq);
        }
        for (int i = 0; i < 16; ++i) y[i] ^= p[i];
    }
}

void aes_ghash(const aes_gcm_context *ctx, unsigned char y[16], const unsigned char *data, size_t len)
{
    hash_threaded(ctx, aes_gf128_mul, y, data, len);
}

static void gcm_inc32(unsigned char ctr[16])
{
    for (int i = 15; i >= 12; --i)
        if (++ctr[i]) break;
}

int aes_crypt_ctr32(aes_gcm_context *ctx, size_t length, unsigned char ctr[16], const unsigned char *input,
                    unsigned char *output)
{
    unsigned char ks[16];
    ensure_tables();
    while (length) {
        const size_t n = length < 16 ? length : 16;
        encrypt_block(&ctx->enc, ctr, ks);
        gcm_inc32(ctr);
        for (size_t i = 0; i < n; ++i) output[i] = (unsigned char)(input[i] ^ ks[i]);
        input += n;
        output += n;
        length -= n;
    }
    return 0;
}

static void gcm_put64(unsigned char *p, uint64_t v)
{
    for (int i = 0; i < 8; ++i) p[i] = (unsigned char)(v >> (56 - 8 * i));
}

void aes_gcm_j0(const aes_gcm_context *ctx, const unsigned char *iv, size_t iv_len, unsigned char j0[16])
{
    memset(j0, 0, 16);
    if (iv_len == 12) {
        memcpy(j0, iv, 12);
        j0[15] = 1;
        return;
    }
    unsigned char lb[16] = {0};
    gcm_put64(lb + 8, (uint64_t)iv_len * 8);
    aes_ghash(ctx, j0, iv, iv_len);
    aes_ghash(ctx, j0, lb, 16);
}

int aes_crypt_gcm(aes_gcm_context *ctx, int mode, size_t length, const unsigned char *iv, size_t iv_len,
                  const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                  unsigned char tag[16])
{
    if (iv_len == 0 || (uint64_t)length > AES_GCM_MAX_BYTES || (uint64_t)aad_len >> 61 || (uint64_t)iv_len >> 61)
        return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    unsigned char j0[16], ekj0[16], ctr[16], y[16] = {0}, lb[16];
    ensure_tables();
    aes_gcm_j0(ctx, iv, iv_len, j0);
    encrypt_block(&ctx->enc, j0, ekj0);
    memcpy(ctr, j0, 16);
    gcm_inc32(ctr);
    aes_ghash(ctx, y, aad, aad_len);
    /* the hash is over the ciphertext: before decrypting it, after producing
     * it, so that input == output works in both directions */
    if (mode == AES_DECRYPT) aes_ghash(ctx, y, input, length);
    aes_crypt_ctr32(ctx, length, ctr, input, output);
    if (mode != AES_DECRYPT) aes_ghash(ctx, y, output, length);
    gcm_put64(lb, (uint64_t)aad_len * 8);
    gcm_put64(lb + 8, (uint64_t)length * 8);
    aes_ghash(ctx, y, lb, 16);
    for (int i = 0; i < 16; ++i) tag[i] = (unsigned char)(y[i] ^ ekj0[i]);
    return 0;
}

int aes_gcm_auth_decrypt(aes_gcm_context *ctx, size_t length, const unsigned char *iv, size_t iv_len,
                         const unsigned char *aad, size_t aad_len, const unsigned char *tag, size_t tag_len,
                         const unsigned char *input, unsigned char *output)
{
    if (tag_len < 4 || tag_len > 16) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    unsigned char t[16];
    const int r = aes_crypt_gcm(ctx, AES_DECRYPT, length, iv, iv_len, aad, aad_len, input, output, t);
    if (r) return r;
    unsigned diff = 0; /* every byte compared, whatever the earlier ones gave */
    for (size_t i = 0; i < tag_len; ++i) diff |= (unsigned)(t[i] ^ tag[i]);
    if (diff) {
        memset(output, 0, length);
        return POLARSSL_ERR_GCM_AUTH_FAILED;
    }
    return 0;
}

/* ---------------------------------------------------------------------------
 * AES-GCM-SIV (RFC 8452), written from the RFC.  POLYVAL's field is
 * x^128 + x^127 + x^126 + x^121 + 1 and a block is a LITTLE-endian 128-bit
 * number: bit 0 of byte 0 is the coefficient of x^0, "times x" is a one-bit
 * left shift of that number, and a bit shifted out of byte 15 is folded back
 * as x^127 + x^126 + x^121 + 1 (0xC2 into byte 15, 0x01 into byte 0).  The
 * product is dot(a, b) = a . b . x^-128.  Y . H goes through the same
 * positional nibble tables as GHASH's (aes_gcm_context.tab, ghash_mul_h):
 * tab[p][n] = dot(nibble n at nibble position p, H), each a sum of the
 * products H . x^(i - 128); only the doubling and the bit order differ.
 * ------------------------------------------------------------------------- */
static void polyval_mulx(unsigned char v[16])
{
    const unsigned carry = v[15] >> 7;
    for (int i = 15; i > 0; --i) v[i] = (unsigned char)((v[i] << 1) | (v[i - 1] >> 7));
    v[0] = (unsigned char)(v[0] << 1);
    if (carry) {
        v[15] ^= 0xC2;
        v[0] ^= 0x01;
    }
}

void aes_polyval_dot(unsigned char z[16], const unsigned char x[16], const unsigned char y[16])
{
    unsigned char acc[16] = {0};
    /* bit i of x adds y . x^i; every step divides by x, 128 times in all */
    for (int i = 0; i < 128; ++i) {
        if (x[i / 8] & (1u << (i % 8)))
            for (int j = 0; j < 16; ++j) acc[j] ^= y[j];
        const unsigned low = acc[0] & 1u;
        for (int j = 0; j < 15; ++j) acc[j] = (unsigned char)((acc[j] >> 1) | (acc[j + 1] << 7));
        acc[15] >>= 1;
        if (low) acc[15] ^= 0xE1; /* x^-1 = x^127 + x^126 + x^125 + x^120 */
    }
    memcpy(z, acc, 16);
}

/* ctx->tab for Y -> dot(Y, h); ctx->enc is left alone */
static void polyval_set_h(aes_gcm_context *ctx, const unsigned char h[16])
{
    static const unsigned char one[16] = {1};
    unsigned char p[128][16]; /* dot(x^i, H) = H . x^(i - 128) */
    memcpy(ctx->h, h, 16);
    aes_polyval_dot(p[0], h, one);
    for (int i = 1; i < 128; ++i) {
        memcpy(p[i], p[i - 1], 16);
        polyval_mulx(p[i]);
    }
    for (int pos = 0; pos < 32; ++pos)
        for (int n = 0; n < 16; ++n) {
            /* nibble position 2 i is byte i's high nibble: powers 8 i + 4 .. 8 i + 7 */
            const int base = 8 * (pos / 2) + (pos % 2 ? 0 : 4);
            unsigned char e[16] = {0};
            for (int k = 0; k < 4; ++k) /* the nibble's lowest bit is the lowest power */
                if (n & (1 << k))
                    for (int j = 0; j < 16; ++j) e[j] ^= p[base + k][j];
            memcpy(ctx->tab[pos][n], e, 16);
        }
}

void aes_polyval(const unsigned char h[16], unsigned char y[16], const unsigned char *data, size_t len)
{
    aes_gcm_context ctx;
    polyval_set_h(&ctx, h);
    hash_threaded(&ctx, aes_polyval_dot, y, data, len);
}

int aes_gcmsiv_derive(aes_context *kgk, const unsigned char nonce[12], unsigned char authkey[16],
                      unsigned char enckey[32])
{
    if (kgk->nr != 10 && kgk->nr != 14) return POLARSSL_ERR_AES_INVALID_KEY_LENGTH;
    const int enc_bytes = kgk->nr == 10 ? 16 : 32;
    unsigned char in[16] = {0}, blk[16];
    ensure_tables();
    memcpy(in + 4, nonce, 12);
    for (int i = 0; i < 2 + enc_bytes / 8; ++i) {
        in[0] = (unsigned char)i; /* le32(i), i <= 5 */
        encrypt_block(kgk, in, blk);
        memcpy(i < 2 ? authkey + 8 * i : enckey + 8 * (i - 2), blk, 8);
    }
    return enc_bytes;
}

int aes_crypt_ctr_le32(aes_context *enc, size_t length, unsigned char ctr[16], const unsigned char *input,
                       unsigned char *output)
{
    unsigned char ks[16];
    ensure_tables();
    while (length) {
        const size_t n = length < 16 ? length : 16;
        encrypt_block(enc, ctr, ks);
        store_le32(ctr, load_le32(ctr) + 1u); /* wraps at 2^32; bytes 4..15 never change */
        for (size_t i = 0; i < n; ++i) output[i] = (unsigned char)(input[i] ^ ks[i]);
        input += n;
        output += n;
        length -= n;
    }
    return 0;
}

static void put64_le(unsigned char *p, uint64_t v)
{
    for (int i = 0; i < 8; ++i) p[i] = (unsigned char)(v >> (8 * i));
}

int aes_crypt_gcmsiv(aes_context *kgk, int mode, size_t length, const unsigned char nonce[12],
                     const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                     const unsigned char *tag_in, unsigned char tag[16])
{
    if ((uint64_t)length > AES_GCM_SIV_MAX_BYTES || (uint64_t)aad_len > AES_GCM_SIV_MAX_BYTES)
        return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    if (mode == AES_DECRYPT && !tag_in) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    unsigned char authkey[16], enckey[32], ctr[16], s[16] = {0}, lb[16];
    const int enc_bytes = aes_gcmsiv_derive(kgk, nonce, authkey, enckey);
    if (enc_bytes < 0) return enc_bytes;
    aes_context enc;
    aes_setkey_enc(&enc, enckey, (unsigned)enc_bytes * 8);
    ensure_tables();
    /* a decryption runs the counter mode from the RECEIVED tag, then hashes
     * the plaintext it gave; an encryption hashes first: in place both ways */
    if (mode == AES_DECRYPT) {
        memcpy(ctr, tag_in, 16);
        ctr[15] |= 0x80;
        aes_crypt_ctr_le32(&enc, length, ctr, input, output);
    }
    const unsigned char *pt = mode == AES_DECRYPT ? output : input;
    aes_polyval(authkey, s, aad, aad_len);
    aes_polyval(authkey, s, pt, length);
    put64_le(lb, (uint64_t)aad_len * 8);
    put64_le(lb + 8, (uint64_t)length * 8);
    aes_polyval(authkey, s, lb, 16);
    for (int i = 0; i < 12; ++i) s[i] ^= nonce[i];
    s[15] &= 0x7F;
    encrypt_block(&enc, s, s);
    if (mode != AES_DECRYPT) {
        memcpy(ctr, s, 16);
        ctr[15] |= 0x80;
        aes_crypt_ctr_le32(&enc, length, ctr, input, output);
    }
    memcpy(tag, s, 16);
    return 0;
}

int aes_gcmsiv_auth_decrypt(aes_context *kgk, size_t length, const unsigned char nonce[12], const unsigned char *aad,
                            size_t aad_len, const unsigned char tag[16], const unsigned char *input,
                            unsigned char *output)
{
    unsigned char t[16];
    const int r = aes_crypt_gcmsiv(kgk, AES_DECRYPT, length, nonce, aad, aad_len, input, output, tag, t);
    if (r) return r;
    unsigned diff = 0; /* every byte compared, whatever the earlier ones gave */
    for (int i = 0; i < 16; ++i) diff |= (unsigned)(t[i] ^ tag[i]);
    if (diff) {
        memset(output, 0, length);
        return POLARSSL_ERR_GCM_AUTH_FAILED;
    }
    return 0;
}

/* ---------------------------------------------------------------------------
 * AES-OCB3 (RFC 7253), written from the RFC.  Strings are big-endian 128-bit
 * blocks: double() shifts the 16 bytes left by one bit and folds a bit shifted
 * out of byte 0 back as 0x87 into byte 15.
 * ------------------------------------------------------------------------- */
static void ocb_double(unsigned char out[16], const unsigned char in[16])
{
    const unsigned carry = in[0] >> 7;
    for (int i = 0; i < 15; ++i) out[i] = (unsigned char)((in[i] << 1) | (in[i + 1] >> 7));
    out[15] = (unsigned char)((in[15] << 1) ^ (carry ? 0x87 : 0));
}

static inline void xor16(unsigned char *d, const unsigned char *a, const unsigned char *b)
{
    for (int i = 0; i < 16; ++i) d[i] = (unsigned char)(a[i] ^ b[i]);
}

/* L_*, L_$ and L_0..L_32 from the encryption schedule already in ctx->enc */
static void ocb_set_l(aes_ocb_context *ctx)
{
    const unsigned char zero[16] = {0};
    ensure_tables();
    encrypt_block(&ctx->enc, zero, ctx->l_star);
    ocb_double(ctx->l_dollar, ctx->l_star);
    ocb_double(ctx->l[0], ctx->l_dollar);
    for (int j = 1; j <= 32; ++j) ocb_double(ctx->l[j], ctx->l[j - 1]);
}

int aes_ocb_setkey(aes_ocb_context *ctx, const unsigned char *key, unsigned int keybits)
{
    int r = aes_setkey_enc(&ctx->enc, key, keybits);
    if (r == 0) r = aes_setkey_dec(&ctx->dec, key, keybits);
    if (r) return r;
    ocb_set_l(ctx);
    return 0;
}

int aes_ocb_offset0(const aes_ocb_context *ctx, const unsigned char *nonce, size_t nonce_len, size_t tag_len,
                    unsigned char out[16])
{
    if (!nonce || nonce_len < 1 || nonce_len > 15 || tag_len < 1 || tag_len > 16)
        return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    /* Nonce = num2str(TAGLEN mod 128, 7) || 0* || 1 || N */
    unsigned char nb[16] = {0}, stretch[24];
    nb[0] = (unsigned char)(((8 * tag_len) % 128) << 1);
    nb[15 - nonce_len] |= 1;
    memcpy(nb + 16 - nonce_len, nonce, nonce_len);
    const unsigned bottom = nb[15] & 63u;
    nb[15] &= 0xC0;
    ensure_tables();
    encrypt_block(&ctx->enc, nb, stretch); /* Ktop */
    for (int i = 0; i < 8; ++i) stretch[16 + i] = (unsigned char)(stretch[i] ^ stretch[i + 1]);
    const unsigned bs = bottom / 8, bb = bottom % 8;
    for (int i = 0; i < 16; ++i)
        out[i] = (unsigned char)((stretch[i + bs] << bb) | (bb ? stretch[i + bs + 1] >> (8 - bb) : 0));
    return 0;
}

void aes_ocb_offset(const aes_ocb_context *ctx, const unsigned char offset0[16], uint64_t i, unsigned char out[16])
{
    unsigned char o[16];
    memcpy(o, offset0, 16);
    const uint64_t g = i ^ (i >> 1);
    for (int j = 0; j <= 32; ++j)
        if ((g >> j) & 1u) xor16(o, o, ctx->l[j]);
    memcpy(out, o, 16);
}

static inline int ocb_ntz(uint64_t i) { return __builtin_ctzll(i); }

void aes_ocb_hash(const aes_ocb_context *ctx, const unsigned char *aad, size_t len, unsigned char out[16])
{
    unsigned char off[16] = {0}, sum[16] = {0}, t[16];
    ensure_tables();
    uint64_t i = 0;
    for (; len >= 16; aad += 16, len -= 16) {
        ++i;
        xor16(off, off, ctx->l[ocb_ntz(i)]);
        xor16(t, aad, off);
        encrypt_block(&ctx->enc, t, t);
        xor16(sum, sum, t);
    }
    if (len) {
        xor16(off, off, ctx->l_star);
        memset(t, 0, 16);
        memcpy(t, aad, len);
        t[len] = 0x80;
        xor16(t, t, off);
        encrypt_block(&ctx->enc, t, t);
        xor16(sum, sum, t);
    }
    memcpy(out, sum, 16);
}

static void ocb_blocks_serial(const aes_ocb_context *ctx, int mode, const unsigned char offset0[16], uint64_t first,
                              uint64_t nblocks, const unsigned char *in, unsigned char *out, unsigned char cs[16])
{
    unsigned char off[16], t[16];
    aes_ocb_offset(ctx, offset0, first, off);
    for (uint64_t k = 0; k < nblocks; ++k, in += 16, out += 16) {
        xor16(off, off, ctx->l[ocb_ntz(first + k + 1)]);
        if (mode == AES_ENCRYPT) {
            xor16(cs, cs, in);
            xor16(t, in, off);
            encrypt_block(&ctx->enc, t, t);
            xor16(out, t, off);
        } else {
            xor16(t, in, off);
            decrypt_block(&ctx->dec, t, t);
            xor16(out, t, off);
            xor16(cs, cs, out);
        }
    }
}

typedef struct {
    const aes_ocb_context *ctx;
    int mode;
    const unsigned char *offset0;
    uint64_t first, nblocks;
    const unsigned char *in;
    unsigned char *out;
    unsigned char cs[16];
} ocb_job;

static void *ocb_worker(void *arg)
{
    ocb_job *j = (ocb_job *)arg;
    ocb_blocks_serial(j->ctx, j->mode, j->offset0, j->first, j->nblocks, j->in, j->out, j->cs);
    return NULL;
}

/* Large calls (the device tests' oracle) run T pieces on T threads, each from
 * the closed-form offset of its first block, and XOR the pieces' checksums. */
int aes_crypt_ocb_blocks(const aes_ocb_context *ctx, int mode, const unsigned char offset0[16], uint64_t first_block,
                         uint64_t nblocks, const unsigned char *input, unsigned char *output,
                         unsigned char checksum[16])
{
    enum { MAXT = 8 };
    if (first_block > AES_OCB_MAX_BLOCKS || nblocks > AES_OCB_MAX_BLOCKS - first_block)
        return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    ensure_tables();
    if (nblocks < ((uint64_t)1 << 16)) {
        ocb_blocks_serial(ctx, mode, offset0, first_block, nblocks, input, output, checksum);
        return 0;
    }
    ocb_job jobs[MAXT];
    pthread_t th[MAXT];
    const uint64_t per = nblocks / MAXT;
    for (uint64_t t = 0; t < MAXT; ++t) {
        jobs[t].ctx = ctx;
        jobs[t].mode = mode;
        jobs[t].offset0 = offset0;
        jobs[t].first = first_block + t * per;
        jobs[t].nblocks = t + 1 == MAXT ? nblocks - t * per : per;
        jobs[t].in = input + 16 * t * per;
        jobs[t].out = output + 16 * t * per;
        memset(jobs[t].cs, 0, 16);
    }
    for (size_t t = 1; t < MAXT; ++t) pthread_create(&th[t], NULL, ocb_worker, &jobs[t]);
    ocb_worker(&jobs[0]);
    for (size_t t = 1; t < MAXT; ++t) pthread_join(th[t], NULL);
    for (size_t t = 0; t < MAXT; ++t) xor16(checksum, checksum, jobs[t].cs);
    return 0;
}

int aes_crypt_ocb(const aes_ocb_context *ctx, int mode, size_t length, const unsigned char *nonce, size_t nonce_len,
                  const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                  unsigned char tag[16], size_t tag_len)
{
    unsigned char off[16], off0[16], cs[16] = {0}, t[16];
    if ((uint64_t)length > AES_OCB_MAX_BYTES) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    if (aes_ocb_offset0(ctx, nonce, nonce_len, tag_len, off0)) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    /* this copy's tables: in a process that holds two copies of this file the
     * calls above and below may run in the other one (see aes_gcm_setkey) */
    ensure_tables();
    const uint64_t m = (uint64_t)length / 16;
    const size_t r = length % 16;
    aes_crypt_ocb_blocks(ctx, mode, off0, 0, m, input, output, cs);
    aes_ocb_offset(ctx, off0, m, off);
    if (r) {
        unsigned char pad[16], p[16] = {0};
        const unsigned char *in = input + 16 * m;
        unsigned char *out = output + 16 * m;
        xor16(off, off, ctx->l_star);
        encrypt_block(&ctx->enc, off, pad);
        for (size_t i = 0; i < r; ++i) {
            const unsigned char c = (unsigned char)(in[i] ^ pad[i]);
            p[i] = mode == AES_ENCRYPT ? in[i] : c; /* the plaintext, either way */
            out[i] = c;
        }
        p[r] = 0x80;
        xor16(cs, cs, p);
    }
    xor16(t, cs, off);
    xor16(t, t, ctx->l_dollar);
    encrypt_block(&ctx->enc, t, t);
    aes_ocb_hash(ctx, aad, aad_len, off);
    xor16(t, t, off);
    memset(tag, 0, 16);
    memcpy(tag, t, tag_len);
    return 0;
}

int aes_ocb_auth_decrypt(const aes_ocb_context *ctx, size_t length, const unsigned char *nonce, size_t nonce_len,
                         const unsigned char *aad, size_t aad_len, const unsigned char *tag, size_t tag_len,
                         const unsigned char *input, unsigned char *output)
{
    unsigned char t[16];
    const int r = aes_crypt_ocb(ctx, AES_DECRYPT, length, nonce, nonce_len, aad, aad_len, input, output, t, tag_len);
    if (r) return r;
    unsigned diff = 0; /* every byte compared, whatever the earlier ones gave */
    for (size_t i = 0; i < tag_len; ++i) diff |= (unsigned)(t[i] ^ tag[i]);
    if (diff) {
        if (length) memset(output, 0, length);
        return POLARSSL_ERR_OCB_AUTH_FAILED;
    }
    return 0;
}

/* ---------------------------------------------------------------------------
 * AES-CCM (NIST SP 800-38C, RFC 3610), written from the two documents: the tag
 * is a CBC-MAC over B0 || encoded AAD || data (each zero-padded to a block), the
 * data runs in counter mode on A_1 .., the tag is MSB_M(T ^ E(A_0)).
 * ------------------------------------------------------------------------- */
static int ccm_lengths_ok(size_t length, size_t nonce_len, size_t aad_len, size_t tag_len)
{
    if (nonce_len < 7 || nonce_len > 13) return 0;
    if (tag_len < 4 || tag_len > 16 || (tag_len & 1)) return 0;
    const unsigned L = 15u - (unsigned)nonce_len; /* 2 .. 8 */
    if (L < 8 && ((uint64_t)length >> (8 * L))) return 0;
    if ((uint64_t)aad_len >> 32) return 0; /* the 6-byte encoding; the 10-byte one is not built */
    return 1;
}

/* flags || N || [v]_L */
static void ccm_block(unsigned char b[16], unsigned flags, const unsigned char *nonce, size_t nonce_len, uint64_t v)
{
    b[0] = (unsigned char)flags;
    memcpy(b + 1, nonce, nonce_len);
    for (size_t i = 15; i > nonce_len; --i, v >>= 8) b[i] = (unsigned char)v;
}

int aes_crypt_ccm(const aes_context *ctx, int mode, size_t length, const unsigned char *nonce, size_t nonce_len,
                  const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                  unsigned char tag[16], size_t tag_len)
{
    if (!ccm_lengths_ok(length, nonce_len, aad_len, tag_len)) return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
    ensure_tables();
    const unsigned L = 15u - (unsigned)nonce_len;
    unsigned char x[16], a[16], s[16], s0[16];
    ccm_block(x, (aad_len ? 64u : 0u) + 8u * (((unsigned)tag_len - 2u) / 2u) + (L - 1u), nonce, nonce_len, length);
    encrypt_block(ctx, x, x);
    if (aad_len) {
        /* the length's encoding, the AAD, zeros up to a block */
        unsigned char hdr[6];
        size_t h;
        if (aad_len < 0xFF00) {
            hdr[0] = (unsigned char)(aad_len >> 8), hdr[1] = (unsigned char)aad_len, h = 2;
        } else {
            hdr[0] = 0xFF, hdr[1] = 0xFE, h = 6;
            for (int i = 0; i < 4; ++i) hdr[2 + i] = (unsigned char)((uint64_t)aad_len >> (24 - 8 * i));
        }
        size_t fill = 0;
        for (size_t i = 0; i < h; ++i) x[fill++] ^= hdr[i];
        for (size_t i = 0; i < aad_len; ++i) {
            x[fill++] ^= aad[i];
            if (fill == 16) encrypt_block(ctx, x, x), fill = 0;
        }
        if (fill) encrypt_block(ctx, x, x);
    }
    ccm_block(a, L - 1u, nonce, nonce_len, 0);
    encrypt_block(ctx, a, s0);
    uint64_t ctr = 0;
    for (size_t at = 0; at < length; at += 16) {
        const size_t n = length - at < 16 ? length - at : 16;
        ccm_block(a, L - 1u, nonce, nonce_len, ++ctr);
        encrypt_block(ctx, a, s);
        for (size_t i = 0; i < n; ++i) {
            const unsigned char c = (unsigned char)(input[at + i] ^ s[i]);
            x[i] ^= mode == AES_ENCRYPT ? input[at + i] : c; /* the plaintext, either way */
            output[at + i] = c;
        }
        encrypt_block(ctx, x, x);
    }
    memset(tag, 0, 16);
    for (size_t i = 0; i < tag_len; ++i) tag[i] = (unsigned char)(x[i] ^ s0[i]);
    return 0;
}

int aes_ccm_auth_decrypt(const aes_context *ctx, size_t length, const unsigned char *nonce, size_t nonce_len,
                         const unsigned char *aad, size_t aad_len, const unsigned char *tag, size_t tag_len,
                         const unsigned char *input, unsigned char *output)
{
    unsigned char t[16];
    const int r = aes_crypt_ccm(ctx, AES_DECRYPT, length, nonce, nonce_len, aad, aad_len, input, output, t, tag_len);
    if (r) return r;
    unsigned diff = 0; /* every byte compared, whatever the earlier ones gave */
    for (size_t i = 0; i < tag_len; ++i) diff |= (unsigned)(t[i] ^ tag[i]);
    if (diff) {
        if (length) memset(output, 0, length);
        return POLARSSL_ERR_CCM_AUTH_FAILED;
    }
    return 0;
}

/* ---------------------------------------------------------------------------
 * Self test: FIPS-197 appendix C, SP 800-38A F.1/F.2/F.3/F.5, RFC 3686 #1-#3,
 * and the 10,000-iteration Monte-Carlo ECB/CBC chains of the NIST
 * rijndael-vals set that the reference's self-test runs
 * (/root/reference/aes-modes/aes.c:912-950 vectors, loop :1084-1200).
 * ------------------------------------------------------------------------- */
static int hexval(char c)
{
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}
static size_t unhex(const char *s, unsigned char *out)
{
    size_t n = 0;
    while (s[0] && s[1]) {
        out[n++] = (unsigned char)(hexval(s[0]) * 16 + hexval(s[1]));
        s += 2;
    }
    return n;
}

static const char *SP_PT =
    "6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
    "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710";
static const char *SP_KEY[3] = {
    "2b7e151628aed2a6abf7158809cf4f3c",
    "8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b",
    "603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"};
static const char *SP_ECB[3] = {
    "3ad77bb40d7a3660a89ecaf32466ef97f5d3d58503b9699de785895a96fdbaaf"
    "43b1cd7f598ece23881b00e3ed0306887b0c785e27e8ad3f8223207104725dd4",
    "bd334f1d6e45f25ff712a214571fa5cc974104846d0ad3ad7734ecb3ecee4eef"
    "ef7afd2270e2e60adce0ba2face6444e9a4b41ba738d6c72fb16691603c18e0e",
    "f3eed1bdb5d2a03c064b5a7e3db181f8591ccb10d410ed26dc5ba74a31362870"
    "b6ed21b99ca6f4f9f153e7b1beafed1d23304b7a39f9f3ff067d8d8f9e24ecc7"};
static const char *SP_CBC[3] = {
    "7649abac8119b246cee98e9b12e9197d5086cb9b507219ee95db113a917678b2"
    "73bed6b8e3c1743b7116e69e222295163ff1caa1681fac09120eca307586e1a7",
    "4f021db243bc633d7178183a9fa071e8b4d9ada9ad7dedf4e5e738763f69145a"
    "571b242012fb7ae07fa9baac3df102e008b0e27988598881d920a9e64f5615cd",
    "f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d"
    "39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b"};
static const char *SP_CFB[3] = {
    "3b3fd92eb72dad20333449f8e83cfb4ac8a64537a0b3a93fcde3cdad9f1ce58b"
    "26751f67a3cbb140b1808cf187a4f4dfc04b05357c5d1c0eeac4c66f9ff7f2e6",
    "cdc80d6fddf18cab34c25909c99a417467ce7f7f81173621961a2b70171d3d7a"
    "2e1e8a1dd59b88b1c8e60fed1efac4c9c05f9f9ca9834fa042ae8fba584b09ff",
    "dc7e84bfda79164b7ecd8486985d386039ffed143b28b1c832113c6331e5407b"
    "df10132415e54b92a13ed0a8267ae2f975a385741ab9cef82031623d55b1e471"};
static const char *SP_CTR[3] = {
    "874d6191b620e3261bef6864990db6ce9806f66b7970fdff8617187bb9fffdff"
    "5ae4df3edbd5d35e5b4f09020db03eab1e031dda2fbe03d1792170a0f3009cee",
    "1abc932417521ca24f2b0459fe7e6e0b090339ec0aa6faefd5ccc2c6f4ce8e94"
    "1e36b26bd1ebc670d1bd1d665620abf74f78a7f6d29809585a97daec58c6b050",
    "601ec313775789a5b7a7f504bbf3d228f443e3ca4d62b59aca84e990cacaf5c5"
    "2b0930daa23de94ce87017ba2d84988ddfc9c58db67aada613c2dd08457941a6"};

/* RFC 3686: key, counter block (nonce||iv||00000001), plaintext, ciphertext */
static const char *RFC3686[3][4] = {
    {"ae6852f8121067cc4bf7a5765577f39e", "00000030000000000000000000000001",
     "53696e676c6520626c6f636b206d7367", "e4095d4fb7a7b3792d6175a3261311b8"},
    {"7e24067817fae0d743d6ce1f32539163", "006cb6dbc0543b59da48d90b00000001",
     "000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f",
     "5104a106168a72d9790d41ee8edad388eb2e1efc46da57c8fce630df9141be28"},
    {"7691be035e5020a8ac6e618529f9a0dc", "00e0017b27777f3f4a1786f000000001",
     "000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20212223",
     "c1cf48a89f2ffdd9cf4652e9efdb72d74540a42bde6d7836d59a5ceaaef3105325b2072f"}};

static int report(int verbose, const char *name, int ok)
{
    if (verbose) printf("  %s: %s\n", name, ok ? "passed" : "failed");
    return ok ? 0 : 1;
}

/* Monte-Carlo results after 10,000 chained operations from an all-zero key
 * (128/192/256), block and IV (NIST rijndael-vals) */
static const char *MC_ECB_ENC[3] = {"c34c052cc0da8d73451afe5f03be297f", "f3f6752ae8d7831138f041560631b114",
                                    "8b79eecc93a0ee5dff30b4ea21636da4"};
static const char *MC_ECB_DEC[3] = {"44416ac2d1f53c583303917e6be9ebe0", "48e31e9e256718f29229319c19f15ba4",
                                    "058ccffdbbcb382d1f6f56585d8a4ade"};
static const char *MC_CBC_ENC[3] = {"8a05fc5e095af4848a08d328d3688e3d", "7bd966d53ad8c1bb85d2adfae87bb104",
                                    "fe3c53653e2f45b56fcd88b2cc898ff0"};
static const char *MC_CBC_DEC[3] = {"faca37e0b0c85373df706e73f7c9af86", "5df678dd17ba4e75b61768c6adef7c7b",
                                    "4804e1818fe6297519a3e88c57310413"};

int aes_monte_carlo(int mode, int bits, unsigned char result[16])
{
    unsigned char key[32] = {0}, buf[16] = {0}, iv[16] = {0}, prv[16] = {0};
    aes_context ctx;
    const int dec = (mode == AES_MC_ECB_DEC || mode == AES_MC_CBC_DEC);
    int r = dec ? aes_setkey_dec(&ctx, key, (unsigned)bits) : aes_setkey_enc(&ctx, key, (unsigned)bits);
    if (r) return r;
    for (int j = 0; j < 10000; ++j) {
        switch (mode) {
        case AES_MC_ECB_ENC: aes_crypt_ecb(&ctx, AES_ENCRYPT, buf, buf); break;
        case AES_MC_ECB_DEC: aes_crypt_ecb(&ctx, AES_DECRYPT, buf, buf); break;
        case AES_MC_CBC_DEC: aes_crypt_cbc(&ctx, AES_DECRYPT, 16, iv, buf, buf); break;
        case AES_MC_CBC_ENC: { /* the ciphertext becomes the next IV (in iv) and the
                                  previous ciphertext the next plaintext */
            unsigned char tmp[16];
            aes_crypt_cbc(&ctx, AES_ENCRYPT, 16, iv, buf, buf);
            memcpy(tmp, prv, 16);
            memcpy(prv, buf, 16);
            memcpy(buf, tmp, 16);
            break;
        }
        default: return POLARSSL_ERR_AES_INVALID_INPUT_LENGTH;
        }
    }
    memcpy(result, mode == AES_MC_CBC_ENC ? prv : buf, 16);
    return 0;
}

const char *aes_monte_carlo_expected(int mode, int bits)
{
    const int k = (bits - 128) / 64;
    if (k < 0 || k > 2 || bits % 64) return NULL;
    switch (mode) {
    case AES_MC_ECB_ENC: return MC_ECB_ENC[k];
    case AES_MC_ECB_DEC: return MC_ECB_DEC[k];
    case AES_MC_CBC_ENC: return MC_CBC_ENC[k];
    case AES_MC_CBC_DEC: return MC_CBC_DEC[k];
    default: return NULL;
    }
}

/* RFC 8452 appendix A (POLYVAL, the derivation) and appendix C (sealed
 * outputs: ciphertext || tag); the last two rows are from an independent model
 * of the RFC: key 00.., nonce a0..ab, AAD bytes 100..120, plaintext bytes 1..49 */
static const char *SIV_VEC[][5] = {
    /* key, nonce, aad, plaintext, ciphertext || tag */
    {"01000000000000000000000000000000", "030000000000000000000000", "", "", "dc20e2d83f25705bb49e439eca56de25"},
    {"01000000000000000000000000000000", "030000000000000000000000", "", "0100000000000000",
     "b5d839330ac7b786578782fff6013b815b287c22493a364c"},
    {"01000000000000000000000000000000", "030000000000000000000000", "01", "0200000000000000",
     "1e6daba35669f4273b0a1a2560969cdf790d99759abd1508"},
    {"0100000000000000000000000000000000000000000000000000000000000000", "030000000000000000000000", "", "",
     "07f5f4169bbf55a8400cd47ea6fd400f"},
    {"0100000000000000000000000000000000000000000000000000000000000000", "030000000000000000000000", "",
     "0100000000000000", "c2ef328e5c71c83b843122130f7364b761e0b97427e3df28"},
    {"000102030405060708090a0b0c0d0e0f", "a0a1a2a3a4a5a6a7a8a9aaab", NULL, NULL,
     "65483eb7d1533466ead8e673d7270e99ea4ffe611498a5f768131b4cd04e371ea2cdcbb60c093766b35139add04a79ddf740928eb78fabb"
     "f8f4ee555ae38f2d815"},
    {"000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f", "a0a1a2a3a4a5a6a7a8a9aaab", NULL, NULL,
     "c2f39d921b077cbba73072360062d524e91677592a794769b8106c9d4dfbf643dbda8d4cac178311cf1ca57ec80cad12c052296c35a730a"
     "ce425c50d199ebfd125"},
};

int aes_gcmsiv_self_test(int verbose)
{
    int fails = 0;
    char name[64];
    unsigned char key[32], nonce[12], aad[32], pt[64], ref[96], out[96], tag[16], h[16], y[16] = {0}, x[32];
    aes_context kgk;

    unhex("25629347589242761d31f826ba4b757b", h);
    unhex("4f4f95668c83dfb6401762bb2d01a262d1a24ddd2721d006bbe45f20d3c9f362", x);
    unhex("f7a3b47b846119fae5b7866cf5e5b77e", ref);
    aes_polyval(h, y, x, 32);
    fails += report(verbose, "RFC 8452 A POLYVAL", memcmp(y, ref, 16) == 0);

    unhex("ee8e1ed9ff2540ae8f2ba9f50bc2f27c", key);
    unhex("752abad3e0afb5f434dc4310", nonce);
    aes_setkey_enc(&kgk, key, 128);
    unsigned char ak[16], ek[32];
    int ok = aes_gcmsiv_derive(&kgk, nonce, ak, ek) == 16;
    unhex("310728d9911f1f3837b24316c3fab9a0", ref);
    ok = ok && memcmp(ak, ref, 16) == 0;
    unhex("a4c5ae6249963279c100be4d7e2c6edd", ref);
    fails += report(verbose, "RFC 8452 A key derivation", ok && memcmp(ek, ref, 16) == 0);

    for (size_t v = 0; v < sizeof SIV_VEC / sizeof SIV_VEC[0]; ++v) {
        const size_t kl = unhex(SIV_VEC[v][0], key);
        size_t al, n;
        unhex(SIV_VEC[v][1], nonce);
        if (SIV_VEC[v][2]) {
            al = unhex(SIV_VEC[v][2], aad);
            n = unhex(SIV_VEC[v][3], pt);
        } else {
            al = 21;
            n = 49;
            for (size_t i = 0; i < al; ++i) aad[i] = (unsigned char)(100 + i);
            for (size_t i = 0; i < n; ++i) pt[i] = (unsigned char)(1 + i);
        }
        ok = unhex(SIV_VEC[v][4], ref) == n + 16;
        aes_setkey_enc(&kgk, key, (unsigned)(kl * 8));
        ok = ok && aes_crypt_gcmsiv(&kgk, AES_ENCRYPT, n, nonce, aad, al, pt, out, NULL, tag) == 0;
        ok = ok && memcmp(out, ref, n) == 0 && memcmp(tag, ref + n, 16) == 0;
        /* and back, in place */
        ok = ok && aes_gcmsiv_auth_decrypt(&kgk, n, nonce, aad, al, tag, out, out) == 0 && memcmp(out, pt, n) == 0;
        snprintf(name, sizeof name, "AES-GCM-SIV-%d vector #%d", (int)(kl * 8), (int)v + 1);
        fails += report(verbose, name, ok);
    }
    return fails;
}

int aes_self_test(int verbose)
{
    int fails = 0;
    char name[64];
    unsigned char key[32], pt[64], ref[64], out[64], iv[16], sb[16];
    aes_context ctx;

    /* FIPS-197 appendix C: key 00..(n-1), pt 00112233..ff */
    static const char *fips_ct[3] = {"69c4e0d86a7b0430d8cdb78070b4c55a",
                                     "dda97ca4864cdfe06eaf70a0ec0d7191",
                                     "8ea2b7ca516745bfeafc49904b496089"};
    for (int k = 0; k < 3; ++k) {
        int bits = 128 + 64 * k;
        for (int i = 0; i < 32; ++i) key[i] = (unsigned char)i;
        unhex("00112233445566778899aabbccddeeff", pt);
        unhex(fips_ct[k], ref);
        aes_setkey_enc(&ctx, key, (unsigned)bits);
        aes_crypt_ecb(&ctx, AES_ENCRYPT, pt, out);
        snprintf(name, sizeof name, "FIPS-197 C.%d AES-%d (enc)", k + 1, bits);
        fails += report(verbose, name, memcmp(out, ref, 16) == 0);
        aes_setkey_dec(&ctx, key, (unsigned)bits);
        aes_crypt_ecb(&ctx, AES_DECRYPT, ref, out);
        snprintf(name, sizeof name, "FIPS-197 C.%d AES-%d (dec)", k + 1, bits);
        fails += report(verbose, name, memcmp(out, pt, 16) == 0);
    }

    unhex(SP_PT, pt);
    for (int k = 0; k < 3; ++k) {
        int bits = 128 + 64 * k;
        unhex(SP_KEY[k], key);

        /* ECB */
        unhex(SP_ECB[k], ref);
        aes_setkey_enc(&ctx, key, (unsigned)bits);
        for (int b = 0; b < 4; ++b) aes_crypt_ecb(&ctx, AES_ENCRYPT, pt + 16 * b, out + 16 * b);
        snprintf(name, sizeof name, "AES-ECB-%d (enc)", bits);
        fails += report(verbose, name, memcmp(out, ref, 64) == 0);
        aes_setkey_dec(&ctx, key, (unsigned)bits);
        for (int b = 0; b < 4; ++b) aes_crypt_ecb(&ctx, AES_DECRYPT, ref + 16 * b, out + 16 * b);
        snprintf(name, sizeof name, "AES-ECB-%d (dec)", bits);
        fails += report(verbose, name, memcmp(out, pt, 64) == 0);

        /* CBC */
        unhex(SP_CBC[k], ref);
        aes_setkey_enc(&ctx, key, (unsigned)bits);
        unhex("000102030405060708090a0b0c0d0e0f", iv);
        aes_crypt_cbc(&ctx, AES_ENCRYPT, 64, iv, pt, out);
        snprintf(name, sizeof name, "AES-CBC-%d (enc)", bits);
        fails += report(verbose, name, memcmp(out, ref, 64) == 0);
        aes_setkey_dec(&ctx, key, (unsigned)bits);
        unhex("000102030405060708090a0b0c0d0e0f", iv);
        aes_crypt_cbc(&ctx, AES_DECRYPT, 64, iv, ref, out);
        snprintf(name, sizeof name, "AES-CBC-%d (dec)", bits);
        fails += report(verbose, name, memcmp(out, pt, 64) == 0);

        /* CFB128 (byte-granular resume exercised by a 13/51 split) */
        unhex(SP_CFB[k], ref);
        aes_setkey_enc(&ctx, key, (unsigned)bits);
        int off = 0;
        unhex("000102030405060708090a0b0c0d0e0f", iv);
        aes_crypt_cfb128(&ctx, AES_ENCRYPT, 13, &off, iv, pt, out);
        aes_crypt_cfb128(&ctx, AES_ENCRYPT, 51, &off, iv, pt + 13, out + 13);
        snprintf(name, sizeof name, "AES-CFB128-%d (enc)", bits);
        fails += report(verbose, name, memcmp(out, ref, 64) == 0);
        off = 0;
        unhex("000102030405060708090a0b0c0d0e0f", iv);
        aes_crypt_cfb128(&ctx, AES_DECRYPT, 64, &off, iv, ref, out);
        snprintf(name, sizeof name, "AES-CFB128-%d (dec)", bits);
        fails += report(verbose, name, memcmp(out, pt, 64) == 0);

        /* CTR (resume across a 7/57 split) */
        unhex(SP_CTR[k], ref);
        unhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff", iv);
        off = 0;
        aes_crypt_ctr(&ctx, 7, &off, iv, sb, pt, out);
        aes_crypt_ctr(&ctx, 57, &off, iv, sb, pt + 7, out + 7);
        snprintf(name, sizeof name, "AES-CTR-%d (enc)", bits);
        fails += report(verbose, name, memcmp(out, ref, 64) == 0);
    }

    for (int v = 0; v < 3; ++v) {
        size_t kl = unhex(RFC3686[v][0], key);
        unhex(RFC3686[v][1], iv);
        size_t n = unhex(RFC3686[v][2], pt);
        unhex(RFC3686[v][3], ref);
        aes_setkey_enc(&ctx, key, (unsigned)(kl * 8));
        int off = 0;
        aes_crypt_ctr(&ctx, (int)n, &off, iv, sb, pt, out);
        snprintf(name, sizeof name, "RFC 3686 AES-CTR test vector #%d", v + 1);
        fails += report(verbose, name, memcmp(out, ref, n) == 0);
    }
    fails += aes_gcmsiv_self_test(verbose);
    static const char *mc_name[4] = {"ECB", "ECB", "CBC", "CBC"};
    for (int mode = 0; mode < 4; ++mode)
        for (int k = 0; k < 3; ++k) {
            const int bits = 128 + 64 * k;
            unsigned char got[16];
            unhex(aes_monte_carlo_expected(mode, bits), ref);
            snprintf(name, sizeof name, "AES-%s-%d (%s) Monte-Carlo x10000", mc_name[mode], bits,
                     (mode & 1) ? "dec" : "enc");
            fails += report(verbose, name, aes_monte_carlo(mode, bits, got) == 0 && memcmp(got, ref, 16) == 0);
        }
    if (verbose) printf("\n");
    return fails ? 1 : 0;
}
