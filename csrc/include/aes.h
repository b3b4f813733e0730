/*
 * aes.h -- AES-128/192/256 block cipher, CPU reference ("oracle") API.
 *
 * Source-compatible with the reference's PolarSSL-derived API
 * (/root/reference/aes-modes/aes.h:31-161): same function names, argument
 * order, AES_ENCRYPT/AES_DECRYPT values, error codes and aes_context field
 * names (nr, rk, buf).  Implementation is new (csrc/cpu/aes.c) and differs
 * from the reference where the reference is defective:
 *   - table generation is thread safe (pthread_once), reference aes.c:448-452
 *     used an unsynchronised flag;
 *   - CFB128 and the self test are always compiled in (reference compiled
 *     them out, aes.c:818,903).
 *
 * Byte streams are FIPS-197 / SP 800-38A exact.  Round keys are kept as
 * little-endian 32-bit column words (byte 0 of the column in bits 0..7), one
 * word per `unsigned long` slot for source compatibility.
 */
#ifndef OTC_AES_H
#define OTC_AES_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define AES_ENCRYPT 1
#define AES_DECRYPT 0

#define POLARSSL_ERR_AES_INVALID_KEY_LENGTH   -0x0020
#define POLARSSL_ERR_AES_INVALID_INPUT_LENGTH -0x0022

typedef struct {
    int nr;                 /* number of rounds: 10, 12 or 14 */
    unsigned long *rk;      /* points into buf */
    unsigned long buf[68];  /* round-key words (low 32 bits used) */
} aes_context;

#ifdef __cplusplus
extern "C" {
#endif

int aes_setkey_enc(aes_context *ctx, const unsigned char *key, unsigned int keysize);
int aes_setkey_dec(aes_context *ctx, const unsigned char *key, unsigned int keysize);

int aes_crypt_ecb(aes_context *ctx, int mode,
                  const unsigned char input[16], unsigned char output[16]);

int aes_crypt_cbc(aes_context *ctx, int mode, size_t length, unsigned char iv[16],
                  const unsigned char *input, unsigned char *output);

int aes_crypt_cfb128(aes_context *ctx, int mode, size_t length, int *iv_off,
                     unsigned char iv[16], const unsigned char *input,
                     unsigned char *output);

int aes_crypt_ctr(aes_context *ctx, int length, int *nc_off,
                  unsigned char nonce_counter[16], unsigned char stream_block[16],
                  const unsigned char *input, unsigned char *output);

int aes_self_test(int verbose);

/* ---- extensions (not in the reference API) ------------------------------ */

/* Copy the (4*(nr+1)) round-key words into a packed uint32 array; returns the
 * word count.  This is the format uploaded to the GPU kernels. */
int aes_export_rk32(const aes_context *ctx, uint32_t *out);
/* Inverse of aes_export_rk32: a context over (4*(nr+1)) packed round-key
 * words (either direction's schedule). */
int aes_import_rk32(aes_context *ctx, const uint32_t *rk, int nr);

/* Multi-threaded bulk helpers used by the CPU-baseline harness and the tests.
 * Counter semantics = aes_crypt_ctr with nc_off == 0 (full 128-bit BE add). */
int aes_ctr_bulk(const aes_context *ctx, const unsigned char nonce_counter[16],
                 const unsigned char *input, unsigned char *output, size_t length,
                 int nthreads);
int aes_ecb_bulk(const aes_context *ctx, int mode, const unsigned char *input,
                 unsigned char *output, size_t length, int nthreads);

/* XTS-AES (IEEE 1619 / SP 800-38E), shaped like the later PolarSSL / mbed TLS
 * API (the reference's aes.c predates the mode; this is written from the
 * standard).  The key is K1 || K2, 256 or 512 bits in all; `tweak` is always
 * an encryption schedule.  Equal halves are accepted. */
typedef struct {
    aes_context crypt; /* K1, the direction of the setkey call */
    aes_context tweak; /* K2 */
} aes_xts_context;
int aes_xts_setkey_enc(aes_xts_context *ctx, const unsigned char *key, unsigned int keybits);
int aes_xts_setkey_dec(aes_xts_context *ctx, const unsigned char *key, unsigned int keybits);
/* one data unit of 16 bytes .. 16 MiB (2^20 blocks); a length that is not a
 * multiple of 16 uses ciphertext stealing.  data_unit: the 128-bit
 * little-endian tweak number.  May run in place. */
int aes_crypt_xts(aes_xts_context *ctx, int mode, size_t length, const unsigned char data_unit[16],
                  const unsigned char *input, unsigned char *output);
/* nunits consecutive units; unit s uses tweak0 + s (128-bit little-endian
 * add, carry through all 16 bytes).  unit_bytes % 16 == 0 unless nunits == 1. */
int aes_crypt_xts_units(aes_xts_context *ctx, int mode, size_t unit_bytes, size_t nunits,
                        const unsigned char tweak0[16], const unsigned char *input, unsigned char *output);

/* AES-GCM (NIST SP 800-38D), written from the standard (the reference has no
 * authenticated mode).  The host GHASH is the tests' oracle and hashes AAD
 * and IVs for the device calls; it is table driven but no fast path. */
#define POLARSSL_ERR_GCM_AUTH_FAILED -0x0012
#define AES_GCM_MAX_BYTES ((((uint64_t)1) << 36) - 32) /* plaintext bytes of one message */
typedef struct {
    aes_context enc;          /* K, an encryption schedule (GCM never decrypts a block) */
    unsigned char h[16];      /* H = E_K(0^128) */
    uint64_t tab[32][16][2];  /* tab[p][n] = (nibble n at nibble position p) . H, as 16 memory-order bytes */
} aes_gcm_context;
int aes_gcm_setkey(aes_gcm_context *ctx, const unsigned char *key, unsigned int keybits);
/* GHASH under an H given directly (ctx->enc is left alone) */
void aes_gcm_set_h(aes_gcm_context *ctx, const unsigned char h[16]);
/* z = x . y in GF(2^128), GCM's bit order; a bit loop, for constants */
void aes_gf128_mul(unsigned char z[16], const unsigned char x[16], const unsigned char y[16]);
/* y = GHASH_H continued from y over len bytes, the last partial block zero-padded */
void aes_ghash(const aes_gcm_context *ctx, unsigned char y[16], const unsigned char *data, size_t len);
/* J0: IV || 0^31 || 1 for 12-byte IVs, else GHASH(IV padded || 0^64 || [8 iv_len]_64) */
void aes_gcm_j0(const aes_gcm_context *ctx, const unsigned char *iv, size_t iv_len, unsigned char j0[16]);
/* GCM's counter mode: bytes 12..15 of ctr increment big-endian and wrap at
 * 2^32 without carry; ctr is left at the next block's value */
int aes_crypt_ctr32(aes_gcm_context *ctx, size_t length, unsigned char ctr[16], const unsigned char *input,
                    unsigned char *output);
/* mode AES_ENCRYPT / AES_DECRYPT; tag: the COMPUTED tag in both directions.
 * iv_len >= 1, length <= AES_GCM_MAX_BYTES.  May run in place. */
int aes_crypt_gcm(aes_gcm_context *ctx, int mode, size_t length, const unsigned char *iv, size_t iv_len,
                  const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                  unsigned char tag[16]);
/* decrypts and compares tag_len (4..16) tag bytes in constant time; on a
 * mismatch output is zeroed and POLARSSL_ERR_GCM_AUTH_FAILED returned */
int aes_gcm_auth_decrypt(aes_gcm_context *ctx, size_t length, const unsigned char *iv, size_t iv_len,
                         const unsigned char *aad, size_t aad_len, const unsigned char *tag, size_t tag_len,
                         const unsigned char *input, unsigned char *output);

/* AES-GCM-SIV (RFC 8452), written from the RFC: the nonce-misuse-resistant
 * AEAD.  The caller's key is a key-GENERATING key (128 or 256 bits; `kgk` is
 * its encryption schedule): every nonce (exactly 12 bytes) derives a POLYVAL
 * key and an encryption key from it.  The tag is E(POLYVAL over AAD and
 * PLAINTEXT, folded with the nonce), and the counter mode starts at the tag
 * with bit 7 of byte 15 set; its counter is bytes 0..3, little-endian.  The
 * tag is always 16 bytes; plaintext and AAD have at most 2^36 bytes each. */
#define AES_GCM_SIV_MAX_BYTES (((uint64_t)1) << 36)
/* z = dot(x, y) = x . y . x^-128 in POLYVAL's field and little-endian bit
 * order; a bit loop, for constants */
void aes_polyval_dot(unsigned char z[16], const unsigned char x[16], const unsigned char y[16]);
/* y = POLYVAL under h continued from y over len bytes, the last partial block zero-padded */
void aes_polyval(const unsigned char h[16], unsigned char y[16], const unsigned char *data, size_t len);
/* RFC 8452 section 4: block i is E_K(le32(i) || nonce)[0:8]; blocks 0..1 are
 * the authentication key, 2..3 (AES-128) or 2..5 (AES-256) the encryption
 * key.  Returns the encryption key's bytes (16 or 32), or
 * POLARSSL_ERR_AES_INVALID_KEY_LENGTH for a 192-bit schedule. */
int aes_gcmsiv_derive(aes_context *kgk, const unsigned char nonce[12], unsigned char authkey[16],
                      unsigned char enckey[32]);
/* GCM-SIV's counter mode: bytes 0..3 of ctr increment little-endian and wrap
 * at 2^32 without carry, bytes 4..15 never change; ctr is left at the next
 * block's value */
int aes_crypt_ctr_le32(aes_context *enc, size_t length, unsigned char ctr[16], const unsigned char *input,
                       unsigned char *output);
/* mode AES_ENCRYPT / AES_DECRYPT; tag: the COMPUTED tag in both directions.
 * A decryption runs its counter mode from tag_in, the received tag (an
 * encryption ignores it).  May run in place. */
int aes_crypt_gcmsiv(aes_context *kgk, int mode, size_t length, const unsigned char nonce[12],
                     const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                     const unsigned char *tag_in, unsigned char tag[16]);
/* decrypts and compares the 16 tag bytes in constant time; on a mismatch
 * output is zeroed and POLARSSL_ERR_GCM_AUTH_FAILED returned */
int aes_gcmsiv_auth_decrypt(aes_context *kgk, size_t length, const unsigned char nonce[12], const unsigned char *aad,
                            size_t aad_len, const unsigned char tag[16], const unsigned char *input,
                            unsigned char *output);
/* the RFC's POLYVAL, derivation and sealed vectors (part of aes_self_test);
 * returns how many failed */
int aes_gcmsiv_self_test(int verbose);

/* AES-OCB3 (RFC 7253), written from the RFC (the reference has no
 * authenticated mode): one block-cipher call per block, the tag from an XOR of
 * the plaintext blocks.  Offset_i = Offset_0 ^ XOR{ L_j : bit j of i ^ (i >> 1) },
 * so every block is independent; a message has at most 2^36 bytes, block
 * indices reach 2^32 and the table L_0 .. L_32.  Tag lengths are in BYTES
 * (1..16) and enter the nonce block: another length, another ciphertext. */
#define POLARSSL_ERR_OCB_AUTH_FAILED -0x0014
#define AES_OCB_MAX_BYTES (((uint64_t)1) << 36)
#define AES_OCB_MAX_BLOCKS (((uint64_t)1) << 32)
typedef struct {
    aes_context enc;             /* K, encryption schedule */
    aes_context dec;             /* K, decryption schedule */
    unsigned char l_star[16];    /* L_* = E_K(0^128) */
    unsigned char l_dollar[16];  /* L_$ = double(L_*) */
    unsigned char l[33][16];     /* L_0 = double(L_$), L_j = double(L_{j-1}) */
} aes_ocb_context;
int aes_ocb_setkey(aes_ocb_context *ctx, const unsigned char *key, unsigned int keybits);
/* Offset_0 of (nonce, tag length): nonce_len 1..15, tag_len 1..16 bytes */
int aes_ocb_offset0(const aes_ocb_context *ctx, const unsigned char *nonce, size_t nonce_len, size_t tag_len,
                    unsigned char out[16]);
/* Offset_i by the closed form, 0 <= i <= 2^32 */
void aes_ocb_offset(const aes_ocb_context *ctx, const unsigned char offset0[16], uint64_t i, unsigned char out[16]);
/* HASH(K, A); an empty A hashes to 0 */
void aes_ocb_hash(const aes_ocb_context *ctx, const unsigned char *aad, size_t len, unsigned char out[16]);
/* blocks first_block + 1 .. first_block + nblocks of the message whose
 * Offset_0 is given; the XOR of their plaintexts is XORed into checksum.
 * first_block + nblocks <= 2^32.  May run in place. */
int aes_crypt_ocb_blocks(const aes_ocb_context *ctx, int mode, const unsigned char offset0[16], uint64_t first_block,
                         uint64_t nblocks, const unsigned char *input, unsigned char *output,
                         unsigned char checksum[16]);
/* mode AES_ENCRYPT / AES_DECRYPT; tag: the COMPUTED tag in both directions,
 * its first tag_len bytes, the rest of the 16 zero.  May run in place. */
int aes_crypt_ocb(const aes_ocb_context *ctx, int mode, size_t length, const unsigned char *nonce, size_t nonce_len,
                  const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                  unsigned char tag[16], size_t tag_len);
/* decrypts and compares the tag_len (1..16) tag bytes in constant time; on a
 * mismatch output is zeroed and POLARSSL_ERR_OCB_AUTH_FAILED returned */
int aes_ocb_auth_decrypt(const aes_ocb_context *ctx, size_t length, const unsigned char *nonce, size_t nonce_len,
                         const unsigned char *aad, size_t aad_len, const unsigned char *tag, size_t tag_len,
                         const unsigned char *input, unsigned char *output);

/* AES-CCM (NIST SP 800-38C, RFC 3610), written from the two documents (the
 * reference has no authenticated mode).  nonce_len 7..13 bytes (L = 15 -
 * nonce_len), tag_len one of 4, 6, .., 16 bytes, length < 2^(8L), aad_len <
 * 2^32 (the 2- and the 6-byte length encodings).  ctx: the ENCRYPTION schedule,
 * in both directions.  May run in place. */
#define POLARSSL_ERR_CCM_AUTH_FAILED -0x0016
/* mode AES_ENCRYPT / AES_DECRYPT; tag: the COMPUTED tag in both directions,
 * its first tag_len bytes, the rest of the 16 zero */
int aes_crypt_ccm(const aes_context *ctx, int mode, size_t length, const unsigned char *nonce, size_t nonce_len,
                  const unsigned char *aad, size_t aad_len, const unsigned char *input, unsigned char *output,
                  unsigned char tag[16], size_t tag_len);
/* decrypts and compares the tag_len tag bytes in constant time; on a mismatch
 * output is zeroed and POLARSSL_ERR_CCM_AUTH_FAILED returned */
int aes_ccm_auth_decrypt(const aes_context *ctx, size_t length, const unsigned char *nonce, size_t nonce_len,
                         const unsigned char *aad, size_t aad_len, const unsigned char *tag, size_t tag_len,
                         const unsigned char *input, unsigned char *output);

/* Monte-Carlo known-answer chains of the reference self-test
 * (aes-modes/aes.c:1084-1200): 10,000 chained operations from an all-zero
 * key / block / IV.  aes_monte_carlo writes the final block (CBC-enc: the last
 * ciphertext); aes_monte_carlo_expected returns the published value (hex). */
#define AES_MC_ECB_ENC 0
#define AES_MC_ECB_DEC 1
#define AES_MC_CBC_ENC 2
#define AES_MC_CBC_DEC 3
int aes_monte_carlo(int mode, int bits, unsigned char result[16]);
const char *aes_monte_carlo_expected(int mode, int bits);

/* 128-bit big-endian counter add: ctr += blocks. */
void aes_ctr128_add(unsigned char ctr[16], uint64_t blocks);

/* Raw tables (generated on first use), exposed for table-driven kernels and
 * tests: forward S-box, inverse S-box, forward T0 and inverse T0 tables. */
const uint8_t  *aes_sbox(void);
const uint8_t  *aes_inv_sbox(void);
const uint32_t *aes_te0(void);
const uint32_t *aes_td0(void);

#ifdef __cplusplus
}
#endif

#endif /* OTC_AES_H */
