/*
 * chacha.h -- CPU oracle of ChaCha20, Poly1305 and the ChaCha20-Poly1305 AEAD
 * (RFC 8439), written from the RFC.  The device kernels (csrc/hip/chacha.hip)
 * are verified against these functions.
 *
 * Layout: the IETF one -- state words 0-3 the constants, 4-11 the key, 12 the
 * 32-bit block counter, 13-15 the 96-bit nonce, all little-endian.
 *
 * Counter wrap: RFC 8439 leaves a 32-bit counter overflow undefined and
 * implementations differ (some carry into the first nonce word, some wrap to
 * 0 and repeat keystream).  These functions refuse: a call whose last block
 * index would exceed 2^32 - 1 returns CHACHA_ERR_COUNTER and touches nothing.
 */
#ifndef OTC_CHACHA_H
#define OTC_CHACHA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHACHA_ERR_COUNTER -0x0024     /* the block counter would pass 2^32 - 1 */
#define CHACHA_ERR_AUTH_FAILED -0x0012 /* the tag did not match; the output was zeroed */
/* bytes of one AEAD message: counters 1 .. 2^32 - 1 */
#define CHACHA20_POLY1305_MAX_BYTES ((((uint64_t)1 << 32) - 1) * 64)

/* one 64-byte keystream block */
void chacha20_block(const unsigned char key[32], const unsigned char nonce[12], uint32_t counter,
                    unsigned char out[64]);

/* out = in ^ keystream from block `counter`; any byte count, in == out allowed.
 * 0, or CHACHA_ERR_COUNTER with out untouched. */
int chacha20_crypt(const unsigned char key[32], const unsigned char nonce[12], uint32_t counter,
                   const unsigned char *in, unsigned char *out, size_t n);

/* tag = Poly1305 of n bytes under the one-time key r || s (r is clamped here) */
void poly1305_mac(const unsigned char key[32], const unsigned char *data, size_t n, unsigned char tag[16]);

/* The pieces of poly1305_mac for callers that hash in parts (the device
 * engine hashes the AAD on the host): the accumulator as five 26-bit limbs,
 * kept partially reduced (every limb < 2^27). */
typedef struct {
    uint32_t r[5], h[5];
    unsigned char s[16];
} poly1305_state;
void poly1305_init(poly1305_state *st, const unsigned char key[32]);
/* whole 16-byte blocks only (each carries its 2^128 bit) */
void poly1305_blocks(poly1305_state *st, const unsigned char *data, size_t nblocks);
/* a final block of 1..15 bytes (gets the 0x01 byte) */
void poly1305_last(poly1305_state *st, const unsigned char *data, size_t n);
/* data zero-padded to a multiple of 16 (the AEAD's pad16) */
void poly1305_pad16(poly1305_state *st, const unsigned char *data, size_t n);
void poly1305_finish(poly1305_state *st, unsigned char tag[16]);

/* RFC 8439 section 2.8: out = the ciphertext, tag = the 16-byte tag.
 * 0, or CHACHA_ERR_COUNTER for more than CHACHA20_POLY1305_MAX_BYTES. */
int chacha20_poly1305_encrypt(const unsigned char key[32], const unsigned char nonce[12], const unsigned char *aad,
                              size_t aad_len, const unsigned char *in, unsigned char *out, size_t n,
                              unsigned char tag[16]);
/* compares the tag in constant time; on a mismatch zeroes out and returns
 * CHACHA_ERR_AUTH_FAILED */
int chacha20_poly1305_auth_decrypt(const unsigned char key[32], const unsigned char nonce[12],
                                   const unsigned char *aad, size_t aad_len, const unsigned char tag[16],
                                   const unsigned char *in, unsigned char *out, size_t n);
/* the computed tag of a ciphertext (what both directions of the device call return) */
int chacha20_poly1305_tag(const unsigned char key[32], const unsigned char nonce[12], const unsigned char *aad,
                          size_t aad_len, const unsigned char *ct, size_t n, unsigned char tag[16]);

#ifdef __cplusplus
}
#endif

#endif
