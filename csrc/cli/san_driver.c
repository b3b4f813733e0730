/*
 * san_driver.c -- exercises every multi-threaded and table-initialising path
 * of the CPU library under a sanitizer build (tests/test_sanitizers_cpu.py
 * builds it with -fsanitize=thread and with -fsanitize=address,undefined).
 *
 * Covers the reference's real races: the lazily built
 * AES tables (reference aes.c:359,448-452 set aes_init_done without any
 * synchronisation; here pthread_once) hit from many threads at once, and the
 * threaded CTR / ECB / XOR workers with remainders (reference test.c:50 and
 * aes-modes/test.c:33 drop them).  Every threaded result is compared with the
 * single-threaded one.  The ChaCha20 / Poly1305 / AEAD oracle (chacha.c) runs
 * over exactly sized heap buffers at every length around its block sizes, so
 * an out-of-bounds access or a misaligned word access shows.  Exit code 0 =
 * all equal.  That part needs csrc/cpu/chacha.c and -DOTC_SAN_CHACHA; without
 * the macro the driver is the AES / ARC4 one it was.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aes.h"
#include "arc4.h"
#ifdef OTC_SAN_CHACHA /* built with csrc/cpu/chacha.c (make san-check does) */
#include "chacha.h"
#endif

#define NT 8

static unsigned char g_key[32];

static void *setkey_worker(void *arg)
{
    aes_context ctx;
    unsigned char blk[16] = {0}, out[16];
    int bits = 128 + 64 * (int)((size_t)arg % 3);
    if (aes_setkey_enc(&ctx, g_key, (unsigned)bits) != 0) return (void *)1;
    aes_crypt_ecb(&ctx, AES_ENCRYPT, blk, out);
    if (aes_setkey_dec(&ctx, g_key, (unsigned)bits) != 0) return (void *)1;
    aes_crypt_ecb(&ctx, AES_DECRYPT, out, blk);
    for (int i = 0; i < 16; ++i)
        if (blk[i]) return (void *)1;
    return NULL;
}

static int check(const char *what, const unsigned char *a, const unsigned char *b, size_t n)
{
    if (memcmp(a, b, n)) {
        fprintf(stderr, "MISMATCH %s\n", what);
        return 1;
    }
    return 0;
}

#ifdef OTC_SAN_CHACHA
/* chacha.c over heap buffers of exactly n bytes (ASan redzones right behind
 * them), odd offsets included: split calls equal one call, the AEAD round
 * trips, a flipped bit is refused with zeroed output, the counter wrap is
 * refused with the output untouched */
static int chacha_checks(void)
{
    int bad = 0;
    unsigned char nonce[12], tag[16], tag2[16];
    for (int i = 0; i < 12; ++i) nonce[i] = (unsigned char)(0xA0 + i);
    for (size_t n = 0; n <= 200; ++n) {
        unsigned char *in = malloc(n + 1), *o1 = malloc(n + 1), *o2 = malloc(n + 1), *aad = malloc(n % 37 + 1);
        for (size_t i = 0; i < n; ++i) in[i] = (unsigned char)(i * 73 + n);
        for (size_t i = 0; i < n % 37; ++i) aad[i] = (unsigned char)(i + 1);
        /* one call against a call split on a block boundary (from offset 1: unaligned words) */
        bad |= chacha20_crypt(g_key, nonce, 7, in + 1, o1 + 1, n) != 0;
        const size_t head = n >= 64 ? 64 : 0;
        bad |= chacha20_crypt(g_key, nonce, 7, in + 1, o2 + 1, head) != 0;
        bad |= chacha20_crypt(g_key, nonce, 7 + (uint32_t)(head / 64), in + 1 + head, o2 + 1 + head, n - head) != 0;
        bad |= check("chacha20 split", o1 + 1, o2 + 1, n);
        poly1305_mac(g_key, in + 1, n, tag);
        poly1305_mac(g_key, in + 1, n, tag2);
        bad |= check("poly1305", tag, tag2, 16);
        /* the AEAD: round trip, then a flipped tag bit */
        bad |= chacha20_poly1305_encrypt(g_key, nonce, aad, n % 37, in + 1, o1 + 1, n, tag) != 0;
        bad |= chacha20_poly1305_auth_decrypt(g_key, nonce, aad, n % 37, tag, o1 + 1, o2 + 1, n) != 0;
        bad |= check("chacha20_poly1305 round trip", in + 1, o2 + 1, n);
        tag[n % 16] ^= 1;
        memset(o2, 0xA5, n + 1);
        bad |= chacha20_poly1305_auth_decrypt(g_key, nonce, aad, n % 37, tag, o1 + 1, o2 + 1, n) != CHACHA_ERR_AUTH_FAILED;
        for (size_t i = 0; i < n; ++i) bad |= o2[1 + i] != 0;
        bad |= o2[0] != 0xA5;
        free(in);
        free(o1);
        free(o2);
        free(aad);
    }
    /* the wrap: the last block may be 2^32 - 1 and no further */
    unsigned char buf[65], out[65];
    memset(buf, 1, sizeof buf);
    memset(out, 0xA5, sizeof out);
    bad |= chacha20_crypt(g_key, nonce, 0xFFFFFFFFu, buf, out, 64) != 0;
    memset(out, 0xA5, sizeof out);
    bad |= chacha20_crypt(g_key, nonce, 0xFFFFFFFFu, buf, out, 65) != CHACHA_ERR_COUNTER;
    for (int i = 0; i < 65; ++i) bad |= out[i] != 0xA5;
    if (bad) fprintf(stderr, "MISMATCH chacha\n");
    return bad;
}
#else
static int chacha_checks(void) { return 0; }
#endif

int main(void)
{
    int bad = 0;
    for (int i = 0; i < 32; ++i) g_key[i] = (unsigned char)(17 * i + 3);

    /* 1. first table use from NT threads at once */
    pthread_t th[NT];
    for (size_t i = 0; i < NT; ++i) pthread_create(&th[i], NULL, setkey_worker, (void *)i);
    for (int i = 0; i < NT; ++i) {
        void *r = NULL;
        pthread_join(th[i], &r);
        bad |= r != NULL;
    }

    /* 2. threaded bulk helpers vs one thread, odd length (remainders) */
    const size_t n = 3 * 4096 + 16 * 7 + 5, ne = n & ~(size_t)15;
    unsigned char *in = malloc(n), *o1 = malloc(n), *o8 = malloc(n), *ks = malloc(n);
    for (size_t i = 0; i < n; ++i) {
        in[i] = (unsigned char)(i * 131 + 7);
        ks[i] = (unsigned char)(i * 29 + 1);
    }
    unsigned char ctr0[16];
    memset(ctr0, 0xFF, 16);
    ctr0[0] = 0x12; /* forces a carry through 64-bit words mid-buffer */
    aes_context ctx;
    aes_setkey_enc(&ctx, g_key, 256);
    aes_ctr_bulk(&ctx, ctr0, in, o1, n, 1);
    aes_ctr_bulk(&ctx, ctr0, in, o8, n, NT);
    bad |= check("aes_ctr_bulk", o1, o8, n);
    aes_ecb_bulk(&ctx, AES_ENCRYPT, in, o1, ne, 1);
    aes_ecb_bulk(&ctx, AES_ENCRYPT, in, o8, ne, NT);
    bad |= check("aes_ecb_bulk", o1, o8, ne);
    arc4_crypt_mt(n, in, ks, o1, 1);
    arc4_crypt_mt(n, in, ks, o8, NT);
    bad |= check("arc4_crypt_mt", o1, o8, n);

    /* 3. self tests (both ciphers, every mode) */
    bad |= aes_self_test(0) != 0;
    bad |= arc4_self_test(0) != 0;

    /* 4. ChaCha20, Poly1305 and the AEAD */
    bad |= chacha_checks();

    free(in);
    free(o1);
    free(o8);
    free(ks);
    printf(bad ? "san_driver: FAIL\n" : "san_driver: OK\n");
    return bad;
}
