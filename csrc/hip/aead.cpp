/*
 * aead.cpp -- the hash and authenticated-encryption ops of the C API (otc.h):
 * GHASH and AES-GCM (counter mode: engine.cpp's ctr32_run; hash: aes_gcm.hip),
 * AES-OCB3 (aes_ocb.hip),
 * ChaCha20, Poly1305 and ChaCha20-Poly1305 (chacha.hip), batched GCM
 * (aes_gcm_batch.hip and the batched CTR kernel), batched
 * ChaCha20-Poly1305 (chacha_batch.hip), batched OCB3
 * (aes_ocb_batch.hip), batched CCM (aes_ccm_batch.hip), batched GCM-SIV
 * (aes_gcm_siv_batch.hip) and batched GCM
 * with a key per record (aes_gcm_mk_batch.hip): the argument checks, what an
 * op computes on the host (J0, the AAD's hash, the one-time key, the length
 * blocks) and the order of its launches.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <cstdint>
#include <string>
#include <vector>

#include "aes.h"
#include "chacha.h"
#include "otc.h"
#include "otc_device.h"
#include "engine_internal.h"
#include "ccm_dev.h"

using namespace otc_rt;

/* a hash workspace that could not be had, as the caller's error: no memory,
 * more bytes than the hash's levels reach (where the op has no check of its
 * own in front: `too_many`), or whatever else HIP said, behind `what` */
static int ws_fail(hipError_t e, const char *what, const std::string &nomem, const std::string &too_many = "")
{
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return set_err(OTC_ERR_NOMEM, nomem);
    if (e == hipErrorInvalidValue && !too_many.empty()) return set_err(OTC_ERR_ARG, too_many);
    return hip_fail(e, what);
}

/* ---- GHASH, the GCM key, AES-GCM ------------------------------------------ */
extern "C" int otc_ghash_spans(uint64_t *spans, int max) { return otc_impl::ghash_spans(spans, spans ? max : 0); }

extern "C" int otc_ghash(const void *data, size_t nbytes, const uint8_t h[16], const uint8_t y0[16], void *y_dev,
                         void *stream)
{
    Range rg("otc_ghash");
    if (!h || !y0 || !y_dev) return set_err(OTC_ERR_ARG, "null argument");
    if ((uintptr_t)y_dev & 3u) return set_err(OTC_ERR_ARG, "ghash: the result must be 4-byte aligned");
    if (nbytes > ((uint64_t)1 << 36)) return set_err(OTC_ERR_ARG, "ghash: more than 2^36 bytes");
    if (nbytes && !data) return set_err(OTC_ERR_ARG, "ghash: null buffer");
    if ((uintptr_t)data & 15u) return set_err(OTC_ERR_ARG, "ghash: device buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    void *ws = nullptr;
    hipError_t e = otc_impl::ghash_ws_alloc(nbytes, st, &ws);
    if (e != hipSuccess) return ws_fail(e, "ghash workspace", "ghash: no memory for the tables and partials");
    e = otc_impl::ghash_run(data, nbytes, h, y0, nullptr, nullptr, y_dev, ws, st);
    if (e != hipSuccess) return hip_fail(e, "ghash launch");
    return OTC_OK;
}

extern "C" int otc_gcm_key_init(otc_gcm_key *k, const uint8_t *key, int keybits)
{
    if (!k || !key) return set_err(OTC_ERR_ARG, "null argument");
    aes_gcm_context g;
    if (aes_gcm_setkey(&g, key, (unsigned)keybits)) return set_err(OTC_ERR_ARG, "invalid AES key size (must be 128/192/256)");
    if (int r = otc_aes_key_init(&k->enc, key, keybits, OTC_DIR_ENCRYPT)) return r;
    memcpy(k->h, g.h, 16);
    return OTC_OK;
}

extern "C" int otc_aes_gcm(const void *in, void *out, size_t nbytes, const otc_gcm_key *k, int dir, const uint8_t *iv,
                           size_t iv_len, const uint8_t *aad, size_t aad_len, void *tag_dev, int impl, void *stream)
{
    Range rg("otc_aes_gcm");
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(&k->enc, OTC_DIR_ENCRYPT)) return r;
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (!iv || iv_len == 0) return set_err(OTC_ERR_ARG, "gcm: the IV must have at least 1 byte");
    if (aad_len && !aad) return set_err(OTC_ERR_ARG, "gcm: null aad");
    if ((uint64_t)iv_len >> 61 || (uint64_t)aad_len >> 61) return set_err(OTC_ERR_ARG, "gcm: IV or AAD too long");
    if (!tag_dev || ((uintptr_t)tag_dev & 3u)) return set_err(OTC_ERR_ARG, "gcm: the tag must be 4-byte aligned device memory");
    if (nbytes > AES_GCM_MAX_BYTES) return set_err(OTC_ERR_ARG, "gcm: a message has at most 2^36 - 32 bytes");
    if (int r = check_bufs(in, out, nbytes, true, "aes_gcm")) return r;
    if (int r = check_impl(impl)) return r;
    hipStream_t st = (hipStream_t)stream;

    /* what does not depend on the data, on the host */
    aes_gcm_context g;
    aes_import_rk32(&g.enc, k->enc.rk, k->enc.nr);
    aes_gcm_set_h(&g, k->h);
    uint8_t j0[16], ekj0[16], ctr[16], y0[16] = {0}, lenblock[16];
    aes_gcm_j0(&g, iv, iv_len, j0);
    aes_crypt_ecb(&g.enc, AES_ENCRYPT, j0, ekj0);
    memcpy(ctr, j0, 16);
    for (int i = 15; i >= 12; --i)
        if (++ctr[i]) break;
    aes_ghash(&g, y0, aad, aad_len);
    store_be64(lenblock, (uint64_t)aad_len * 8);
    store_be64(lenblock + 8, (uint64_t)nbytes * 8);

    /* the hash's memory first: a failure leaves out and the tag untouched */
    void *ws = nullptr;
    hipError_t e = otc_impl::ghash_ws_alloc(nbytes, st, &ws);
    if (e != hipSuccess) return ws_fail(e, "gcm workspace", "gcm: no memory for the hash's tables and partials");
    if (dir == OTC_DIR_ENCRYPT && nbytes) {
        if (int r = ctr32_run(in, out, nbytes, &k->enc, ctr, impl, stream)) {
            if (ws) (void)otc_dev::ws_free(ws, st);
            return r;
        }
    }
    /* over the ciphertext: out of an encryption, in of a decryption */
    e = otc_impl::ghash_run(dir == OTC_DIR_ENCRYPT ? out : in, nbytes, k->h, y0, lenblock, ekj0, tag_dev, ws, st);
    if (e != hipSuccess) return hip_fail(e, "gcm hash launch");
    if (dir == OTC_DIR_DECRYPT && nbytes) return ctr32_run(in, out, nbytes, &k->enc, ctr, impl, stream);
    return OTC_OK;
}

/* ---- POLYVAL, GCM-SIV's counter mode, AES-GCM-SIV (RFC 8452) ------------------ */
extern "C" int otc_polyval_spans(uint64_t *spans, int max) { return otc_impl::polyval_spans(spans, spans ? max : 0); }

extern "C" int otc_ctr_le32_spans(uint64_t *spans, int max) { return otc_impl::ctr_le32_spans(spans, spans ? max : 0); }

extern "C" int otc_polyval(const void *data, size_t nbytes, const uint8_t h[16], const uint8_t y0[16], void *y_dev,
                           void *stream)
{
    Range rg("otc_polyval");
    if (!h || !y0 || !y_dev) return set_err(OTC_ERR_ARG, "null argument");
    if ((uintptr_t)y_dev & 3u) return set_err(OTC_ERR_ARG, "polyval: the result must be 4-byte aligned");
    if (nbytes > OTC_GCM_SIV_MAX_BYTES) return set_err(OTC_ERR_ARG, "polyval: more than 2^36 bytes");
    if (nbytes && !data) return set_err(OTC_ERR_ARG, "polyval: null buffer");
    if ((uintptr_t)data & 15u) return set_err(OTC_ERR_ARG, "polyval: device buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    void *ws = nullptr;
    hipError_t e = otc_impl::polyval_ws_alloc(nbytes, st, &ws);
    if (e != hipSuccess) return ws_fail(e, "polyval workspace", "polyval: no memory for the tables and partials");
    e = otc_impl::polyval_run(data, nbytes, h, y0, nullptr, y_dev, ws, st);
    if (e != hipSuccess) return hip_fail(e, "polyval launch");
    return OTC_OK;
}

/* [a, a + 16) meets [b, b + n) */
static bool tag_overlaps(const void *a, const void *b, size_t n)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return n && x < y + n && y < x + 16;
}

extern "C" int otc_aes_ctr_le32(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const void *ctr0_dev,
                                void *stream)
{
    Range rg("otc_aes_ctr_le32");
    if (int r = check_key(k, OTC_DIR_ENCRYPT)) return r;
    if (!ctr0_dev || ((uintptr_t)ctr0_dev & 3u))
        return set_err(OTC_ERR_ARG, "aes_ctr_le32: the counter block must be 4-byte aligned device memory");
    if (nbytes > OTC_GCM_SIV_MAX_BYTES) return set_err(OTC_ERR_ARG, "aes_ctr_le32: more than 2^32 blocks");
    if (int r = check_bufs(in, out, nbytes, true, "aes_ctr_le32")) return r;
    if (tag_overlaps(ctr0_dev, out, nbytes)) return set_err(OTC_ERR_ARG, "aes_ctr_le32: the counter block lies in the output");
    set_last_impl(OTC_IMPL_TTABLE);
    const hipError_t e = otc_impl::ctr_le32_run(in, out, nbytes, *k, ctr0_dev, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "aes_ctr_le32 launch");
    return OTC_OK;
}

extern "C" int otc_gcm_siv_key_init(otc_gcm_siv_key *k, const uint8_t *key, int keybits)
{
    if (!k || !key) return set_err(OTC_ERR_ARG, "null argument");
    if (keybits != 128 && keybits != 256) return set_err(OTC_ERR_ARG, "gcm_siv: the key has 128 or 256 bits");
    return otc_aes_key_init(&k->kgk, key, keybits, OTC_DIR_ENCRYPT);
}

extern "C" int otc_aes_gcm_siv(const void *in, void *out, size_t nbytes, const otc_gcm_siv_key *k, int dir,
                               const uint8_t nonce[12], const uint8_t *aad, size_t aad_len, const void *tag_in_dev,
                               void *tag_dev, void *stream)
{
    Range rg("otc_aes_gcm_siv");
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(&k->kgk, OTC_DIR_ENCRYPT)) return r;
    if (k->kgk.nr != 10 && k->kgk.nr != 14) return set_err(OTC_ERR_ARG, "gcm_siv: the key has 128 or 256 bits");
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (!nonce) return set_err(OTC_ERR_ARG, "gcm_siv: null nonce");
    if (aad_len && !aad) return set_err(OTC_ERR_ARG, "gcm_siv: null aad");
    if ((uint64_t)aad_len > OTC_GCM_SIV_MAX_BYTES) return set_err(OTC_ERR_ARG, "gcm_siv: the AAD has at most 2^36 bytes");
    if (!tag_dev || ((uintptr_t)tag_dev & 3u))
        return set_err(OTC_ERR_ARG, "gcm_siv: the tag must be 4-byte aligned device memory");
    const bool enc = dir == OTC_DIR_ENCRYPT;
    if (!enc && (!tag_in_dev || ((uintptr_t)tag_in_dev & 3u)))
        return set_err(OTC_ERR_ARG, "gcm_siv: decryption needs the received tag, 4-byte aligned device memory");
    if ((uint64_t)nbytes > OTC_GCM_SIV_MAX_BYTES) return set_err(OTC_ERR_ARG, "gcm_siv: a message has at most 2^36 bytes");
    if (int r = check_bufs(in, out, nbytes, true, "aes_gcm_siv")) return r;
    /* the counter mode reads a tag while it writes out, and the hash reads in (out) before the tag is written */
    if (tag_overlaps(tag_dev, out, nbytes) || tag_overlaps(tag_dev, in, nbytes) ||
        (!enc && tag_overlaps(tag_in_dev, out, nbytes)))
        return set_err(OTC_ERR_ARG, "gcm_siv: a tag lies in the data");
    hipStream_t st = (hipStream_t)stream;
    set_last_impl(OTC_IMPL_TTABLE);

    /* what does not depend on the data, on the host: the nonce's two keys, the
     * AAD's hash state, the length block */
    aes_context kgk;
    aes_import_rk32(&kgk, k->kgk.rk, k->kgk.nr);
    uint8_t authkey[16], enckey[32], y0[16] = {0};
    const int enc_bytes = aes_gcmsiv_derive(&kgk, nonce, authkey, enckey);
    otc_aes_key ek;
    if (enc_bytes < 0) return set_err(OTC_ERR_ARG, "gcm_siv: the key has 128 or 256 bits");
    if (int r = otc_aes_key_init(&ek, enckey, enc_bytes * 8, OTC_DIR_ENCRYPT)) return r;
    aes_polyval(authkey, y0, aad, aad_len);
    otc_impl::SivTag siv{};
    for (int i = 0; i < 8; ++i) {
        siv.lenblock[i] = (uint8_t)(((uint64_t)aad_len * 8) >> (8 * i));
        siv.lenblock[8 + i] = (uint8_t)(((uint64_t)nbytes * 8) >> (8 * i));
    }
    memcpy(siv.nonce, nonce, 12);
    siv.enc = &ek;

    /* the hash's memory first: a failure leaves out and the tag untouched */
    void *ws = nullptr;
    hipError_t e = otc_impl::polyval_ws_alloc(nbytes, st, &ws);
    if (e != hipSuccess) return ws_fail(e, "gcm_siv workspace", "gcm_siv: no memory for the hash's tables and partials");
    /* a decryption's counter mode starts at the RECEIVED tag, in device memory as it is */
    if (!enc && (e = otc_impl::ctr_le32_run(in, out, nbytes, ek, tag_in_dev, st)) != hipSuccess) {
        if (ws) (void)otc_dev::ws_free(ws, st);
        return hip_fail(e, "gcm_siv ctr launch");
    }
    /* over the plaintext: in of an encryption, out of a decryption */
    e = otc_impl::polyval_run(enc ? in : out, nbytes, authkey, y0, &siv, tag_dev, ws, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_siv hash launch");
    /* an encryption's starts at the tag the finisher has just written */
    if (enc && (e = otc_impl::ctr_le32_run(in, out, nbytes, ek, tag_dev, st)) != hipSuccess)
        return hip_fail(e, "gcm_siv ctr launch");
    return OTC_OK;
}

/* ---- AES-OCB3 (RFC 7253) ---------------------------------------------------- */
extern "C" int otc_ocb_spans(uint64_t *spans, int max) { return otc_impl::ocb_spans(spans, spans ? max : 0); }

extern "C" int otc_ocb_key_init(otc_ocb_key *k, const uint8_t *key, int keybits)
{
    if (!k || !key) return set_err(OTC_ERR_ARG, "null argument");
    aes_ocb_context c;
    if (aes_ocb_setkey(&c, key, (unsigned)keybits)) return set_err(OTC_ERR_ARG, "invalid AES key size (must be 128/192/256)");
    if (int r = otc_aes_key_init(&k->enc, key, keybits, OTC_DIR_ENCRYPT)) return r;
    if (int r = otc_aes_key_init(&k->dec, key, keybits, OTC_DIR_DECRYPT)) return r;
    memcpy(k->l_star, c.l_star, 16);
    memcpy(k->l_dollar, c.l_dollar, 16);
    memcpy(k->l, c.l, sizeof k->l);
    return OTC_OK;
}

/* what both OCB calls check of the key and the direction */
static int ocb_check_key(const otc_ocb_key *k, int dir)
{
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(&k->enc, OTC_DIR_ENCRYPT)) return r;
    if (int r = check_key(&k->dec, OTC_DIR_DECRYPT)) return r;
    if (k->enc.nr != k->dec.nr) return set_err(OTC_ERR_ARG, "ocb: the two schedules are of different keys");
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    return OTC_OK;
}

/* the host oracle's context over the key's encryption schedule and L table:
 * the offsets and the AAD's hash never run the inverse cipher, so c.dec stays unset */
static void ocb_host_ctx(aes_ocb_context &c, const otc_ocb_key *k)
{
    aes_import_rk32(&c.enc, k->enc.rk, k->enc.nr);
    memcpy(c.l_star, k->l_star, 16);
    memcpy(c.l_dollar, k->l_dollar, 16);
    memcpy(c.l, k->l, sizeof c.l);
}

extern "C" int otc_aes_ocb_blocks(const void *in, void *out, uint64_t nblocks, const otc_ocb_key *k, int dir,
                                  const uint8_t offset0[16], uint64_t first_block, void *checksum_dev, void *stream)
{
    Range rg("otc_aes_ocb_blocks");
    if (int r = ocb_check_key(k, dir)) return r;
    if (!offset0) return set_err(OTC_ERR_ARG, "ocb_blocks: null offset");
    if (!checksum_dev || ((uintptr_t)checksum_dev & 15u))
        return set_err(OTC_ERR_ARG, "ocb_blocks: the checksum must be 16-byte aligned device memory");
    if (first_block > AES_OCB_MAX_BLOCKS || nblocks > AES_OCB_MAX_BLOCKS - first_block)
        return set_err(OTC_ERR_ARG, "ocb_blocks: block indices would pass 2^32");
    if (int r = check_bufs(in, out, (size_t)nblocks * 16, true, "aes_ocb_blocks")) return r;
    set_last_impl(OTC_IMPL_TTABLE);
    const hipError_t e = otc_impl::ocb_bulk(in, out, first_block, nblocks, dir == OTC_DIR_ENCRYPT ? k->enc : k->dec,
                                            offset0, k->l, checksum_dev, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "aes_ocb_blocks launch");
    return OTC_OK;
}

extern "C" int otc_aes_ocb(const void *in, void *out, size_t nbytes, const otc_ocb_key *k, int dir, const uint8_t *nonce,
                           size_t nonce_len, const uint8_t *aad, size_t aad_len, int tag_bytes, void *tag_dev,
                           void *stream)
{
    Range rg("otc_aes_ocb");
    if (int r = ocb_check_key(k, dir)) return r;
    if (!nonce || nonce_len < 1 || nonce_len > 15) return set_err(OTC_ERR_ARG, "ocb: the nonce has 1 to 15 bytes");
    if (tag_bytes < 1 || tag_bytes > 16) return set_err(OTC_ERR_ARG, "ocb: a tag has 1 to 16 bytes");
    if (aad_len && !aad) return set_err(OTC_ERR_ARG, "ocb: null aad");
    if (!tag_dev || ((uintptr_t)tag_dev & 3u)) return set_err(OTC_ERR_ARG, "ocb: the tag must be 4-byte aligned device memory");
    if ((uint64_t)nbytes > OTC_OCB_MAX_BYTES) return set_err(OTC_ERR_ARG, "ocb: a message has at most 2^36 bytes");
    if (int r = check_bufs(in, out, nbytes, true, "aes_ocb")) return r;
    hipStream_t st = (hipStream_t)stream;
    set_last_impl(OTC_IMPL_TTABLE);

    /* what does not depend on the data, on the host */
    aes_ocb_context c;
    ocb_host_ctx(c, k);
    const uint64_t m = (uint64_t)nbytes / 16;
    const uint32_t r = (uint32_t)(nbytes % 16);
    uint8_t off0[16], off_m[16], hash[16];
    aes_ocb_offset0(&c, nonce, nonce_len, (size_t)tag_bytes, off0);
    aes_ocb_offset(&c, off0, m, off_m);
    aes_ocb_hash(&c, aad, aad_len, hash);

    /* the tag's 16 bytes collect the whole blocks' checksum; the finisher reads it and writes the tag over it */
    hipError_t e = hipSuccess;
    if (m) {
        if ((e = otc_impl::ocb_clear(tag_dev, st)) != hipSuccess) return hip_fail(e, "aes_ocb checksum clear");
        e = otc_impl::ocb_bulk(in, out, 0, m, dir == OTC_DIR_ENCRYPT ? k->enc : k->dec, off0, k->l, tag_dev, st);
        if (e != hipSuccess) return hip_fail(e, "aes_ocb launch");
    }
    e = otc_impl::ocb_finish((const uint8_t *)in + 16 * m, (uint8_t *)out + 16 * m, r, dir == OTC_DIR_DECRYPT, k->enc,
                             off_m, k->l_star, k->l_dollar, hash, tag_bytes, m ? tag_dev : nullptr, tag_dev, st);
    if (e != hipSuccess) return hip_fail(e, "aes_ocb finisher launch");
    return OTC_OK;
}

/* ---- ChaCha20, Poly1305, ChaCha20-Poly1305 (RFC 8439) ---------------------- */
/* what every ChaCha20 call checks before anything is launched: the buffers
 * (any alignment; the same buffer or disjoint) and the 32-bit block counter,
 * which this engine never lets wrap */
static int chacha_check(const void *in, const void *out, size_t nbytes, uint32_t counter, const char *what)
{
    const uint64_t nblk = (uint64_t)nbytes / 64 + (nbytes % 64 ? 1 : 0);
    if ((uint64_t)counter + nblk > ((uint64_t)1 << 32))
        return set_err(OTC_ERR_ARG, std::string(what) + ": the 32-bit block counter would pass 2^32 - 1");
    if (nbytes == 0) return OTC_OK;
    if (!in || !out) return set_err(OTC_ERR_ARG, std::string(what) + ": null buffer");
    if (partial_overlap(in, out, nbytes))
        return set_err(OTC_ERR_ARG, std::string(what) + ": input and output overlap partially");
    return OTC_OK;
}

extern "C" int otc_chacha20(const void *in, void *out, size_t nbytes, const uint8_t key[32], const uint8_t nonce[12],
                            uint32_t counter, void *stream)
{
    Range rg("otc_chacha20");
    if (!key || !nonce) return set_err(OTC_ERR_ARG, "chacha20: null key or nonce");
    if (int r = chacha_check(in, out, nbytes, counter, "chacha20")) return r;
    const hipError_t e = otc_impl::chacha20_run(in, out, nbytes, key, nonce, counter, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "chacha20 launch");
    return OTC_OK;
}

extern "C" int otc_poly1305_spans(uint64_t *spans, int max) { return otc_impl::poly1305_spans(spans, spans ? max : 0); }

/* the hash over device data from a host-side state: workspace first, then the kernels */
static int poly1305_dev(const void *data, size_t nbytes, const poly1305_state &ps, const uint8_t *lenblock, bool pad16,
                        void *tag_dev, void *ws, hipStream_t st, const char *what)
{
    const hipError_t e = otc_impl::poly1305_run(data, nbytes, ps.r, ps.h, ps.s, lenblock, pad16, tag_dev, ws, st);
    if (e != hipSuccess) return hip_fail(e, what);
    return OTC_OK;
}

static int poly1305_ws(size_t nbytes, hipStream_t st, void **ws, const char *what)
{
    const hipError_t e = otc_impl::poly1305_ws_alloc(nbytes, st, ws);
    if (e == hipSuccess) return OTC_OK;
    return ws_fail(e, what, std::string(what) + ": no memory for the hash's partials", std::string(what) + ": too many bytes");
}

extern "C" int otc_poly1305(const void *data, size_t nbytes, const uint8_t key[32], void *tag_dev, void *stream)
{
    Range rg("otc_poly1305");
    if (!key || !tag_dev) return set_err(OTC_ERR_ARG, "poly1305: null argument");
    if ((uintptr_t)tag_dev & 3u) return set_err(OTC_ERR_ARG, "poly1305: the tag must be 4-byte aligned");
    if (nbytes && !data) return set_err(OTC_ERR_ARG, "poly1305: null buffer");
    if (nbytes && ((uintptr_t)data & 15u)) return set_err(OTC_ERR_ARG, "poly1305: device buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    poly1305_state ps;
    poly1305_init(&ps, key);
    void *ws = nullptr;
    if (int r = poly1305_ws(nbytes, st, &ws, "poly1305")) return r;
    return poly1305_dev(data, nbytes, ps, nullptr, false, tag_dev, ws, st, "poly1305 launch");
}

extern "C" int otc_chacha20_poly1305(const void *in, void *out, size_t nbytes, const uint8_t key[32], int dir,
                                     const uint8_t nonce[12], const uint8_t *aad, size_t aad_len, void *tag_dev,
                                     void *stream)
{
    Range rg("otc_chacha20_poly1305");
    if (!key || !nonce) return set_err(OTC_ERR_ARG, "chacha20_poly1305: null key or nonce");
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (aad_len && !aad) return set_err(OTC_ERR_ARG, "chacha20_poly1305: null aad");
    if (!tag_dev || ((uintptr_t)tag_dev & 3u))
        return set_err(OTC_ERR_ARG, "chacha20_poly1305: the tag must be 4-byte aligned device memory");
    if ((uint64_t)nbytes > CHACHA20_POLY1305_MAX_BYTES)
        return set_err(OTC_ERR_ARG, "chacha20_poly1305: a message has at most (2^32 - 1) * 64 bytes");
    if (int r = check_bufs(in, out, nbytes, true, "chacha20_poly1305")) return r;
    hipStream_t st = (hipStream_t)stream;

    /* what does not depend on the data, on the host: the one-time key (block
     * 0), the hash state after the AAD, the length block */
    uint8_t b0[64], lenblock[16];
    chacha20_block(key, nonce, 0, b0);
    poly1305_state ps;
    poly1305_init(&ps, b0);
    poly1305_pad16(&ps, aad, aad_len);
    for (int i = 0; i < 8; ++i) {
        lenblock[i] = (uint8_t)((uint64_t)aad_len >> (8 * i));
        lenblock[8 + i] = (uint8_t)((uint64_t)nbytes >> (8 * i));
    }

    /* the hash's memory first: a failure leaves out and the tag untouched */
    void *ws = nullptr;
    if (int r = poly1305_ws(nbytes, st, &ws, "chacha20_poly1305")) return r;
    hipError_t e;
    if (dir == OTC_DIR_ENCRYPT && (e = otc_impl::chacha20_run(in, out, nbytes, key, nonce, 1, st)) != hipSuccess) {
        if (ws) (void)otc_dev::ws_free(ws, st);
        return hip_fail(e, "chacha20_poly1305 cipher launch");
    }
    /* over the ciphertext: out of an encryption, in of a decryption */
    if (int r = poly1305_dev(dir == OTC_DIR_ENCRYPT ? out : in, nbytes, ps, lenblock, true, tag_dev, ws, st,
                             "chacha20_poly1305 hash launch"))
        return r;
    if (dir == OTC_DIR_DECRYPT && (e = otc_impl::chacha20_run(in, out, nbytes, key, nonce, 1, st)) != hipSuccess)
        return hip_fail(e, "chacha20_poly1305 cipher launch");
    return OTC_OK;
}

/* ---- what the batched AEADs' planners share ----------------------------- */
/* One record's buffers as otc_gcm_msg, otc_chacha_msg and otc_ocb_msg all hold them (in,
 * out, nbytes, aad, aad_bytes): what is wrong with them, or null. */
template <class Msg>
static const char *batch_record_fault(const Msg &d, uint64_t max_bytes, uint64_t max_aad, const char *too_big)
{
    if (d.nbytes > max_bytes) return too_big;
    if (d.aad_bytes > max_aad) return "more than 64 KiB of AAD";
    if (d.aad_bytes && !d.aad) return "null aad";
    if (!d.nbytes) return nullptr;
    if (!d.in || !d.out) return "null buffer";
    if ((d.in | d.out) & 15u) return "data buffers must be 16-byte aligned";
    if (partial_overlap((const void *)d.in, (const void *)d.out, d.nbytes)) return "input and output overlap partially";
    return nullptr;
}

/* The three checks across records: no two outputs share bytes, no record reads
 * what another writes, no AAD lies in any output.  0, or bad(record, what). */
template <class Msg, class Bad>
static int batch_overlaps(const Msg *msgs, size_t nmsg, Bad bad)
{
    struct Iv {
        uint64_t lo, hi;
        size_t m;
    };
    std::vector<Iv> outs; /* the non-empty outputs, to find records that overlap */
    for (size_t m = 0; m < nmsg; ++m)
        if (msgs[m].nbytes) outs.push_back({msgs[m].out, msgs[m].out + msgs[m].nbytes, m});
    std::sort(outs.begin(), outs.end(), [](const Iv &a, const Iv &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < outs.size(); ++i)
        if (outs[i].lo < outs[i - 1].hi) return bad(outs[i].m, "its output overlaps another record's");
    for (size_t m = 0; m < nmsg; ++m) { /* no record reads what another writes */
        const Msg &d = msgs[m];
        if (!d.nbytes) continue;
        auto it = std::upper_bound(outs.begin(), outs.end(), d.in,
                                   [](uint64_t a, const Iv &o) { return a < o.hi; }); /* first output ending past in */
        for (; it != outs.end() && it->lo < d.in + d.nbytes; ++it)
            if (it->m != m) return bad(m, "its input overlaps another record's output");
    }
    for (size_t m = 0; m < nmsg; ++m) { /* an encryption writes every output before the hash reads the AADs */
        const Msg &d = msgs[m];
        if (!d.aad_bytes) continue;
        auto it = std::upper_bound(outs.begin(), outs.end(), d.aad, [](uint64_t a, const Iv &o) { return a < o.hi; });
        if (it != outs.end() && it->lo < d.aad + d.aad_bytes) return bad(m, "its AAD overlaps a record's output");
    }
    return 0;
}

/* ---- batched GCM: many records, own IVs, one tag array --------------------- */
extern "C" int otc_gcm_batch_spans(uint64_t *spans, int max) { return otc_impl::gcm_batch_spans(spans, spans ? max : 0); }

extern "C" size_t otc_gcm_batch_table_bytes(void) { return otc_impl::gcm_batch_table_bytes(); }

extern "C" size_t otc_gcm_batch_ws_bytes(size_t nmsg) { return nmsg * 32; /* J0[], then E_K(J0)[] */ }

extern "C" int otc_gcm_batch_tables(const otc_gcm_key *k, void *tab_dev, void *stream)
{
    Range rg("otc_gcm_batch_tables");
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(&k->enc, OTC_DIR_ENCRYPT)) return r;
    if (!tab_dev || ((uintptr_t)tab_dev & 15u))
        return set_err(OTC_ERR_ARG, "gcm_batch: the tables must be 16-byte aligned device memory");
    const hipError_t e = otc_impl::gcm_batch_tables(k->h, tab_dev, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gcm_batch tables launch");
    return OTC_OK;
}

extern "C" int64_t otc_gcm_batch_plan(const otc_gcm_msg *msgs, size_t nmsg, int tile_blocks, otc_ctr_msg *ctr_msgs,
                                      uint32_t *tile_msg, uint64_t *tile_first)
{
    if (!check_tile_blocks(tile_blocks))
        return set_err(OTC_ERR_ARG, "gcm_batch: tile_blocks must be 64, 128 or 256");
    if (nmsg == 0) return 0;
    if (!msgs) return set_err(OTC_ERR_ARG, "gcm_batch: null descriptors");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_batch: more than 2^32 - 1 records");
    auto bad = [](size_t m, const char *what) {
        return set_err(OTC_ERR_ARG, "gcm_batch: record " + std::to_string(m) + ": " + what);
    };
    /* at most 65536 blocks: the counter's low 32 bits, started at 2, never wrap */
    for (size_t m = 0; m < nmsg; ++m)
        if (const char *f = batch_record_fault(msgs[m], OTC_GCM_BATCH_MAX_BYTES, OTC_GCM_BATCH_MAX_AAD,
                                               "more than 1 MiB of data (use otc_aes_gcm)"))
            return bad(m, f);
    if (int r = batch_overlaps(msgs, nmsg, bad)) return r;
    const uint64_t tile_bytes = 16ull * (uint64_t)tile_blocks;
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m) {
        const uint64_t nt = (msgs[m].nbytes + tile_bytes - 1) / tile_bytes;
        if (ctr_msgs) ctr_msgs[m] = otc_ctr_msg{msgs[m].in, msgs[m].out, msgs[m].nbytes, 0, 0, 0, 0};
        t = tile_map_fill(tile_msg, tile_first, m, t, nt);
    }
    return (int64_t)t;
}

/* 16 lanes per record for short records, 64 for long ones: measured on
 * uniform batches, 16 wins at 1, 4 and 8 KiB records (x3.4, x1.8, x1.2), 64 at
 * 16 KiB (x1.3); a mean of 768 hashed blocks (12 KiB), between the last two,
 * is where the choice changes -- nothing between them was measured.  SUPPOSED,
 * not measured: a group of records waits for the serial chain of its longest,
 * nb / lanes multiplications, so one record above 4096 blocks also takes 64;
 * no batch of mixed sizes has been timed (aes_gcm_batch.hip, docs/PERF.md
 * "Batched AES-GCM"). */
extern "C" int otc_gcm_batch_lanes(const otc_gcm_msg *msgs, size_t nmsg)
{
    uint64_t total = 0;
    for (size_t m = 0; msgs && m < nmsg; ++m) {
        const uint64_t nb = (msgs[m].aad_bytes + 15) / 16 + (msgs[m].nbytes + 15) / 16 + 1;
        if (nb > 4096) return otc_impl::GB_LANES_LONG;
        total += nb;
    }
    return nmsg && total / nmsg > 768 ? otc_impl::GB_LANES_LONG : otc_impl::GB_LANES_SHORT;
}

/* what otc_ghash_batch and otc_aes_gcm_batch check alike */
static int gcm_batch_common(const otc_gcm_msg *msgs_dev, const void *tab_dev, const void *out16, const char *out_name,
                            int &lanes)
{
    if (lanes == 0) lanes = otc_impl::GB_LANES_LONG;
    if (lanes != otc_impl::GB_LANES_SHORT && lanes != otc_impl::GB_LANES_LONG)
        return set_err(OTC_ERR_ARG, "gcm_batch: lanes must be 16 or 64 (0: 64)");
    if (!msgs_dev || !tab_dev || !out16) return set_err(OTC_ERR_ARG, "gcm_batch: null array");
    if ((uintptr_t)msgs_dev & 7u) return set_err(OTC_ERR_ARG, "gcm_batch: misaligned descriptor array");
    if ((uintptr_t)tab_dev & 15u) return set_err(OTC_ERR_ARG, "gcm_batch: the tables must be 16-byte aligned");
    if ((uintptr_t)out16 & 15u) return set_err(OTC_ERR_ARG, std::string("gcm_batch: ") + out_name + " must be 16-byte aligned");
    return OTC_OK;
}

extern "C" int otc_ghash_batch(const otc_gcm_msg *msgs_dev, size_t nmsg, const void *tab_dev, void *s_dev, int lanes,
                               void *stream)
{
    Range rg("otc_ghash_batch");
    if (nmsg == 0) return OTC_OK;
    if (int r = gcm_batch_common(msgs_dev, tab_dev, s_dev, "the hash array", lanes)) return r;
    const hipError_t e = otc_impl::ghash_batch_run(msgs_dev, nmsg, tab_dev, s_dev, nullptr, nullptr, 16, nullptr, false,
                                                   lanes, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "ghash_batch launch");
    return OTC_OK;
}

extern "C" int otc_aes_gcm_batch(const otc_gcm_msg *msgs_dev, otc_ctr_msg *ctr_msgs_dev, const uint32_t *tile_msg_dev,
                                 const uint64_t *tile_first_dev, uint64_t ntiles, int tile_blocks, size_t nmsg,
                                 const otc_gcm_key *k, const otc_aes_key *key_dev, const void *tab_dev, int dir,
                                 const uint8_t *ivs_dev, void *tags_dev, const uint8_t *expect_dev, int tag_bytes,
                                 uint8_t *ok_dev, void *ws_dev, int lanes, void *stream)
{
    Range rg("otc_aes_gcm_batch");
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(&k->enc, OTC_DIR_ENCRYPT)) return r;
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (!check_tile_blocks(tile_blocks))
        return set_err(OTC_ERR_ARG, "gcm_batch: tile_blocks must be 64, 128 or 256");
    if (tag_bytes < 4 || tag_bytes > 16) return set_err(OTC_ERR_ARG, "gcm_batch: a tag has 4 to 16 bytes");
    if (nmsg == 0) return OTC_OK;
    if (int r = gcm_batch_common(msgs_dev, tab_dev, tags_dev, "the tag array", lanes)) return r;
    if (!ctr_msgs_dev || !key_dev || !ws_dev) return set_err(OTC_ERR_ARG, "gcm_batch: null array");
    if (ntiles && (!tile_msg_dev || !tile_first_dev)) return set_err(OTC_ERR_ARG, "gcm_batch: null tile map");
    if ((((uintptr_t)ctr_msgs_dev) | ((uintptr_t)key_dev) | ((uintptr_t)tile_first_dev)) & 7u ||
        ((uintptr_t)tile_msg_dev & 3u))
        return set_err(OTC_ERR_ARG, "gcm_batch: misaligned descriptor arrays");
    if ((uintptr_t)ws_dev & 15u) return set_err(OTC_ERR_ARG, "gcm_batch: the workspace must be 16-byte aligned");
    if (dir == OTC_DIR_DECRYPT && (!expect_dev || !ok_dev))
        return set_err(OTC_ERR_ARG, "gcm_batch: decryption needs the expected tags and the verdict array");
    if (dir == OTC_DIR_DECRYPT) {
        /* the expected tags are compared with what this call computes: never its own output */
        const uintptr_t e0 = (uintptr_t)expect_dev, e1 = e0 + nmsg * (size_t)tag_bytes;
        const uintptr_t t0 = (uintptr_t)tags_dev, v0 = (uintptr_t)ok_dev;
        if ((e0 < t0 + nmsg * 16 && t0 < e1) || (e0 < v0 + nmsg && v0 < e1))
            return set_err(OTC_ERR_ARG, "gcm_batch: the expected tags overlap the computed tags or the verdicts");
    }
    if (!ivs_dev) return set_err(OTC_ERR_ARG, "gcm_batch: null IVs");
    hipStream_t st = (hipStream_t)stream;
    set_last_impl(OTC_IMPL_TTABLE);
    uint8_t *j0 = (uint8_t *)ws_dev, *ekj0 = j0 + nmsg * 16;
    const bool enc = dir == OTC_DIR_ENCRYPT;

    hipError_t e = otc_impl::gcm_batch_prep(ivs_dev, nmsg, ctr_msgs_dev, j0, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_batch prep launch");
    /* E_K(J0[]): the grid T-table kernel, ECB over nmsg blocks */
    const otc_impl::Job job{otc_impl::JOB_ECB_ENC, j0, ekj0, nmsg, &k->enc, nullptr, 0};
    if ((e = otc_impl::tt_run(job, nmsg, st)) != hipSuccess) return hip_fail(e, "gcm_batch E_K(J0) launch");
    /* the CTR half: the batched kernel's static split (the claimed form
     * allocates its counter) */
    auto ctr = [&] {
        return ntiles ? otc_impl::tt_ctr_batch(ctr_msgs_dev, key_dev, tile_msg_dev, tile_first_dev, ntiles, tile_blocks,
                                               k->enc.nr, st, nullptr)
                      : hipSuccess;
    };
    if (enc && (e = ctr()) != hipSuccess) return hip_fail(e, "gcm_batch ctr launch");
    /* over the ciphertext: out of an encryption, in of a decryption */
    e = otc_impl::ghash_batch_run(msgs_dev, nmsg, tab_dev, tags_dev, ekj0, enc ? nullptr : expect_dev, tag_bytes,
                                  enc ? nullptr : ok_dev, enc, lanes, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_batch hash launch");
    if (!enc) {
        if ((e = ctr()) != hipSuccess) return hip_fail(e, "gcm_batch ctr launch");
        if ((e = otc_impl::gcm_batch_wipe(msgs_dev, nmsg, ok_dev, st)) != hipSuccess)
            return hip_fail(e, "gcm_batch wipe launch");
    }
    return OTC_OK;
}

/* ---- batched ChaCha20-Poly1305: many records, own key and nonce each -------- */
extern "C" int otc_chacha_batch_spans(uint64_t *spans, int max)
{
    return otc_impl::chacha_batch_spans(spans, spans ? max : 0);
}

extern "C" size_t otc_chacha_batch_ws_bytes(size_t nmsg) { return nmsg * 32; /* r (clamped) || s per record */ }

extern "C" int64_t otc_chacha_batch_plan(const otc_chacha_msg *msgs, size_t nmsg, size_t nkeys, uint32_t *tile_msg,
                                         uint64_t *tile_first)
{
    if (nmsg == 0) return 0;
    if (!msgs) return set_err(OTC_ERR_ARG, "chacha_batch: null descriptors");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "chacha_batch: more than 2^32 - 1 records");
    auto bad = [](size_t m, const char *what) {
        return set_err(OTC_ERR_ARG, "chacha_batch: record " + std::to_string(m) + ": " + what);
    };
    /* at most 16384 blocks from counter 1: the 32-bit counter never wraps; an
     * empty record has a key too (its tag's one-time key comes from it) */
    for (size_t m = 0; m < nmsg; ++m) {
        if (msgs[m].key >= nkeys) return bad(m, "key index out of range");
        if (const char *f = batch_record_fault(msgs[m], OTC_CHACHA_BATCH_MAX_BYTES, OTC_CHACHA_BATCH_MAX_AAD,
                                               "more than 1 MiB of data (use otc_chacha20_poly1305)"))
            return bad(m, f);
    }
    if (int r = batch_overlaps(msgs, nmsg, bad)) return r;
    const uint64_t tile_bytes = 4096; /* one pass: 64 blocks of 64 bytes */
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m) t = tile_map_fill(tile_msg, tile_first, m, t, (msgs[m].nbytes + tile_bytes - 1) / tile_bytes);
    return (int64_t)t;
}

/* 16 lanes per record for short records, 64 for long ones.  Measured on
 * uniform batches of 64 MiB with a 13-byte AAD (docs/PERF.md "Batched
 * ChaCha20-Poly1305", benchmarks/chacha_batch.py --lanes-table), the hash
 * alone: 16 lanes win at 256 B, 1 KiB and 4 KiB records (18, 66 and 258 hashed
 * blocks: x3.9, x2.8, x1.6), 64 lanes at 16 KiB and 64 KiB (1026 and 4098
 * blocks: x1.25, x3.0); the whole encryption agrees at every size.  The
 * choice changes between 258 and 1026 blocks, and nothing between them was
 * measured: 512 blocks (8 KiB), their geometric mean, is where the rule puts
 * it.  GCM's 768 does not carry over: this fold is log2 L cross-lane steps,
 * not a serial chain of L + 1.  SUPPOSED, not measured: that the MEAN of a
 * mixed batch decides -- no batch of mixed sizes has been timed.  Records do
 * not wait for one another across waves here (no workgroup barrier), so one
 * long record does not switch the whole batch, unlike otc_gcm_batch_lanes. */
extern "C" int otc_chacha_batch_lanes(const otc_chacha_msg *msgs, size_t nmsg)
{
    uint64_t total = 0;
    for (size_t m = 0; msgs && m < nmsg; ++m) total += (msgs[m].aad_bytes + 15) / 16 + (msgs[m].nbytes + 15) / 16 + 1;
    return nmsg && total / nmsg > 512 ? otc_impl::CB_LANES_LONG : otc_impl::CB_LANES_SHORT;
}

/* what otc_poly1305_batch and otc_chacha20_poly1305_batch check alike */
static int chacha_batch_common(const otc_chacha_msg *msgs_dev, const void *tags_dev, int &lanes)
{
    if (lanes == 0) lanes = otc_impl::CB_LANES_LONG;
    if (lanes != otc_impl::CB_LANES_SHORT && lanes != otc_impl::CB_LANES_LONG)
        return set_err(OTC_ERR_ARG, "chacha_batch: lanes must be 16 or 64 (0: 64)");
    if (!msgs_dev || !tags_dev) return set_err(OTC_ERR_ARG, "chacha_batch: null array");
    if ((uintptr_t)msgs_dev & 7u) return set_err(OTC_ERR_ARG, "chacha_batch: misaligned descriptor array");
    if ((uintptr_t)tags_dev & 15u) return set_err(OTC_ERR_ARG, "chacha_batch: the tag array must be 16-byte aligned");
    return OTC_OK;
}

extern "C" int otc_poly1305_batch(const otc_chacha_msg *msgs_dev, size_t nmsg, const uint8_t *otk_dev, void *tags_dev,
                                  int lanes, void *stream)
{
    Range rg("otc_poly1305_batch");
    if (nmsg == 0) return OTC_OK;
    if (int r = chacha_batch_common(msgs_dev, tags_dev, lanes)) return r;
    if (!otk_dev) return set_err(OTC_ERR_ARG, "chacha_batch: null array");
    if ((uintptr_t)otk_dev & 3u) return set_err(OTC_ERR_ARG, "chacha_batch: misaligned one-time key array");
    const hipError_t e = otc_impl::poly1305_batch_run(msgs_dev, nmsg, otk_dev, tags_dev, nullptr, nullptr, false, lanes,
                                                      (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "poly1305_batch launch");
    return OTC_OK;
}

extern "C" int otc_chacha20_poly1305_batch(const otc_chacha_msg *msgs_dev, const uint32_t *tile_msg_dev,
                                           const uint64_t *tile_first_dev, uint64_t ntiles, size_t nmsg,
                                           const uint8_t *keys_dev, int dir, const uint8_t *nonces_dev, void *tags_dev,
                                           const uint8_t *expect_dev, uint8_t *ok_dev, void *ws_dev, int lanes,
                                           void *stream)
{
    Range rg("otc_chacha20_poly1305_batch");
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (nmsg == 0) return OTC_OK;
    if (int r = chacha_batch_common(msgs_dev, tags_dev, lanes)) return r;
    if (!keys_dev || !ws_dev) return set_err(OTC_ERR_ARG, "chacha_batch: null array");
    if (ntiles && (!tile_msg_dev || !tile_first_dev)) return set_err(OTC_ERR_ARG, "chacha_batch: null tile map");
    if (((uintptr_t)tile_first_dev & 7u) || ((uintptr_t)tile_msg_dev & 3u) || ((uintptr_t)keys_dev & 3u))
        return set_err(OTC_ERR_ARG, "chacha_batch: misaligned tile map or key array");
    if ((uintptr_t)ws_dev & 15u) return set_err(OTC_ERR_ARG, "chacha_batch: the workspace must be 16-byte aligned");
    if (dir == OTC_DIR_DECRYPT && (!expect_dev || !ok_dev))
        return set_err(OTC_ERR_ARG, "chacha_batch: decryption needs the expected tags and the verdict array");
    if (dir == OTC_DIR_DECRYPT) {
        /* the expected tags are compared with what this call computes: never its own output */
        const uintptr_t e0 = (uintptr_t)expect_dev, e1 = e0 + nmsg * 16;
        const uintptr_t t0 = (uintptr_t)tags_dev, v0 = (uintptr_t)ok_dev;
        if ((e0 < t0 + nmsg * 16 && t0 < e1) || (e0 < v0 + nmsg && v0 < e1))
            return set_err(OTC_ERR_ARG, "chacha_batch: the expected tags overlap the computed tags or the verdicts");
    }
    if (!nonces_dev) return set_err(OTC_ERR_ARG, "chacha_batch: null nonces");
    hipStream_t st = (hipStream_t)stream;
    const bool enc = dir == OTC_DIR_ENCRYPT;

    hipError_t e = otc_impl::chacha_batch_prep(msgs_dev, nmsg, keys_dev, nonces_dev, ws_dev, st);
    if (e != hipSuccess) return hip_fail(e, "chacha_batch prep launch");
    auto cipher = [&] {
        return otc_impl::chacha20_batch_run(msgs_dev, keys_dev, nonces_dev, tile_msg_dev, tile_first_dev, ntiles, st);
    };
    if (enc && (e = cipher()) != hipSuccess) return hip_fail(e, "chacha_batch cipher launch");
    /* over the ciphertext: out of an encryption, in of a decryption */
    e = otc_impl::poly1305_batch_run(msgs_dev, nmsg, ws_dev, tags_dev, enc ? nullptr : expect_dev, enc ? nullptr : ok_dev,
                                     enc, lanes, st);
    if (e != hipSuccess) return hip_fail(e, "chacha_batch hash launch");
    if (!enc) {
        if ((e = cipher()) != hipSuccess) return hip_fail(e, "chacha_batch cipher launch");
        if ((e = otc_impl::chacha_batch_wipe(msgs_dev, nmsg, ok_dev, st)) != hipSuccess)
            return hip_fail(e, "chacha_batch wipe launch");
    }
    return OTC_OK;
}

/* ---- batched AES-OCB3: many records, one key, own nonce and tag each --------- */
extern "C" int otc_ocb_batch_spans(uint64_t *spans, int max) { return otc_impl::ocb_batch_spans(spans, spans ? max : 0); }

extern "C" size_t otc_ocb_batch_ws_bytes(size_t nmsg) { return nmsg * 48; /* Offset_0[], checksum[], HASH[] */ }

extern "C" int64_t otc_ocb_batch_plan(const otc_ocb_msg *msgs, size_t nmsg, uint32_t *tile_msg, uint64_t *tile_first)
{
    if (nmsg == 0) return 0;
    if (!msgs) return set_err(OTC_ERR_ARG, "ocb_batch: null descriptors");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "ocb_batch: more than 2^32 - 1 records");
    auto bad = [](size_t m, const char *what) {
        return set_err(OTC_ERR_ARG, "ocb_batch: record " + std::to_string(m) + ": " + what);
    };
    /* at most 65536 blocks: the kernels carry L_0 .. L_16 */
    for (size_t m = 0; m < nmsg; ++m)
        if (const char *f = batch_record_fault(msgs[m], OTC_OCB_BATCH_MAX_BYTES, OTC_OCB_BATCH_MAX_AAD,
                                               "more than 1 MiB of data (use otc_aes_ocb)"))
            return bad(m, f);
    if (int r = batch_overlaps(msgs, nmsg, bad)) return r;
    const uint64_t tile_blocks = 64; /* whole blocks only: the finisher takes the trailing bytes */
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m)
        t = tile_map_fill(tile_msg, tile_first, m, t, (msgs[m].nbytes / 16 + tile_blocks - 1) / tile_blocks);
    return (int64_t)t;
}

extern "C" int otc_aes_ocb_batch(const otc_ocb_msg *msgs_dev, const uint32_t *tile_msg_dev,
                                 const uint64_t *tile_first_dev, uint64_t ntiles, size_t nmsg, const otc_ocb_key *k,
                                 int dir, const uint8_t *nonces_dev, void *tags_dev, const uint8_t *expect_dev,
                                 uint8_t *ok_dev, void *ws_dev, void *stream)
{
    Range rg("otc_aes_ocb_batch");
    if (int r = ocb_check_key(k, dir)) return r;
    if (nmsg == 0) return OTC_OK;
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "ocb_batch: more than 2^32 - 1 records");
    if (!msgs_dev || !tags_dev || !ws_dev) return set_err(OTC_ERR_ARG, "ocb_batch: null array");
    if ((uintptr_t)msgs_dev & 7u) return set_err(OTC_ERR_ARG, "ocb_batch: misaligned descriptor array");
    if ((uintptr_t)tags_dev & 15u) return set_err(OTC_ERR_ARG, "ocb_batch: the tag array must be 16-byte aligned");
    if (ntiles && (!tile_msg_dev || !tile_first_dev)) return set_err(OTC_ERR_ARG, "ocb_batch: null tile map");
    if (((uintptr_t)tile_first_dev & 7u) || ((uintptr_t)tile_msg_dev & 3u))
        return set_err(OTC_ERR_ARG, "ocb_batch: misaligned tile map");
    if ((uintptr_t)ws_dev & 15u) return set_err(OTC_ERR_ARG, "ocb_batch: the workspace must be 16-byte aligned");
    if (dir == OTC_DIR_DECRYPT && (!expect_dev || !ok_dev))
        return set_err(OTC_ERR_ARG, "ocb_batch: decryption needs the expected tags and the verdict array");
    if (dir == OTC_DIR_DECRYPT) {
        /* the expected tags are compared with what this call computes: never its own output */
        const uintptr_t e0 = (uintptr_t)expect_dev, e1 = e0 + nmsg * 16;
        const uintptr_t t0 = (uintptr_t)tags_dev, v0 = (uintptr_t)ok_dev;
        if ((e0 < t0 + nmsg * 16 && t0 < e1) || (e0 < v0 + nmsg && v0 < e1))
            return set_err(OTC_ERR_ARG, "ocb_batch: the expected tags overlap the computed tags or the verdicts");
    }
    if (!nonces_dev) return set_err(OTC_ERR_ARG, "ocb_batch: null nonces");
    hipStream_t st = (hipStream_t)stream;
    set_last_impl(OTC_IMPL_TTABLE);
    const bool enc = dir == OTC_DIR_ENCRYPT;

    hipError_t e = otc_impl::ocb_batch_prep(msgs_dev, nmsg, *k, nonces_dev, ws_dev, st);
    if (e != hipSuccess) return hip_fail(e, "ocb_batch prep launch");
    e = otc_impl::ocb_batch_bulk(msgs_dev, nmsg, tile_msg_dev, tile_first_dev, ntiles, *k, !enc, ws_dev, st);
    if (e != hipSuccess) return hip_fail(e, "ocb_batch bulk launch");
    e = otc_impl::ocb_batch_finish(msgs_dev, nmsg, *k, ws_dev, tags_dev, enc ? nullptr : expect_dev,
                                   enc ? nullptr : ok_dev, st);
    if (e != hipSuccess) return hip_fail(e, "ocb_batch finish launch");
    if (!enc && (e = otc_impl::ocb_batch_wipe(msgs_dev, nmsg, ok_dev, st)) != hipSuccess)
        return hip_fail(e, "ocb_batch wipe launch");
    return OTC_OK;
}

/* ---- batched AES-CCM: many records, one key, one record per lane ---------------- */
extern "C" int otc_ccm_batch_spans(uint64_t *spans, int max) { return otc_impl::ccm_batch_spans(spans, spans ? max : 0); }

extern "C" size_t otc_ccm_batch_ws_bytes(size_t) { return 0; /* the AAD is chained in the records' kernel */ }

static bool ccm_tag_len_ok(int t) { return t >= 4 && t <= 16 && !(t & 1); }

extern "C" int otc_ccm_batch_plan(const otc_ccm_msg *msgs, size_t nmsg, int nonce_len, uint32_t *order)
{
    if (nonce_len < 7 || nonce_len > 13) return set_err(OTC_ERR_ARG, "ccm_batch: a nonce has 7 to 13 bytes");
    if (nmsg == 0) return OTC_OK;
    if (!msgs) return set_err(OTC_ERR_ARG, "ccm_batch: null descriptors");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "ccm_batch: more than 2^32 - 1 records");
    auto bad = [](size_t m, const char *what) {
        return set_err(OTC_ERR_ARG, "ccm_batch: record " + std::to_string(m) + ": " + what);
    };
    /* the length field has L = 15 - nonce_len bytes (2 .. 8); the cap is below 2^24 */
    const int L = 15 - nonce_len;
    const uint64_t field = L >= 3 ? (uint64_t)OTC_CCM_BATCH_MAX_BYTES + 1 : (uint64_t)1 << (8 * L);
    for (size_t m = 0; m < nmsg; ++m) {
        if (const char *f = batch_record_fault(msgs[m], OTC_CCM_BATCH_MAX_BYTES, OTC_CCM_BATCH_MAX_AAD,
                                               "more than 1 MiB of data"))
            return bad(m, f);
        if (msgs[m].nbytes >= field) return bad(m, "its length does not fit the length field of this nonce length");
    }
    if (int r = batch_overlaps(msgs, nmsg, bad)) return r;
    static_assert(sizeof(otc_ccm_msg) % 8 == 0, "ccm_order_fill strides in 64-bit words");
    if (order && ccm_order_fill(order, &msgs[0].nbytes, sizeof(otc_ccm_msg) / 8, nmsg))
        return set_err(OTC_ERR_NOMEM, "ccm_batch: no memory for the order's sort");
    return OTC_OK;
}

extern "C" int otc_aes_ccm_batch(const otc_ccm_msg *msgs_dev, const uint32_t *order_dev, size_t nmsg,
                                 const otc_aes_key *key, int dir, const uint8_t *nonces_dev, int nonce_len,
                                 void *tags_dev, int tag_len, const uint8_t *expect_dev, uint8_t *ok_dev, void *ws_dev,
                                 void *stream)
{
    Range rg("otc_aes_ccm_batch");
    (void)ws_dev; /* otc_ccm_batch_ws_bytes is 0 */
    if (!key) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(key, OTC_DIR_ENCRYPT)) return r;
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (nonce_len < 7 || nonce_len > 13) return set_err(OTC_ERR_ARG, "ccm_batch: a nonce has 7 to 13 bytes");
    if (!ccm_tag_len_ok(tag_len)) return set_err(OTC_ERR_ARG, "ccm_batch: a tag has 4, 6, 8, 10, 12, 14 or 16 bytes");
    if (nmsg == 0) return OTC_OK;
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "ccm_batch: more than 2^32 - 1 records");
    if (!msgs_dev || !order_dev || !tags_dev) return set_err(OTC_ERR_ARG, "ccm_batch: null array");
    if ((uintptr_t)msgs_dev & 7u) return set_err(OTC_ERR_ARG, "ccm_batch: misaligned descriptor array");
    if ((uintptr_t)order_dev & 3u) return set_err(OTC_ERR_ARG, "ccm_batch: misaligned order array");
    if (dir == OTC_DIR_DECRYPT && (!expect_dev || !ok_dev))
        return set_err(OTC_ERR_ARG, "ccm_batch: decryption needs the expected tags and the verdict array");
    if (dir == OTC_DIR_DECRYPT) {
        /* the expected tags are compared with what this call computes: never its own output */
        const uintptr_t e0 = (uintptr_t)expect_dev, e1 = e0 + nmsg * (size_t)tag_len;
        const uintptr_t t0 = (uintptr_t)tags_dev, v0 = (uintptr_t)ok_dev;
        if ((e0 < t0 + nmsg * (size_t)tag_len && t0 < e1) || (e0 < v0 + nmsg && v0 < e1))
            return set_err(OTC_ERR_ARG, "ccm_batch: the expected tags overlap the computed tags or the verdicts");
    }
    if (!nonces_dev) return set_err(OTC_ERR_ARG, "ccm_batch: null nonces");
    hipStream_t st = (hipStream_t)stream;
    set_last_impl(OTC_IMPL_TTABLE);
    const bool enc = dir == OTC_DIR_ENCRYPT;

    hipError_t e = otc_impl::ccm_batch_run(msgs_dev, order_dev, nmsg, *key, !enc, nonces_dev, nonce_len,
                                           (uint8_t *)tags_dev, tag_len, enc ? nullptr : expect_dev,
                                           enc ? nullptr : ok_dev, st);
    if (e != hipSuccess) return hip_fail(e, "ccm_batch records launch");
    if (!enc && (e = otc_impl::ccm_batch_wipe(msgs_dev, nmsg, ok_dev, st)) != hipSuccess)
        return hip_fail(e, "ccm_batch wipe launch");
    return OTC_OK;
}

/* ---- batched AES-GCM-SIV: many records, one key-generating key, own nonce each -- */
extern "C" int otc_gcm_siv_batch_spans(uint64_t *spans, int max)
{
    return otc_impl::gcm_siv_batch_spans(spans, spans ? max : 0);
}

/* H_m[], S_m[], then an otc_aes_key per record: the derived keys */
extern "C" size_t otc_gcm_siv_batch_ws_bytes(size_t nmsg) { return nmsg * (32 + sizeof(otc_aes_key)); }

extern "C" int64_t otc_gcm_siv_batch_plan(const otc_gcm_msg *msgs, size_t nmsg, uint32_t *tile_msg, uint64_t *tile_first)
{
    if (nmsg == 0) return 0;
    if (!msgs) return set_err(OTC_ERR_ARG, "gcm_siv_batch: null descriptors");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_siv_batch: more than 2^32 - 1 records");
    auto bad = [](size_t m, const char *what) {
        return set_err(OTC_ERR_ARG, "gcm_siv_batch: record " + std::to_string(m) + ": " + what);
    };
    /* at most 65536 blocks: the 32-bit counter passes no value twice within a record */
    for (size_t m = 0; m < nmsg; ++m)
        if (const char *f = batch_record_fault(msgs[m], OTC_GCM_SIV_BATCH_MAX_BYTES, OTC_GCM_SIV_BATCH_MAX_AAD,
                                               "more than 1 MiB of data (use otc_aes_gcm_siv)"))
            return bad(m, f);
    if (int r = batch_overlaps(msgs, nmsg, bad)) return r;
    const uint64_t tile_bytes = 16ull * OTC_GCM_SIV_BATCH_TILE_BLOCKS;
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m)
        t = tile_map_fill(tile_msg, tile_first, m, t, (msgs[m].nbytes + tile_bytes - 1) / tile_bytes);
    return (int64_t)t;
}

/* 16 lanes per record unless the records are long.  A record never leaves its
 * wave in either form (aes_gcm_siv_batch.hip), so per record the 16-lane form
 * always costs fewer products: nb / 16 + 9 for four records against nb / 64 + 13
 * for one.  What the 64-lane form buys is waves: a batch of few long records
 * fills the chip only with one wave per record.  Measured on uniform batches of
 * 64 MiB with a 13-byte AAD (docs/PERF.md "Batched AES-GCM-SIV"); the rule puts
 * the change at a mean of 512 hashed blocks (8 KiB), ChaCha's value, whose fold
 * has the same shape.  SUPPOSED, not measured: that the MEAN of a mixed batch
 * decides, and that the record count does not enter. */
extern "C" int otc_gcm_siv_batch_lanes(const otc_gcm_msg *msgs, size_t nmsg)
{
    uint64_t total = 0;
    for (size_t m = 0; msgs && m < nmsg; ++m) total += (msgs[m].aad_bytes + 15) / 16 + (msgs[m].nbytes + 15) / 16 + 1;
    return nmsg && total / nmsg > 512 ? otc_impl::GSB_LANES_LONG : otc_impl::GSB_LANES_SHORT;
}

static int gsb_lanes_ok(int &lanes)
{
    if (lanes == 0) lanes = otc_impl::GSB_LANES_LONG;
    if (lanes != otc_impl::GSB_LANES_SHORT && lanes != otc_impl::GSB_LANES_LONG)
        return set_err(OTC_ERR_ARG, "gcm_siv_batch: lanes must be 16 or 64 (0: 64)");
    return OTC_OK;
}

extern "C" int otc_polyval_batch(const otc_gcm_msg *msgs_dev, size_t nmsg, const void *h_dev, void *s_dev, int lanes,
                                 void *stream)
{
    Range rg("otc_polyval_batch");
    if (nmsg == 0) return OTC_OK;
    if (int r = gsb_lanes_ok(lanes)) return r;
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_siv_batch: more than 2^32 - 1 records");
    if (!msgs_dev || !h_dev || !s_dev) return set_err(OTC_ERR_ARG, "gcm_siv_batch: null array");
    if ((uintptr_t)msgs_dev & 7u) return set_err(OTC_ERR_ARG, "gcm_siv_batch: misaligned descriptor array");
    if (((uintptr_t)h_dev | (uintptr_t)s_dev) & 15u)
        return set_err(OTC_ERR_ARG, "gcm_siv_batch: the key and hash arrays must be 16-byte aligned");
    const hipError_t e = otc_impl::polyval_batch_run(msgs_dev, nmsg, h_dev, s_dev, false, lanes, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "polyval_batch launch");
    return OTC_OK;
}

extern "C" int otc_aes_ctr_le32_batch(const otc_gcm_msg *msgs_dev, const otc_aes_key *keys_dev, const void *ctrs_dev,
                                      const uint32_t *tile_msg_dev, const uint64_t *tile_first_dev, uint64_t ntiles,
                                      size_t nmsg, int nr, void *stream)
{
    Range rg("otc_aes_ctr_le32_batch");
    if (nr != 10 && nr != 12 && nr != 14) return set_err(OTC_ERR_ARG, "ctr_le32_batch: nr must be 10, 12 or 14");
    if (nmsg == 0 || ntiles == 0) return OTC_OK;
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "ctr_le32_batch: more than 2^32 - 1 records");
    if (!msgs_dev || !keys_dev || !ctrs_dev) return set_err(OTC_ERR_ARG, "ctr_le32_batch: null array");
    if (!tile_msg_dev || !tile_first_dev) return set_err(OTC_ERR_ARG, "ctr_le32_batch: null tile map");
    if ((((uintptr_t)msgs_dev | (uintptr_t)tile_first_dev) & 7u) || ((uintptr_t)tile_msg_dev & 3u))
        return set_err(OTC_ERR_ARG, "ctr_le32_batch: misaligned descriptor arrays");
    if ((uintptr_t)keys_dev & 15u) return set_err(OTC_ERR_ARG, "ctr_le32_batch: the schedules must be 16-byte aligned");
    if ((uintptr_t)ctrs_dev & 3u) return set_err(OTC_ERR_ARG, "ctr_le32_batch: the counter blocks must be 4-byte aligned");
    set_last_impl(OTC_IMPL_TTABLE);
    const hipError_t e = otc_impl::ctr_le32_batch_run(msgs_dev, keys_dev, ctrs_dev, tile_msg_dev, tile_first_dev, ntiles,
                                                      nr, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "ctr_le32_batch launch");
    return OTC_OK;
}

extern "C" int otc_aes_gcm_siv_batch(const otc_gcm_msg *msgs_dev, const uint32_t *tile_msg_dev,
                                     const uint64_t *tile_first_dev, uint64_t ntiles, size_t nmsg,
                                     const otc_gcm_siv_key *k, int dir, const uint8_t *nonces_dev, void *tags_dev,
                                     const uint8_t *expect_dev, uint8_t *ok_dev, void *ws_dev, int lanes, void *stream)
{
    Range rg("otc_aes_gcm_siv_batch");
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(&k->kgk, OTC_DIR_ENCRYPT)) return r;
    if (k->kgk.nr != 10 && k->kgk.nr != 14) return set_err(OTC_ERR_ARG, "gcm_siv: the key has 128 or 256 bits");
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (nmsg == 0) return OTC_OK;
    if (int r = gsb_lanes_ok(lanes)) return r;
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_siv_batch: more than 2^32 - 1 records");
    if (!msgs_dev || !tags_dev || !ws_dev) return set_err(OTC_ERR_ARG, "gcm_siv_batch: null array");
    if ((uintptr_t)msgs_dev & 7u) return set_err(OTC_ERR_ARG, "gcm_siv_batch: misaligned descriptor array");
    if ((uintptr_t)tags_dev & 15u) return set_err(OTC_ERR_ARG, "gcm_siv_batch: the tag array must be 16-byte aligned");
    if (ntiles && (!tile_msg_dev || !tile_first_dev)) return set_err(OTC_ERR_ARG, "gcm_siv_batch: null tile map");
    if (((uintptr_t)tile_first_dev & 7u) || ((uintptr_t)tile_msg_dev & 3u))
        return set_err(OTC_ERR_ARG, "gcm_siv_batch: misaligned tile map");
    if ((uintptr_t)ws_dev & 15u) return set_err(OTC_ERR_ARG, "gcm_siv_batch: the workspace must be 16-byte aligned");
    if (dir == OTC_DIR_DECRYPT && (!expect_dev || !ok_dev))
        return set_err(OTC_ERR_ARG, "gcm_siv_batch: decryption needs the expected tags and the verdict array");
    if (dir == OTC_DIR_DECRYPT) {
        /* the expected tags are compared with what this call computes: never its own output */
        const uintptr_t e0 = (uintptr_t)expect_dev, e1 = e0 + nmsg * 16;
        const uintptr_t t0 = (uintptr_t)tags_dev, v0 = (uintptr_t)ok_dev;
        if ((e0 < t0 + nmsg * 16 && t0 < e1) || (e0 < v0 + nmsg && v0 < e1))
            return set_err(OTC_ERR_ARG, "gcm_siv_batch: the expected tags overlap the computed tags or the verdicts");
        if (e0 & 3u) return set_err(OTC_ERR_ARG, "gcm_siv_batch: the expected tags must be 4-byte aligned");
    }
    if (!nonces_dev) return set_err(OTC_ERR_ARG, "gcm_siv_batch: null nonces");
    hipStream_t st = (hipStream_t)stream;
    set_last_impl(OTC_IMPL_TTABLE);
    const bool enc = dir == OTC_DIR_ENCRYPT;
    const int nr = k->kgk.nr;
    uint8_t *h = (uint8_t *)ws_dev, *s = h + nmsg * 16;
    otc_aes_key *keys = (otc_aes_key *)(s + nmsg * 16);

    hipError_t e = otc_impl::gcm_siv_batch_derive(k->kgk, nonces_dev, nmsg, h, keys, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_siv_batch derive launch");
    /* the counter block of a record is its tag: the computed one, or a decryption's received one */
    auto ctr = [&](const void *ctrs) {
        return otc_impl::ctr_le32_batch_run(msgs_dev, keys, ctrs, tile_msg_dev, tile_first_dev, ntiles, nr, st);
    };
    if (!enc && (e = ctr(expect_dev)) != hipSuccess) return hip_fail(e, "gcm_siv_batch ctr launch");
    /* over the plaintext: in of an encryption, out of a decryption */
    if ((e = otc_impl::polyval_batch_run(msgs_dev, nmsg, h, s, !enc, lanes, st)) != hipSuccess)
        return hip_fail(e, "gcm_siv_batch hash launch");
    e = otc_impl::gcm_siv_batch_final(s, nonces_dev, keys, nmsg, nr, tags_dev, enc ? nullptr : expect_dev,
                                      enc ? nullptr : ok_dev, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_siv_batch finisher launch");
    if (enc && (e = ctr(tags_dev)) != hipSuccess) return hip_fail(e, "gcm_siv_batch ctr launch");
    if (!enc && (e = otc_impl::gcm_siv_batch_wipe(msgs_dev, nmsg, ok_dev, st)) != hipSuccess)
        return hip_fail(e, "gcm_siv_batch wipe launch");
    return OTC_OK;
}

/* ---- batched GCM, a key per record -------------------------------------------- */
extern "C" int otc_gcm_mk_batch_spans(uint64_t *spans, int max)
{
    return otc_impl::gcm_mk_batch_spans(spans, spans ? max : 0);
}

extern "C" size_t otc_gcm_mk_batch_table_bytes(size_t nkeys) { return otc_impl::gcm_mk_batch_table_bytes(nkeys); }

extern "C" size_t otc_gcm_mk_batch_ws_bytes(size_t nmsg) { return nmsg * 32; /* J0[], then the hashes */ }

static bool gcm_mk_rounds(int nr) { return nr == 10 || nr == 12 || nr == 14; }

extern "C" int otc_gcm_mk_batch_tables(const otc_aes_key *keys_dev, size_t nkeys, int nr, void *tab_dev, void *stream)
{
    Range rg("otc_gcm_mk_batch_tables");
    if (!gcm_mk_rounds(nr)) return set_err(OTC_ERR_ARG, "gcm_mk_batch: nr must be 10, 12 or 14");
    if (nkeys == 0) return OTC_OK;
    if (!keys_dev || ((uintptr_t)keys_dev & 7u))
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: the schedules must be 8-byte aligned device memory");
    if (!tab_dev || ((uintptr_t)tab_dev & 15u))
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: the tables must be 16-byte aligned device memory");
    const hipError_t e = otc_impl::gcm_mk_batch_tables(keys_dev, nkeys, nr, tab_dev, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gcm_mk_batch tables launch");
    return OTC_OK;
}

extern "C" int64_t otc_gcm_mk_batch_plan(const otc_gcm_mk_msg *msgs, size_t nmsg, size_t nkeys, int tile_blocks,
                                         otc_ctr_msg *ctr_msgs, uint32_t *tile_msg, uint64_t *tile_first)
{
    if (!check_tile_blocks(tile_blocks))
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: tile_blocks must be 64, 128 or 256");
    if (nmsg == 0) return 0;
    if (!msgs) return set_err(OTC_ERR_ARG, "gcm_mk_batch: null descriptors");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_mk_batch: more than 2^32 - 1 records");
    auto bad = [](size_t m, const char *what) {
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: record " + std::to_string(m) + ": " + what);
    };
    /* at most 65536 blocks: the counter's low 32 bits, started at 2, never wrap; an
     * empty record has a key too (its tag comes from it) */
    for (size_t m = 0; m < nmsg; ++m) {
        if (msgs[m].key >= nkeys || msgs[m].key > 0xFFFFFFFFull) return bad(m, "key index out of range");
        if (const char *f = batch_record_fault(msgs[m], OTC_GCM_BATCH_MAX_BYTES, OTC_GCM_BATCH_MAX_AAD,
                                               "more than 1 MiB of data (use otc_aes_gcm)"))
            return bad(m, f);
    }
    if (int r = batch_overlaps(msgs, nmsg, bad)) return r;
    const uint64_t tile_bytes = 16ull * (uint64_t)tile_blocks;
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m) {
        const uint64_t nt = (msgs[m].nbytes + tile_bytes - 1) / tile_bytes;
        if (ctr_msgs) ctr_msgs[m] = otc_ctr_msg{msgs[m].in, msgs[m].out, msgs[m].nbytes, 0, 0, (uint32_t)msgs[m].key, 0};
        t = tile_map_fill(tile_msg, tile_first, m, t, nt);
    }
    return (int64_t)t;
}

/* 16 lanes per record for short records, 64 for long ones.  The fold is
 * otc_gcm_siv_batch_lanes' (log2 L cross-lane steps, no serial chain, no
 * workgroup barrier) and the rule started from that one's 512 hashed blocks.
 * MEASURED for this kernel on uniform batches of 64 MiB, 256 keys, a 13-byte
 * AAD (docs/PERF.md "Batched AES-GCM, a key per record", benchmarks/
 * gcm_mk_batch.py --lanes-table), the hash alone: 16 lanes win at 1, 4 and 8 KiB
 * records (66, 258 and 514 hashed blocks: x3.4, x2.0, x1.3), 64 lanes at 16 KiB
 * (1026 blocks: x1.27); the whole encryption agrees at every size.  So 512 was
 * too low here -- a record's copy of 5 tables costs less in front of the Horner
 * passes than GCM-SIV's 4 squarings, which favours the 16-lane form longer --
 * and the choice changes between 514 and 1026 blocks, where nothing was
 * measured: 768 blocks (12 KiB) is where the rule puts it.  SUPPOSED, not
 * measured: that the MEAN of a mixed batch decides -- no batch of mixed sizes
 * has been timed. */
extern "C" int otc_gcm_mk_batch_lanes(const otc_gcm_mk_msg *msgs, size_t nmsg)
{
    uint64_t total = 0;
    for (size_t m = 0; msgs && m < nmsg; ++m) total += (msgs[m].aad_bytes + 15) / 16 + (msgs[m].nbytes + 15) / 16 + 1;
    return nmsg && total / nmsg > 768 ? otc_impl::GMK_LANES_LONG : otc_impl::GMK_LANES_SHORT;
}

/* what otc_ghash_mk_batch and otc_aes_gcm_mk_batch check alike */
static int gcm_mk_batch_common(const otc_gcm_mk_msg *msgs_dev, const void *tab_dev, const void *out16,
                               const char *out_name, int &lanes)
{
    if (lanes == 0) lanes = otc_impl::GMK_LANES_LONG;
    if (lanes != otc_impl::GMK_LANES_SHORT && lanes != otc_impl::GMK_LANES_LONG)
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: lanes must be 16 or 64 (0: 64)");
    if (!msgs_dev || !tab_dev || !out16) return set_err(OTC_ERR_ARG, "gcm_mk_batch: null array");
    if ((uintptr_t)msgs_dev & 7u) return set_err(OTC_ERR_ARG, "gcm_mk_batch: misaligned descriptor array");
    if ((uintptr_t)tab_dev & 15u) return set_err(OTC_ERR_ARG, "gcm_mk_batch: the tables must be 16-byte aligned");
    if ((uintptr_t)out16 & 15u)
        return set_err(OTC_ERR_ARG, std::string("gcm_mk_batch: ") + out_name + " must be 16-byte aligned");
    return OTC_OK;
}

extern "C" int otc_ghash_mk_batch(const otc_gcm_mk_msg *msgs_dev, size_t nmsg, const void *tab_dev, void *s_dev,
                                  int lanes, void *stream)
{
    Range rg("otc_ghash_mk_batch");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_mk_batch: more than 2^32 - 1 records");
    if (int r = gcm_mk_batch_common(msgs_dev, tab_dev, s_dev, "the hash array", lanes)) return r;
    if (nmsg == 0) return OTC_OK;
    const hipError_t e = otc_impl::ghash_mk_batch_run(msgs_dev, nmsg, tab_dev, s_dev, false, lanes, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gcm_mk_batch hash launch");
    return OTC_OK;
}

extern "C" int otc_aes_gcm_mk_batch(const otc_gcm_mk_msg *msgs_dev, otc_ctr_msg *ctr_msgs_dev,
                                    const uint32_t *tile_msg_dev, const uint64_t *tile_first_dev, uint64_t ntiles,
                                    int tile_blocks, size_t nmsg, const otc_aes_key *keys_dev, size_t nkeys, int nr,
                                    const void *tab_dev, int dir, const uint8_t *ivs_dev, void *tags_dev,
                                    const uint8_t *expect_dev, int tag_bytes, uint8_t *ok_dev, void *ws_dev, int lanes,
                                    void *stream)
{
    Range rg("otc_aes_gcm_mk_batch");
    if (!gcm_mk_rounds(nr)) return set_err(OTC_ERR_ARG, "gcm_mk_batch: nr must be 10, 12 or 14");
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (!check_tile_blocks(tile_blocks))
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: tile_blocks must be 64, 128 or 256");
    if (tag_bytes < 4 || tag_bytes > 16) return set_err(OTC_ERR_ARG, "gcm_mk_batch: a tag has 4 to 16 bytes");
    if (nmsg == 0) return OTC_OK;
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_mk_batch: more than 2^32 - 1 records");
    if (nkeys == 0) return set_err(OTC_ERR_ARG, "gcm_mk_batch: no keys");
    if (int r = gcm_mk_batch_common(msgs_dev, tab_dev, tags_dev, "the tag array", lanes)) return r;
    if (!ctr_msgs_dev || !keys_dev || !ws_dev) return set_err(OTC_ERR_ARG, "gcm_mk_batch: null array");
    if (ntiles && (!tile_msg_dev || !tile_first_dev)) return set_err(OTC_ERR_ARG, "gcm_mk_batch: null tile map");
    if ((((uintptr_t)ctr_msgs_dev) | ((uintptr_t)keys_dev) | ((uintptr_t)tile_first_dev)) & 7u ||
        ((uintptr_t)tile_msg_dev & 3u))
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: misaligned descriptor arrays");
    if ((uintptr_t)ws_dev & 15u) return set_err(OTC_ERR_ARG, "gcm_mk_batch: the workspace must be 16-byte aligned");
    if (dir == OTC_DIR_DECRYPT && (!expect_dev || !ok_dev))
        return set_err(OTC_ERR_ARG, "gcm_mk_batch: decryption needs the expected tags and the verdict array");
    if (dir == OTC_DIR_DECRYPT) {
        /* the expected tags are compared with what this call computes: never its own output */
        const uintptr_t e0 = (uintptr_t)expect_dev, e1 = e0 + nmsg * (size_t)tag_bytes;
        const uintptr_t t0 = (uintptr_t)tags_dev, v0 = (uintptr_t)ok_dev;
        if ((e0 < t0 + nmsg * 16 && t0 < e1) || (e0 < v0 + nmsg && v0 < e1))
            return set_err(OTC_ERR_ARG, "gcm_mk_batch: the expected tags overlap the computed tags or the verdicts");
    }
    if (!ivs_dev) return set_err(OTC_ERR_ARG, "gcm_mk_batch: null IVs");
    hipStream_t st = (hipStream_t)stream;
    set_last_impl(OTC_IMPL_TTABLE);
    uint8_t *j0 = (uint8_t *)ws_dev, *s = j0 + nmsg * 16;
    const bool enc = dir == OTC_DIR_ENCRYPT;

    hipError_t e = otc_impl::gcm_batch_prep(ivs_dev, nmsg, ctr_msgs_dev, j0, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_mk_batch prep launch");
    /* the CTR half: the batched kernel's static split, a key index per message */
    auto ctr = [&] {
        return ntiles ? otc_impl::tt_ctr_batch(ctr_msgs_dev, keys_dev, tile_msg_dev, tile_first_dev, ntiles, tile_blocks,
                                               nr, st, nullptr)
                      : hipSuccess;
    };
    if (enc && (e = ctr()) != hipSuccess) return hip_fail(e, "gcm_mk_batch ctr launch");
    /* over the ciphertext: out of an encryption, in of a decryption */
    if ((e = otc_impl::ghash_mk_batch_run(msgs_dev, nmsg, tab_dev, s, enc, lanes, st)) != hipSuccess)
        return hip_fail(e, "gcm_mk_batch hash launch");
    e = otc_impl::gcm_mk_batch_final(msgs_dev, keys_dev, j0, s, nmsg, nr, tags_dev, enc ? nullptr : expect_dev, tag_bytes,
                                     enc ? nullptr : ok_dev, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_mk_batch finisher launch");
    if (!enc) {
        if ((e = ctr()) != hipSuccess) return hip_fail(e, "gcm_mk_batch ctr launch");
        if ((e = otc_impl::gcm_mk_batch_wipe(msgs_dev, nmsg, ok_dev, st)) != hipSuccess)
            return hip_fail(e, "gcm_mk_batch wipe launch");
    }
    return OTC_OK;
}
