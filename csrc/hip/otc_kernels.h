/*
 * otc_kernels.h -- the host entry points of the kernel files (aes_tt.hip,
 * aes_xts.hip, aes_ocb.hip, aes_ocb_batch.hip, aes_ccm_batch.hip, aes_gcm.hip, aes_gcm_siv.hip, aes_gcm_siv_batch.hip, aes_gcm_batch.hip, aes_gcm_mk_batch.hip, aes_bs.hip, chacha.hip,
 * chacha_batch.hip, stream_ops.hip), declared once: included by their callers (engine.cpp,
 * aead.cpp, split.cpp) and by the files that define them, so every
 * definition is checked against the declaration its callers see.  Not part
 * of the public C API (otc.h).
 */
#ifndef OTC_KERNELS_H
#define OTC_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "otc.h"
#include "otc_device.h"

namespace otc_impl {

using otc_dev::Ctr128;
using otc_dev::SplitClaim;

/* One call of ECB or of a parallel decryption, as every kernel family takes
 * it: the grid T-table kernel, the T-table claim kernel and the bitsliced
 * claim kernel each fill their parameter block from this in one place. */
enum JobMode : int { JOB_ECB_ENC, JOB_ECB_DEC, JOB_CBC_DEC, JOB_CFB_DEC, JOB_CBC_DEC_SEG, JOB_CFB_DEC_SEG };
struct Job {
    JobMode mode;
    const void *in;
    void *out;
    uint64_t nblocks;
    const otc_aes_key *key;
    const uint8_t *iv;   /* 16 bytes (segment modes: IV of segment 0, IV_s = iv + s); null for ECB */
    uint64_t seg_blocks; /* segment modes: blocks per segment (>= 1) */
};
inline bool job_is_seg(const Job &j) { return j.mode == JOB_CBC_DEC_SEG || j.mode == JOB_CFB_DEC_SEG; }
/* log2 of a power-of-two segment length, else -1 (such segments run on the
 * grid T-table kernel only) */
inline int seg_shift_of(uint64_t seg_blocks)
{
    return seg_blocks && !(seg_blocks & (seg_blocks - 1)) ? __builtin_ctzll(seg_blocks) : -1;
}

/* The kernels take the round count as a template argument: f(the constant
 * 10, 12 or 14 as a std::integral_constant) for a key's nr */
template <class F>
hipError_t with_rounds(int nr, F f)
{
    switch (nr) {
    case 10: return f(std::integral_constant<int, 10>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 14: return f(std::integral_constant<int, 14>{});
    default: return hipErrorInvalidValue;
    }
}

/* ---- aes_tt.hip ---------------------------------------------------------- */
/* `cl` of tt_ctr, tt_seg_encrypt and tt_ctr_batch: null for the grid kernel,
 * else the persistent claim kernel over cl's units (claim_alone) */
/* the grid T-table kernel over the first nblocks blocks of the job (segment
 * modes: rounded up to whole segments) */
hipError_t tt_run(const Job &j, uint64_t nblocks, hipStream_t st);
/* the T-table claim kernel: the whole buffer, units from the back of `cl`,
 * plus the blocks past its last unit (power-of-two segments only) */
hipError_t tt_claim(const Job &j, SplitClaim cl, hipStream_t st);
hipError_t tt_ctr(const void *in, void *out, size_t nbytes, const otc_aes_key &K, Ctr128 c, bool wrap64,
                  hipStream_t st, const SplitClaim *cl = nullptr);
uint64_t tt_ctr_claim_units(size_t nbytes, uint64_t ctr_lo);
hipError_t tt_ctr_shift(const void *body_in, void *body_out, size_t len, const otc_aes_key &K, Ctr128 c,
                        hipStream_t st);
hipError_t xor_small(const void *in, void *out, uint32_t n, const uint8_t *ks, hipStream_t st);
/* CBC (cfb false) or CFB128 encryption of nseg segments; cl: 64-segment units */
hipError_t tt_seg_encrypt(bool cfb, const void *in, void *out, uint64_t seg_blocks, uint64_t nseg,
                          const otc_aes_key &K, Ctr128 iv0, hipStream_t st, const SplitClaim *cl);
/* cl null: the static split over the waves; else claimed runs of BATCH_UNIT tiles */
hipError_t tt_ctr_batch(const otc_ctr_msg *msgs, const otc_aes_key *keys, const uint32_t *tile_msg,
                        const uint64_t *tile_first, uint64_t ntiles, int tile_blocks, int nr, hipStream_t st,
                        const SplitClaim *cl);
uint64_t tt_ctr_batch_units(uint64_t ntiles);
int strace_read_tt(unsigned long long *buf, int max);

/* ---- aes_xts.hip --------------------------------------------------------- */
/* XTS over nblocks whole blocks in units of unit_blocks (1 .. 2^20); unit s
 * uses tweak number tweak0 + s (128-bit little-endian).  K1: the data key in
 * the call's direction, K2: the tweak key's encryption schedule. */
hipError_t xts_bulk(const void *in, void *out, uint64_t nblocks, uint32_t unit_blocks, const otc_aes_key &K1,
                    const otc_aes_key &K2, const uint8_t tweak0[16], hipStream_t st);
/* ciphertext stealing: the last 16 + r bytes of ONE unit of 16 m + r bytes
 * (queued behind xts_bulk over its first m - 1 blocks) */
hipError_t xts_steal(const void *in, void *out, uint32_t m, uint32_t r, const otc_aes_key &K1, const otc_aes_key &K2,
                     const uint8_t tweak0[16], hipStream_t st);

/* ---- aes_ocb.hip --------------------------------------------------------- */
/* the bulk kernel's boundaries in bytes, smallest first; returns how many there are */
int ocb_spans(uint64_t *spans, int max);
/* zero the 16 bytes of a checksum accumulator (4-byte aligned), in stream order */
hipError_t ocb_clear(void *checksum, hipStream_t st);
/* OCB3 over the whole blocks first_block + 1 .. first_block + nblocks of the
 * message whose Offset_0 is given (first_block + nblocks <= 2^32); in and out
 * address the first of them.  K: the key in the call's direction, l: L_0 ..
 * L_32.  The XOR of the blocks' plaintexts is XORed into the 16 device bytes
 * at checksum (4-byte aligned). */
hipError_t ocb_bulk(const void *in, void *out, uint64_t first_block, uint64_t nblocks, const otc_aes_key &K,
                    const uint8_t offset0[16], const uint8_t (*l)[16], void *checksum, hipStream_t st);
/* the trailing r < 16 bytes at in / out (offset_m: Offset of the last whole
 * block) and the tag: tag[0 .. tag_bytes) = the tag, the rest of its 16 bytes
 * zero.  checksum: the whole blocks' (it may be the tag's own 16 bytes), or
 * null for none.  Kenc: the encryption schedule, in both directions. */
hipError_t ocb_finish(const void *in, void *out, uint32_t r, bool dec, const otc_aes_key &Kenc,
                      const uint8_t offset_m[16], const uint8_t l_star[16], const uint8_t l_dollar[16],
                      const uint8_t hash[16], int tag_bytes, const void *checksum, void *tag, hipStream_t st);

/* ---- aes_gcm.hip --------------------------------------------------------- */
/* byte sizes of the GHASH decomposition's pieces, smallest first; returns how many there are */
int ghash_spans(uint64_t *spans, int max);
/* whether the levels reach nbytes (they reach 2^37 bytes) */
bool ghash_fits(uint64_t nbytes);
/* the per-call tables and partials of ghash_run over nbytes, stream-ordered
 * (behind otc_fault_inject_alloc); *ws stays null for nbytes == 0 */
hipError_t ghash_ws_alloc(uint64_t nbytes, hipStream_t st, void **ws);
/* out16 (device) = GHASH_h continued from y0 over nbytes of device data, or,
 * with lenblock and ekj0, the GCM tag ((Y ^ lenblock) . H) ^ ekj0.  Frees ws
 * behind its kernels, also when it fails. */
hipError_t ghash_run(const void *data, uint64_t nbytes, const uint8_t h[16], const uint8_t y0[16],
                     const uint8_t *lenblock, const uint8_t *ekj0, void *out16, void *ws, hipStream_t st);

/* ---- aes_gcm_siv.hip ----------------------------------------------------- */
/* byte sizes of the POLYVAL decomposition's pieces (GHASH's), smallest first; returns how many there are */
int polyval_spans(uint64_t *spans, int max);
/* the per-call tables and partials of polyval_run over nbytes, stream-ordered
 * (behind otc_fault_inject_alloc); *ws stays null for nbytes == 0 */
hipError_t polyval_ws_alloc(uint64_t nbytes, hipStream_t st, void **ws);
/* what turns the hash into the GCM-SIV tag: the length block, the nonce and
 * the derived encryption key's schedule */
struct SivTag {
    uint8_t lenblock[16];
    uint8_t nonce[12];
    const otc_aes_key *enc;
};
/* out16 (device) = POLYVAL_h continued from y0 over nbytes of device data, or,
 * with siv, the tag E(dot(Y ^ lenblock, H) ^ nonce, bit 127 cleared).  Frees
 * ws behind its kernels, also when it fails. */
hipError_t polyval_run(const void *data, uint64_t nbytes, const uint8_t h[16], const uint8_t y0[16], const SivTag *siv,
                       void *out16, void *ws, hipStream_t st);
/* byte sizes at which k_aes_ctr_le32 takes another path, smallest first (as ocb_spans) */
int ctr_le32_spans(uint64_t *spans, int max);
/* out = in ^ keystream of GCM-SIV's counter mode under K (an encryption
 * schedule) from the counter block in the 16 device bytes at ctr0_dev
 * (4-byte aligned), read in stream order; nbytes <= 2^36 */
hipError_t ctr_le32_run(const void *in, void *out, uint64_t nbytes, const otc_aes_key &K, const void *ctr0_dev,
                        hipStream_t st);

/* ---- aes_gcm_batch.hip --------------------------------------------------- */
/* lanes per record of the batched hash kernel's two forms */
constexpr int GB_LANES_SHORT = 16, GB_LANES_LONG = 64;
/* the batched hash kernel's boundaries in hashed blocks, smallest first */
int gcm_batch_spans(uint64_t *spans, int max);
size_t gcm_batch_table_bytes();
/* the per-key table image (H^16, H^64, H) from h, and the kernels' LDS opt-in */
hipError_t gcm_batch_tables(const uint8_t h[16], void *tab, hipStream_t st);
/* out16[m] = GHASH of record m (its `out` data with hash_out, else its `in`),
 * XORed with ekj0[m] if given; with ok, ok[m] = the first tag_bytes bytes equal
 * expect[m].  lanes: GB_LANES_SHORT or GB_LANES_LONG per record */
hipError_t ghash_batch_run(const otc_gcm_msg *msgs, uint64_t nmsg, const void *tab, void *out16, const void *ekj0,
                           const uint8_t *expect, int tag_bytes, uint8_t *ok, bool hash_out, int lanes, hipStream_t st);
/* ivs (nmsg x 12) -> the counters of ctr_msgs (IV || 00000002) and j0 (IV || 00000001) */
hipError_t gcm_batch_prep(const uint8_t *ivs, uint64_t nmsg, otc_ctr_msg *ctr_msgs, void *j0, hipStream_t st);
/* zero the output of every record with ok[m] == 0.  One kernel for both batched
 * AEADs: it reads `out` and `nbytes`, which otc_gcm_msg and otc_chacha_msg keep
 * in the same columns of a 48-byte descriptor */
hipError_t batch_wipe(const void *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st);
inline hipError_t gcm_batch_wipe(const otc_gcm_msg *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st)
{
    return batch_wipe(msgs, nmsg, ok, st);
}
inline hipError_t chacha_batch_wipe(const otc_chacha_msg *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st)
{
    return batch_wipe(msgs, nmsg, ok, st);
}

/* ---- aes_bs.hip ---------------------------------------------------------- */
hipError_t bs_ctr(const void *in, void *out, size_t nbytes, const otc_aes_key &K, Ctr128 c, bool wrap64,
                  hipStream_t st);
/* the bitsliced claim kernel: the whole buffer, units from the front of `cl` */
hipError_t bs_claim(const Job &j, SplitClaim cl, hipStream_t st);
hipError_t bs_preload();
int strace_read_bs(unsigned long long *buf, int max);

/* ---- chacha.hip ---------------------------------------------------------- */
/* out = in ^ ChaCha20 keystream (RFC 8439 layout) from block `counter`; any
 * byte count and alignment; the caller has checked that the counter does not
 * pass 2^32 - 1 */
hipError_t chacha20_run(const void *in, void *out, uint64_t nbytes, const uint8_t key[32], const uint8_t nonce[12],
                        uint32_t counter, hipStream_t st);
/* byte sizes of the Poly1305 decomposition's pieces, smallest first; returns how many there are */
int poly1305_spans(uint64_t *spans, int max);
/* the per-call partials of poly1305_run over nbytes, stream-ordered (behind
 * otc_fault_inject_alloc); *ws stays null for nbytes == 0 */
hipError_t poly1305_ws_alloc(uint64_t nbytes, hipStream_t st, void **ws);
/* out16 (device) = Poly1305 under the clamped r (five 26-bit limbs) and s,
 * continued from the state h0 (limbs) over nbytes of 16-byte aligned device
 * data.  lenblock: the AEAD's 16-byte length block, hashed last.  pad16: a
 * short last block is zero-padded to a full one (the AEAD), else it gets the
 * 0x01 byte.  Frees ws behind its kernels, also when it fails. */
hipError_t poly1305_run(const void *data, uint64_t nbytes, const uint32_t r[5], const uint32_t h0[5],
                        const uint8_t s[16], const uint8_t *lenblock, bool pad16, void *out16, void *ws,
                        hipStream_t st);

/* ---- chacha_batch.hip ----------------------------------------------------- */
/* lanes per record of the batched Poly1305 kernel's two forms */
constexpr int CB_LANES_SHORT = 16, CB_LANES_LONG = 64;
/* the batched hash kernel's boundaries in hashed blocks, smallest first */
int chacha_batch_spans(uint64_t *spans, int max);
/* otk[m] (32 bytes, 16-byte aligned array) = bytes 0..31 of block 0 under
 * (keys[msgs[m].key], nonces[m]), r clamped */
hipError_t chacha_batch_prep(const otc_chacha_msg *msgs, uint64_t nmsg, const uint8_t *keys, const uint8_t *nonces,
                             void *otk, hipStream_t st);
/* out = in ^ keystream from block 1 for every record, tile by tile */
hipError_t chacha20_batch_run(const otc_chacha_msg *msgs, const uint8_t *keys, const uint8_t *nonces,
                              const uint32_t *tile_msg, const uint64_t *tile_first, uint64_t ntiles, hipStream_t st);
/* tags[m] = the AEAD's Poly1305 tag of record m (its `out` data with hash_out,
 * else its `in`) under otk[m]; with ok, ok[m] = the tag equals expect[m], and
 * the tag of a record that fails is zeroed.  lanes: CB_LANES_SHORT or _LONG */
hipError_t poly1305_batch_run(const otc_chacha_msg *msgs, uint64_t nmsg, const void *otk, void *tags,
                              const uint8_t *expect, uint8_t *ok, bool hash_out, int lanes, hipStream_t st);

/* ---- aes_ocb_batch.hip ---------------------------------------------------- */
/* the bulk kernel's boundaries in bytes, smallest first; returns how many there are */
int ocb_batch_spans(uint64_t *spans, int max);
/* ws (16-byte aligned, 48 bytes per record): Offset_0[m] under (k, nonces[m]),
 * a zero checksum[m], HASH(K, aad[m]) */
hipError_t ocb_batch_prep(const otc_ocb_msg *msgs, uint64_t nmsg, const otc_ocb_key &k, const uint8_t *nonces, void *ws,
                          hipStream_t st);
/* the whole blocks of every record, tile by tile; their plaintexts' XOR into checksum[m] */
hipError_t ocb_batch_bulk(const otc_ocb_msg *msgs, uint64_t nmsg, const uint32_t *tile_msg, const uint64_t *tile_first,
                          uint64_t ntiles, const otc_ocb_key &k, bool dec, void *ws, hipStream_t st);
/* the trailing bytes and tags[m]; with ok (a decryption), ok[m] = the tag equals
 * expect[m], and the tag of a record that fails is zeroed */
hipError_t ocb_batch_finish(const otc_ocb_msg *msgs, uint64_t nmsg, const otc_ocb_key &k, void *ws, void *tags,
                            const uint8_t *expect, uint8_t *ok, hipStream_t st);
inline hipError_t ocb_batch_wipe(const otc_ocb_msg *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st)
{
    return batch_wipe(msgs, nmsg, ok, st);
}

/* ---- aes_ccm_batch.hip ---------------------------------------------------- */
/* the kernel's boundaries, smallest first (otc.h otc_ccm_batch_spans); returns how many there are */
int ccm_batch_spans(uint64_t *spans, int max);
/* every record in one launch, lane t on record order[t]: out, tags[m] (tag_len
 * bytes each, any alignment); with dec, ok[m] = the tag equals expect[m], and the
 * tag of a record that fails is zeroed.  K: the encryption schedule, either way */
hipError_t ccm_batch_run(const otc_ccm_msg *msgs, const uint32_t *order, uint64_t nmsg, const otc_aes_key &K, bool dec,
                         const uint8_t *nonces, int nonce_len, uint8_t *tags, int tag_len, const uint8_t *expect,
                         uint8_t *ok, hipStream_t st);
inline hipError_t ccm_batch_wipe(const otc_ccm_msg *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st)
{
    return batch_wipe(msgs, nmsg, ok, st);
}

/* ---- aes_gcm_siv_batch.hip ------------------------------------------------- */
/* lanes per record of the batched POLYVAL kernel's two forms */
constexpr int GSB_LANES_SHORT = 16, GSB_LANES_LONG = 64;
/* the batched hash kernel's boundaries in hashed blocks, smallest first */
int gcm_siv_batch_spans(uint64_t *spans, int max);
/* per record: h[m] (nmsg x 16, 16-byte aligned) = the POLYVAL key and keys[m] =
 * the expanded encryption key that kgk (nr 10 or 14) and nonces[m] derive */
hipError_t gcm_siv_batch_derive(const otc_aes_key &kgk, const uint8_t *nonces, uint64_t nmsg, void *h, otc_aes_key *keys,
                                hipStream_t st);
/* s[m] (nmsg x 16, 16-byte aligned) = POLYVAL under h[m] of record m's padded AAD,
 * padded data (its `out` with hash_out, else its `in`) and length block.
 * lanes: GSB_LANES_SHORT or GSB_LANES_LONG per record */
hipError_t polyval_batch_run(const otc_gcm_msg *msgs, uint64_t nmsg, const void *h, void *s, bool hash_out, int lanes,
                             hipStream_t st);
/* tags[m] = E_{keys[m]}((s[m] ^ nonces[m]) with bit 127 cleared); with ok (a
 * decryption), ok[m] = the tag equals expect[m], and the tag of a record that
 * fails is zeroed */
hipError_t gcm_siv_batch_final(const void *s, const uint8_t *nonces, const otc_aes_key *keys, uint64_t nmsg, int nr,
                               void *tags, const uint8_t *expect, uint8_t *ok, hipStream_t st);
/* GCM-SIV's counter mode for every record, tile by tile (256 blocks): record m
 * under keys[m] (nr rounds each) from the counter block ctrs[m] (nmsg x 16
 * bytes, 4-byte aligned), both read in stream order */
hipError_t ctr_le32_batch_run(const otc_gcm_msg *msgs, const otc_aes_key *keys, const void *ctrs,
                              const uint32_t *tile_msg, const uint64_t *tile_first, uint64_t ntiles, int nr,
                              hipStream_t st);
inline hipError_t gcm_siv_batch_wipe(const otc_gcm_msg *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st)
{
    return batch_wipe(msgs, nmsg, ok, st);
}

/* ---- aes_gcm_mk_batch.hip -------------------------------------------------- */
/* lanes per record of the many-key batched hash kernel's two forms */
constexpr int GMK_LANES_SHORT = 16, GMK_LANES_LONG = 64;
/* the batched hash kernel's boundaries in hashed blocks, smallest first */
int gcm_mk_batch_spans(uint64_t *spans, int max);
/* bytes of the table image of nkeys keys: seven nibble tables of 256 bytes each per key */
size_t gcm_mk_batch_table_bytes(size_t nkeys);
/* tab (16-byte aligned) = the table images of the GHASH keys E_K(0^128) of the
 * nkeys encryption schedules at keys (nr rounds each) */
hipError_t gcm_mk_batch_tables(const otc_aes_key *keys, uint64_t nkeys, int nr, void *tab, hipStream_t st);
/* s[m] (nmsg x 16, 16-byte aligned) = GHASH under the key whose image is
 * tab[msgs[m].key] of record m's padded AAD, padded data (its `out` with
 * hash_out, else its `in`) and length block.  lanes: GMK_LANES_SHORT or _LONG */
hipError_t ghash_mk_batch_run(const otc_gcm_mk_msg *msgs, uint64_t nmsg, const void *tab, void *s, bool hash_out,
                              int lanes, hipStream_t st);
/* tags[m] = s[m] ^ E_{keys[msgs[m].key]}(j0[m]); with ok (a decryption), ok[m] =
 * the first tag_bytes bytes equal expect[m], and the tag of a record that fails
 * is zeroed */
hipError_t gcm_mk_batch_final(const otc_gcm_mk_msg *msgs, const otc_aes_key *keys, const void *j0, const void *s,
                              uint64_t nmsg, int nr, void *tags, const uint8_t *expect, int tag_bytes, uint8_t *ok,
                              hipStream_t st);
inline hipError_t gcm_mk_batch_wipe(const otc_gcm_mk_msg *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st)
{
    return batch_wipe(msgs, nmsg, ok, st);
}

/* ---- stream_ops.hip ------------------------------------------------------ */
hipError_t k_xor(const void *a, const void *b, void *out, size_t n, hipStream_t st);
hipError_t k_fill_random(void *p, size_t n, uint64_t seed, hipStream_t st);
hipError_t k_checksum(const void *p, size_t n, uint64_t *out, hipStream_t st);
hipError_t k_clock(uint64_t *out, uint64_t delay_ticks, uint64_t ticks, hipStream_t st);
hipError_t k_rc4_multi(const uint8_t *keys, int keylen, size_t nstreams, size_t len, size_t drop, const void *in,
                       void *out, hipStream_t st);
hipError_t k_rc4_states(void *states, size_t nstreams, size_t len, const void *in, void *out, hipStream_t st);

} // namespace otc_impl

#endif
