/*
 * otc.h -- public C API of the MI355X (gfx950) bulk symmetric-cipher engine.
 *
 * Layers (re-designed MI355X-first):
 *   L1/L2 device kernels  -> otc_aes_* / otc_rc4_* / otc_xor  (device pointers,
 *                            asynchronous on a caller-supplied hipStream_t)
 *   L3 engine runtime     -> otc_ctx_* (persistent per-device state, tables,
 *                            streams, pinned staging ring) and otc_stream_*
 *                            (host-memory pipelined H2D | kernel | D2H)
 *   L4 multi-GPU          -> otc_multi_* (single-process RCCL over xGMI) ; the
 *                            one-process-per-GPU path lives in
 *                            our_tree_amd/parallel (torch.distributed / RCCL)
 *
 * Reference counterparts: BlockCipher/AES host class
 * (/root/reference/aes-gpu/Source/BlockCipher.h:48-107, AES.h:84-147,
 * AES.cu:50-282) and the CUDA kernels (AES.cu:284-502).  Unlike the reference,
 * every entry point returns an error code (no silent launch failures,
 * AES.cu:250), nothing is allocated per call, and any length is accepted.
 *
 * Streams are passed as `void *` (a hipStream_t; NULL = default stream) so the
 * header is usable from plain C and from ctypes.
 */
#ifndef OTC_H
#define OTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- errors -------------------------------------------------------------- */
#define OTC_OK 0
#define OTC_ERR_ARG -1        /* bad argument (length, key size, alignment) */
#define OTC_ERR_HIP -2        /* a HIP runtime call failed; see otc_last_error() */
#define OTC_ERR_RCCL -3       /* an RCCL call failed */
#define OTC_ERR_UNSUPPORTED -4
#define OTC_ERR_NOMEM -5

const char *otc_last_error(void);

/* ---- keys ---------------------------------------------------------------- */
#define OTC_DIR_ENCRYPT 1
#define OTC_DIR_DECRYPT 0

/* Expanded key passed BY VALUE as a kernel argument, so round keys land in
 * SGPRs (wave-uniform) with no per-launch copy.  rk: LE column words as in
 * aes_export_rk32(); for OTC_DIR_DECRYPT the equivalent-inverse schedule. */
typedef struct {
    uint32_t rk[60];
    int32_t nr;   /* 10 / 12 / 14 */
    int32_t dir;  /* OTC_DIR_* */
    int32_t bits; /* 128 / 192 / 256 */
    int32_t pad;
} otc_aes_key;

int otc_aes_key_init(otc_aes_key *k, const uint8_t *key, int bits, int dir);

/* ---- implementation selection ------------------------------------------- */
#define OTC_IMPL_AUTO 0     /* the measured winner (docs/PERF.md rounds 5-6): bitsliced for CTR calls >= 2 GiB
                               (AES-256: >= 1 GiB), the persistent T-table CTR kernel from 512 MiB; for ECB / CBC / CFB decryption and the power-of-two segment
                               decryptions the split below from 2 GiB and the persistent T-table claim kernel
                               alone from 512 MiB; segment encryption: the persistent T-table claim kernel from
                               1 GiB; the grid T-table otherwise
                               (OTC_IMPL=ttable|bitslice|split env overrides for the whole process, each where it
                               applies: split for ECB and the decryptions only) */
#define OTC_IMPL_TTABLE 1   /* LDS-resident replicated T-table kernel */
#define OTC_IMPL_BITSLICE 2 /* bitsliced VALU kernel alone: 32 blocks per lane (CTR, ECB, the decryptions; their
                               claim kernels take every 2048-block unit and one T-table workgroup the blocks past
                               the last); segment encryption has no VALU kernel and runs the T-table */
#define OTC_IMPL_SPLIT 3    /* the T-table and the bitsliced kernel CONCURRENTLY over one buffer, each on a
                               pooled CU-masked stream, co-resident on every CU -- LDS and VALU busy at once --
                               claiming units from one counter: ECB, the CBC / CFB decryptions and the segment
                               decryptions ("auto" for these >= 2 GiB).  CTR has no split (it lost to the
                               bitsliced kernel on both HIP runtimes, removed in round 6): a CTR call with
                               OTC_IMPL_SPLIT takes the auto choice */

/* The kernel family `impl` resolves to for a call of nbytes with a bits-bit
 * key (mode 1: CTR, 0: ECB encryption, 2: ECB / CBC decryption, 3: CFB128
 * decryption, 4: CBC / CFB128 decryption of power-of-two segments, 5: CBC /
 * CFB128 encryption of segments < 8 MiB); -1 for an invalid impl or mode. */
int otc_pick_impl(int impl, int bits, int mode, uint64_t nbytes);
/* What the calling thread's last AES call ran: OTC_IMPL_TTABLE,
 * OTC_IMPL_BITSLICE or OTC_IMPL_SPLIT (OTC_IMPL_AUTO before any call).  Set
 * by otc_aes_ctr / _rfc3686 / _ctr_stream, otc_aes_ecb, the CBC / CFB128
 * decryptions and every segment call; a split or bitsliced request that fell
 * back to the T-table (too few units, no memory for the claim counter, the
 * bitsliced half failing to launch) reports OTC_IMPL_TTABLE. */
int otc_last_impl(void);
/* Split accounting, a profiling mode (off by default): with
 * otc_split_stats(1) every split call on this thread waits for its kernels
 * and records its claim counter; otc_split_last_units then gives the units
 * the bitsliced side (front) and the T-table side (back) took in the last
 * such call, of nunits (2048-block units, or 64-segment units for segment
 * encryption).  Under impl "bitslice" front == nunits. */
void otc_split_stats(int on);
/* Why the calling thread's last split / bitsliced-claim request ran the
 * T-table alone ("" when it did not fall back): too few claim units, no
 * memory for the claim counter, the per-device pool of auxiliary streams
 * exhausted (at most 4 concurrent split calls per device, each holding two
 * dedicated hardware queues), or the bitsliced half failing to launch. */
const char *otc_split_fallback_reason(void);
int otc_split_last_units(uint64_t *front, uint64_t *back, uint64_t *nunits);
/* Diagnostic builds only (-DOTC_SPLIT_TRACE=1): copy out and reset the
 * wave-start records of the split's kernels (which: 0 T-table, 1 bitsliced),
 * pairs {s_memrealtime, tag << 32 | HW_ID}; returns the count, or -1
 * in the shipped build. */
int otc_split_trace(int which, unsigned long long *buf, int max);

/* ---- device ops (device pointers; async on `stream`) ---------------------
 * All functions accept any byte length; the trailing partial block of CTR is
 * handled inside the kernel.  ECB/CBC lengths must be multiples of 16.
 * In-place (in == out) is allowed except for otc_aes_cbc_decrypt and
 * otc_aes_cfb128_decrypt (they read the previous ciphertext block).
 */
int otc_aes_ecb(const void *in, void *out, size_t nbytes, const otc_aes_key *k, int impl,
                void *stream);

/* CTR with a full 128-bit big-endian counter starting at ctr0 (the semantics
 * of aes_crypt_ctr with nc_off == 0).  `block_offset` is added to ctr0 first
 * (128-bit add with carry) -- this is how shards of one stream are encrypted
 * independently. */
int otc_aes_ctr(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                const uint8_t ctr0[16], uint64_t block_offset, int impl, void *stream);

/* Resumable CTR stream on device buffers with the PolarSSL context semantics
 * (reference aes-modes/aes.c:869-900): nonce_counter = counter of the NEXT
 * block to generate, stream_block = keystream of the current block, nc_off =
 * bytes of it already used.  Calls may split the stream at any byte; in and
 * out may be misaligned but must share their alignment modulo 16.  The
 * context is updated on return (the launches are asynchronous on `stream`). */
typedef struct {
    uint8_t nonce_counter[16];
    uint8_t stream_block[16];
    size_t nc_off;
} otc_aes_ctr_ctx;
int otc_aes_ctr_ctx_init(otc_aes_ctr_ctx *ctx, const uint8_t nonce_counter[16]);
int otc_aes_ctr_stream(otc_aes_ctr_ctx *ctx, const otc_aes_key *k, size_t length, const void *in, void *out,
                       int impl, void *stream);

/* CTR with the AES-NI/RFC 3686 counter layout nonce[4] || ivec[8] || BE32(1),
 * the low 8 bytes incremented as a 64-bit big-endian integer
 * (reference aesni.c:120-152). */
int otc_aes_ctr_rfc3686(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                        const uint8_t nonce[4], const uint8_t ivec[8], uint64_t block_offset,
                        int impl, void *stream);

/* CBC decryption (parallel): P_i = D(C_i) ^ C_{i-1}, C_{-1} = iv.  _impl:
 * with a kernel choice (OTC_IMPL_*; the plain form is OTC_IMPL_AUTO). */
int otc_aes_cbc_decrypt(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                        const uint8_t iv[16], void *stream);
int otc_aes_cbc_decrypt_impl(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                             const uint8_t iv[16], int impl, void *stream);

/* CBC encryption over `nseg` independent segments of `seg_bytes` each
 * (contiguous, segment s at offset s*seg_bytes).  Segment s uses
 * IV_s = iv0 + s (128-bit big-endian add), the "plain64"-style sector IV.
 * A single segment (nseg == 1) is exact single-stream CBC, serial. */
int otc_aes_cbc_encrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                 const otc_aes_key *k, const uint8_t iv0[16], void *stream);
/* _impl: accepted for symmetry; every impl runs the T-table kernels (one
 * serial chain per lane): the persistent claim kernel from 1 GiB (at least
 * 1024 segments), the grid kernel below (its workgroups sized so every CU
 * gets chains).  A VALU
 * kernel for this mode lost at every size and was removed (round 6). */
int otc_aes_cbc_encrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                      const otc_aes_key *k, const uint8_t iv0[16], int impl, void *stream);
/* Same, decryption side (fully parallel).  _impl: with a kernel choice --
 * "auto" runs the T-table + bitsliced split from 2 GiB of power-of-two
 * segments and the persistent T-table claim kernel alone from 512 MiB;
 * OTC_IMPL_BITSLICE runs the bitsliced segment claim kernel alone; other
 * segment sizes: T-table. */
int otc_aes_cbc_decrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                 const otc_aes_key *k, const uint8_t iv0[16], void *stream);
int otc_aes_cbc_decrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                      const otc_aes_key *k, const uint8_t iv0[16], int impl, void *stream);

/* CFB128 over nseg independent segments of seg_bytes (multiple of 16) with
 * IV_s = iv0 + s (128-bit BE add) -- the parallel form of the serial CFB
 * chain, like otc_aes_cbc_encrypt_segments.  Encryption keys for both
 * directions.  Encrypt may run in place; decrypt may not. */
int otc_aes_cfb128_encrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                    const otc_aes_key *k, const uint8_t iv0[16], void *stream);
int otc_aes_cfb128_encrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                         const otc_aes_key *k, const uint8_t iv0[16], int impl, void *stream);
int otc_aes_cfb128_decrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                    const otc_aes_key *k, const uint8_t iv0[16], void *stream);
int otc_aes_cfb128_decrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                         const otc_aes_key *k, const uint8_t iv0[16], int impl, void *stream);

/* XTS-AES (IEEE 1619 / SP 800-38E) over nunits data units (sectors) of
 * unit_bytes each, fully parallel in both directions.  The key is K1 || K2:
 * `data` is K1's schedule in the call's direction, `tweak` K2's -- always an
 * encryption schedule.  Equal key halves are accepted: this is the primitive,
 * and a policy such as SP 800-38E's K1 != K2 belongs to its caller.
 * Unit s uses tweak number tweak0 + s, a 128-bit LITTLE-endian value (add
 * with carry through all 16 bytes; dm-crypt plain64 is LE64(sector) || 0^8).
 * unit_bytes is 16 .. 2^24 (2^20 blocks) and a multiple of 16 when nunits > 1;
 * a single unit may have any length in that range and then ends with
 * ciphertext stealing.  The direction comes from the key; in place is allowed
 * both ways; buffers are 16-byte aligned as for otc_aes_ecb.  nunits == 0
 * launches nothing.  Runs the grid T-table kernels of aes_xts.hip
 * (otc_last_impl: OTC_IMPL_TTABLE), tuned for units up to 64 KiB. */
typedef struct {
    otc_aes_key data;
    otc_aes_key tweak; /* always an encryption schedule */
} otc_xts_key;
int otc_xts_key_init(otc_xts_key *k, const uint8_t *key, int keybits /* 256 | 512 */, int dir);
int otc_aes_xts(const void *in, void *out, size_t unit_bytes, size_t nunits, const otc_xts_key *k,
                const uint8_t tweak0[16], void *stream);

/* AES-GCM (NIST SP 800-38D) of ONE message in device memory, 128/192/256-bit
 * keys: nbytes is 0 .. 2^36 - 32 (any byte count), the IV any length >= 1
 * (12 bytes: J0 = IV || 0^31 || 1; others through GHASH, as the standard
 * says).  iv and aad are HOST memory -- AAD is for headers; hash large
 * device-resident data with otc_ghash.  dir is OTC_DIR_ENCRYPT or
 * OTC_DIR_DECRYPT; tag_dev is 16 bytes of device memory that receive the
 * COMPUTED tag in both directions (comparing it with a received tag is the
 * caller's: ops.gcm_decrypt does it with one readback).  Everything that does
 * not depend on the data -- J0, E_K(J0), the AAD's hash state, the length
 * block -- is computed on the host and travels by value, so the call does not
 * synchronise and can be captured in a graph.  Stream order: encrypt: CTR32
 * from inc32(J0), then GHASH over out; decrypt: GHASH over in, then CTR32 --
 * in place works both ways; the hash ends in a one-wave kernel that writes
 * the tag.
 * nbytes == 0 launches only that.  Buffers are 16-byte aligned.  The hash's
 * per-call tables and partials are stream-ordered allocations made BEFORE
 * anything is launched: a failure (otc_fault_inject_alloc covers it) leaves
 * out and tag_dev untouched.  impl chooses the CTR half's kernel, which is
 * what otc_last_impl reports; the hash has one (csrc/hip/aes_gcm.hip). */
typedef struct {
    otc_aes_key enc; /* K's encryption schedule: GCM never runs the inverse cipher */
    uint8_t h[16];   /* H = E_K(0^128) */
} otc_gcm_key;
int otc_gcm_key_init(otc_gcm_key *k, const uint8_t *key, int keybits);
int otc_aes_gcm(const void *in, void *out, size_t nbytes, const otc_gcm_key *k, int dir, const uint8_t *iv,
                size_t iv_len, const uint8_t *aad, size_t aad_len, void *tag_dev, int impl, void *stream);
/* GCM's counter mode: bytes 12..15 of ctr0 increment big-endian and wrap at
 * 2^32, bytes 0..11 never change.  The CTR kernels of otc_aes_ctr, every
 * impl: a call crosses the wrap at most once and is split there, on a block
 * boundary, into two launches.  nbytes is at most 2^32 blocks. */
int otc_aes_ctr32(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const uint8_t ctr0[16], int impl,
                  void *stream);
/* y_dev[16] (device) = GHASH_h continued from y0 over nbytes (0 .. 2^36) of
 * device data, 16-byte aligned, the last partial block zero-padded; h and y0
 * are host memory.  Parallel over the whole chip. */
int otc_ghash(const void *data, size_t nbytes, const uint8_t h[16], const uint8_t y0[16], void *y_dev, void *stream);
/* Byte sizes of the pieces the GHASH kernel cuts its data into, smallest
 * first (a pass of 64 lanes, a batch of passes, a wave's span, a workgroup's
 * spans, a level-2 span, a level-3 span): lengths around them are where the
 * kernel takes another path.  Writes up to max of them; returns the count. */
int otc_ghash_spans(uint64_t *spans, int max);

/* AES-GCM-SIV (RFC 8452) of ONE message in device memory, 128- or 256-bit
 * keys: the AEAD that stays safe when a nonce repeats under a key (a repeat
 * shows only whether two messages were equal).  The caller's key is a key-
 * GENERATING key: every call derives the nonce's POLYVAL key and encryption
 * key from it on the host (4 or 6 block encryptions and a key expansion) and
 * hashes the AAD there; nonce (exactly 12 bytes) and aad are HOST memory.
 * nbytes and aad_len are 0 .. 2^36 each; the tag is always 16 bytes.  dir is
 * OTC_DIR_ENCRYPT or OTC_DIR_DECRYPT; tag_dev is 16 bytes of 4-byte aligned
 * device memory that receive the COMPUTED tag in both directions.  The tag is
 * also the counter mode's initial counter block, so it never leaves the
 * device: an encryption's counter kernel reads it where the finisher wrote
 * it, a decryption's reads the RECEIVED tag from tag_in_dev (16 bytes of
 * 4-byte aligned device memory; an encryption ignores it) -- comparing the
 * two is the caller's (ops.gcm_siv_ops.gcm_siv_decrypt does it with one
 * readback).  The call does not synchronise and can be captured in a graph.
 * Stream order: encrypt: POLYVAL over in, the finisher (tag_dev), the counter
 * mode from tag_dev; decrypt: the counter mode from tag_in_dev, POLYVAL over
 * out, the finisher.  In place works both ways; neither tag may lie in the
 * data.  Buffers are 16-byte aligned.  The hash's per-call tables and
 * partials are stream-ordered allocations made BEFORE anything is launched: a
 * failure (otc_fault_inject_alloc covers it) leaves out and tag_dev
 * untouched.  otc_last_impl: OTC_IMPL_TTABLE (there is one kernel family,
 * csrc/hip/aes_gcm_siv.hip). */
#define OTC_GCM_SIV_MAX_BYTES (((uint64_t)1) << 36)
typedef struct {
    otc_aes_key kgk; /* the key-generating key's encryption schedule */
} otc_gcm_siv_key;
int otc_gcm_siv_key_init(otc_gcm_siv_key *k, const uint8_t *key, int keybits /* 128 | 256 */);
int otc_aes_gcm_siv(const void *in, void *out, size_t nbytes, const otc_gcm_siv_key *k, int dir,
                    const uint8_t nonce[12], const uint8_t *aad, size_t aad_len, const void *tag_in_dev, void *tag_dev,
                    void *stream);
/* GCM-SIV's counter mode: bytes 0..3 of the counter block increment
 * little-endian and wrap at 2^32 without carry, bytes 4..15 never change, and
 * bit 7 of byte 15 is forced on.  The initial counter block is 16 bytes of
 * 4-byte aligned DEVICE memory outside out, read in stream order -- what an
 * earlier kernel on the stream wrote there is what counts.  k is an
 * encryption schedule of any key size; nbytes is at most 2^32 blocks, so one
 * launch covers the wrap. */
int otc_aes_ctr_le32(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const void *ctr0_dev,
                     void *stream);
/* y_dev[16] (device) = POLYVAL_h (RFC 8452 section 3) continued from y0 over
 * nbytes (0 .. 2^36) of device data, 16-byte aligned, the last partial block
 * zero-padded; h and y0 are host memory.  Parallel over the whole chip: GHASH's
 * level kernel over tables in POLYVAL's convention. */
int otc_polyval(const void *data, size_t nbytes, const uint8_t h[16], const uint8_t y0[16], void *y_dev, void *stream);
/* otc_ghash_spans for POLYVAL (the same pieces), and otc_ocb_spans for the
 * counter kernel (a lane's block, one load of a wave, a pass, a wave's run, a
 * workgroup's chunk, the full grid's first step) */
int otc_polyval_spans(uint64_t *spans, int max);
int otc_ctr_le32_spans(uint64_t *spans, int max);

/* AES-OCB3 (RFC 7253) of ONE message in device memory, 128/192/256-bit keys:
 * an AEAD in one pass -- one block-cipher call per block, the tag from an XOR
 * of the plaintext blocks (csrc/hip/aes_ocb.hip).  nbytes is 0 .. 2^36 (any
 * byte count), the nonce 1..15 bytes, tag_bytes 1..16; the tag length enters
 * the nonce block, so another tag length gives another ciphertext.  nonce and
 * aad are HOST memory, as in otc_aes_gcm.  dir is OTC_DIR_ENCRYPT or
 * OTC_DIR_DECRYPT; tag_dev is 16 bytes of 4-byte aligned device memory that
 * receive the COMPUTED tag in both directions: its first tag_bytes are the
 * tag, the rest zero (comparing it with a received tag is the caller's:
 * ops.ocb_decrypt does it with one readback).  Offset_0, HASH(K, A) and the
 * last whole block's offset are computed on the host and travel by value: the
 * call does not synchronise, allocates nothing and can be captured in a
 * graph.  Stream order: tag_dev is cleared and collects the whole blocks'
 * checksum from the bulk kernel; a one-lane finisher handles the trailing
 * bytes and turns the checksum into the tag.  Fewer than 16 bytes launch only
 * the finisher.  Buffers are 16-byte aligned; in place is allowed both ways.
 * Every bad argument is OTC_ERR_ARG before any HIP call.  otc_last_impl:
 * OTC_IMPL_TTABLE (there is one kernel family and no impl argument). */
#define OTC_OCB_MAX_BYTES (((uint64_t)1) << 36)
typedef struct {
    otc_aes_key enc;      /* K's encryption schedule */
    otc_aes_key dec;      /* K's decryption schedule (equivalent inverse) */
    uint8_t l_star[16];   /* L_* = E_K(0^128) */
    uint8_t l_dollar[16]; /* L_$ = double(L_*) */
    uint8_t l[33][16];    /* L_0 = double(L_$), L_j = double(L_{j-1}) */
} otc_ocb_key;
int otc_ocb_key_init(otc_ocb_key *k, const uint8_t *key, int keybits);
int otc_aes_ocb(const void *in, void *out, size_t nbytes, const otc_ocb_key *k, int dir, const uint8_t *nonce,
                size_t nonce_len, const uint8_t *aad, size_t aad_len, int tag_bytes, void *tag_dev, void *stream);
/* The primitive: the whole blocks first_block + 1 .. first_block + nblocks of
 * a message whose Offset_0 (host memory, 16 bytes) is given, in and out
 * addressing the first of them; first_block + nblocks <= 2^32.  The XOR of
 * those blocks' plaintexts is XORed into the 16 device bytes at checksum_dev
 * (16-byte aligned; the caller zeroes them before the first piece).  A
 * message can be cut across calls, streams or devices this way; the caller
 * finishes it (the trailing bytes and the tag: aes.h aes_crypt_ocb shows how). */
int otc_aes_ocb_blocks(const void *in, void *out, uint64_t nblocks, const otc_ocb_key *k, int dir,
                       const uint8_t offset0[16], uint64_t first_block, void *checksum_dev, void *stream);
/* Byte sizes at which the bulk kernel takes another path, smallest first (a
 * lane's block, one load of a wave, a pass, a wave's run, a workgroup's chunk,
 * and the full grid's first step -- past it workgroups take a second grid
 * step), like otc_ghash_spans. */
int otc_ocb_spans(uint64_t *spans, int max);

/* ---- ChaCha20, Poly1305, ChaCha20-Poly1305 (RFC 8439) ----------------------
 * The IETF layout: a 32-byte key, a 12-byte nonce, a 32-bit block counter
 * (state word 12).  key, nonce and aad are HOST memory; the data is device
 * memory; calls are asynchronous on the caller's stream, do not synchronise
 * and can be captured in a graph.  One kernel family (csrc/hip/chacha.hip):
 * otc_last_impl and otc_pick_impl do not know these modes.
 *
 * Counter wrap: RFC 8439 leaves an overflow of the 32-bit counter undefined
 * and implementations differ (some carry into the first nonce word, some wrap
 * to 0 and repeat keystream).  This engine refuses: a call with
 * counter + ceil(nbytes / 64) > 2^32 returns OTC_ERR_ARG before any HIP call;
 * a call whose last block is exactly 2^32 - 1 is fine.
 *
 * otc_chacha20: out = in ^ keystream from block `counter`.  Any byte count,
 * any alignment (buffers that are not both 16-byte aligned run on the
 * byte-wise edge kernel, which is slower); in == out or disjoint. */
int otc_chacha20(const void *in, void *out, size_t nbytes, const uint8_t key[32], const uint8_t nonce[12],
                 uint32_t counter, void *stream);
/* tag_dev[16] (device, 4-byte aligned) = Poly1305 of nbytes of device data
 * (16-byte aligned) under the one-time key r || s (r is clamped here).
 * Parallel over the whole chip; its partials are one stream-ordered
 * allocation made before anything is launched (OTC_ERR_NOMEM leaves tag_dev
 * untouched; otc_fault_inject_alloc covers it). */
int otc_poly1305(const void *data, size_t nbytes, const uint8_t key[32], void *tag_dev, void *stream);
/* Byte sizes of the pieces the Poly1305 kernel cuts its data into, smallest
 * first (a pass of 64 lanes, a batch of passes, a wave's span, a workgroup's
 * spans, a level-2 span, a level-3 span), like otc_ghash_spans. */
int otc_poly1305_spans(uint64_t *spans, int max);
/* The AEAD of RFC 8439 section 2.8 over ONE message in device memory: nbytes
 * is 0 .. (2^32 - 1) * 64, buffers 16-byte aligned.  The one-time Poly1305
 * key (block 0), the hash state after the AAD and the length block are
 * computed on the host and travel by value.  tag_dev receives the COMPUTED
 * tag in both directions (comparing it is the caller's, as with otc_aes_gcm).
 * Stream order: encrypt: ChaCha20 from counter 1, then Poly1305 over out;
 * decrypt: Poly1305 over in, then ChaCha20 -- in place works both ways.
 * nbytes == 0 launches only the hash's finishing kernel.  The workspace is
 * allocated before anything is launched: OTC_ERR_NOMEM leaves out and tag_dev
 * untouched. */
int otc_chacha20_poly1305(const void *in, void *out, size_t nbytes, const uint8_t key[32], int dir,
                          const uint8_t nonce[12], const uint8_t *aad, size_t aad_len, void *tag_dev, void *stream);

/* CFB128 decryption (parallel): P_i = C_i ^ E(C_{i-1}), C_{-1} = iv;
 * nbytes % 16 == 0; encryption key.  _impl: with a kernel choice (the plain
 * form is OTC_IMPL_AUTO: the T-table + bitsliced split from 2 GiB, the
 * persistent T-table claim kernel from 512 MiB, like ECB encryption). */
int otc_aes_cfb128_decrypt(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                           const uint8_t iv[16], void *stream);
int otc_aes_cfb128_decrypt_impl(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                                const uint8_t iv[16], int impl, void *stream);

/* ---- batched CTR: many independent messages in ONE launch -----------------
 * The serving shape (packets, sectors, objects of a few KiB, each with its own
 * key and counter): one launch per message is launch-bound (µs each) and far
 * from the >> 256 workgroups the chip needs.  Here the work unit is a tile of
 * `tile_blocks` 16-byte blocks of one message (64, 128 or 256 = one wave x 1,
 * 2 or 4 blocks per lane: small messages waste less of a small tile, large
 * tiles hide more LDS latency); every array below is DEVICE memory:
 *   msgs[m]        message descriptor (device addresses, length, key index,
 *                  initial 128-bit big-endian counter as two numeric halves)
 *   keys[k]        expanded encryption keys (all with `nr` rounds)
 *   tile_msg[t]    message of tile t          } from otc_ctr_batch_plan()
 *   tile_first[m]  first tile of message m    }
 * in == out (in place) is allowed per message; distinct messages must not
 * overlap.  Messages of 0 bytes have no tiles. */
#define OTC_BATCH_TILE_BLOCKS 256 /* default and largest tile */
typedef struct {
    uint64_t in;      /* device address of the input */
    uint64_t out;     /* device address of the output */
    uint64_t nbytes;
    uint64_t ctr_hi;  /* initial counter, bytes 0..7 as a big-endian number */
    uint64_t ctr_lo;  /* bytes 8..15 */
    uint32_t key;     /* index into keys[] */
    uint32_t align;   /* 0: tiles start at the message's first block.
                         OTC_BATCH_ALIGNED | shift: counter-aligned tiles,
                         shift = ctr_lo mod tile_blocks, so every tile
                         starts at a counter multiple of tile_blocks (the first
                         tile is partial) and rounds 1-2 are mostly computed
                         once per tile (counter-mode caching: 133 instead of
                         160 LDS lookups per AES-128 block) -- for messages of
                         many tiles */
} otc_ctr_msg;
#define OTC_BATCH_ALIGNED 0x80000000u

/* Host planner: fills tile_msg (may be NULL to only count) and tile_first for
 * host copies of the descriptors (honouring each message's `align` word);
 * returns the number of tiles. */
uint64_t otc_ctr_batch_plan(const otc_ctr_msg *msgs, size_t nmsg, int tile_blocks, uint32_t *tile_msg,
                            uint64_t *tile_first);

int otc_aes_ctr_batch(const otc_ctr_msg *msgs, const otc_aes_key *keys, const uint32_t *tile_msg,
                      const uint64_t *tile_first, uint64_t ntiles, int tile_blocks, int nr, void *stream);

/* ---- batched AES-GCM ------------------------------------------------------
 * Many records under ONE key, each with its own 12-byte IV, its own AAD and
 * its own 16-byte tag: record m is SP 800-38D GCM under (key, iv[m], aad[m]).
 * The shape of TLS records, ESP / QUIC packets and sealed sectors, where
 * otc_aes_gcm's per-call cost (an allocation, 384 KiB of tables, one launch per
 * level) is all there is.  One key per batch is what makes this the fast path: the
 * positional hash tables are 64 KiB per constant and cannot be held per record.
 * Records under many keys go to otc_aes_gcm_mk_batch below, which hashes on
 * 256-byte tables per key.
 *
 * Limits (the planner checks them on host copies of the descriptors): data
 * 0 .. OTC_GCM_BATCH_MAX_BYTES per record, any byte count -- larger messages
 * belong to otc_aes_gcm; AAD 0 .. OTC_GCM_BATCH_MAX_AAD, device memory, any
 * alignment; data buffers 16-byte aligned; in == out allowed per record;
 * distinct records must not overlap, and no AAD may overlap any record's
 * output (an encryption writes the outputs before it hashes the AADs).  A record of 0 bytes is valid, with AAD
 * (GMAC) or without.  Only 12-byte IVs: other lengths need a hash to form J0.
 * The cap makes a record at most 65536 blocks, so from IV || 00000002 the low
 * 32 counter bits never wrap and the 128-bit add of the batched CTR kernel IS
 * GCM's CTR32 here.
 *
 * The IVs are DEVICE data supplied to every run (n x 12 bytes): a replayed
 * batch must bring new IVs, and IV uniqueness under a key is the caller's
 * duty.  A run is one linear chain of launches on `stream` -- no allocation,
 * no host synchronisation, no second stream -- so it can be captured in a graph:
 *   encrypt: prep -> E_K(J0[]) -> CTR batch -> batched GHASH over out -> tags
 *   decrypt: prep -> E_K(J0[]) -> batched GHASH over in -> tags, verdicts
 *            -> CTR batch -> wipe
 * prep writes IV || 00000002 into the otc_ctr_msg descriptors and J0 = IV ||
 * 00000001 into the workspace.  On decryption the first tag_bytes (4 .. 16)
 * bytes of every computed tag are compared on the device with expect_dev
 * (n x tag_bytes; OR of the XORs, no early exit), ok_dev[m] becomes 1 or 0,
 * and after the CTR pass the output of every record with ok_dev[m] == 0 is
 * zeroed (in place: the ciphertext with it), and so is its row of tags_dev:
 * the computed tag of a forged record is the valid tag of that forgery and is
 * not handed out.  expect_dev must not overlap tags_dev or ok_dev (rejected).  otc_last_impl: OTC_IMPL_TTABLE. */
#define OTC_GCM_BATCH_MAX_BYTES (1u << 20)
#define OTC_GCM_BATCH_MAX_AAD (1u << 16)
typedef struct {
    uint64_t in;        /* device addresses */
    uint64_t out;
    uint64_t nbytes;
    uint64_t aad;
    uint64_t aad_bytes;
    uint64_t reserved;
} otc_gcm_msg;

/* The per-key hash tables (H^16, H^64 and H, 64 KiB each) in tab_dev, 16-byte
 * aligned device memory of otc_gcm_batch_table_bytes(): once per key. */
size_t otc_gcm_batch_table_bytes(void);
int otc_gcm_batch_tables(const otc_gcm_key *k, void *tab_dev, void *stream);
/* Host planner over HOST copies of the descriptors: checks the caps, the
 * alignment, partial overlap of a record's in and out, overlap between
 * records and of an AAD with any output; fills the CTR half's descriptors (counters left zero: prep writes
 * them), tile map and tile_first -- any of the three may be NULL to only
 * count.  Returns the number of tiles (records of 0 bytes have none), or
 * OTC_ERR_ARG with a message. */
int64_t otc_gcm_batch_plan(const otc_gcm_msg *msgs, size_t nmsg, int tile_blocks, otc_ctr_msg *ctr_msgs,
                           uint32_t *tile_msg, uint64_t *tile_first);
/* the caller-owned workspace of a run: J0[] and E_K(J0)[], 16-byte aligned */
size_t otc_gcm_batch_ws_bytes(size_t nmsg);
/* How many lanes hash one record: the kernel has a 16-lane form (four records
 * per wave, a short fold: short records) and a 64-lane form (one wave per
 * record: long ones).  Both compute the same; the choice is speed only.  From
 * HOST copies of the descriptors: 64 when the records hash more than 768 blocks
 * (12 KiB) on average or one of them more than 4096 (64 KiB), else 16. */
int otc_gcm_batch_lanes(const otc_gcm_msg *msgs, size_t nmsg);
/* The hash by itself: s_dev[m] (nmsg x 16, 16-byte aligned) = GHASH_H of
 * record m's AAD, `in` data and length block.  lanes: 16 or 64 (0: 64). */
int otc_ghash_batch(const otc_gcm_msg *msgs_dev, size_t nmsg, const void *tab_dev, void *s_dev, int lanes,
                    void *stream);
/* tags_dev: nmsg x 16, 16-byte aligned, the COMPUTED tags in both directions
 * (decryption: zero for the records that fail);
 * expect_dev / ok_dev: decryption only.  key_dev: a device copy of k->enc, 8-byte
 * aligned (the keys[] array of the batched CTR kernel, which reads round keys
 * from memory; the call itself copies nothing).  lanes: as otc_ghash_batch.
 * nmsg == 0 launches nothing. */
int otc_aes_gcm_batch(const otc_gcm_msg *msgs_dev, otc_ctr_msg *ctr_msgs_dev, const uint32_t *tile_msg_dev,
                      const uint64_t *tile_first_dev, uint64_t ntiles, int tile_blocks, size_t nmsg,
                      const otc_gcm_key *k, const otc_aes_key *key_dev, const void *tab_dev, int dir,
                      const uint8_t *ivs_dev, void *tags_dev, const uint8_t *expect_dev, int tag_bytes, uint8_t *ok_dev,
                      void *ws_dev, int lanes, void *stream);
/* The batched hash kernel's own boundaries in HASHED BLOCKS (AAD, data and
 * length block together), smallest first: a pass of the 16-lane form (16), its
 * batch of passes which is also a pass of the 64-lane form (64), a batch of
 * those (256).  Writes up to max of them; returns the count. */
int otc_gcm_batch_spans(uint64_t *spans, int max);

/* ---- batched ChaCha20-Poly1305 ----------------------------------------------
 * Many records, each with its OWN key (an index into a key array), its own
 * 12-byte nonce, its own AAD and its own 16-byte tag: record m is RFC 8439
 * section 2.8 under (keys[msgs[m].key], nonces[m], aad[m]) -- ciphertext =
 * data XOR the ChaCha20 keystream from counter 1, one-time key = bytes 0..31 of
 * block 0, tag = Poly1305 over pad16(AAD) || pad16(ciphertext) ||
 * le64(aad_bytes) || le64(nbytes).  The shape of WireGuard and QUIC packets,
 * TLS 1.3 records and SSH packets, where otc_chacha20_poly1305's per-call cost
 * (a host-side block, the host-side powers of r, an allocation, three or four
 * launches) is all there is.  Poly1305 has no tables and its key is one-time
 * per record by construction, so a key per record costs nothing extra: the
 * one-time keys and the powers of r are made on the device
 * (csrc/hip/chacha_batch.hip).
 *
 * Limits (the planner checks them on host copies of the descriptors): data
 * 0 .. OTC_CHACHA_BATCH_MAX_BYTES per record, any byte count -- larger
 * messages belong to otc_chacha20_poly1305; AAD 0 .. OTC_CHACHA_BATCH_MAX_AAD,
 * device memory, any alignment; data buffers 16-byte aligned; in == out allowed
 * per record; distinct records must not overlap, no input may overlap another
 * record's output, and no AAD may overlap any record's output (an encryption
 * writes the outputs before it hashes the AADs).  A record of 0 bytes is
 * valid, with AAD or without.  Tags are 16 bytes.
 *
 * The nonces are DEVICE data supplied to every run (n x 12 bytes): a replayed
 * batch must bring new nonces, and nonce uniqueness under a key is the
 * caller's duty.  A run is one linear chain of launches on `stream` -- no
 * allocation, no host synchronisation, no second stream -- so it can be
 * captured in a graph:
 *   encrypt: prep -> batched ChaCha20 -> batched Poly1305 over out -> tags
 *   decrypt: prep -> batched Poly1305 over in -> tags, verdicts
 *            -> batched ChaCha20 -> wipe
 * prep writes every record's one-time key (r clamped, then s) into the
 * workspace.  On decryption every computed tag is compared on the device with
 * expect_dev (n x 16; OR of the XORs, no early exit), ok_dev[m] becomes 1 or
 * 0, and after the cipher pass the output of every record with ok_dev[m] == 0
 * is zeroed (in place: the ciphertext with it), and so is its row of tags_dev:
 * the computed tag of a forged record is the valid tag of that forgery and is
 * not handed out.  expect_dev must not overlap tags_dev or ok_dev (rejected).
 * One kernel family: otc_last_impl does not know these calls. */
#define OTC_CHACHA_BATCH_MAX_BYTES (1u << 20)
#define OTC_CHACHA_BATCH_MAX_AAD (1u << 16)
typedef struct {
    uint64_t in;        /* device addresses */
    uint64_t out;
    uint64_t nbytes;
    uint64_t aad;
    uint64_t aad_bytes; /* the five columns of otc_gcm_msg, on purpose: the wipe kernel serves both */
    uint64_t key;       /* index into keys_dev */
} otc_chacha_msg;

/* Host planner over HOST copies of the descriptors: checks the caps, null
 * pointers, the alignment, key < nkeys, partial overlap of a record's in and
 * out, overlap between records and of an AAD with any output; fills the tile
 * map (a tile is one 4 KiB pass of one record) -- either array may be NULL to
 * only count.  Returns the number of tiles (records of 0 bytes have none), or
 * OTC_ERR_ARG with a message that names the record.  Needs no device. */
int64_t otc_chacha_batch_plan(const otc_chacha_msg *msgs, size_t nmsg, size_t nkeys, uint32_t *tile_msg,
                              uint64_t *tile_first);
/* the caller-owned workspace of a run: the one-time keys, 32 bytes per record, 16-byte aligned */
size_t otc_chacha_batch_ws_bytes(size_t nmsg);
/* How many lanes hash one record: 16 (four records per wave) or 64 (one wave
 * per record).  Both compute the same; the choice is speed only.  From HOST
 * copies of the descriptors: 64 when the records hash more than 512 blocks
 * (8 KiB) on average, else 16 (measured at 256 B .. 64 KiB records; what the
 * rule rests on and what of it is supposed: aead.cpp). */
int otc_chacha_batch_lanes(const otc_chacha_msg *msgs, size_t nmsg);
/* The batched hash kernel's own boundaries in HASHED BLOCKS (AAD, data and
 * length block together), smallest first: a pass of the 16-lane form (16), its
 * batch of passes which is also a pass of the 64-lane form (64), a batch of
 * those (256).  Writes up to max of them; returns the count. */
int otc_chacha_batch_spans(uint64_t *spans, int max);
/* The hash by itself: tags_dev[m] (nmsg x 16, 16-byte aligned) = Poly1305 under
 * the one-time key otk_dev[m] (r || s, 32 bytes, r clamped here; the array
 * 4-byte aligned) of record m's pad16(AAD) || pad16(`in` data) || lengths.
 * lanes: 16 or 64 (0: 64). */
int otc_poly1305_batch(const otc_chacha_msg *msgs_dev, size_t nmsg, const uint8_t *otk_dev, void *tags_dev, int lanes,
                       void *stream);
/* keys_dev: nkeys x 32 bytes, 4-byte aligned.  nonces_dev: nmsg x 12 bytes, any
 * alignment.  tags_dev: nmsg x 16, 16-byte aligned, the COMPUTED tags in both
 * directions (decryption: zero for the records that fail); expect_dev (nmsg x
 * 16, any alignment) / ok_dev: decryption only.  ws_dev:
 * otc_chacha_batch_ws_bytes(nmsg), 16-byte aligned.  lanes: as
 * otc_poly1305_batch.  nmsg == 0 launches nothing; ntiles == 0 (all records
 * empty) skips the cipher.  Every bad argument is OTC_ERR_ARG before any HIP
 * call. */
int otc_chacha20_poly1305_batch(const otc_chacha_msg *msgs_dev, const uint32_t *tile_msg_dev,
                                const uint64_t *tile_first_dev, uint64_t ntiles, size_t nmsg, const uint8_t *keys_dev,
                                int dir, const uint8_t *nonces_dev, void *tags_dev, const uint8_t *expect_dev,
                                uint8_t *ok_dev, void *ws_dev, int lanes, void *stream);

/* ---- batched AES-OCB3 ---------------------------------------------------------
 * Many records under ONE key (otc_ocb_key: one key per batch, as for the
 * batched GCM), each with its own 12-byte nonce, its own AAD and its own
 * 16-byte tag: record m is RFC 7253 OCB3 with TAGLEN 128 under (key,
 * nonces[m], aad[m]) and equals otc_aes_ocb on that record alone, byte for
 * byte.  Other nonce and tag lengths stay with otc_aes_ocb.  OCB reads the data
 * ONCE (the two other batched AEADs read it in the cipher pass and again in
 * the hash pass); Offset_0 and HASH(K, A), which otc_aes_ocb computes on the
 * host, are made on the device (csrc/hip/aes_ocb_batch.hip).
 *
 * Limits (the planner checks them on host copies of the descriptors): data
 * 0 .. OTC_OCB_BATCH_MAX_BYTES per record, any byte count -- larger messages
 * belong to otc_aes_ocb; AAD 0 .. OTC_OCB_BATCH_MAX_AAD, device memory, any
 * alignment; data buffers 16-byte aligned; in == out allowed per record;
 * distinct records must not overlap, no input may overlap another record's
 * output, and no AAD may overlap any record's output.  A record of 0 bytes is
 * valid, with AAD or without.
 *
 * The nonces are DEVICE data supplied to every run (n x 12 bytes): a replayed
 * batch must bring new nonces, and nonce uniqueness under the key is the
 * caller's duty.  A run is one linear chain of launches on `stream` -- no
 * allocation, no host synchronisation, no second stream -- so it can be
 * captured in a graph:
 *   encrypt: prep -> bulk -> finish (tags)
 *   decrypt: prep -> bulk -> finish (tags, verdicts) -> wipe
 * prep writes every record's Offset_0 and HASH(K, A) into the workspace and
 * clears its checksum; the bulk kernel takes the whole blocks, tile by tile,
 * and collects the checksums; finish takes the trailing bytes and makes the
 * tags.  OCB's checksum is over the plaintext, so a decryption decrypts before
 * it can judge: every computed tag is compared on the device with expect_dev
 * (n x 16; OR of the XORs, no early exit), ok_dev[m] becomes 1 or 0, and the
 * output of every record with ok_dev[m] == 0 is zeroed (in place: the
 * ciphertext with it), and so is its row of tags_dev.  expect_dev must not
 * overlap tags_dev or ok_dev (rejected).  otc_last_impl: OTC_IMPL_TTABLE. */
#define OTC_OCB_BATCH_MAX_BYTES (1u << 20)
#define OTC_OCB_BATCH_MAX_AAD (1u << 16)
typedef struct {
    uint64_t in;        /* device addresses */
    uint64_t out;
    uint64_t nbytes;
    uint64_t aad;
    uint64_t aad_bytes; /* the five columns of otc_gcm_msg, on purpose: the wipe kernel serves all three */
    uint64_t reserved;
} otc_ocb_msg;

/* Host planner over HOST copies of the descriptors: checks the caps, null
 * pointers, the alignment, partial overlap of a record's in and out, overlap
 * between records and of an AAD with any output; fills the tile map (a tile is
 * 64 whole blocks, 1 KiB, of one record: ceil(nbytes / 16 / 64) tiles, none for
 * a record under 16 bytes) -- either array may be NULL to only count.  Returns
 * the number of tiles, or OTC_ERR_ARG with a message that names the record.
 * Needs no device. */
int64_t otc_ocb_batch_plan(const otc_ocb_msg *msgs, size_t nmsg, uint32_t *tile_msg, uint64_t *tile_first);
/* the caller-owned workspace of a run: Offset_0[], checksum[] and HASH[], 16
 * bytes per record each, 16-byte aligned */
size_t otc_ocb_batch_ws_bytes(size_t nmsg);
/* The bulk kernel's boundaries in BYTES, smallest first: a block, a slot (one
 * tile), a wave pass (four slots), a workgroup step, the full grid's first
 * step -- past it a workgroup takes a second step.  Writes up to max of them;
 * returns the count. */
int otc_ocb_batch_spans(uint64_t *spans, int max);
/* nonces_dev: nmsg x 12 bytes, any alignment.  tags_dev: nmsg x 16, 16-byte
 * aligned, the COMPUTED tags in both directions (decryption: zero for the
 * records that fail); expect_dev (nmsg x 16, any alignment) / ok_dev:
 * decryption only.  ws_dev: otc_ocb_batch_ws_bytes(nmsg), 16-byte aligned.
 * The key, its L table and its round keys travel by value.  nmsg == 0 launches
 * nothing; ntiles == 0 (no record has a whole block) skips the bulk kernel.
 * Every bad argument is OTC_ERR_ARG before any HIP call. */
int otc_aes_ocb_batch(const otc_ocb_msg *msgs_dev, const uint32_t *tile_msg_dev, const uint64_t *tile_first_dev,
                      uint64_t ntiles, size_t nmsg, const otc_ocb_key *k, int dir, const uint8_t *nonces_dev,
                      void *tags_dev, const uint8_t *expect_dev, uint8_t *ok_dev, void *ws_dev, void *stream);

/* ---- batched AES-CCM ------------------------------------------------------------
 * Many records under ONE key (an otc_aes_key ENCRYPTION schedule, in both
 * directions: CCM never runs the inverse cipher), each with its own nonce, its
 * own AAD and its own tag: record m is NIST SP 800-38C / RFC 3610 AES-CCM under
 * (key, nonces[m], aad[m]).  The nonce length (7 .. 13 bytes; L = 15 -
 * nonce_len) and the tag length (4, 6, .., 16 bytes) are the BATCH's.  CCM's
 * tag is a CBC-MAC, one serial chain per record, so the kernel runs one record
 * per lane, the chain and the counter mode as two blocks in flight, and reads
 * the data once (csrc/hip/aes_ccm_batch.hip).  There is no single-message
 * kernel: one message is one chain on one lane, a batch of one.
 *
 * Limits (the planner checks them on host copies of the descriptors): data
 * 0 .. OTC_CCM_BATCH_MAX_BYTES per record and below 2^(8 L), any byte count;
 * AAD 0 .. OTC_CCM_BATCH_MAX_AAD, device memory, any alignment (both encodings
 * of its length occur: 2 bytes below 0xFF00, 6 from there); data buffers
 * 16-byte aligned; in == out allowed per record; distinct records must not
 * overlap, no input may overlap another record's output, and no AAD may overlap
 * any record's output.  A record of 0 bytes is valid, with AAD or without.
 *
 * The nonces are DEVICE data supplied to every run (n x nonce_len bytes): a
 * replayed batch must bring new nonces, and nonce uniqueness under the key is
 * the caller's duty.  A run is one linear chain of launches on `stream` -- no
 * allocation, no host synchronisation, no second stream -- so it can be
 * captured in a graph:
 *   encrypt: records (out, tags)
 *   decrypt: records (out, tags, verdicts) -> wipe
 * The MAC is over the plaintext, so a decryption decrypts before it can judge:
 * every computed tag is compared on the device with expect_dev (n x tag_len; OR
 * of the XORs, no early exit), ok_dev[m] becomes 1 or 0, and the output of every
 * record with ok_dev[m] == 0 is zeroed (in place: the ciphertext with it), and
 * so is its row of tags_dev.  expect_dev must not overlap tags_dev or ok_dev
 * (rejected).  otc_last_impl: OTC_IMPL_TTABLE. */
#define OTC_CCM_BATCH_MAX_BYTES (1u << 20)
#define OTC_CCM_BATCH_MAX_AAD (1u << 16)
typedef struct {
    uint64_t in;        /* device addresses */
    uint64_t out;
    uint64_t nbytes;
    uint64_t aad;
    uint64_t aad_bytes; /* the five columns of otc_gcm_msg, on purpose: the wipe kernel serves this one too */
    uint64_t reserved;
} otc_ccm_msg;

/* Host planner over HOST copies of the descriptors: checks nonce_len, the caps
 * (nbytes <= OTC_CCM_BATCH_MAX_BYTES and nbytes < 2^(8 (15 - nonce_len)): with a
 * 13-byte nonce 65535 bytes pass and 65536 do not), null pointers, the
 * alignment, partial overlap of a record's in and out, overlap between records
 * and of an AAD with any output; fills order[nmsg] (may be NULL to only check):
 * the records sorted by their data's block count, longest first, records of one
 * count in their own order -- lane t of the kernel takes record order[t], so the
 * lanes of a wave end together.  Any permutation of 0 .. nmsg - 1 is a valid
 * order.  Returns OTC_OK, or OTC_ERR_ARG with a message that names the record.
 * Needs no device. */
int otc_ccm_batch_plan(const otc_ccm_msg *msgs, size_t nmsg, int nonce_len, uint32_t *order);
/* the caller-owned workspace of a run: none today (the AAD is chained in the
 * records' kernel), so 0, and ws_dev may then be NULL */
size_t otc_ccm_batch_ws_bytes(size_t nmsg);
/* The kernel's boundaries, smallest first: a block and a lane's burst (8
 * blocks) in BYTES; a wave, a workgroup and the full grid's first step -- past
 * it a wave takes a second record per lane -- in RECORDS.  Writes up to max of
 * them; returns the count. */
int otc_ccm_batch_spans(uint64_t *spans, int max);
/* order_dev: nmsg x uint32, a permutation (otc_ccm_batch_plan).  nonces_dev:
 * nmsg x nonce_len bytes, any alignment.  tags_dev: nmsg x tag_len bytes, any
 * alignment, the COMPUTED tags in both directions (decryption: zero for the
 * records that fail); expect_dev (nmsg x tag_len) / ok_dev: decryption only.
 * The round keys travel by value.  nmsg == 0 launches nothing.  Every bad
 * argument is OTC_ERR_ARG before any HIP call. */
int otc_aes_ccm_batch(const otc_ccm_msg *msgs_dev, const uint32_t *order_dev, size_t nmsg, const otc_aes_key *key,
                      int dir, const uint8_t *nonces_dev, int nonce_len, void *tags_dev, int tag_len,
                      const uint8_t *expect_dev, uint8_t *ok_dev, void *ws_dev, void *stream);

/* ---- batched AES-GCM-SIV ------------------------------------------------------
 * Many records under ONE key-generating key (otc_gcm_siv_key, 128 or 256 bits),
 * each with its own 12-byte nonce, its own AAD and its own 16-byte tag: record m
 * is RFC 8452 AES-GCM-SIV under (key, nonces[m], aad[m]) and equals
 * otc_aes_gcm_siv on that record alone, byte for byte.  The shape the mode was
 * made for -- many short records from senders that cannot coordinate nonces --
 * and the one where otc_aes_gcm_siv's per-call cost (the derivation, a key
 * expansion and the AAD's hash on the host, an allocation, 384 KiB of tables,
 * four or more launches) is all there is.  In this mode the nonce decides both
 * of a record's keys, so nothing per key is shared between records: the POLYVAL
 * key H_m, the encryption key K_m and its schedule are made on the device, per
 * record, and the hash multiplies on 256-byte tables that it builds per record
 * in LDS (csrc/hip/aes_gcm_siv_batch.hip).
 *
 * Limits (the planner checks them on host copies of the descriptors): data
 * 0 .. OTC_GCM_SIV_BATCH_MAX_BYTES per record, any byte count -- larger messages
 * belong to otc_aes_gcm_siv; AAD 0 .. OTC_GCM_SIV_BATCH_MAX_AAD, device memory,
 * any alignment; data buffers 16-byte aligned; in == out allowed per record;
 * distinct records must not overlap, no input may overlap another record's
 * output, and no AAD may overlap any record's output.  A record of 0 bytes is
 * valid, with AAD or without.  The descriptor is otc_gcm_msg.
 *
 * The nonces are DEVICE data supplied to every run (n x 12 bytes).  A run is one
 * linear chain of launches on `stream` -- no allocation, no host
 * synchronisation, no second stream -- so it can be captured in a graph:
 *   encrypt: derive -> batched POLYVAL over in -> finisher (tags)
 *            -> batched CTR-LE32 from the tags
 *   decrypt: derive -> batched CTR-LE32 from the RECEIVED tags
 *            -> batched POLYVAL over out -> finisher (tags, verdicts) -> wipe
 * The tag is the counter mode's initial counter block and never leaves the
 * device.  GCM-SIV hashes the plaintext, so a decryption decrypts before it can
 * judge: every computed tag is compared on the device with expect_dev (n x 16;
 * all 16 bytes, OR of the XORs, no early exit), ok_dev[m] becomes 1 or 0, and the
 * output of every record with ok_dev[m] == 0 is zeroed (in place: the ciphertext
 * with it), and so is its row of tags_dev.  expect_dev must not overlap tags_dev
 * or ok_dev (rejected).  otc_last_impl: OTC_IMPL_TTABLE. */
#define OTC_GCM_SIV_BATCH_MAX_BYTES (1u << 20)
#define OTC_GCM_SIV_BATCH_MAX_AAD (1u << 16)
#define OTC_GCM_SIV_BATCH_TILE_BLOCKS 256 /* the counter kernel's tile: 4 KiB of one record */

/* Host planner over HOST copies of the descriptors: checks the caps, null
 * pointers, the alignment, partial overlap of a record's in and out, overlap
 * between records and of an AAD with any output; fills the counter kernel's
 * tile map (ceil(nbytes / 4096) tiles per record) -- either array may be NULL to
 * only count.  Returns the number of tiles (records of 0 bytes have none), or
 * OTC_ERR_ARG with a message that names the record.  Needs no device. */
int64_t otc_gcm_siv_batch_plan(const otc_gcm_msg *msgs, size_t nmsg, uint32_t *tile_msg, uint64_t *tile_first);
/* the caller-owned workspace of a run, 16-byte aligned: H_m[] and S_m[] (16
 * bytes per record each), then every record's expanded encryption key (an
 * otc_aes_key, 256 bytes).  It holds KEY MATERIAL after a run: the derived keys
 * of every record -- the caller clears it when the batch is done with. */
size_t otc_gcm_siv_batch_ws_bytes(size_t nmsg);
/* How many lanes hash one record: 16 (four records per wave) or 64 (one wave per
 * record).  Both compute the same; the choice is speed only.  From HOST copies
 * of the descriptors (what the rule rests on: aead.cpp). */
int otc_gcm_siv_batch_lanes(const otc_gcm_msg *msgs, size_t nmsg);
/* The batched hash kernel's own boundaries in HASHED BLOCKS (AAD, data and
 * length block together), smallest first: a pass of the 16-lane form (16), its
 * batch of passes which is also a pass of the 64-lane form (64), a batch of
 * those (256).  Writes up to max of them; returns the count. */
int otc_gcm_siv_batch_spans(uint64_t *spans, int max);
/* The hash by itself: s_dev[m] (nmsg x 16, 16-byte aligned) = POLYVAL under the
 * key h_dev[m] (nmsg x 16, 16-byte aligned) of record m's pad16(AAD) ||
 * pad16(`in` data) || le64(8 aad_bytes) le64(8 nbytes).  lanes: 16 or 64 (0: 64). */
int otc_polyval_batch(const otc_gcm_msg *msgs_dev, size_t nmsg, const void *h_dev, void *s_dev, int lanes, void *stream);
/* The counter mode by itself: record m's out = in ^ keystream under the
 * encryption schedule keys_dev[m] (every one with nr rounds; 16-byte aligned)
 * from the counter block ctrs_dev[m] (nmsg x 16 bytes, 4-byte aligned, outside
 * every output), as otc_aes_ctr_le32 counts: bytes 0..3 little-endian modulo
 * 2^32 without carry, bit 7 of byte 15 forced on.  Tile map from
 * otc_gcm_siv_batch_plan. */
int otc_aes_ctr_le32_batch(const otc_gcm_msg *msgs_dev, const otc_aes_key *keys_dev, const void *ctrs_dev,
                           const uint32_t *tile_msg_dev, const uint64_t *tile_first_dev, uint64_t ntiles, size_t nmsg,
                           int nr, void *stream);
/* nonces_dev: nmsg x 12 bytes, any alignment.  tags_dev: nmsg x 16, 16-byte
 * aligned, the COMPUTED tags in both directions (decryption: zero for the
 * records that fail); expect_dev (nmsg x 16, 4-byte aligned: the counter kernel
 * reads it) / ok_dev: decryption only.  ws_dev:
 * otc_gcm_siv_batch_ws_bytes(nmsg), 16-byte aligned.  lanes: as
 * otc_polyval_batch.  nmsg == 0 launches nothing; ntiles == 0 (all records
 * empty) skips the counter kernel and still makes the tags.  Every bad argument
 * is OTC_ERR_ARG before any HIP call. */
int otc_aes_gcm_siv_batch(const otc_gcm_msg *msgs_dev, const uint32_t *tile_msg_dev, const uint64_t *tile_first_dev,
                          uint64_t ntiles, size_t nmsg, const otc_gcm_siv_key *k, int dir, const uint8_t *nonces_dev,
                          void *tags_dev, const uint8_t *expect_dev, uint8_t *ok_dev, void *ws_dev, int lanes,
                          void *stream);

/* ---- batched AES-GCM, a key per record ---------------------------------------
 * Many records, each under its OWN key (an index into an array of expanded
 * encryption keys), with its own 12-byte IV, its own AAD and its own tag: record
 * m is SP 800-38D GCM under (keys[msgs[m].key], iv[m], aad[m]) and equals
 * otc_aes_gcm on that record alone, byte for byte.  The shape of a server's TLS
 * records, ESP / QUIC packets and sealed sectors, which come from many
 * connections with a key each.  otc_aes_gcm_batch stays the faster call where
 * one key covers the batch.  GHASH runs here as POLYVAL (RFC 8452 appendix A) on
 * nibble tables of 256 bytes, seven per key (1792 bytes), built on the device
 * once per key and copied by every record (csrc/hip/aes_gcm_mk_batch.hip).
 *
 * ONE key size per batch (`nr`: 10, 12 or 14 rounds for every key): the CTR
 * launch has one round count.  That is a decision; a caller with two key sizes
 * makes two batches.
 *
 * Limits, IVs, AADs, overlap rules, tag_bytes, the verdicts on the device, the
 * wipe of failed records and of their tag rows, and what a run may do (one
 * linear chain of launches on `stream`, no allocation, no host synchronisation,
 * capturable in a graph) are exactly otc_aes_gcm_batch's:
 *   encrypt: prep -> CTR batch -> batched GHASH over out -> finisher (tags)
 *   decrypt: prep -> batched GHASH over in -> finisher (tags, verdicts)
 *            -> CTR batch -> wipe
 * The finisher forms tag = GHASH ^ E_{K_m}(J0_m) with the schedule read from
 * keys_dev.  otc_last_impl: OTC_IMPL_TTABLE.
 *
 * keys_dev (nkeys otc_aes_key, 256 bytes each) and the table image hold
 * KEY MATERIAL: the schedules and what derives from the hash keys E_K(0^128).
 * Clearing them when the batch is done with is the caller's job. */
typedef struct {
    uint64_t in;        /* device addresses */
    uint64_t out;
    uint64_t nbytes;
    uint64_t aad;
    uint64_t aad_bytes; /* otc_chacha_msg's columns, on purpose: the wipe kernel serves this one too */
    uint64_t key;       /* index into keys_dev and into the table image */
} otc_gcm_mk_msg;

/* Host planner over HOST copies of the descriptors: otc_gcm_batch_plan's checks
 * and key < nkeys; fills the CTR half's descriptors (key index set, counters left
 * zero: prep writes them), tile map and tile_first -- any of the three may be
 * NULL to only count.  Returns the number of tiles (records of 0 bytes have
 * none), or OTC_ERR_ARG with a message "gcm_mk_batch: record M: ...".  Needs no
 * device. */
int64_t otc_gcm_mk_batch_plan(const otc_gcm_mk_msg *msgs, size_t nmsg, size_t nkeys, int tile_blocks,
                              otc_ctr_msg *ctr_msgs, uint32_t *tile_msg, uint64_t *tile_first);
/* bytes of the table image of nkeys keys (1792 each), 16-byte aligned device memory */
size_t otc_gcm_mk_batch_table_bytes(size_t nkeys);
/* Builds the table image of the nkeys schedules at keys_dev (device memory,
 * 8-byte aligned, every one an ENCRYPTION schedule with nr rounds) into tab_dev:
 * one launch on `stream`; once per plan, and again when the keys change. */
int otc_gcm_mk_batch_tables(const otc_aes_key *keys_dev, size_t nkeys, int nr, void *tab_dev, void *stream);
/* the caller-owned workspace of a run: J0[] and the hashes, 32 bytes per record, 16-byte aligned */
size_t otc_gcm_mk_batch_ws_bytes(size_t nmsg);
/* How many lanes hash one record: 16 (four records per wave) or 64 (one wave per
 * record).  Both compute the same; the choice is speed only.  From HOST copies
 * of the descriptors (what the rule rests on: aead.cpp). */
int otc_gcm_mk_batch_lanes(const otc_gcm_mk_msg *msgs, size_t nmsg);
/* The batched hash kernel's own boundaries in HASHED BLOCKS (AAD, data and
 * length block together), smallest first: 16, 64, 256, as otc_gcm_batch_spans. */
int otc_gcm_mk_batch_spans(uint64_t *spans, int max);
/* The hash by itself: s_dev[m] (nmsg x 16, 16-byte aligned) = GHASH, under the
 * hash key of key msgs[m].key, of record m's AAD, `in` data and length block.
 * tab_dev: the image from otc_gcm_mk_batch_tables.  lanes: 16 or 64 (0: 64). */
int otc_ghash_mk_batch(const otc_gcm_mk_msg *msgs_dev, size_t nmsg, const void *tab_dev, void *s_dev, int lanes,
                       void *stream);
/* The arguments of otc_aes_gcm_batch, with keys_dev / nkeys / nr in place of k /
 * key_dev: the schedule array serves the CTR kernel and the finisher, tab_dev is
 * its table image.  nmsg == 0 launches nothing.  Every bad argument is
 * OTC_ERR_ARG before any HIP call. */
int otc_aes_gcm_mk_batch(const otc_gcm_mk_msg *msgs_dev, otc_ctr_msg *ctr_msgs_dev, const uint32_t *tile_msg_dev,
                         const uint64_t *tile_first_dev, uint64_t ntiles, int tile_blocks, size_t nmsg,
                         const otc_aes_key *keys_dev, size_t nkeys, int nr, const void *tab_dev, int dir,
                         const uint8_t *ivs_dev, void *tags_dev, const uint8_t *expect_dev, int tag_bytes,
                         uint8_t *ok_dev, void *ws_dev, int lanes, void *stream);

/* out = a ^ b (the device arc4_crypt combiner). */
int otc_xor(const void *a, const void *b, void *out, size_t nbytes, void *stream);

/* Many independent RC4 streams, one per lane: stream s uses key
 * keys[s*keylen .. +keylen) (device memory) and produces `len` bytes.
 * If `in` is non-NULL: out[s*len + n] = in[s*len + n] ^ ks_s[n], else the raw
 * keystream is written.  `drop` keystream bytes are discarded first
 * (RC4-drop[n]). */
int otc_rc4_multi(const uint8_t *keys, int keylen, size_t nstreams, size_t len, size_t drop,
                  const void *in, void *out, void *stream);

/* rc4.h on the device (rc4_crypt for many states at once): states is a
 * DEVICE array of nstreams `struct rc4_state` (rc4.h, e.g. set up with
 * rc4_init on the host and copied over); stream s continues from states[s],
 * processes len bytes at in + s*len -> out + s*len (in == out allowed), and
 * its state is written back, so calls resume exactly like rc4_crypt. */
int otc_rc4_crypt_batch(void *states, size_t nstreams, size_t len, const void *in, void *out, void *stream);

/* Deterministic pseudo-random fill (synthetic plaintext). */
int otc_fill_random(void *p, size_t nbytes, uint64_t seed, void *stream);

/* 64-bit XOR-fold checksum of a device buffer (nbytes % 8 == 0) into
 * *out_dev (device pointer to one uint64). */
int otc_checksum(const void *p, size_t nbytes, uint64_t *out_dev, void *stream);

/* Clock probe: a one-wave kernel on `stream` that sleeps `delay_s`, then
 * measures the shader clock over `window_s` seconds of real time; run it on a
 * side stream beside a workload.  out_dev[0] = shader cycles, out_dev[1] =
 * 100 MHz ticks, so GHz = 0.1 * out[0] / out[1]. */
int otc_clock_probe(uint64_t *out_dev, double delay_s, double window_s, void *stream);

/* ---- device memory / sync helpers (so C harnesses need no HIP headers) --- */
void *otc_dev_malloc(size_t nbytes);
void otc_dev_free(void *p);
#define OTC_H2D 0
#define OTC_D2H 1
#define OTC_D2D 2
int otc_memcpy(void *dst, const void *src, size_t nbytes, int kind);
int otc_memset(void *p, int v, size_t nbytes);
/* Elapsed device time of `op` run `iters` times on the default stream,
 * bracketed by hipEvents (kernel-only timing). */
typedef int (*otc_op_fn)(void *arg);
int otc_time_op(otc_op_fn op, void *arg, int iters, double *ms_per_iter);
/* Clock (GHz) the chip holds while running `op` back to back (>= 0.3 s). */
int otc_measure_clock(otc_op_fn op, void *arg, double *ghz);

/* ---- device info ------------------------------------------------------- */
int otc_device_count(void);
int otc_device_cus(int dev);           /* compute units */
int otc_device_clock_khz(int dev);     /* peak shader clock */
int otc_set_device(int dev);
int otc_device_sync(void);
/* A HIP stream for C callers (ordered with the default stream, so events on
 * the default stream bracket work queued on it); NULL on failure. */
void *otc_stream_create(void);
void otc_stream_destroy(void *stream);
/* a and b each wait for the work the other has queued so far (a join point
 * for work split by hand over two streams) */
int otc_stream_join(void *a, void *b);

/* ---- L3 engine: host-memory streaming pipeline -----------------------------
 * Encrypt/decrypt a HOST buffer through one GPU with a pinned staging ring:
 * H2D(k+1) | kernel(k) | D2H(k-1) on three HIP streams.  `host_in` /
 * `host_out` may be pageable (staged through the pinned ring) or already
 * pinned/registered (copied directly).  chunk_bytes: 0 = default (256 MiB).
 */
typedef struct otc_engine otc_engine;

otc_engine *otc_engine_create(int device, size_t chunk_bytes, int depth);
/* flags: OTC_ENGINE_DEFAULT -- the three streams get hardware queues of their
 * own (all-CU-masked streams), so the pipeline overlaps in a process whose
 * other streams (torch, RCCL) fill the 4 pooled queues HIP gives a process;
 * OTC_ENGINE_POOLED_QUEUES -- plain non-blocking streams on the pooled queues
 * (the A/B arm; docs/PERF.md "Round 6"). */
#define OTC_ENGINE_DEFAULT 0
#define OTC_ENGINE_POOLED_QUEUES 1
otc_engine *otc_engine_create_ex(int device, size_t chunk_bytes, int depth, int flags);
void otc_engine_destroy(otc_engine *e);

#define OTC_MODE_ECB 0
#define OTC_MODE_CTR 1
#define OTC_MODE_CBC_DEC 2
#define OTC_MODE_XOR 3

typedef struct {
    double total_ms;      /* wall time of the whole call */
    double kernel_ms;     /* sum of kernel times (hipEvent, kernel stream) */
    double h2d_ms, d2h_ms; /* sum of copy times (hipEvent, copy streams) */
    double host_stage_ms; /* host memcpy into / out of the pinned ring (pageable callers) */
    size_t bytes;
    int chunks;
    int numa_node;        /* node of the pinned ring (-1: unknown / OTC_NUMA=0) */
} otc_stream_stats;

int otc_engine_run(otc_engine *e, int mode, const void *host_in, void *host_out, size_t nbytes,
                   const otc_aes_key *k, const uint8_t iv_or_ctr[16], uint64_t block_offset,
                   int impl, otc_stream_stats *stats);

/* NUMA placement (csrc/cpu/numa.c): the GPU's node from sysfs (-1 unknown);
 * the engine allocates its pinned ring there.  otc_engine_staging returns the
 * ring's input slot (NULL until a pageable run allocated it) so tests can
 * check where its pages live (otc_numa_node_of_addr in otc_numa.h). */
int otc_device_numa_node(int dev);
int otc_engine_numa_node(const otc_engine *e);
const void *otc_engine_staging(const otc_engine *e, int slot);

/* Where a pointer lives: pageable host memory, pinned host memory, or device
 * memory (decides between the kernels and the host pipeline). */
#define OTC_PTR_HOST 0
#define OTC_PTR_PINNED 1
#define OTC_PTR_DEVICE 2
int otc_ptr_kind(const void *p);

/* Pin / unpin an existing host range (hipHostRegister) so the engine copies
 * it without staging. */
int otc_host_register(void *p, size_t nbytes);
int otc_host_unregister(void *p);
void *otc_host_alloc_pinned(size_t nbytes);
void otc_host_free_pinned(void *p);

/* ---- L4 multi-GPU (single process, RCCL over xGMI) -----------------------
 * Shard one host-resident CTR/ECB/CBC-dec stream over `ngpus` devices
 * (strategy 0 with OTC_SHARE_GPUS=1: `ngpus` logical shards mapped onto the
 * visible devices round-robin, to rehearse N shards on fewer GPUs).
 * strategy 0 = direct ingest (each GPU streams its own shard from pinned host
 * memory, engine pipeline per GPU, one host thread per GPU);
 * strategy 1 = RCCL root scatter/gather (root H2D, ncclScatter over xGMI,
 * per-GPU kernel, ncclGather, root D2H), chunked.
 * CBC decryption shards receive a 16-byte halo (the previous shard's last
 * ciphertext block).  Results are byte-identical to the 1-GPU path.
 */
typedef struct {
    double total_ms;
    double gbps;
    int ngpus;
    int strategy;
    int numa_nodes_used; /* strategy 0: distinct NUMA nodes the shard threads ran on */
} otc_multi_stats;

int otc_multi_run(int ngpus, int strategy, int mode, const void *host_in, void *host_out,
                  size_t nbytes, const otc_aes_key *k, const uint8_t iv_or_ctr[16], int impl,
                  size_t chunk_bytes, otc_multi_stats *stats);

/* The round plan of strategy 1, a pure function (csrc/cpu/rccl_plan.c, also
 * in the CPU-only library, so the N > 1 plan is tested without GPUs): the
 * stream goes in rounds of ngpus pieces of `piece` bytes each (the equal
 * counts ncclScatter / ncclGather need); the last round is zero-padded.
 * Piece (r, g) covers stream bytes [off, off + bytes) -- bytes 0 for a piece
 * wholly past the end --, starts at CTR block blk0 = off / 16, and for CBC
 * decryption takes its predecessor block from halo slot `halo` (the 16
 * stream bytes before halo_start(halo)), or the IV when halo < 0. */
typedef struct {
    uint64_t round_off;   /* stream offset of round r */
    uint64_t round_bytes; /* stream bytes in round r (< ngpus * piece: the last round) */
    uint64_t pad_bytes;   /* zero padding of round r's root buffer */
    uint64_t off, bytes;  /* piece (r, g) */
    uint64_t blk0;        /* its first block (CTR counter offset) */
    int64_t halo;         /* CBC decryption: halo slot, -1 = the IV */
} otc_rccl_piece;
uint64_t otc_rccl_nrounds(uint64_t nbytes, int ngpus, uint64_t piece);
/* 0, or OTC_ERR_ARG for ngpus < 1, piece == 0 or a (r, g) out of the plan */
int otc_rccl_plan_piece(uint64_t nbytes, int ngpus, uint64_t piece, uint64_t r, int g, otc_rccl_piece *out);
/* stream offset whose preceding 16 bytes fill halo slot i (clamped to nbytes) */
uint64_t otc_rccl_halo_start(uint64_t nbytes, uint64_t piece, uint64_t i);

/* Free the RCCL communicators / buffers that strategy 1 caches between calls
 * and the per-shard engines of strategy 0 (rebuilt on demand). */
void otc_multi_release(void);
/* Everything the library caches between calls (today: otc_multi_release). */
void otc_release_resources(void);

/* Test hook: make the (after+1)-th runtime allocation from now fail once
 * (device buffers, NUMA-pinned host windows, per-call kernel tables), so the
 * error paths can be exercised on a healthy GPU; after < 0 disarms. */
void otc_fault_inject_alloc(long after);
/* The hook's countdown: >= 0 while armed (that many allocations still pass
 * before the one that fails), -1 once the failure has fired or when disarmed.
 * A test reads it after the call under test to know its fault landed. */
long otc_fault_inject_pending(void);

/* Device-resident multi-GPU CTR: buffers dev_bufs[g] (already on GPU g) hold
 * shard g of `shard_bytes`; all GPUs encrypt in place concurrently with the
 * right counter offsets.  Returns elapsed ms (wall, all GPUs). */
int otc_multi_ctr_resident(int ngpus, void *const *dev_bufs, size_t shard_bytes,
                           const otc_aes_key *k, const uint8_t ctr0[16], int impl,
                           double *elapsed_ms);

/* Library self description / tests */
int otc_bitslice_selftest(int verbose);
/* host runs of the depth-first output transpose and of the bitsliced CTR
 * output phase built on it (csrc/cpu/bs_selftest.cpp) */
int otc_bs_dfs_transpose(uint32_t *m, const int *steps, int nsteps);
int otc_bs_ctr_out_model(const uint32_t *planes, const uint32_t *rk, const uint32_t *pt, uint32_t *out, int dfs,
                         int ls, int first, int cap, int *order);
const char *otc_build_info(void);
/* JSON object naming the HIP runtime / driver and RCCL versions this process
 * runs on and the mapped libamdhip64 / librccl paths (/proc/self/maps): in a
 * torch process they are torch's bundled copies, elsewhere /opt/rocm's. */
int otc_runtime_info(char *buf, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* OTC_H */
