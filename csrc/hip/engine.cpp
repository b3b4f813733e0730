/*
 * engine.cpp -- the cipher ops of the MI355X engine's C API (otc.h): the
 * thread's error slot, key init and the checks every op shares; every AES mode
 * (ECB, CTR and its resumable stream, RFC 3686, CTR32, batched CTR, CBC,
 * CFB128, the segment modes, XTS); otc_xor, the RC4 ops, otc_fill_random,
 * otc_checksum, otc_clock_probe; the AES-NI-shaped API (otc_aesni.h).  Kernels
 * are launched asynchronously on the caller's stream with the expanded key as
 * a by-value kernel argument: no per-call copies.  Elsewhere: aead.cpp (hashes
 * and AEADs), runtime.cpp (workspaces, devices, streams, memory, timing),
 * split.cpp (kernel choice, claimed runs), pipeline.cpp (streaming, multi-GPU).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>

#include "aes.h"
#include "otc.h"
#include "otc_aesni.h"
#include "otc_device.h"
#include "engine_internal.h"

using otc_dev::Ctr128;
using otc_dev::SplitClaim;
using otc_impl::Job;

namespace otc_rt {

namespace {
thread_local std::string g_err;
/* the kernel family the calling thread's last AES call ran (otc_last_impl) */
thread_local int g_last_impl = OTC_IMPL_AUTO;
}

int set_err(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

std::string last_err() { return g_err; }

int hip_fail(hipError_t e, const char *what)
{
    return set_err(OTC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

Ctr128 ctr_add(Ctr128 c, uint64_t n, bool wrap64)
{
    uint64_t lo = c.lo + n;
    if (!wrap64 && lo < c.lo) c.hi += 1;
    c.lo = lo;
    return c;
}

int check_key(const otc_aes_key *k, int dir)
{
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (k->nr != 10 && k->nr != 12 && k->nr != 14) return set_err(OTC_ERR_ARG, "bad key (nr)");
    if (k->dir != dir)
        return set_err(OTC_ERR_ARG, dir == OTC_DIR_ENCRYPT ? "key schedule is not an encryption schedule"
                                                           : "key schedule is not a decryption schedule");
    return OTC_OK;
}

void set_last_impl(int impl) { g_last_impl = impl; }

/* Device buffers of the cipher ops: non-null, 16-byte aligned (every kernel
 * moves 16 B per lane with global_load/store_dwordx4), and either the same
 * buffer (in place, where the mode allows it) or disjoint -- a partial overlap
 * would race between workgroups. */
int check_bufs(const void *in, const void *out, size_t nbytes, bool inplace_ok, const char *what)
{
    if (nbytes == 0) return OTC_OK;
    if (!in || !out) return set_err(OTC_ERR_ARG, std::string(what) + ": null buffer");
    if (((uintptr_t)in | (uintptr_t)out) & 15u)
        return set_err(OTC_ERR_ARG, std::string(what) + ": device buffers must be 16-byte aligned");
    if (in == out) {
        if (!inplace_ok) return set_err(OTC_ERR_ARG, std::string(what) + ": in-place operation is not supported");
        return OTC_OK;
    }
    if (partial_overlap(in, out, nbytes))
        return set_err(OTC_ERR_ARG, std::string(what) + ": input and output overlap partially");
    return OTC_OK;
}

} // namespace otc_rt

using namespace otc_rt;

namespace {

/* Segment encryption: T-table kernels only, for every impl -- the grid
 * kernel, or from segenc_persistent's size the persistent claim kernel
 * (64-segment units). */
hipError_t seg_enc_run(bool cfb, const void *in, void *out, size_t seg_bytes, size_t nseg, const otc_aes_key &K,
                       Ctr128 iv0, hipStream_t st)
{
    const size_t seg_blocks = seg_bytes / 16;
    g_last_impl = OTC_IMPL_TTABLE;
    auto launch = [&](const SplitClaim *cl) {
        return otc_impl::tt_seg_encrypt(cfb, in, out, seg_blocks, nseg, K, iv0, st, cl);
    };
    if (!segenc_persistent(seg_bytes * nseg, nseg)) return launch(nullptr);
    return claim_alone(nseg / otc_dev::SEG_UNIT, 16, st, launch);
}

/* what the segment calls check alike, after their key and segment length */
int check_seg_args(const void *in, const void *out, size_t seg_bytes, size_t nseg, const uint8_t iv0[16],
                   bool inplace_ok, int impl, const char *what)
{
    if (!iv0) return set_err(OTC_ERR_ARG, "null iv");
    if (nseg && seg_bytes > SIZE_MAX / nseg) return set_err(OTC_ERR_ARG, "size overflow");
    if (int r = check_bufs(in, out, seg_bytes * nseg, inplace_ok, what)) return r;
    return check_impl(impl);
}

} // namespace

/* ---- errors / keys ------------------------------------------------------ */
extern "C" const char *otc_last_error(void)
{
    thread_local std::string copy;
    copy = last_err();
    return copy.c_str();
}

extern "C" int otc_aes_key_init(otc_aes_key *k, const uint8_t *key, int bits, int dir)
{
    if (!k || !key) return set_err(OTC_ERR_ARG, "null argument");
    aes_context ctx;
    int r = (dir == OTC_DIR_ENCRYPT) ? aes_setkey_enc(&ctx, key, (unsigned)bits)
                                     : aes_setkey_dec(&ctx, key, (unsigned)bits);
    if (r) return set_err(OTC_ERR_ARG, "invalid AES key size (must be 128/192/256)");
    memset(k, 0, sizeof *k);
    aes_export_rk32(&ctx, k->rk);
    k->nr = ctx.nr;
    k->dir = dir;
    k->bits = bits;
    return OTC_OK;
}

extern "C" int otc_last_impl(void) { return g_last_impl; }

/* ---- device ops --------------------------------------------------------- */
extern "C" int otc_aes_ecb(const void *in, void *out, size_t nbytes, const otc_aes_key *k, int impl,
                           void *stream)
{
    Range rg("otc_aes_ecb");
    if (nbytes % 16) return set_err(OTC_ERR_ARG, "ECB length must be a multiple of 16");
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_bufs(in, out, nbytes, true, "aes_ecb")) return r;
    if (int r = check_impl(impl)) return r;
    if (nbytes == 0) return OTC_OK;
    const Job job{k->dir == OTC_DIR_ENCRYPT ? otc_impl::JOB_ECB_ENC : otc_impl::JOB_ECB_DEC,
                  in, out, nbytes / 16, k, nullptr, 0};
    const hipError_t e = job_run(job, impl, (hipStream_t)stream, &g_last_impl);
    if (e != hipSuccess) return hip_fail(e, "aes_ecb launch");
    return OTC_OK;
}

static int ctr_common(const void *in, void *out, size_t nbytes, const otc_aes_key *k, Ctr128 c, bool wrap64,
                      int impl, void *stream)
{
    int r = check_key(k, OTC_DIR_ENCRYPT);
    if (r) return r;
    if ((r = check_bufs(in, out, nbytes, true, "aes_ctr"))) return r;
    if ((r = check_impl(impl))) return r; /* before the empty-call return, as otc_aes_ecb */
    if (nbytes == 0) return OTC_OK;
    hipStream_t st = (hipStream_t)stream;
    const int im = pick_impl(impl, k->bits, nbytes);
    g_last_impl = im;
    hipError_t e;
    if (im == OTC_IMPL_BITSLICE) {
        e = otc_impl::bs_ctr(in, out, nbytes, *k, c, wrap64, st);
    } else if (nbytes >= tt_ctr_persistent_min()) {
        /* the T-table as a persistent claim kernel (first units handed out,
         * the rest claimed): no CU waits on another's static share */
        e = claim_alone(otc_impl::tt_ctr_claim_units(nbytes, c.lo), 2, st, [&](const SplitClaim *cl) {
            return otc_impl::tt_ctr(in, out, nbytes, *k, c, wrap64, st, cl);
        });
    } else {
        e = otc_impl::tt_ctr(in, out, nbytes, *k, c, wrap64, st);
    }
    if (e != hipSuccess) return hip_fail(e, "aes_ctr launch");
    return OTC_OK;
}

extern "C" int otc_aes_ctr(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const uint8_t ctr0[16],
                           uint64_t block_offset, int impl, void *stream)
{
    Range rg("otc_aes_ctr");
    if (!ctr0) return set_err(OTC_ERR_ARG, "null counter");
    return ctr_common(in, out, nbytes, k, ctr_add(ctr_from_bytes(ctr0), block_offset, false), false, impl, stream);
}

/* ---- resumable CTR stream (PolarSSL aes_crypt_ctr semantics on device) ----
 * Reference: aes-modes/aes.c:869-900 -- byte-granular nc_off, the keystream
 * block of the current counter kept in stream_block, the counter advanced when
 * a block is generated.  The host edge does the partial blocks: the head
 * (bytes left in stream_block) is one tiny XOR launch with those bytes as
 * kernel arguments, the tail's keystream block is computed on the host (one
 * AES block) and kept in the context; the kernels do every whole block.  A
 * body left misaligned by the head runs the funnel-shift kernel. */
extern "C" int otc_aes_ctr_ctx_init(otc_aes_ctr_ctx *ctx, const uint8_t nonce_counter[16])
{
    if (!ctx || !nonce_counter) return set_err(OTC_ERR_ARG, "null argument");
    memset(ctx, 0, sizeof *ctx);
    memcpy(ctx->nonce_counter, nonce_counter, 16);
    return OTC_OK;
}

extern "C" int otc_aes_ctr_stream(otc_aes_ctr_ctx *ctx, const otc_aes_key *k, size_t length, const void *in,
                                  void *out, int impl, void *stream)
{
    Range rg("otc_aes_ctr_stream");
    if (!ctx) return set_err(OTC_ERR_ARG, "null context");
    if (ctx->nc_off > 15) return set_err(OTC_ERR_ARG, "nc_off must be 0..15");
    int r = check_key(k, OTC_DIR_ENCRYPT);
    if (r) return r;
    if (length == 0) return OTC_OK;
    if (!in || !out) return set_err(OTC_ERR_ARG, "aes_ctr_stream: null buffer");
    if (partial_overlap(in, out, length))
        return set_err(OTC_ERR_ARG, "aes_ctr_stream: input and output overlap partially");
    if (((uintptr_t)in & 15u) != ((uintptr_t)out & 15u))
        return set_err(OTC_ERR_ARG, "aes_ctr_stream: in and out must have the same alignment modulo 16");
    hipStream_t st = (hipStream_t)stream;
    const size_t n0 = ctx->nc_off;
    const size_t head = n0 ? std::min(length, (size_t)16 - n0) : 0;
    if (head) {
        hipError_t e = otc_impl::xor_small(in, out, (uint32_t)head, ctx->stream_block + n0, st);
        if (e != hipSuccess) return hip_fail(e, "ctr_stream head");
    }
    const size_t body = length - head;
    if (body == 0) {
        ctx->nc_off = (n0 + head) & 15u;
        return OTC_OK;
    }
    const uint8_t *bi = (const uint8_t *)in + head;
    uint8_t *bo = (uint8_t *)out + head;
    const Ctr128 c = ctr_from_bytes(ctx->nonce_counter);
    if ((((uintptr_t)bi) & 15u) == 0) {
        if ((r = ctr_common(bi, bo, body, k, c, false, impl, stream))) return r;
    } else {
        hipError_t e = otc_impl::tt_ctr_shift(bi, bo, body, *k, c, st);
        if (e != hipSuccess) return hip_fail(e, "ctr_stream body (misaligned)");
    }
    const uint64_t full = body / 16, tail = body % 16;
    if (tail) { /* keep the keystream block of the partial tail */
        Ctr128 t = ctr_add(c, full, false);
        uint8_t cb[16];
        store_be64(cb, t.hi);
        store_be64(cb + 8, t.lo);
        aes_context actx;
        aes_import_rk32(&actx, k->rk, k->nr);
        aes_crypt_ecb(&actx, AES_ENCRYPT, cb, ctx->stream_block);
    }
    const Ctr128 nx = ctr_add(c, full + (tail ? 1 : 0), false);
    store_be64(ctx->nonce_counter, nx.hi);
    store_be64(ctx->nonce_counter + 8, nx.lo);
    ctx->nc_off = (size_t)tail;
    return OTC_OK;
}

extern "C" int otc_aes_ctr_rfc3686(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                                   const uint8_t nonce[4], const uint8_t ivec[8], uint64_t block_offset, int impl,
                                   void *stream)
{
    Range rg("otc_aes_ctr_rfc3686");
    if (!nonce || !ivec) return set_err(OTC_ERR_ARG, "null nonce/ivec");
    uint8_t cb[16];
    memcpy(cb, nonce, 4);
    memcpy(cb + 4, ivec, 8);
    cb[12] = 0; cb[13] = 0; cb[14] = 0; cb[15] = 1;
    return ctr_common(in, out, nbytes, k, ctr_add(ctr_from_bytes(cb), block_offset, true), true, impl, stream);
}

extern "C" uint64_t otc_ctr_batch_plan(const otc_ctr_msg *msgs, size_t nmsg, int tile_blocks, uint32_t *tile_msg,
                                       uint64_t *tile_first)
{
    if (!check_tile_blocks(tile_blocks)) return 0;
    const uint64_t tile_bytes = 16ull * (uint64_t)tile_blocks;
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m) {
        const uint64_t shift = (msgs[m].align & OTC_BATCH_ALIGNED) ? 16ull * (msgs[m].align & 0xFFFFu) : 0;
        const uint64_t nt = msgs[m].nbytes ? (msgs[m].nbytes + shift + tile_bytes - 1) / tile_bytes : 0;
        t = tile_map_fill(tile_msg, tile_first, m, t, nt);
    }
    return t;
}

/* Descriptors live in device memory, so per-message checks (alignment,
 * overlap) are the planner's job on the host (our_tree_amd.ops.CtrBatch);
 * here only the launch arguments are validated. */
extern "C" int otc_aes_ctr_batch(const otc_ctr_msg *msgs, const otc_aes_key *keys, const uint32_t *tile_msg,
                                 const uint64_t *tile_first, uint64_t ntiles, int tile_blocks, int nr, void *stream)
{
    Range rg("otc_aes_ctr_batch");
    if (!check_tile_blocks(tile_blocks)) return set_err(OTC_ERR_ARG, "ctr_batch: tile_blocks must be 64, 128 or 256");
    if (ntiles == 0) return OTC_OK;
    if (!msgs || !keys || !tile_msg || !tile_first) return set_err(OTC_ERR_ARG, "ctr_batch: null array");
    if (nr != 10 && nr != 12 && nr != 14) return set_err(OTC_ERR_ARG, "ctr_batch: nr must be 10, 12 or 14");
    if ((((uintptr_t)msgs) | ((uintptr_t)keys) | ((uintptr_t)tile_first)) & 7u || ((uintptr_t)tile_msg & 3u))
        return set_err(OTC_ERR_ARG, "ctr_batch: misaligned descriptor arrays");
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](const SplitClaim *cl) {
        return otc_impl::tt_ctr_batch(msgs, keys, tile_msg, tile_first, ntiles, tile_blocks, nr, st, cl);
    };
    /* large batches: claimed tile runs (first one handed out) instead of the
     * static split over the waves (A/B: OTC_BATCH_CLAIM_MIN_TILES) */
    static const uint64_t min_tiles = [] {
        uint64_t v = 0;
        return env_u64("OTC_BATCH_CLAIM_MIN_TILES", &v) ? v : (uint64_t)65536;
    }();
    const hipError_t e =
        ntiles >= min_tiles ? claim_alone(otc_impl::tt_ctr_batch_units(ntiles), 2, st, launch) : launch(nullptr);
    if (e != hipSuccess) return hip_fail(e, "ctr_batch launch");
    return OTC_OK;
}

extern "C" int otc_aes_cbc_decrypt_impl(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                                        const uint8_t iv[16], int impl, void *stream)
{
    Range rg("otc_aes_cbc_decrypt");
    int r = check_key(k, OTC_DIR_DECRYPT);
    if (r) return r;
    if (nbytes % 16) return set_err(OTC_ERR_ARG, "CBC length must be a multiple of 16");
    if (!iv) return set_err(OTC_ERR_ARG, "null iv");
    if ((r = check_bufs(in, out, nbytes, nbytes <= 16, "aes_cbc_decrypt"))) return r;
    if ((r = check_impl(impl))) return r;
    if (nbytes == 0) return OTC_OK;
    const Job job{otc_impl::JOB_CBC_DEC, in, out, nbytes / 16, k, iv, 0};
    const hipError_t e = job_run(job, impl, (hipStream_t)stream, &g_last_impl);
    if (e != hipSuccess) return hip_fail(e, "cbc_decrypt launch");
    return OTC_OK;
}

extern "C" int otc_aes_cbc_decrypt(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                                   const uint8_t iv[16], void *stream)
{
    return otc_aes_cbc_decrypt_impl(in, out, nbytes, k, iv, OTC_IMPL_AUTO, stream);
}

extern "C" int otc_aes_cbc_encrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                                 const otc_aes_key *k, const uint8_t iv0[16], int impl, void *stream)
{
    Range rg("otc_aes_cbc_encrypt_segments");
    int r = check_key(k, OTC_DIR_ENCRYPT);
    if (r) return r;
    if (seg_bytes % 16) return set_err(OTC_ERR_ARG, "segment length must be a multiple of 16");
    if ((r = check_seg_args(in, out, seg_bytes, nseg, iv0, true, impl, "aes_cbc_encrypt_segments"))) return r;
    if (nseg == 0 || seg_bytes == 0) return OTC_OK;
    const hipError_t e = seg_enc_run(false, in, out, seg_bytes, nseg, *k, ctr_from_bytes(iv0), (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "cbc_encrypt_segments launch");
    return OTC_OK;
}

extern "C" int otc_aes_cbc_encrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                            const otc_aes_key *k, const uint8_t iv0[16], void *stream)
{
    return otc_aes_cbc_encrypt_segments_impl(in, out, seg_bytes, nseg, k, iv0, OTC_IMPL_AUTO, stream);
}

extern "C" int otc_aes_cbc_decrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                                 const otc_aes_key *k, const uint8_t iv0[16], int impl, void *stream)
{
    Range rg("otc_aes_cbc_decrypt_segments");
    int r = check_key(k, OTC_DIR_DECRYPT);
    if (r) return r;
    if (seg_bytes % 16) return set_err(OTC_ERR_ARG, "segment length must be a multiple of 16");
    size_t sb = seg_bytes / 16;
    if (sb == 0) return set_err(OTC_ERR_ARG, "empty segments");
    if ((r = check_seg_args(in, out, seg_bytes, nseg, iv0, false, impl, "aes_cbc_decrypt_segments"))) return r;
    if (nseg == 0) return OTC_OK;
    const Job job{otc_impl::JOB_CBC_DEC_SEG, in, out, (uint64_t)sb * nseg, k, iv0, sb};
    const hipError_t e = job_run(job, impl, (hipStream_t)stream, &g_last_impl);
    if (e != hipSuccess) return hip_fail(e, "cbc_decrypt_segments launch");
    return OTC_OK;
}

extern "C" int otc_aes_cbc_decrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                            const otc_aes_key *k, const uint8_t iv0[16], void *stream)
{
    return otc_aes_cbc_decrypt_segments_impl(in, out, seg_bytes, nseg, k, iv0, OTC_IMPL_AUTO, stream);
}

/* CFB128 over independent segments (IV_s = iv0 + s, like the CBC sector
 * mode): encryption is one serial chain per segment (one lane each, the
 * sector kernel with the CFB chain step); decryption is fully parallel with
 * IV_s at every segment start.  Both use the ENCRYPTION key schedule. */
static int cfb_seg_common(const void *in, void *out, size_t seg_bytes, size_t nseg, const otc_aes_key *k,
                          const uint8_t iv0[16], void *stream, bool decrypt, const char *what,
                          int impl = OTC_IMPL_AUTO)
{
    int r = check_key(k, OTC_DIR_ENCRYPT);
    if (r) return r;
    if (seg_bytes % 16) return set_err(OTC_ERR_ARG, "segment length must be a multiple of 16");
    /* decrypt reads block i-1 of the input while another lane writes block
     * i-1 of the output: in place only for encryption (lane-private chains) */
    if ((r = check_seg_args(in, out, seg_bytes, nseg, iv0, !decrypt, impl, what))) return r;
    if (nseg == 0 || seg_bytes == 0) return OTC_OK;
    const Job job{otc_impl::JOB_CFB_DEC_SEG, in, out, (uint64_t)(seg_bytes / 16) * nseg, k, iv0, seg_bytes / 16};
    const hipError_t e = decrypt ? job_run(job, impl, (hipStream_t)stream, &g_last_impl)
                                 : seg_enc_run(true, in, out, seg_bytes, nseg, *k, ctr_from_bytes(iv0), (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, what);
    return OTC_OK;
}

extern "C" int otc_aes_cfb128_encrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                               const otc_aes_key *k, const uint8_t iv0[16], void *stream)
{
    return otc_aes_cfb128_encrypt_segments_impl(in, out, seg_bytes, nseg, k, iv0, OTC_IMPL_AUTO, stream);
}

extern "C" int otc_aes_cfb128_encrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                                    const otc_aes_key *k, const uint8_t iv0[16], int impl,
                                                    void *stream)
{
    Range rg("otc_aes_cfb128_encrypt_segments");
    return cfb_seg_common(in, out, seg_bytes, nseg, k, iv0, stream, false, "cfb128_encrypt_segments", impl);
}

extern "C" int otc_aes_cfb128_decrypt_segments_impl(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                                    const otc_aes_key *k, const uint8_t iv0[16], int impl,
                                                    void *stream)
{
    Range rg("otc_aes_cfb128_decrypt_segments");
    return cfb_seg_common(in, out, seg_bytes, nseg, k, iv0, stream, true, "cfb128_decrypt_segments", impl);
}

extern "C" int otc_aes_cfb128_decrypt_segments(const void *in, void *out, size_t seg_bytes, size_t nseg,
                                               const otc_aes_key *k, const uint8_t iv0[16], void *stream)
{
    return otc_aes_cfb128_decrypt_segments_impl(in, out, seg_bytes, nseg, k, iv0, OTC_IMPL_AUTO, stream);
}

extern "C" int otc_aes_cfb128_decrypt_impl(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                                           const uint8_t iv[16], int impl, void *stream)
{
    Range rg("otc_aes_cfb128_decrypt");
    int r = check_key(k, OTC_DIR_ENCRYPT);
    if (r) return r;
    if (nbytes % 16) return set_err(OTC_ERR_ARG, "CFB128 device path needs a multiple of 16 bytes");
    if (!iv) return set_err(OTC_ERR_ARG, "null iv");
    if ((r = check_bufs(in, out, nbytes, nbytes <= 16, "aes_cfb128_decrypt"))) return r;
    if ((r = check_impl(impl))) return r;
    if (nbytes == 0) return OTC_OK;
    const Job job{otc_impl::JOB_CFB_DEC, in, out, nbytes / 16, k, iv, 0};
    const hipError_t e = job_run(job, impl, (hipStream_t)stream, &g_last_impl);
    if (e != hipSuccess) return hip_fail(e, "cfb_decrypt launch");
    return OTC_OK;
}

extern "C" int otc_aes_cfb128_decrypt(const void *in, void *out, size_t nbytes, const otc_aes_key *k,
                                      const uint8_t iv[16], void *stream)
{
    return otc_aes_cfb128_decrypt_impl(in, out, nbytes, k, iv, OTC_IMPL_AUTO, stream);
}

/* ---- XTS ------------------------------------------------------------------ */
extern "C" int otc_xts_key_init(otc_xts_key *k, const uint8_t *key, int keybits, int dir)
{
    if (!k || !key) return set_err(OTC_ERR_ARG, "null argument");
    if (keybits != 256 && keybits != 512)
        return set_err(OTC_ERR_ARG, "invalid XTS key size (K1 || K2 must be 256 or 512 bits)");
    if (dir != OTC_DIR_ENCRYPT && dir != OTC_DIR_DECRYPT) return set_err(OTC_ERR_ARG, "bad direction");
    if (int r = otc_aes_key_init(&k->data, key, keybits / 2, dir)) return r;
    return otc_aes_key_init(&k->tweak, key + keybits / 16, keybits / 2, OTC_DIR_ENCRYPT);
}

extern "C" int otc_aes_xts(const void *in, void *out, size_t unit_bytes, size_t nunits, const otc_xts_key *k,
                           const uint8_t tweak0[16], void *stream)
{
    Range rg("otc_aes_xts");
    if (!k) return set_err(OTC_ERR_ARG, "null key");
    if (int r = check_key(&k->tweak, OTC_DIR_ENCRYPT)) return r;
    if ((k->data.nr != 10 && k->data.nr != 14) || k->data.nr != k->tweak.nr ||
        (k->data.dir != OTC_DIR_ENCRYPT && k->data.dir != OTC_DIR_DECRYPT))
        return set_err(OTC_ERR_ARG, "bad XTS key (two AES-128 or two AES-256 schedules)");
    if (!tweak0) return set_err(OTC_ERR_ARG, "null tweak");
    if (unit_bytes < 16) return set_err(OTC_ERR_ARG, "XTS data unit must be at least 16 bytes");
    if (unit_bytes > ((size_t)16 << 20)) return set_err(OTC_ERR_ARG, "XTS data unit above 2^20 blocks");
    if (nunits > 1 && unit_bytes % 16)
        return set_err(OTC_ERR_ARG, "XTS data units of several must be multiples of 16 bytes");
    if (nunits && unit_bytes > SIZE_MAX / nunits) return set_err(OTC_ERR_ARG, "size overflow");
    if (int r = check_bufs(in, out, unit_bytes * nunits, true, "aes_xts")) return r;
    if (nunits == 0) return OTC_OK;
    hipStream_t st = (hipStream_t)stream;
    g_last_impl = OTC_IMPL_TTABLE;
    const uint32_t m = (uint32_t)(unit_bytes / 16), r = (uint32_t)(unit_bytes % 16);
    /* whole blocks: the bulk kernel; a stolen tail (one unit only): the bulk
     * kernel up to block m - 2, then the last 16 + r bytes behind it */
    const uint64_t nblocks = r ? m - 1u : (uint64_t)m * nunits;
    hipError_t e = otc_impl::xts_bulk(in, out, nblocks, r ? (m > 1 ? m - 1u : 1u) : m, k->data, k->tweak, tweak0, st);
    if (e == hipSuccess && r) e = otc_impl::xts_steal(in, out, m, r, k->data, k->tweak, tweak0, st);
    if (e != hipSuccess) return hip_fail(e, "aes_xts launch");
    return OTC_OK;
}

/* ---- CTR32: GCM's counter mode (the hash and the mode itself: aead.cpp) --- */
/* GCM's counter: the low 32 bits wrap, the upper 96 never change.  Up to the
 * wrap the CTR kernels' 128-bit add cannot carry out of the low word, so the
 * call is ctr_common as it is, twice when it crosses the wrap. */
int otc_rt::ctr32_run(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const uint8_t ctr0[16], int impl,
                     void *stream)
{
    if (!ctr0) return set_err(OTC_ERR_ARG, "null counter");
    if (nbytes > ((uint64_t)1 << 36)) return set_err(OTC_ERR_ARG, "ctr32: more than 2^32 blocks");
    if (int r = check_bufs(in, out, nbytes, true, "aes_ctr32")) return r; /* the whole range, before any launch */
    const Ctr128 c = ctr_from_bytes(ctr0);
    const uint64_t to_wrap = ((uint64_t)1 << 32) - (c.lo & 0xFFFFFFFFull); /* blocks before the low word is 0 again */
    if ((nbytes + 15) / 16 <= to_wrap) return ctr_common(in, out, nbytes, k, c, false, impl, stream);
    const size_t head = (size_t)to_wrap * 16;
    if (int r = ctr_common(in, out, head, k, c, false, impl, stream)) return r;
    const Ctr128 c2{c.hi, c.lo & ~0xFFFFFFFFull};
    return ctr_common((const uint8_t *)in + head, (uint8_t *)out + head, nbytes - head, k, c2, false, impl, stream);
}

extern "C" int otc_aes_ctr32(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const uint8_t ctr0[16],
                             int impl, void *stream)
{
    Range rg("otc_aes_ctr32");
    return ctr32_run(in, out, nbytes, k, ctr0, impl, stream);
}

extern "C" int otc_xor(const void *a, const void *b, void *out, size_t nbytes, void *stream)
{
    Range rg("otc_xor");
    if (int r = check_bufs(a, out, nbytes, true, "xor")) return r;
    if (int r = check_bufs(b, out, nbytes, true, "xor")) return r;
    if (nbytes == 0) return OTC_OK;
    hipError_t e = otc_impl::k_xor(a, b, out, nbytes, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "xor launch");
    return OTC_OK;
}

extern "C" int otc_rc4_multi(const uint8_t *keys, int keylen, size_t nstreams, size_t len, size_t drop,
                             const void *in, void *out, void *stream)
{
    Range rg("otc_rc4_multi");
    if (keylen < 1 || keylen > 256) return set_err(OTC_ERR_ARG, "RC4 key length must be 1..256");
    if (nstreams == 0 || len == 0) return OTC_OK;
    if (!keys || !out) return set_err(OTC_ERR_ARG, "rc4_multi: null buffer");
    if (len > SIZE_MAX / nstreams) return set_err(OTC_ERR_ARG, "size overflow");
    if (in && partial_overlap(in, out, nstreams * len))
        return set_err(OTC_ERR_ARG, "rc4_multi: input and output overlap partially");
    hipError_t e = otc_impl::k_rc4_multi(keys, keylen, nstreams, len, drop, in, out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "rc4_multi launch");
    return OTC_OK;
}

extern "C" int otc_rc4_crypt_batch(void *states, size_t nstreams, size_t len, const void *in, void *out,
                                   void *stream)
{
    Range rg("otc_rc4_crypt_batch");
    if (nstreams == 0 || len == 0) return OTC_OK;
    if (!states || !in || !out) return set_err(OTC_ERR_ARG, "rc4_crypt_batch: null buffer");
    if ((uintptr_t)states & 3u) return set_err(OTC_ERR_ARG, "rc4_crypt_batch: states must be 4-byte aligned");
    if (len > SIZE_MAX / nstreams) return set_err(OTC_ERR_ARG, "size overflow");
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, n = nstreams * len;
    if (partial_overlap(in, out, n))
        return set_err(OTC_ERR_ARG, "rc4_crypt_batch: input and output overlap partially");
    /* every state is written back in place: it must not alias the data */
    if (nstreams > SIZE_MAX / 264) return set_err(OTC_ERR_ARG, "size overflow");
    const uintptr_t s = (uintptr_t)states, sn = (uintptr_t)nstreams * 264u;
    if ((s < a + n && a < s + sn) || (s < b + n && b < s + sn))
        return set_err(OTC_ERR_ARG, "rc4_crypt_batch: states overlap the input or output");
    hipError_t e = otc_impl::k_rc4_states(states, nstreams, len, in, out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "rc4_crypt_batch launch");
    return OTC_OK;
}

extern "C" int otc_fill_random(void *p, size_t nbytes, uint64_t seed, void *stream)
{
    Range rg("otc_fill_random");
    if (nbytes == 0) return OTC_OK;
    if (int r = check_bufs(p, p, nbytes, true, "fill_random")) return r;
    hipError_t e = otc_impl::k_fill_random(p, nbytes, seed, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "fill_random launch");
    return OTC_OK;
}

extern "C" int otc_checksum(const void *p, size_t nbytes, uint64_t *out_dev, void *stream)
{
    Range rg("otc_checksum");
    if (nbytes % 8) return set_err(OTC_ERR_ARG, "checksum length must be a multiple of 8");
    if (!out_dev || (nbytes && !p)) return set_err(OTC_ERR_ARG, "checksum: null buffer");
    if (((uintptr_t)p | (uintptr_t)out_dev) & 7u) return set_err(OTC_ERR_ARG, "checksum: buffers must be 8-byte aligned");
    hipError_t e = otc_impl::k_checksum(p, nbytes, out_dev, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "checksum launch");
    return OTC_OK;
}

extern "C" int otc_clock_probe(uint64_t *out_dev, double delay_s, double window_s, void *stream)
{
    if (!out_dev || ((uintptr_t)out_dev & 7u)) return set_err(OTC_ERR_ARG, "clock_probe: bad output buffer");
    if (!(delay_s >= 0.0) || !(window_s > 0.0) || delay_s + window_s > 60.0)
        return set_err(OTC_ERR_ARG, "clock_probe: delay/window out of range (total <= 60 s)");
    const uint64_t hz = 100000000ull; /* s_memrealtime */
    hipError_t e = otc_impl::k_clock(out_dev, (uint64_t)(delay_s * hz), (uint64_t)(window_s * hz) + 1,
                                     (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "clock_probe launch");
    return OTC_OK;
}

/* ---- AES-NI-shaped bulk API (otc_aesni.h) ------------------------------- */
static int key_from_sched(otc_aes_key *k, const unsigned char *sched, int nr, int dir)
{
    if (!sched) return set_err(OTC_ERR_ARG, "null key schedule");
    if (nr != 10 && nr != 12 && nr != 14) return set_err(OTC_ERR_ARG, "number_of_rounds must be 10, 12 or 14");
    memset(k, 0, sizeof *k);
    memcpy(k->rk, sched, 16u * (unsigned)(nr + 1)); /* FIPS byte order = LE words on the host */
    k->nr = nr;
    k->dir = dir;
    k->bits = 32 * (nr - 6);
    return OTC_OK;
}

extern "C" int otc_AES_ECB_encrypt(const unsigned char *in, unsigned char *out, unsigned long length,
                                   const unsigned char *key, int number_of_rounds, void *stream)
{
    otc_aes_key k;
    if (int r = key_from_sched(&k, key, number_of_rounds, OTC_DIR_ENCRYPT)) return r;
    return otc_aes_ecb(in, out, length, &k, OTC_IMPL_AUTO, stream);
}

extern "C" int otc_AES_ECB_decrypt(const unsigned char *in, unsigned char *out, unsigned long length,
                                   const unsigned char *key, int number_of_rounds, void *stream)
{
    otc_aes_key k;
    if (int r = key_from_sched(&k, key, number_of_rounds, OTC_DIR_DECRYPT)) return r;
    return otc_aes_ecb(in, out, length, &k, OTC_IMPL_AUTO, stream);
}

extern "C" int otc_AES_CTR_encrypt(const unsigned char *in, unsigned char *out, const unsigned char ivec[8],
                                   const unsigned char nonce[4], unsigned long length, const unsigned char *key,
                                   int number_of_rounds, void *stream)
{
    otc_aes_key k;
    if (int r = key_from_sched(&k, key, number_of_rounds, OTC_DIR_ENCRYPT)) return r;
    return otc_aes_ctr_rfc3686(in, out, length, &k, nonce, ivec, 0, OTC_IMPL_AUTO, stream);
}

