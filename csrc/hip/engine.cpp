/*
 * engine.cpp -- host runtime of the MI355X cipher engine (C API in otc.h).
 *
 * Replaces the reference's BlockCipher/AES host class
 * (/root/reference/aes-gpu/Source/AES.cu:50-282), which did a synchronous
 * cudaMalloc -> pageable H2D -> launch -> D2H -> cudaFree per call, queried
 * device properties inside the timed region and never checked an error.
 * Here:
 *   - kernels are launched asynchronously on the caller's stream with the
 *     expanded key as a by-value kernel argument (no per-call copies);
 *   - the streaming engine (otc_engine_*) owns a pinned staging ring and three
 *     HIP streams per device, so H2D(k+1) | kernel(k) | D2H(k-1) overlap;
 *   - the multi-GPU path (otc_multi_*) shards one stream over devices, either
 *     by direct per-GPU ingest or by an RCCL scatter/gather over xGMI from a
 *     root GPU, with CTR counter offsets and CBC halos computed by the planner.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "aes.h"
#include "chacha.h"
#include "otc.h"
#include "otc_aesni.h"
#include "otc_device.h"
#include "engine_internal.h"

using otc_dev::Ctr128;
using otc_dev::SplitClaim;
using otc_impl::Job;

/* ------------------------------------------------------------------------- */
namespace otc_rt {

namespace {
thread_local std::string g_err;
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

} // namespace otc_rt

namespace otc_dev {
namespace {
std::atomic<long> g_fault_alloc{-1};
}
bool alloc_fault()
{
    /* armed with n >= 0: allocations n+1 from now fail once, then disarm */
    return g_fault_alloc.load(std::memory_order_relaxed) >= 0 &&
           g_fault_alloc.fetch_sub(1, std::memory_order_relaxed) == 0;
}

/* ---- per-call workspaces (otc_device.h ws_alloc / ws_free) ---------------- */
namespace {
struct WsBlock {
    void *p;
    size_t bytes;
    int dev;
    hipEvent_t done;  /* recorded behind the block's last use when it is kept */
    hipStream_t last; /* the stream it was returned on */
};
std::mutex g_ws_mu;
std::vector<WsBlock> g_ws_kept; /* returned blocks, oldest first */
std::vector<WsBlock> g_ws_out;  /* handed out: a few at a time, found by a scan */
/* larger blocks (the CTR tables of calls beyond ~5 GiB) are not kept: their
 * calls run for milliseconds, and the pool should have the memory back */
constexpr size_t WS_MAX_BLOCK = (size_t)32 << 20;
constexpr size_t WS_MAX_KEPT = 16, WS_MAX_KEPT_BYTES = (size_t)64 << 20; /* per device */

bool ws_plain(size_t bytes, hipStream_t st)
{
    if (bytes > WS_MAX_BLOCK) return true;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return true; /* unknown: the path that is right under capture */
    }
    return cap != hipStreamCaptureStatusNone;
}

/* the block's last use has run: no stream has to wait for it */
bool ws_idle(const WsBlock &b)
{
    if (hipEventQuery(b.done) == hipSuccess) return true;
    (void)hipGetLastError(); /* hipErrorNotReady */
    return false;
}

bool ws_over(int dev)
{
    size_t n = 0, total = 0;
    for (const WsBlock &b : g_ws_kept)
        if (b.dev == dev) ++n, total += b.bytes;
    return n > WS_MAX_KEPT || total > WS_MAX_KEPT_BYTES;
}
} // namespace

hipError_t ws_alloc(void **p, size_t bytes, hipStream_t st)
{
    *p = nullptr;
    int dev = 0;
    const bool plain = ws_plain(bytes, st) || hipGetDevice(&dev) != hipSuccess;
    if (!plain) {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        /* The smallest kept block that fits without wasting most of itself,
         * among those that couple no streams: returned on this stream (its
         * last use is in front of this call anyway), or idle.  A block still
         * in use on another stream is left alone -- taking it would make
         * this stream wait for that one's work. */
        size_t best = g_ws_kept.size();
        for (size_t i = 0; i < g_ws_kept.size(); ++i) {
            const WsBlock &b = g_ws_kept[i];
            if (b.dev == dev && b.bytes >= bytes && (b.bytes <= 4 * bytes || b.bytes <= ((size_t)1 << 20)) &&
                (best == g_ws_kept.size() || b.bytes < g_ws_kept[best].bytes) && (b.last == st || ws_idle(b)))
                best = i;
        }
        if (best != g_ws_kept.size()) {
            const WsBlock b = g_ws_kept[best];
            /* no wait in either case; kept as the safety should a destroyed
             * stream's handle have come back as `st` */
            if (hipStreamWaitEvent(st, b.done, 0) == hipSuccess) {
                g_ws_kept.erase(g_ws_kept.begin() + (long)best);
                g_ws_out.push_back(b);
                *p = b.p;
                return hipSuccess;
            }
            (void)hipGetLastError();
        }
    }
    const hipError_t e = hipMallocAsync(p, bytes, st);
    if (e != hipSuccess || plain) return e;
    WsBlock b{*p, bytes, dev, nullptr, nullptr};
    if (hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        return hipSuccess; /* not tracked: ws_free hands it straight back to the pool */
    }
    std::lock_guard<std::mutex> lk(g_ws_mu);
    g_ws_out.push_back(b);
    return hipSuccess;
}

hipError_t ws_free(void *p, hipStream_t st)
{
    if (!p) return hipSuccess;
    std::lock_guard<std::mutex> lk(g_ws_mu);
    size_t i = 0;
    while (i < g_ws_out.size() && g_ws_out[i].p != p) ++i;
    if (i == g_ws_out.size()) return hipFreeAsync(p, st);
    WsBlock b = g_ws_out[i];
    g_ws_out.erase(g_ws_out.begin() + (long)i);
    if (hipEventRecord(b.done, st) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipEventDestroy(b.done);
        return hipFreeAsync(p, st);
    }
    b.last = st;
    g_ws_kept.push_back(b);
    /* Over this device's limits: its oldest idle blocks go back to the pool
     * (idle: freeing them through `st` waits for nothing).  If the limits
     * still do not hold -- every other block is in use somewhere -- this
     * block is not kept either and takes the pool's stream-ordered free. */
    for (size_t k = 0; k + 1 < g_ws_kept.size() && ws_over(b.dev);) {
        const WsBlock v = g_ws_kept[k];
        if (v.dev != b.dev || !ws_idle(v)) {
            ++k;
            continue;
        }
        g_ws_kept.erase(g_ws_kept.begin() + (long)k);
        if (hipFreeAsync(v.p, st) != hipSuccess) (void)hipGetLastError();
        (void)hipEventDestroy(v.done);
    }
    if (ws_over(b.dev)) {
        g_ws_kept.pop_back();
        (void)hipEventDestroy(b.done);
        return hipFreeAsync(p, st);
    }
    return hipSuccess;
}

void ws_release_all()
{
    std::vector<WsBlock> kept;
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        kept.swap(g_ws_kept);
    }
    for (const WsBlock &b : kept) {
        if (hipEventSynchronize(b.done) != hipSuccess || hipFree(b.p) != hipSuccess) (void)hipGetLastError();
        (void)hipEventDestroy(b.done);
    }
}
} // namespace otc_dev

extern "C" void otc_fault_inject_alloc(long after) { otc_dev::g_fault_alloc.store(after < 0 ? -1 : after); }

extern "C" long otc_fault_inject_pending(void)
{
    /* the countdown itself: alloc_fault leaves it at -1 when it fires */
    const long v = otc_dev::g_fault_alloc.load(std::memory_order_relaxed);
    return v < 0 ? -1 : v;
}

using namespace otc_rt;

namespace {

/* the kernel family the calling thread's last AES call ran (otc_last_impl) */
thread_local int g_last_impl = OTC_IMPL_AUTO;

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
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (a < b + nbytes && b < a + nbytes)
        return set_err(OTC_ERR_ARG, std::string(what) + ": input and output overlap partially");
    return OTC_OK;
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
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (a != b && a < b + length && b < a + length)
        return set_err(OTC_ERR_ARG, "aes_ctr_stream: input and output overlap partially");
    if ((a & 15u) != (b & 15u))
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
        for (int i = 0; i < 8; ++i) cb[i] = (uint8_t)(t.hi >> (56 - 8 * i));
        for (int i = 0; i < 8; ++i) cb[8 + i] = (uint8_t)(t.lo >> (56 - 8 * i));
        aes_context actx;
        aes_import_rk32(&actx, k->rk, k->nr);
        aes_crypt_ecb(&actx, AES_ENCRYPT, cb, ctx->stream_block);
    }
    const Ctr128 nx = ctr_add(c, full + (tail ? 1 : 0), false);
    for (int i = 0; i < 8; ++i) ctx->nonce_counter[i] = (uint8_t)(nx.hi >> (56 - 8 * i));
    for (int i = 0; i < 8; ++i) ctx->nonce_counter[8 + i] = (uint8_t)(nx.lo >> (56 - 8 * i));
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
    if (tile_blocks != 64 && tile_blocks != 128 && tile_blocks != 256) return 0;
    const uint64_t tile_bytes = 16ull * (uint64_t)tile_blocks;
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m) {
        const uint64_t shift = (msgs[m].align & OTC_BATCH_ALIGNED) ? 16ull * (msgs[m].align & 0xFFFFu) : 0;
        const uint64_t nt = msgs[m].nbytes ? (msgs[m].nbytes + shift + tile_bytes - 1) / tile_bytes : 0;
        if (tile_first) tile_first[m] = t;
        if (tile_msg)
            for (uint64_t k = 0; k < nt; ++k) tile_msg[t + k] = (uint32_t)m;
        t += nt;
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
    if (tile_blocks != 64 && tile_blocks != 128 && tile_blocks != 256)
        return set_err(OTC_ERR_ARG, "ctr_batch: tile_blocks must be 64, 128 or 256");
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
        const char *v = getenv("OTC_BATCH_CLAIM_MIN_TILES");
        return v && *v ? (uint64_t)strtoull(v, nullptr, 10) : (uint64_t)65536;
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

/* ---- GCM: CTR32, GHASH, the authenticated mode ---------------------------- */
/* GCM's counter: the low 32 bits wrap, the upper 96 never change.  Up to the
 * wrap the CTR kernels' 128-bit add cannot carry out of the low word, so the
 * call is ctr_common as it is, twice when it crosses the wrap. */
static int ctr32_run(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const uint8_t ctr0[16], int impl,
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

extern "C" int otc_ghash_spans(uint64_t *spans, int max)
{
    uint64_t none;
    return otc_impl::ghash_spans(spans ? spans : &none, spans ? max : 0);
}

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
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? set_err(OTC_ERR_NOMEM, "ghash: no memory for the tables and partials")
                                        : hip_fail(e, "ghash workspace");
    }
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
    for (int i = 0; i < 8; ++i) {
        lenblock[i] = (uint8_t)(((uint64_t)aad_len * 8) >> (56 - 8 * i));
        lenblock[8 + i] = (uint8_t)(((uint64_t)nbytes * 8) >> (56 - 8 * i));
    }

    /* the hash's memory first: a failure leaves out and the tag untouched */
    void *ws = nullptr;
    hipError_t e = otc_impl::ghash_ws_alloc(nbytes, st, &ws);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? set_err(OTC_ERR_NOMEM, "gcm: no memory for the hash's tables and partials")
                                        : hip_fail(e, "gcm workspace");
    }
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
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (a != b && a < b + nbytes && b < a + nbytes)
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

extern "C" int otc_poly1305_spans(uint64_t *spans, int max)
{
    uint64_t none;
    return otc_impl::poly1305_spans(spans ? spans : &none, spans ? max : 0);
}

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
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return set_err(OTC_ERR_NOMEM, std::string(what) + ": no memory for the hash's partials");
    if (e == hipErrorInvalidValue) return set_err(OTC_ERR_ARG, std::string(what) + ": too many bytes");
    return hip_fail(e, what);
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

/* ---- batched GCM: many records, own IVs, one tag array --------------------- */
extern "C" int otc_gcm_batch_spans(uint64_t *spans, int max)
{
    uint64_t none;
    return otc_impl::gcm_batch_spans(spans ? spans : &none, spans ? max : 0);
}

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
    if (tile_blocks != 64 && tile_blocks != 128 && tile_blocks != 256)
        return set_err(OTC_ERR_ARG, "gcm_batch: tile_blocks must be 64, 128 or 256");
    if (nmsg == 0) return 0;
    if (!msgs) return set_err(OTC_ERR_ARG, "gcm_batch: null descriptors");
    if (nmsg > 0xFFFFFFFFull) return set_err(OTC_ERR_ARG, "gcm_batch: more than 2^32 - 1 records");
    auto bad = [](size_t m, const char *what) {
        return set_err(OTC_ERR_ARG, "gcm_batch: record " + std::to_string(m) + ": " + what);
    };
    struct Iv {
        uint64_t lo, hi;
        size_t m;
    };
    std::vector<Iv> outs; /* the non-empty outputs, to find records that overlap */
    for (size_t m = 0; m < nmsg; ++m) {
        const otc_gcm_msg &d = msgs[m];
        /* at most 65536 blocks: the counter's low 32 bits, started at 2, never wrap */
        if (d.nbytes > OTC_GCM_BATCH_MAX_BYTES) return bad(m, "more than 1 MiB of data (use otc_aes_gcm)");
        if (d.aad_bytes > OTC_GCM_BATCH_MAX_AAD) return bad(m, "more than 64 KiB of AAD");
        if (d.aad_bytes && !d.aad) return bad(m, "null aad");
        if (!d.nbytes) continue;
        if (!d.in || !d.out) return bad(m, "null buffer");
        if ((d.in | d.out) & 15u) return bad(m, "data buffers must be 16-byte aligned");
        if (d.in != d.out && d.in < d.out + d.nbytes && d.out < d.in + d.nbytes)
            return bad(m, "input and output overlap partially");
        outs.push_back({d.out, d.out + d.nbytes, m});
    }
    std::sort(outs.begin(), outs.end(), [](const Iv &a, const Iv &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < outs.size(); ++i)
        if (outs[i].lo < outs[i - 1].hi) return bad(outs[i].m, "its output overlaps another record's");
    for (size_t m = 0; m < nmsg; ++m) { /* no record reads what another writes */
        const otc_gcm_msg &d = msgs[m];
        if (!d.nbytes) continue;
        auto it = std::upper_bound(outs.begin(), outs.end(), d.in,
                                   [](uint64_t a, const Iv &o) { return a < o.hi; }); /* first output ending past in */
        for (; it != outs.end() && it->lo < d.in + d.nbytes; ++it)
            if (it->m != m) return bad(m, "its input overlaps another record's output");
    }
    for (size_t m = 0; m < nmsg; ++m) { /* an encryption writes every output before the hash reads the AADs */
        const otc_gcm_msg &d = msgs[m];
        if (!d.aad_bytes) continue;
        auto it = std::upper_bound(outs.begin(), outs.end(), d.aad, [](uint64_t a, const Iv &o) { return a < o.hi; });
        if (it != outs.end() && it->lo < d.aad + d.aad_bytes) return bad(m, "its AAD overlaps a record's output");
    }
    const uint64_t tile_bytes = 16ull * (uint64_t)tile_blocks;
    uint64_t t = 0;
    for (size_t m = 0; m < nmsg; ++m) {
        const uint64_t nt = (msgs[m].nbytes + tile_bytes - 1) / tile_bytes;
        if (ctr_msgs) ctr_msgs[m] = otc_ctr_msg{msgs[m].in, msgs[m].out, msgs[m].nbytes, 0, 0, 0, 0};
        if (tile_first) tile_first[m] = t;
        if (tile_msg)
            for (uint64_t k = 0; k < nt; ++k) tile_msg[t + k] = (uint32_t)m;
        t += nt;
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
    if (tile_blocks != 64 && tile_blocks != 128 && tile_blocks != 256)
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
    g_last_impl = OTC_IMPL_TTABLE;
    uint8_t *j0 = (uint8_t *)ws_dev, *ekj0 = j0 + nmsg * 16;
    const bool enc = dir == OTC_DIR_ENCRYPT;

    hipError_t e = otc_impl::gcm_batch_prep(ivs_dev, nmsg, ctr_msgs_dev, j0, st);
    if (e != hipSuccess) return hip_fail(e, "gcm_batch prep launch");
    /* E_K(J0[]): the grid T-table kernel, ECB over nmsg blocks */
    const Job job{otc_impl::JOB_ECB_ENC, j0, ekj0, nmsg, &k->enc, nullptr, 0};
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
    if (in && in != out) {
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, n = nstreams * len;
        if (a < b + n && b < a + n) return set_err(OTC_ERR_ARG, "rc4_multi: input and output overlap partially");
    }
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
    if (in != out && a < b + n && b < a + n)
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

/* ---- device info -------------------------------------------------------- */
extern "C" int otc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int otc_device_cus(int dev)
{
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    return v;
}
extern "C" int otc_device_clock_khz(int dev)
{
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeClockRate, dev) != hipSuccess) return -1;
    return v;
}
extern "C" int otc_set_device(int dev)
{
    HIPCHK(hipSetDevice(dev));
    return OTC_OK;
}
extern "C" int otc_device_sync(void)
{
    HIPCHK(hipDeviceSynchronize());
    return OTC_OK;
}

/* Streams for C harnesses (hipStreamCreate: ordered with the legacy default
 * stream, so hipEvents recorded on the default stream bracket work on them) */
extern "C" void *otc_stream_create(void)
{
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreate(&s);
    if (e != hipSuccess) {
        hip_fail(e, "hipStreamCreate");
        return nullptr;
    }
    return (void *)s;
}
/* a and b each wait for what the other has queued so far: a join point for
 * work split by hand over two streams (otbench's *-split modes) */
extern "C" int otc_stream_join(void *a, void *b)
{
    hipEvent_t ea = nullptr, eb = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ea, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&eb, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ea, (hipStream_t)a);
    if (e == hipSuccess) e = hipEventRecord(eb, (hipStream_t)b);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)a, eb, 0);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)b, ea, 0);
    if (ea) (void)hipEventDestroy(ea); /* released once the waits are satisfied */
    if (eb) (void)hipEventDestroy(eb);
    return e == hipSuccess ? OTC_OK : hip_fail(e, "stream join");
}

extern "C" void otc_stream_destroy(void *s)
{
    if (s) (void)hipStreamDestroy((hipStream_t)s);
}

/* ---- device memory helpers --------------------------------------------- */
extern "C" void *otc_dev_malloc(size_t nbytes)
{
    void *p = nullptr;
    hipError_t e = dev_alloc(&p, nbytes ? nbytes : 16);
    if (e != hipSuccess) {
        hip_fail(e, "hipMalloc");
        return nullptr;
    }
    return p;
}
extern "C" void otc_dev_free(void *p)
{
    if (p) (void)hipFree(p);
}
extern "C" int otc_memcpy(void *dst, const void *src, size_t nbytes, int kind)
{
    hipMemcpyKind k = kind == OTC_H2D ? hipMemcpyHostToDevice : kind == OTC_D2H ? hipMemcpyDeviceToHost
                                                                                : hipMemcpyDeviceToDevice;
    HIPCHK(hipMemcpy(dst, src, nbytes, k));
    return OTC_OK;
}
extern "C" int otc_memset(void *p, int v, size_t nbytes)
{
    HIPCHK(hipMemset(p, v, nbytes));
    return OTC_OK;
}
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

extern "C" int otc_time_op(otc_op_fn op, void *arg, int iters, double *ms_per_iter)
{
    if (!op) return set_err(OTC_ERR_ARG, "null op");
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(ev.a, nullptr));
    for (int i = 0; i < iters; ++i) {
        int r = op(arg);
        if (r) return r;
    }
    HIPCHK(hipEventRecord(ev.b, nullptr));
    HIPCHK(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
    if (ms_per_iter) *ms_per_iter = iters > 0 ? ms / iters : 0.0;
    return OTC_OK;
}

/* Held clock under `op`: the clock probe on its own non-blocking stream,
 * beside >= 0.3 s of back-to-back ops on the default stream. */
extern "C" int otc_measure_clock(otc_op_fn op, void *arg, double *ghz)
{
    if (!op || !ghz) return set_err(OTC_ERR_ARG, "null argument");
    double ms = 0.0;
    if (int r = otc_time_op(op, arg, 1, &ms)) return r;
    const int n = std::max(3, (int)(300.0 / std::max(ms, 1e-3)) + 1);
    struct Res {
        hipStream_t s = nullptr;
        uint64_t *d = nullptr;
        ~Res()
        {
            if (d) (void)hipFree(d);
            if (s) (void)hipStreamDestroy(s);
        }
    } R;
    HIPCHK(hipStreamCreateWithFlags(&R.s, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&R.d, 2 * sizeof(uint64_t)));
    HIPCHK(hipMemset(R.d, 0, 2 * sizeof(uint64_t)));
    if (int r = otc_clock_probe(R.d, 0.2 * n * ms * 1e-3, 0.6 * n * ms * 1e-3, R.s)) return r;
    for (int i = 0; i < n; ++i)
        if (int r = op(arg)) return r;
    HIPCHK(hipDeviceSynchronize());
    uint64_t h[2] = {0, 0};
    HIPCHK(hipMemcpy(h, R.d, sizeof h, hipMemcpyDeviceToHost));
    *ghz = h[1] ? 0.1 * (double)h[0] / (double)h[1] : 0.0;
    return OTC_OK;
}

/* ---- pinned host memory ------------------------------------------------- */
extern "C" int otc_host_register(void *p, size_t nbytes)
{
    HIPCHK(hipHostRegister(p, nbytes, hipHostRegisterDefault));
    return OTC_OK;
}
extern "C" int otc_host_unregister(void *p)
{
    HIPCHK(hipHostUnregister(p));
    return OTC_OK;
}
extern "C" void *otc_host_alloc_pinned(size_t nbytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, nbytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void otc_host_free_pinned(void *p)
{
    if (p) (void)hipHostFree(p);
}

extern "C" const char *otc_build_info(void)
{
    return "otc: MI355X (gfx950) cipher engine; kernels: aes_tt (LDS T-table), aes_bs (bitsliced VALU), "
           "rc4_multi, xor; runtime: pinned 3-stream pipeline, RCCL multi-GPU";
}

/* Which HIP runtime and RCCL this process actually runs on.  libotc.so links
 * libamdhip64.so.7 / librccl.so.1 by SONAME, and torch ships libraries with
 * the same SONAMEs: inside a torch process the library runs on torch's HIP
 * (7.0) and RCCL, in otbench and the CLIs on /opt/rocm's (7.2).  Every A/B
 * record carries this so the two are never compared unawares. */
extern "C" int otc_runtime_info(char *buf, size_t n)
{
    if (!buf || n == 0) return set_err(OTC_ERR_ARG, "null buffer");
    int rt = 0, drv = 0;
    if (hipRuntimeGetVersion(&rt) != hipSuccess) {
        (void)hipGetLastError();
        rt = -1;
    }
    if (hipDriverGetVersion(&drv) != hipSuccess) {
        (void)hipGetLastError();
        drv = -1;
    }
    int rccl = 0;
    if (ncclGetVersion(&rccl) != ncclSuccess) rccl = -1;
    std::string hip_path, rccl_path;
    if (FILE *f = fopen("/proc/self/maps", "r")) {
        char line[4096];
        while (fgets(line, sizeof line, f)) {
            char *p = strchr(line, '/');
            if (!p) continue;
            p[strcspn(p, "\n")] = 0;
            if (hip_path.empty() && strstr(p, "libamdhip64.so")) hip_path = p;
            if (rccl_path.empty() && strstr(p, "librccl.so")) rccl_path = p;
        }
        fclose(f);
    }
    const int w = snprintf(buf, n,
                           "{\"hip_runtime_version\": %d, \"hip_driver_version\": %d, \"rccl_version\": %d, "
                           "\"libamdhip64\": \"%s\", \"librccl\": \"%s\"}",
                           rt, drv, rccl, hip_path.c_str(), rccl_path.c_str());
    return w < 0 || (size_t)w >= n ? set_err(OTC_ERR_ARG, "buffer too small") : OTC_OK;
}
