/*
 * split.cpp -- which kernels an AES call runs, and the claimed runs: the
 * co-resident T-table + bitsliced split of ECB and the parallel decryptions
 * (split_run), and a persistent T-table claim kernel by itself (claim_alone).
 * Both hand out work through a claim counter (otc_device.h SplitClaim); the
 * split also owns the pooled auxiliary streams its two halves run on.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "otc.h"
#include "otc_device.h"
#include "otc_kernels.h"
#include "engine_internal.h"

using otc_dev::SplitClaim;
using otc_impl::Job;

namespace {
/* a first submission on a new auxiliary queue (aux_take) */
__global__ void k_aux_noop() {}
/* the claim word's last value, for otc_split_stats (claim_snapshot) */
__global__ void k_claim_snapshot(unsigned long long *ctr, unsigned long long *host)
{
    const unsigned long long v = __hip_atomic_fetch_add(ctr, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
} // namespace

namespace otc_rt {

namespace {

/* OTC_IMPL_AUTO: the measured winner (docs/PERF.md).  CTR calls of >= 2 GiB
 * (AES-256: >= 1 GiB) run bitsliced, the thresholds below; smaller CTR calls
 * (the bitsliced grid needs ~768 workgroups to fill the chip, plus two table
 * kernels per call) take the T-table.  ECB, CBC / CFB decryption: the
 * co-resident split (split_run below) from SPLIT_MIN bytes, the T-table
 * below that.  Segment encryption: T-table kernels only (engine.cpp
 * seg_enc_run).  OTC_IMPL=ttable|bitslice|split overrides "auto" for the
 * whole process, each where it applies: "split" for ECB and the decryptions
 * only (CTR keeps its auto choice), no override for segment encryption
 * (T-table only). */
int env_impl()
{
    static const int env = [] {
        const char *e = getenv("OTC_IMPL");
        if (!e || !*e || !strcmp(e, "auto")) return OTC_IMPL_AUTO;
        if (!strcmp(e, "ttable")) return OTC_IMPL_TTABLE;
        if (!strcmp(e, "bitslice")) return OTC_IMPL_BITSLICE;
        if (!strcmp(e, "split")) return OTC_IMPL_SPLIT;
        /* an old or mistyped value (e.g. the removed "hybrid") must not
         * silently select a different kernel: say so once */
        fprintf(stderr, "otc: ignoring OTC_IMPL=%s (expected auto, ttable, bitslice or split)\n", e);
        return OTC_IMPL_AUTO;
    }();
    return env;
}

} // namespace

bool env_u64(const char *name, uint64_t *out)
{
    const char *v = getenv(name);
    if (!v || !*v) return false;
    /* digits only, to the end: strtoull alone turns "abc" into 0 -- for a
     * threshold, "every call" -- and takes "-1" and "12x" as numbers */
    char *end = nullptr;
    errno = 0;
    const unsigned long long r = strtoull(v, &end, 10);
    if (*v < '0' || *v > '9' || *end || errno == ERANGE) {
        fprintf(stderr, "otc: ignoring %s=%s (expected a decimal number): the default holds\n", name, v);
        return false;
    }
    *out = r;
    return true;
}

int pick_impl(int impl, int bits, size_t ctr_bytes)
{
    /* CTR has no split: "split" (per call, or OTC_IMPL=split set for the
     * whole process to get the ECB / decryption split) takes the auto choice
     * here.  The co-resident CTR split (bitsliced CTR claim + T-table CTR
     * claim kernels) lost to the bitsliced kernel alone on both HIP runtimes
     * -- AES-128 64 GiB 1600-1629 vs 1659-1669 GB/s, AES-256 16 GiB 1150-1220
     * vs 1222-1229, AES-256 64 GiB within +-2.5% -- and was removed in round
     * 6 (profiles/r6/ctr_split_rt/). */
    if (impl == OTC_IMPL_TTABLE || impl == OTC_IMPL_BITSLICE) return impl;
    const int env = impl == OTC_IMPL_SPLIT ? OTC_IMPL_AUTO : env_impl();
    if (env == OTC_IMPL_TTABLE || env == OTC_IMPL_BITSLICE) return env;
    /* measured crossover (profiles/r3/auto_impl/xover_after_round2_tables):
     * AES-128 2 GiB 1520 vs 1506 GB/s, 1 GiB 1353 vs 1360; AES-256 1 GiB
     * 1056 vs 1049.  AES-192 takes the AES-128 threshold (not measured at
     * 1 GiB; its margin lies between the two). */
    const size_t min_bs = bits == 256 ? ((size_t)1 << 30) : ((size_t)2 << 30);
    return ctr_bytes >= min_bs ? OTC_IMPL_BITSLICE : OTC_IMPL_TTABLE;
}

int check_impl(int impl)
{
    if (impl == OTC_IMPL_AUTO || impl == OTC_IMPL_TTABLE || impl == OTC_IMPL_BITSLICE || impl == OTC_IMPL_SPLIT)
        return OTC_OK;
    return set_err(OTC_ERR_ARG, "impl must be OTC_IMPL_AUTO, OTC_IMPL_TTABLE, OTC_IMPL_BITSLICE or OTC_IMPL_SPLIT");
}

namespace {

/* ---- co-resident T-table + bitsliced split (ECB, CBC / CFB decryption) -----
 * The T-table kernels are LDS-bound (80% of the LDS array's cycles, 224
 * lookups per AES-256 block, VALU a third busy) and leave power on the table:
 * 1.23-1.29 kW with the package power limit active ~55-60% of the time, where
 * the VALU-bound bitsliced kernels hold the ~1.37 kW cap (profiles/r4/power).
 * A T-table workgroup (1024 threads = 4 waves per SIMD at 78-85 VGPRs, 128 or
 * 160 KiB LDS) leaves room for one bitsliced wave per SIMD (152-168 VGPRs, no
 * LDS).  So both kernels run at once on every CU over ONE buffer -- each on
 * a pooled CU-masked stream with a hardware queue of its own (fork / join
 * events with the caller's stream, aux_take) -- and take 2048-block units from a shared
 * counter, the bitsliced kernel from the front and the T-table from the back
 * (otc_device.h SplitClaim), so they finish together on any box: no share to
 * tune, no tail where one kernel runs alone.  Measured: docs/PERF.md
 * "Round 4" (the static shares this replaced: profiles/r4/ecb_split,
 * dec_split, cfb_split). */
struct AuxStream {
    int dev = -1;
    hipStream_t s = nullptr, t = nullptr; /* the bitsliced / the T-table half */
    hipEvent_t fork = nullptr, join = nullptr, join_t = nullptr;
};

/* pooled per device: a call takes one (creating it on first use), enqueues,
 * and returns it, so concurrent callers (one host thread per GPU in
 * otc_multi_run) never share the events they order on */
std::mutex g_aux_mu;
std::vector<AuxStream> g_aux_free;
/* AuxStreams created per device (in the pool or taken).  Each holds two
 * dedicated hardware queues, so the pool is capped: past AUX_MAX concurrent
 * split calls on one device a call runs the T-table alone and records why
 * (otc_split_fallback_reason) instead of taking more device queues. */
constexpr int AUX_MAX = 4;
int g_aux_live[64];
thread_local const char *g_split_fallback = "";

hipError_t aux_take(int dev, AuxStream &out, bool warm)
{
    {
        std::lock_guard<std::mutex> lk(g_aux_mu);
        for (size_t i = 0; i < g_aux_free.size(); ++i)
            if (g_aux_free[i].dev == dev) {
                out = g_aux_free[i];
                g_aux_free.erase(g_aux_free.begin() + (long)i);
                return hipSuccess;
            }
        if (dev < 0 || dev >= 64 || g_aux_live[dev] >= AUX_MAX) {
            g_split_fallback = "auxiliary stream pool exhausted (AUX_MAX concurrent split calls on this device)";
            return hipErrorOutOfMemory;
        }
        ++g_aux_live[dev]; /* reserved; released below if creation fails */
    }
    AuxStream a;
    a.dev = dev;
    /* both halves on streams with an all-CU mask: HIP gives a CU-masked
     * stream a hardware queue of its own.  On pooled queues (4 per process
     * here) a library stream can share one with the caller's stream or with
     * the other half, and then the two kernels run one after the other: in
     * bench.py, beside torch's and RCCL's streams, the CTR split ran at the
     * T-table's speed (1534 GB/s) */
#ifdef OTC_DIAG_POOLED_AUX
    /* A/B arm only (make variant NAME=pooledaux VFLAGS=-DOTC_DIAG_POOLED_AUX):
     * both halves on plain non-blocking streams, i.e. HIP's pooled queues */
    hipError_t e = hipStreamCreateWithFlags(&a.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&a.t, hipStreamNonBlocking);
#else
    hipError_t e = dedicated_stream_create(&a.s);
    if (e == hipSuccess) e = dedicated_stream_create(&a.t);
#endif
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a.fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a.join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a.join_t, hipEventDisableTiming);
    /* A new AuxStream's one-time costs, paid here and not inside the first
     * split (whose T-table half is already queued when the bitsliced half
     * launches -- split_run): the bitsliced code object, and a first
     * submission on each queue.  Without this a process's first split ran
     * its halves one after the other (front 0 in 1 of 64 calls,
     * profiles/r6/coresidency/matrix.jsonl). */
    if (warm && e == hipSuccess && otc_impl::bs_preload() != hipSuccess)
        (void)hipGetLastError(); /* only a warm-up: the split works without it */
    /* not while the caller's stream is being captured into a graph: a
     * synchronisation there would invalidate the caller's capture */
    if (warm && e == hipSuccess) {
        hipLaunchKernelGGL(k_aux_noop, dim3(1), dim3(1), 0, a.s);
        hipLaunchKernelGGL(k_aux_noop, dim3(1), dim3(1), 0, a.t);
        if ((e = hipGetLastError()) == hipSuccess && (e = hipStreamSynchronize(a.s)) == hipSuccess)
            e = hipStreamSynchronize(a.t);
    }
    if (e != hipSuccess) {
        if (a.join_t) (void)hipEventDestroy(a.join_t);
        if (a.join) (void)hipEventDestroy(a.join);
        if (a.fork) (void)hipEventDestroy(a.fork);
        if (a.t) (void)hipStreamDestroy(a.t);
        if (a.s) (void)hipStreamDestroy(a.s);
        std::lock_guard<std::mutex> lk(g_aux_mu);
        --g_aux_live[dev];
        g_split_fallback = "auxiliary stream creation failed";
        return e;
    }
    out = a;
    return hipSuccess;
}

void aux_give(const AuxStream &a)
{
    std::lock_guard<std::mutex> lk(g_aux_mu);
    g_aux_free.push_back(a);
}

/* the smallest call that splits: 2 GiB.  Measured with the kernels truly
 * co-resident (round 5, profiles/r5/split_ab/remeasure_int_lds.jsonl,
 * split_thresholds/thresh2_int_lds.jsonl): against the grid T-table, AES-256
 * ECB wins 15% at 2 GiB, 24% at 4 and 64 GiB, CBC-dec 10% at 2 GiB and 21% at
 * 16 GiB, CFB-dec 26% at 16 GiB; at 1 GiB and below it is mixed (ECB 512 MiB
 * +3%, 1 GiB -13% on one box; CBC-dec 512 MiB -2%, 1 GiB +2%) and at 256 MiB
 * it loses 2-11%: each of the 4096 T-table waves then gets only one or two
 * 32 KiB units, and 256 x 128 KiB of LDS table fills plus the fork / join
 * are a fixed cost.  (Round 4's 896 MiB was measured while the halves ran one
 * after the other: docs/PERF.md round 5.) */
constexpr size_t SPLIT_MIN = (size_t)2 << 30;

int pick_ecb_impl(int impl, size_t nbytes)
{
    if (impl == OTC_IMPL_TTABLE || impl == OTC_IMPL_BITSLICE || impl == OTC_IMPL_SPLIT) return impl;
    const int env = env_impl();
    if (env != OTC_IMPL_AUTO) return env;
    return nbytes >= SPLIT_MIN ? OTC_IMPL_SPLIT : OTC_IMPL_TTABLE;
}

/* Segment decryption (CBC / CFB128 over independent segments of 2^shift
 * blocks, IV_s = iv0 + s): the same split, each kernel computing the segment
 * IVs itself.  Non-power-of-two segments and short calls: the T-table. */
int pick_seg_impl(int impl, size_t nbytes, size_t seg_blocks)
{
    if (otc_impl::seg_shift_of(seg_blocks) < 0) return OTC_IMPL_TTABLE;
    return pick_ecb_impl(impl, nbytes);
}

/* ---- the claim counter ----------------------------------------------------
 * Two words, stream-ordered on the caller's stream.  Word 0: the shared claim
 * word; word 1 (the bitsliced kernel alone): the T-table kernel's own word,
 * preset to "every unit taken".  nullptr: no memory (or the fault hook). */
unsigned long long *claim_counter_new(hipStream_t st)
{
    unsigned long long *ctr = nullptr;
    if (otc_dev::alloc_fault() || otc_dev::ws_alloc((void **)&ctr, 2 * sizeof *ctr, st) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return ctr;
}

/* word 0 zeroed; word 1 only where it is used (tt_word: the T-table's word,
 * all ones -- front + back far past nunits, so its claims fail;
 * hipMemsetD32Async at a 4-byte offset cost ~40 ms per call): one fill kernel
 * per call instead of two (no measurable rate change at 0.5-2 GiB,
 * profiles/r6/claim_tail/one_fill_ab.jsonl). */
hipError_t claim_counter_reset(unsigned long long *ctr, bool tt_word, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(ctr, 0, sizeof *ctr, st);
    return e != hipSuccess || !tt_word ? e : hipMemsetAsync(ctr + 1, 0xFF, sizeof *ctr, st);
}

/* the last units, handed to the T-table waves without a claim (otc_device.h
 * SplitClaim): 16 waves per workgroup, one workgroup per CU */
uint32_t preassigned_back(uint64_t nunits)
{
#ifndef OTC_CLAIM_NO_PREASSIGN /* A/B arm: every unit claimed (make variant VFLAGS=-DOTC_CLAIM_NO_PREASSIGN) */
    return (uint32_t)std::min<uint64_t>(nunits, 16ull * (uint64_t)otc_dev::device_cus());
#else
    (void)nunits;
    return 0;
#endif
}

/* Split accounting (otc_split_stats): off by default -- one relaxed load
 * per claimed call.  On, each claimed call copies its claim word back and
 * waits for it (a profiling mode), so the caller can read how many units each
 * side took. */
std::atomic<int> g_split_stats{0};
thread_local uint64_t g_split_word = 0, g_split_nunits = 0, g_split_ttwaves = 0, g_split_pb = 0;

/* after the kernels of a claimed call, on its stream; bs_only: the bitsliced
 * kernel took every unit (the T-table has its own word) */
hipError_t claim_snapshot(unsigned long long *ctr, uint64_t nunits, uint32_t pb, bool bs_only, hipStream_t st)
{
    if (!g_split_stats.load(std::memory_order_relaxed)) return hipSuccess;
    /* the counter's last value sits where the agent-scope atomics left it:
     * read it with one (an ordinary copy can see a stale line) into pinned
     * host memory */
    thread_local unsigned long long *snap = nullptr;
    if (!snap && hipHostMalloc((void **)&snap, sizeof *snap, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        snap = nullptr;
    }
    if (!snap) return hipSuccess;
    hipLaunchKernelGGL(k_claim_snapshot, dim3(1), dim3(1), 0, st, ctr, snap);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    g_split_word = bs_only ? nunits : *(volatile unsigned long long *)snap;
    g_split_nunits = nunits;
    /* every T-table claim kernel runs 1024-thread workgroups, one per CU;
     * each of their waves ends on one failed claim */
    g_split_ttwaves = bs_only ? 0 : 16ull * (uint64_t)otc_dev::device_cus();
    g_split_pb = pb; /* the T-table's units taken without a claim */
    return hipSuccess;
}

/* The claimed forms of ECB and the decryptions: the co-resident split, the
 * bitsliced claim kernel alone (impl "bitslice"), or the persistent T-table
 * claim kernel alone -- one workgroup per CU, its LDS table filled once,
 * units claimed until none are left.  auto runs the last for the T-table
 * calls of [896 MiB, 2 GiB): against the grid kernel ECB-256 1000 MiB 1089
 * vs 1039, ECB-dec 1073 vs 966, CBC-dec 1049 vs 1017 (round 4's "split", which
 * was this kernel alone: profiles/r4/claim_split/mid_sizes.jsonl); 1 GiB
 * ECB-256 1026 vs 988, AES-128 1282 vs 1238 (profiles/r5/split_thresholds/);
 * round 5 at 1000 MiB (midsize_persistent_vs_grid.jsonl, 2 reps): ECB-256
 * 1068-1074 vs 1027-1031, ECB-dec-256 1053-1056 vs 872-911, CBC / CFB-dec
 * +1%, ECB-128 +2-9%; 1.5 GiB -4..+7%; at 512 MiB and below it ties or
 * loses.  Round 6, with the first claim units handed out (no first-claim
 * queue): from 512 MiB -- ECB-128 512 / 768 MiB +2.8 / +3.7%, ECB-256 +4.4 /
 * +4.4%, ECB-dec-256 +2.8 / +5.5%, CBC-dec-128 -1 / +2.7%; at 256 MiB mixed
 * (-4..+1.5%) (profiles/r6/xover/). */
enum { FORM_SPLIT = 0, FORM_BS = 1, FORM_TT = 2 };
/* OTC_TT_PERSISTENT_MIN_MIB / OTC_SEGENC_PERSISTENT_MIN_MIB: threshold
 * sweeps, and how the suite reaches the persistent kernels at small sizes
 * (tests/test_gpu_claim_forms.py) (read once; unset = the measured defaults;
 * a value too large for size_t: never) */
size_t env_mib(const char *name, size_t dflt)
{
    uint64_t mib = 0;
    if (!env_u64(name, &mib)) return dflt;
    return mib > (SIZE_MAX >> 20) ? SIZE_MAX : (size_t)mib << 20;
}
int split_form(int picked, size_t nbytes)
{
    static const size_t tt_persistent_min = env_mib("OTC_TT_PERSISTENT_MIN_MIB", (size_t)512 << 20);
    if (picked == OTC_IMPL_SPLIT) return FORM_SPLIT;
    if (picked == OTC_IMPL_BITSLICE) return FORM_BS;
    return nbytes >= tt_persistent_min ? FORM_TT : -1;
}

/* The two-kernel split (FORM_SPLIT), or the bitsliced claim kernel alone
 * (FORM_BS: impl "bitslice"): tt_claim on one auxiliary stream and bs_claim
 * on the other, both over the whole buffer (nunits claim units, the T-table
 * kernel also runs what lies past the last unit).  Under FORM_BS the T-table
 * kernel's back counter starts full, so the bitsliced kernel (three
 * workgroups per CU, <= 168 VGPRs; one per CU beside the T-table: 4 T-table
 * waves + 1 bitsliced wave per SIMD) takes every unit and one T-table
 * workgroup runs the rest.  The grid T-table kernel alone (tt_run) where
 * there are too few units, no memory for the counter or no auxiliary stream.
 * *ran: the kernels actually used. */
hipError_t split_run(const Job &job, bool bs_only, hipStream_t st, int *ran)
{
    const uint64_t nunits = job.nblocks / otc_dev::CLAIM_UNIT;
    const unsigned bs_wgs = (unsigned)otc_dev::device_cus() * (bs_only ? 3u : 1u);
    *ran = OTC_IMPL_TTABLE;
    g_split_fallback = "";
    if (nunits < (bs_only ? 1u : 2u) || nunits > 0x7FFFFFFFull) {
        g_split_fallback = "too few claim units";
        return otc_impl::tt_run(job, job.nblocks, st);
    }
    unsigned long long *ctr = claim_counter_new(st);
    if (!ctr) {
        g_split_fallback = "no memory for the claim counter";
        return otc_impl::tt_run(job, job.nblocks, st);
    }
    int dev = 0;
    AuxStream a;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
        (void)hipGetLastError();
        cap = hipStreamCaptureStatusActive; /* unknown: take the safe side */
    }
    if (hipGetDevice(&dev) != hipSuccess || aux_take(dev, a, cap == hipStreamCaptureStatusNone) != hipSuccess) {
        /* no auxiliary stream: the T-table alone still gives the output */
        (void)hipGetLastError();
        (void)otc_dev::ws_free(ctr, st);
        return otc_impl::tt_run(job, job.nblocks, st);
    }
    /* first units handed out without a claim (otc_device.h SplitClaim): the
     * last ones to the T-table waves, the first ones to the bitsliced waves
     * (4 per workgroup) */
    const uint32_t pb = bs_only ? 0u : preassigned_back(nunits);
#ifndef OTC_CLAIM_NO_PREASSIGN
    const uint32_t pf = (uint32_t)std::min<uint64_t>(nunits - pb, 4ull * bs_wgs);
#else
    const uint32_t pf = 0;
#endif
    SplitClaim cl{ctr, (uint32_t)nunits, bs_wgs};
    cl.pf = pf;
    cl.pb = pb;
    SplitClaim cl_tt{bs_only ? ctr + 1 : ctr, (uint32_t)nunits, bs_only ? 1u : 0u};
    cl_tt.pf = bs_only ? 0u : pf;
    cl_tt.pb = pb;
    /* the counter, then fork: the aux streams start after everything queued
     * on st */
    hipError_t e;
    if ((e = claim_counter_reset(ctr, bs_only, st)) == hipSuccess && (e = hipEventRecord(a.fork, st)) == hipSuccess &&
        (e = hipStreamWaitEvent(a.s, a.fork, 0)) == hipSuccess && (e = hipStreamWaitEvent(a.t, a.fork, 0)) == hipSuccess &&
        (e = otc_impl::tt_claim(job, cl_tt, a.t)) == hipSuccess) {
        /* The T-table half is enqueued first on purpose: its 1024-thread,
         * 128-160 KiB-LDS workgroups fit one per CU only when they are placed
         * before the bitsliced ones (two or three 168-VGPR bitsliced
         * workgroups on one CU leave no room for a T-table workgroup there).
         * The bitsliced half's one-time costs (its code object, a first
         * submission on each auxiliary queue) are therefore paid when the
         * AuxStream is created (aux_take), not here: paid here, they let a
         * process's first split call run the T-table half alone (front 0,
         * profiles/r6/coresidency/matrix.jsonl; with the warm-up the first
         * call co-runs, matrix_warm_aux.jsonl).
         * The bitsliced half failing (no memory for its key table, its only
         * step before its launches) leaves the T-table claim kernel to take
         * what it can claim: units [pf, nunits) and the blocks past the last
         * unit -- none of the units under bs_only.  Units [0, pf) (bs_only:
         * every unit) were the bitsliced waves' and are still owed: the grid
         * kernel runs exactly those on st after the join, so no block is
         * enciphered twice when the call is in place (a prefix of a chain is
         * the same call, shorter; whole segments: one longer than a unit is
         * finished past the last owed unit, rewriting what the claim kernel
         * wrote there with the same bytes -- the decryptions read only the
         * input, never in place).  The join is recorded either way (a
         * failure after its launch must still be waited for). */
        const hipError_t eb = otc_impl::bs_claim(job, cl, a.s);
        if (eb != hipSuccess) {
            (void)hipGetLastError();
            g_split_fallback = "the bitsliced half failed to launch";
        }
        if ((e = hipEventRecord(a.join, a.s)) == hipSuccess && (e = hipEventRecord(a.join_t, a.t)) == hipSuccess &&
            (e = hipStreamWaitEvent(st, a.join, 0)) == hipSuccess)
            e = hipStreamWaitEvent(st, a.join_t, 0);
        if (e == hipSuccess) {
            if (eb == hipSuccess) *ran = bs_only ? OTC_IMPL_BITSLICE : OTC_IMPL_SPLIT;
            else if (const uint64_t owed = bs_only ? nunits : (uint64_t)pf)
                e = otc_impl::tt_run(job, owed * otc_dev::CLAIM_UNIT, st);
            if (e == hipSuccess) e = claim_snapshot(ctr, nunits, pb, bs_only, st);
        } else {
            /* no join on st: the counter must outlive both kernels */
            (void)hipStreamSynchronize(a.s);
            (void)hipStreamSynchronize(a.t);
        }
    }
    const hipError_t f = otc_dev::ws_free(ctr, st); /* after the join: both kernels are done with it */
    aux_give(a); /* reusable as soon as the work is enqueued: stream order */
    return e != hipSuccess ? e : f;
}

} // namespace

hipError_t claim_alone(uint64_t nunits, uint64_t min_units, hipStream_t st, LaunchRef launch)
{
    g_split_fallback = ""; /* not a split request: nothing to report if the grid kernel runs */
    if (nunits < min_units || nunits > 0x7FFFFFFFull) return launch(nullptr);
    unsigned long long *ctr = claim_counter_new(st);
    if (!ctr) return launch(nullptr);
    SplitClaim cl{ctr, (uint32_t)nunits, 0u};
    cl.pb = preassigned_back(nunits);
    hipError_t e = claim_counter_reset(ctr, false, st);
    if (e == hipSuccess) e = launch(&cl);
    if (e == hipSuccess) e = claim_snapshot(ctr, nunits, cl.pb, false, st);
    const hipError_t f = otc_dev::ws_free(ctr, st);
    return e != hipSuccess ? e : f;
}

/* CTR on the T-table: the persistent claim kernel from this size (A/B and
 * threshold sweeps: OTC_TT_CTR_PERSISTENT_MIN_MIB) */
size_t tt_ctr_persistent_min()
{
    static const size_t m = env_mib("OTC_TT_CTR_PERSISTENT_MIN_MIB", (size_t)512 << 20);
    return m;
}

/* Segment ENCRYPTION (CBC / CFB128, one serial chain per segment): T-table
 * kernels only, for every impl.  Two forms: the grid kernel, and the
 * persistent claim kernel (64-segment units from one counter, one workgroup
 * per CU, its LDS table filled once), from 2 GiB (from 1 GiB for segments <=
 * 1 KiB), where it beats the grid kernel by 4-15% (AES-256 4 KiB segments:
 * 2 GiB 1027 vs 986, 4 GiB 1040 vs 969, 32 GiB 1142 vs 995; 512 B at 1 GiB
 * 986 vs 951; AES-128 4 GiB 1383 vs 1267); below that the grid kernel (1 GiB
 * of 4 KiB segments: 916 vs 948; profiles/r5/split_thresholds/).  Round 6,
 * first claim units handed out: from 1 GiB for every segment size (AES-256
 * 4 KiB segments: 1 GiB 957-959 vs 948-950, 1.5 GiB 1036 vs 790-801 -- the
 * grid kernel's 384 workgroups there are 1.5 per CU; 512 MiB 542 vs 554-558;
 * profiles/r6/xover/).  A VALU
 * half for this mode (the row-sliced 8-chains-per-lane kernel of round 5)
 * lost at every size -- AES-256 4 GiB 775 vs 1040 GB/s for the claim kernel
 * alone (profiles/r5/split_ab/remeasure_int_lds.jsonl) -- and was removed
 * in round 6 (profiles/r6/retired/). */
bool segenc_persistent(size_t nbytes, size_t nseg)
{
    static const size_t min_bytes = env_mib("OTC_SEGENC_PERSISTENT_MIN_MIB", (size_t)1 << 30);
    return nbytes >= min_bytes && nseg / otc_dev::SEG_UNIT >= 16 && nseg / otc_dev::SEG_UNIT <= 0x7FFFFFFFull;
}

hipError_t job_run(const Job &job, int impl, hipStream_t st, int *ran)
{
    const size_t nbytes = (size_t)job.nblocks * 16;
    const bool seg = otc_impl::job_is_seg(job);
    *ran = seg ? pick_seg_impl(impl, nbytes, job.seg_blocks) : pick_ecb_impl(impl, nbytes);
    switch (seg && otc_impl::seg_shift_of(job.seg_blocks) < 0 ? -1 : split_form(*ran, nbytes)) {
    case FORM_SPLIT: return split_run(job, false, st, ran);
    case FORM_BS: return split_run(job, true, st, ran);
    case FORM_TT:
        return claim_alone(job.nblocks / otc_dev::CLAIM_UNIT, 2, st, [&](const SplitClaim *cl) {
            return cl ? otc_impl::tt_claim(job, *cl, st) : otc_impl::tt_run(job, job.nblocks, st);
        });
    default: return otc_impl::tt_run(job, job.nblocks, st);
    }
}

/* the auxiliary streams of the split (otc_release_resources) */
void aux_release_all()
{
    std::lock_guard<std::mutex> lk(g_aux_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (AuxStream &a : g_aux_free) {
        (void)hipSetDevice(a.dev);
        (void)hipStreamSynchronize(a.s);
        (void)hipStreamSynchronize(a.t);
        (void)hipEventDestroy(a.fork);
        (void)hipEventDestroy(a.join);
        (void)hipEventDestroy(a.join_t);
        (void)hipStreamDestroy(a.s);
        (void)hipStreamDestroy(a.t);
        if (a.dev >= 0 && a.dev < 64) --g_aux_live[a.dev];
    }
    g_aux_free.clear();
    (void)hipSetDevice(cur);
}

} // namespace otc_rt

using namespace otc_rt;

/* mode: 1 CTR, 0 ECB encryption, 2 decryption (ECB / CBC), 3 CFB decryption, 4 segment decryption
 * (power-of-two segments), 5 segment encryption (segments < 8 MiB) */
extern "C" int otc_pick_impl(int impl, int bits, int mode, uint64_t nbytes)
{
    if (check_impl(impl)) return -1;
    if (mode == 0 || mode == 2 || mode == 3 || mode == 4) return pick_ecb_impl(impl, (size_t)nbytes);
    if (mode == 5) return OTC_IMPL_TTABLE;
    if (mode == 1) return pick_impl(impl, bits, (size_t)nbytes);
    return -1;
}

/* which: 0 the T-table kernels' records, 1 the bitsliced (32-block) claim
 * kernels'; -1 in a build without OTC_SPLIT_TRACE */
extern "C" int otc_split_trace(int which, unsigned long long *buf, int max)
{
    if (!buf || max < 0) return set_err(OTC_ERR_ARG, "bad trace buffer");
    if (which != 0 && which != 1) return set_err(OTC_ERR_ARG, "which must be 0 (T-table) or 1 (bitsliced)");
    return which == 0 ? otc_impl::strace_read_tt(buf, max) : otc_impl::strace_read_bs(buf, max);
}

extern "C" const char *otc_split_fallback_reason(void) { return g_split_fallback; }

extern "C" void otc_split_stats(int on) { g_split_stats.store(on ? 1 : 0, std::memory_order_relaxed); }

extern "C" int otc_split_last_units(uint64_t *front, uint64_t *back, uint64_t *nunits)
{
    if (!front || !back || !nunits) return set_err(OTC_ERR_ARG, "null argument");
    /* every T-table wave ends on one failed back claim (+1 each), so the
     * back count less those, plus the units the T-table waves started on
     * without a claim, is what the T-table took; the front took the rest */
    const uint64_t b = g_split_word >> 32, n = g_split_nunits;
    *back = std::min(n, g_split_pb + (b > g_split_ttwaves ? b - g_split_ttwaves : 0));
    *front = n - *back;
    *nunits = n;
    return OTC_OK;
}
