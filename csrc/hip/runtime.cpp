/*
 * runtime.cpp -- what the ops run on, and the C API (otc.h) around them that
 * is not a cipher: the per-call workspace pool (otc_device.h ws_alloc /
 * ws_free) and the allocation fault injection in front of it, device info,
 * streams for C harnesses, device and pinned host memory, event timing and the
 * held-clock measurement, build and runtime info.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "otc.h"
#include "otc_device.h"
#include "engine_internal.h"

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
