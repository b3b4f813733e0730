/*
 * engine_internal.h -- helpers shared by the host runtime translation units
 * (engine.cpp: errors, keys, the AES modes and the stream ops; aead.cpp:
 * GHASH, GCM, ChaCha20-Poly1305 and batched GCM; runtime.cpp: workspaces,
 * devices, streams, memory, timing; split.cpp: kernel choice and the claimed
 * runs; pipeline.cpp: host streaming engine and multi-GPU jobs).
 * Not part of the public C API (otc.h).
 */
#ifndef OTC_ENGINE_INTERNAL_H
#define OTC_ENGINE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <string>
#include <type_traits>
#include <vector>

#include "otc.h"
#include "otc_device.h"
#include "otc_kernels.h"

namespace otc_rt {

using otc_dev::Ctr128;

/* error message of the last failing call on this thread (otc_last_error) */
int set_err(int code, const std::string &msg);
std::string last_err();
int hip_fail(hipError_t e, const char *what);

using otc_dev::ctr_from_bytes;
Ctr128 ctr_add(Ctr128 c, uint64_t n, bool wrap64);
int check_key(const otc_aes_key *k, int dir);

/* ---- engine.cpp: what the AEAD ops share with the AES modes -------------- */
/* device buffers: non-null, 16-byte aligned, the same (where inplace_ok) or disjoint */
int check_bufs(const void *in, const void *out, size_t nbytes, bool inplace_ok, const char *what);
/* CTR with GCM's counter (the low 32 bits wrap): otc_aes_ctr32 without its roctx range */
int ctr32_run(const void *in, void *out, size_t nbytes, const otc_aes_key *k, const uint8_t ctr0[16], int impl,
              void *stream);
/* the kernel family of the calling thread's last AES call (otc_last_impl) */
void set_last_impl(int impl);

/* [a, a + n) and [b, b + n) intersect without being the same range */
inline bool partial_overlap(const void *a, const void *b, size_t n)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x != y && x < y + n && y < x + n;
}

/* v as 8 big-endian bytes */
inline void store_be64(uint8_t *p, uint64_t v)
{
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (56 - 8 * i));
}

/* the batched kernels' tile sizes in blocks; a batch's tile map: record m owns the nt tiles from t on (returns t + nt) */
inline bool check_tile_blocks(int tile_blocks) { return tile_blocks == 64 || tile_blocks == 128 || tile_blocks == 256; }
inline uint64_t tile_map_fill(uint32_t *tile_msg, uint64_t *tile_first, size_t m, uint64_t t, uint64_t nt)
{
    if (tile_first) tile_first[m] = t;
    if (tile_msg)
        for (uint64_t k = 0; k < nt; ++k) tile_msg[t + k] = (uint32_t)m;
    return t + nt;
}

/* ---- split.cpp: which kernels a call runs, and the claimed runs ---------- */
int check_impl(int impl);
/* CTR's choice (no split); ECB's and the decryptions' are made by job_run */
int pick_impl(int impl, int bits, size_t ctr_bytes);
/* a threshold variable: true and *out for a decimal number; unset or empty:
 * false; anything else: false too, and one line on stderr (the callers read
 * each variable once per process) */
bool env_u64(const char *name, uint64_t *out);
/* from these sizes the T-table runs as a persistent claim kernel */
size_t tt_ctr_persistent_min();
bool segenc_persistent(size_t nbytes, size_t nseg);

/* pick (impl, OTC_IMPL, size) and run one ECB / decryption call: the grid
 * T-table kernel, the persistent T-table kernel alone, the co-resident split
 * or the bitsliced claim kernel alone.  *ran: the kernels actually used. */
hipError_t job_run(const otc_impl::Job &job, int impl, hipStream_t st, int *ran);

/* a non-owning reference to a callable, for the span of one call (no
 * allocation, unlike std::function): launch(cl) enqueues the claim kernel,
 * launch(nullptr) the grid kernel */
struct LaunchRef {
    void *obj;
    hipError_t (*call)(void *, const otc_dev::SplitClaim *);
    template <class F>
    LaunchRef(F &&f)
        : obj((void *)&f),
          call([](void *o, const otc_dev::SplitClaim *cl) { return (*(std::remove_reference_t<F> *)o)(cl); })
    {
    }
    hipError_t operator()(const otc_dev::SplitClaim *cl) const { return call(obj, cl); }
};
/* A persistent T-table claim kernel by itself on the caller's stream: nunits
 * claim units, the first ones handed out; the grid kernel when there are
 * fewer than min_units or no memory for the counter. */
hipError_t claim_alone(uint64_t nunits, uint64_t min_units, hipStream_t st, LaunchRef launch);
/* destroy the pooled auxiliary streams of the split */
void aux_release_all();

/* roctx range for rocprofv3 --marker-trace (a no-op unless a tool is
 * attached): every public entry point is one named range. */
struct Range {
    explicit Range(const char *name) { roctxRangePushA(name); }
    ~Range() { roctxRangePop(); }
    Range(const Range &) = delete;
    Range &operator=(const Range &) = delete;
};

/* A stream with a hardware queue of its own: HIP maps ordinary streams onto
 * GPU_MAX_HW_QUEUES (4) pooled queues per device per process, so in a process
 * that also holds torch's, RCCL's and a profiler's streams a library stream can
 * share a queue with an unrelated one and its work waits behind that stream's
 * (barrier packets are processed in queue order).  A stream created with a CU
 * mask -- here all CUs -- always gets a dedicated queue. */
inline hipError_t dedicated_stream_create(hipStream_t *s)
{
    std::vector<uint32_t> mask((size_t)(otc_dev::device_cus() + 31) / 32, 0xFFFFFFFFu);
    return hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data());
}

/* hipMalloc behind the fault-injection hook */
inline hipError_t dev_alloc(void **p, size_t n)
{
    if (otc_dev::alloc_fault()) return hipErrorOutOfMemory;
    return hipMalloc(p, n);
}

} // namespace otc_rt

#define HIPCHK(expr)                                                  \
    do {                                                              \
        hipError_t _e = (expr);                                       \
        if (_e != hipSuccess) return otc_rt::hip_fail(_e, #expr);     \
    } while (0)

#define RCCLCHK(expr)                                                                               \
    do {                                                                                            \
        ncclResult_t _r = (expr);                                                                   \
        if (_r != ncclSuccess)                                                                      \
            return otc_rt::set_err(OTC_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(_r)); \
    } while (0)

#endif
