/*
 * aes_gcm_batch.hip -- GHASH of MANY short records in one launch, and the
 * small kernels around it that make batched AES-GCM (otc_aes_gcm_batch) one
 * linear chain on one stream: prep (IVs -> counters and J0), the batched hash
 * with the tag finisher in it, and the wipe of records that failed.
 *
 * aes_gcm.hip spreads ONE message over the chip, level by level, and builds
 * its tables per call: 0.15 ms of fixed cost that a 4 KiB record cannot carry.
 * Here the unit is the record.  Record m hashes
 *
 *     pad16(AAD_m) || pad16(data_m) || [8 aad_bytes]_64 [8 nbytes]_64
 *
 * from y = 0: nb = ceil(aad/16) + ceil(n/16) + 1 blocks, the length block
 * formed in the kernel from the descriptor.  The decomposition, with L lanes
 * per record -- two instantiations, L = 16 and L = 64:
 *
 *   pass        L consecutive blocks of one record, one per lane.
 *   batch       GB_BATCH = 4 passes, loaded while the batch before it is
 *               multiplied.
 *   record      L lanes: 64 / L records per wave.  Lane j runs Horner under
 *               H^L over the record's blocks L apart, aligned to the END of
 *               the record (the short pass comes first; zero blocks in front
 *               change nothing): A_j = sum_k X_{j+Lk-pad} . (H^L)^(npass-1-k).
 *   workgroup   16 waves: 64 records (L = 16) or 16 (L = 64).  The lanes leave
 *               their accumulators in LDS; lane w of wave 0 folds record w's
 *               under H, Y = (sum_j A_j . H^(L-1-j)) . H -- one serial chain
 *               for all the group's records at once.  The chain starts at the
 *               first lane that any record of the group uses: a group of
 *               6-block records costs 6 steps, not L.  The same lane finishes
 *               the record: tag = Y ^ E_K(J0), and on decryption the verdict
 *               against the expected tag.
 *   grid        persistent workgroups, at most one per CU (128 KiB of tables
 *               in LDS), grid-stride over groups of records.
 *
 * Why two forms.  A record of nb blocks costs nb / L multiplications per lane
 * and then L + 1 serial ones in the fold, during which 15 of the 16 waves
 * wait.  With one wave per record (L = 64, aes_gcm.hip's shape) a 4 KiB record
 * is 5 multiplications against a fold of 65 -- and only 16 records share that
 * fold.  With L = 16 it is 17 against 17, shared by 64 records.  Long records
 * want L = 64: the serial chain of nb / L multiplications is then what a
 * group waits for.  Measured (docs/PERF.md "Batched AES-GCM"): L = 16 is 3.4x
 * faster at 1 KiB records, 1.8x at 4 KiB, 1.2x at 8 KiB; L = 64 is 1.3x faster
 * at 16 KiB.  The caller picks (otc_gcm_batch_lanes).
 *
 * The tables of H^16, H^64 and H (16 x 256 entries of 16 B per constant, see
 * aes_gcm.hip) come from a per-KEY image in device memory that
 * gcm_batch_tables builds once when a batch is planned; a workgroup copies
 * H^L and H to LDS.  gh_mul / gh_swap / gh_mulx, the table builder and the
 * bit order they keep are ghash_dev.h's, shared with aes_gcm.hip.
 *
 * Nothing here reads at or past the end of a record's data or AAD: whole
 * 16-byte loads only where 16 bytes are inside, bytes otherwise.  Every value
 * is written with ordinary vector stores.
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "aes.h"
#include "ghash_dev.h"
#include "otc_device.h"
#include "otc_kernels.h"

namespace otc_impl {

using otc_dev::ld_u4;

namespace {

constexpr uint32_t GB_BATCH = 4;                 /* passes loaded ahead */
constexpr uint32_t GB_WAVES = 16;                /* waves of a workgroup */
constexpr uint32_t GB_NTAB = 3;                  /* the per-key image: H^16, H^64, H */
constexpr uint32_t GB_ACC = GB_WAVES * 68;       /* accumulators: 64 records x 17 or 16 records x 65 */
constexpr uint32_t GB_LDS = (2 * GF_TAB + GB_ACC) * 16 + 64 * 4;
static_assert(GB_LDS <= 160 * 1024, "two tables, the accumulators and the fold starts must fit the CU's LDS");

typedef const __attribute__((address_space(1))) uint8_t *gptr8;

/* one record as the hash sees it */
struct GbRec {
    gptr8 data, aad;
    uint64_t nbytes, aad_bytes;
    uint64_t na, nd; /* blocks of the AAD and of the data */
};

/* the 16 bytes at p + off, those at or past `end` as zero; never reads them */
__device__ __forceinline__ uint4 gb_bytes(gptr8 p, uint64_t off, uint64_t end)
{
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t t = 0; t < 16; ++t) {
        const uint32_t v = off + t < end ? (uint32_t)p[off + t] : 0u;
        w[t >> 2] |= v << (8 * (t & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* block i (< na + nd + 1) of the record's hashed string */
__device__ __forceinline__ uint4 gb_block(const GbRec &R, uint64_t i)
{
    if (i < R.na) return gb_bytes(R.aad, i * 16, R.aad_bytes); /* any alignment: bytes */
    if (i < R.na + R.nd) {
        const uint64_t off = (i - R.na) * 16;
        if (off + 16 <= R.nbytes) return ld_u4<false, true>((const uint8_t *)R.data + off);
        return gb_bytes(R.data, off, R.nbytes);
    }
    const uint64_t ab = R.aad_bytes * 8, db = R.nbytes * 8; /* [8 aad]_64 [8 n]_64, big-endian */
    return make_uint4(__builtin_bswap32((uint32_t)(ab >> 32)), __builtin_bswap32((uint32_t)ab),
                      __builtin_bswap32((uint32_t)(db >> 32)), __builtin_bswap32((uint32_t)db));
}

struct GbParams {
    const otc_gcm_msg *msgs;
    uint64_t nmsg;
    const uint4 *tab;      /* [3][GF_TAB]: H^16, H^64, H */
    uint4 *out;            /* nmsg x 16: GHASH, or with ekj0 the tag (zero where ok[m] becomes 0) */
    const uint4 *ekj0;     /* nmsg x 16 or null */
    const uint8_t *expect; /* nmsg x tag_bytes or null (with ok) */
    uint8_t *ok;           /* nmsg verdicts or null */
    uint32_t tag_bytes;
    uint32_t hash_out;     /* hash the record's `out` (an encryption's ciphertext), else its `in` */
};

/* the passes kb .. kb + GB_BATCH - 1 of a record, one block per lane of its L */
template <uint32_t L>
__device__ __forceinline__ void gb_load(uint4 (&X)[GB_BATCH], const GbRec &R, uint32_t kb, uint32_t npass, uint64_t pad,
                                        uint32_t l)
{
#pragma unroll
    for (uint32_t i = 0; i < GB_BATCH; ++i) {
        const uint64_t v = (uint64_t)(kb + i) * L + l;
        X[i] = (kb + i < npass && v >= pad) ? gb_block(R, v - pad) : make_uint4(0, 0, 0, 0);
    }
}

/* L lanes per record (16 or 64), 64 / L records per wave */
template <uint32_t L>
__global__ __launch_bounds__(64 * GB_WAVES) void k_ghash_batch(GbParams P)
{
    constexpr uint32_t NREC = GB_WAVES * (64 / L); /* records of a workgroup */
    constexpr uint32_t STRIDE = L + 1;             /* accumulators of a record, padded off one bank */
    static_assert(NREC <= 64 && NREC * STRIDE <= GB_ACC, "one wave folds a workgroup's records");
    extern __shared__ __attribute__((aligned(16))) uint4 gb_lds[];
    uint4 *const TL = gb_lds, *const T1 = gb_lds + GF_TAB, *const acc = gb_lds + 2 * GF_TAB;
    uint32_t *const jst = (uint32_t *)(acc + GB_ACC);
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t rec = tid / L, l = tid % L; /* the record of the group this lane works on, and its lane there */
    const uint4 *gl = P.tab + (L == 16 ? 0 : GF_TAB), *g1 = P.tab + 2 * GF_TAB;
    for (uint32_t i = tid; i < GF_TAB; i += 64 * GB_WAVES) {
        TL[i] = ld_u4<false, true>(gl + i);
        T1[i] = ld_u4<false, true>(g1 + i);
    }
    __syncthreads();
    const uint64_t ngroups = (P.nmsg + NREC - 1) / NREC;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t m = g * NREC + rec;
        uint4 A = make_uint4(0, 0, 0, 0);
        uint32_t j0 = L; /* the first lane this record uses; L: none */
        if (m < P.nmsg) {
            const uint64_t *D = (const uint64_t *)(P.msgs + m);
            GbRec R;
            R.data = (gptr8)D[P.hash_out ? 1 : 0];
            R.nbytes = D[2];
            R.aad = (gptr8)D[3];
            R.aad_bytes = D[4];
            R.na = (R.aad_bytes + 15) >> 4;
            R.nd = (R.nbytes + 15) >> 4;
            const uint64_t nb = R.na + R.nd + 1;
            const uint32_t npass = (uint32_t)((nb + L - 1) / L);
            const uint64_t pad = (uint64_t)npass * L - nb; /* zero blocks in front, < L */
            j0 = npass > 1 ? 0u : (uint32_t)pad;
            uint4 X[GB_BATCH], N[GB_BATCH];
            gb_load<L>(X, R, 0, npass, pad, l);
            for (uint32_t kb = 0; kb < npass; kb += GB_BATCH) {
                /* the next batch's loads are in flight during this one's multiplications */
                gb_load<L>(N, R, kb + GB_BATCH, npass, pad, l);
#pragma unroll
                for (uint32_t i = 0; i < GB_BATCH; ++i)
                    if (kb + i < npass) A = xor4(gh_mul(TL, A), X[i]);
#pragma unroll
                for (uint32_t i = 0; i < GB_BATCH; ++i) X[i] = N[i];
            }
        }
        acc[rec * STRIDE + l] = A;
        if (l == 0) jst[rec] = j0;
        __syncthreads();
        if (wave == 0) {
            /* the first lane any record of the group uses: leading zero accumulators change nothing */
            uint32_t js = lane < NREC ? jst[lane] : L;
#pragma unroll
            for (uint32_t o = 32; o; o >>= 1) js = min(js, (uint32_t)__shfl_xor((int)js, (int)o));
            js = min(js, L - 1);
            const uint64_t fm = g * NREC + lane; /* the record whose accumulators this lane folds */
            if (lane < NREC && fm < P.nmsg) {
                const uint4 *a = acc + lane * STRIDE;
                uint4 Y = a[js];
                for (uint32_t j = js + 1; j < L; ++j) Y = xor4(gh_mul(T1, Y), a[j]);
                Y = gh_mul(T1, Y);
                if (P.ekj0) Y = xor4(Y, ld_u4<false, true>(P.ekj0 + fm));
                if (P.ok) {
                    /* the kept bytes against the expected tag: OR of the XORs, no early exit.  The
                     * verdict is formed BEFORE anything is stored, so the expected bytes are never
                     * this kernel's own output (the host also rejects expect overlapping out) */
                    const uint32_t w[4] = {Y.x, Y.y, Y.z, Y.w};
                    const uint8_t *e = P.expect + fm * P.tag_bytes;
                    uint32_t diff = 0;
#pragma unroll
                    for (uint32_t t = 0; t < 16; ++t)
                        if (t < P.tag_bytes) diff |= ((w[t >> 2] >> (8 * (t & 3))) & 0xFFu) ^ (uint32_t)e[t];
                    P.ok[fm] = diff == 0 ? 1 : 0;
                    /* the computed tag of a forged record is the valid tag of the forgery: not handed out */
                    if (diff) Y = make_uint4(0, 0, 0, 0);
                }
                P.out[fm] = Y;
            }
        }
        __syncthreads();
    }
}

/* one thread per record: the CTR half's counter IV || 00000002 into its
 * descriptor (words 3 and 4 of an otc_ctr_msg) and J0 = IV || 00000001 */
__global__ __launch_bounds__(256) void k_gcm_batch_prep(const uint8_t *ivs, uint64_t nmsg, uint64_t *ctr_msgs, uint4 *j0)
{
    const uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= nmsg) return;
    uint32_t b[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) b[i] = ivs[m * 12 + i];
    uint64_t hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) hi = (hi << 8) | b[i];
    const uint64_t top = ((uint64_t)b[8] << 24) | (b[9] << 16) | (b[10] << 8) | b[11];
    ctr_msgs[m * (sizeof(otc_ctr_msg) / 8) + 3] = hi;
    ctr_msgs[m * (sizeof(otc_ctr_msg) / 8) + 4] = (top << 32) | 2u;
    j0[m] = make_uint4(b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24),
                       b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24), 0x01000000u);
}

/* one wave per record: zero the nbytes of output of every record that failed.
 * Serves both batched AEADs (otc_kernels.h batch_wipe): a descriptor is six
 * 64-bit words with `out` in word 1 and `nbytes` in word 2 */
constexpr uint32_t WIPE_WAVES = 4;
constexpr uint32_t WIPE_WORDS = 6;
static_assert(sizeof(otc_gcm_msg) == 8 * WIPE_WORDS && sizeof(otc_chacha_msg) == 8 * WIPE_WORDS &&
                  offsetof(otc_gcm_msg, out) == 8 && offsetof(otc_chacha_msg, out) == 8 &&
                  offsetof(otc_gcm_msg, nbytes) == 16 && offsetof(otc_chacha_msg, nbytes) == 16,
              "the wipe reads the columns the two descriptors share");
__global__ __launch_bounds__(64 * WIPE_WAVES) void k_batch_wipe(const uint64_t *msgs, uint64_t nmsg, const uint8_t *ok)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * WIPE_WAVES;
    for (uint64_t m = (uint64_t)blockIdx.x * WIPE_WAVES + (threadIdx.x >> 6); m < nmsg; m += stride) {
        if (ok[m]) continue;
        uint8_t *out = (uint8_t *)msgs[m * WIPE_WORDS + 1];
        const uint64_t n = msgs[m * WIPE_WORDS + 2], nfull = n >> 4;
        for (uint64_t i = lane; i < nfull; i += 64) *(uint4 *)(out + i * 16) = make_uint4(0, 0, 0, 0);
        if (lane < (n & 15u)) out[nfull * 16 + lane] = 0;
    }
}

/* the opt-in above 64 KiB of dynamic LDS, once per device */
hipError_t gb_opt_in()
{
    static_assert(GB_LANES_SHORT == 16 && GB_LANES_LONG == 64, "the two instantiations below");
    return otc_dev::lds_opt_in<k_ghash_batch<16>, k_ghash_batch<64>>(GB_LDS);
}

} // namespace

int gcm_batch_spans(uint64_t *spans, int max)
{
    const uint64_t all[] = {GB_LANES_SHORT,            /* a pass of the 16-lane form: one block per lane of a record */
                            GB_LANES_LONG,             /* its batch of passes, and a pass of the 64-lane form */
                            GB_BATCH * GB_LANES_LONG}; /* a batch of passes of the 64-lane form */
    static_assert(GB_BATCH * GB_LANES_SHORT == GB_LANES_LONG, "the middle span is both");
    const int n = (int)(sizeof all / sizeof all[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = all[i];
    return n;
}

size_t gcm_batch_table_bytes() { return (size_t)GB_NTAB * GF_TAB * 16; }

hipError_t gcm_batch_tables(const uint8_t h[16], void *tab, hipStream_t st)
{
    /* here, not at the first run: a run may be inside a stream capture */
    hipError_t e = gb_opt_in();
    if (e != hipSuccess) return e;
    GfConsts<GB_NTAB> K{}; /* H^16, H^64, H */
    uint8_t c[16];
    memcpy(c, h, 16);
    memcpy(&K.c[2], c, 16);
    for (int i = 0; i < 4; ++i) aes_gf128_mul(c, c, c); /* H^16 */
    memcpy(&K.c[0], c, 16);
    for (int i = 0; i < 2; ++i) aes_gf128_mul(c, c, c); /* H^64 */
    memcpy(&K.c[1], c, 16);
    hipLaunchKernelGGL(k_gf128_tables<GB_NTAB>, dim3(GB_NTAB * 16), dim3(256), 0, st, K, (uint4 *)tab);
    return hipGetLastError();
}

hipError_t ghash_batch_run(const otc_gcm_msg *msgs, uint64_t nmsg, const void *tab, void *out16, const void *ekj0,
                           const uint8_t *expect, int tag_bytes, uint8_t *ok, bool hash_out, int lanes, hipStream_t st)
{
    if (lanes != GB_LANES_SHORT && lanes != GB_LANES_LONG) return hipErrorInvalidValue;
    hipError_t e = gb_opt_in();
    if (e != hipSuccess) return e;
    GbParams P{};
    P.msgs = msgs;
    P.nmsg = nmsg;
    P.tab = (const uint4 *)tab;
    P.out = (uint4 *)out16;
    P.ekj0 = (const uint4 *)ekj0;
    P.expect = ok ? expect : nullptr;
    P.ok = ok;
    P.tag_bytes = (uint32_t)tag_bytes;
    P.hash_out = hash_out ? 1u : 0u;
    const uint64_t nrec = (uint64_t)GB_WAVES * (64 / (unsigned)lanes); /* records of a workgroup */
    const uint64_t ngroups = (nmsg + nrec - 1) / nrec, cus = (uint64_t)otc_dev::device_cus();
    const dim3 g((unsigned)(ngroups < cus ? ngroups : cus)), b(64 * GB_WAVES);
    if (lanes == GB_LANES_SHORT)
        hipLaunchKernelGGL(k_ghash_batch<16>, g, b, GB_LDS, st, P);
    else
        hipLaunchKernelGGL(k_ghash_batch<64>, g, b, GB_LDS, st, P);
    return hipGetLastError();
}

hipError_t gcm_batch_prep(const uint8_t *ivs, uint64_t nmsg, otc_ctr_msg *ctr_msgs, void *j0, hipStream_t st)
{
    static_assert(sizeof(otc_ctr_msg) == 48, "k_gcm_batch_prep writes words 3 and 4 of 6");
    hipLaunchKernelGGL(k_gcm_batch_prep, dim3((unsigned)((nmsg + 255) / 256)), dim3(256), 0, st, ivs, nmsg,
                       (uint64_t *)ctr_msgs, (uint4 *)j0);
    return hipGetLastError();
}

hipError_t batch_wipe(const void *msgs, uint64_t nmsg, const uint8_t *ok, hipStream_t st)
{
    const uint64_t want = (nmsg + WIPE_WAVES - 1) / WIPE_WAVES, cap = (uint64_t)otc_dev::device_cus() * 8;
    hipLaunchKernelGGL(k_batch_wipe, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * WIPE_WAVES), 0, st,
                       (const uint64_t *)msgs, nmsg, ok);
    return hipGetLastError();
}

} // namespace otc_impl
