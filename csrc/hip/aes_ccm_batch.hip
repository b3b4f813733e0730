/*
 * aes_ccm_batch.hip -- AES-CCM (NIST SP 800-38C, RFC 3610) over MANY short
 * records in one pass (otc_aes_ccm_batch): one key, one nonce length and one tag
 * length per batch, every record with its own nonce, its own AAD and its own tag.
 *
 * CCM's tag is a CBC-MAC: one serial chain per record, so the 16 or 64 lanes per
 * record of the other batched AEADs' hashes have nothing to share.  The only
 * parallelism is across records, and the shape is the segment chains' of
 * aes_tt.hip (seg_chain_g): ONE RECORD PER LANE on the LDS T-table rounds
 * (aes_tt_dev.h, the 128 KiB encryption image in both directions: CCM never
 * runs the inverse cipher), up to 1024 threads, one workgroup per CU.  A
 * record's CBC-MAC call and its counter-mode call are independent, so the lane
 * carries both through enc_rounds4_from<.., B = 2> and reads the data once.
 *
 *   MAC start   X = E(B0), then X = E(X ^ block) over the encoded AAD's blocks
 *               (ccm_dev.h ccm_aad_block: by bytes, any alignment).  The second
 *               call of these steps is the pad the lane needs first: S_0 to
 *               encrypt, S_1 to decrypt (ccm_ctr_first).
 *   data        bursts of CCM_BURST = 8 blocks, loaded back to back with plain
 *               (cached) 16-byte loads -- the next block of a lane sits in the
 *               line just read; with the non-temporal bit the segment chains fell
 *               from ~1115 to ~475 GB/s (aes_tt_dev.h) -- into a ring of eight
 *               registers.  A step takes the ring's head and appends its output,
 *               so after eight steps the ring holds the burst's output in order
 *               and is stored back to back.  The step loop is NOT unrolled: eight
 *               copies of two AES-256 blocks' rounds would not fit the
 *               instruction cache; the ring's 28 moves per step are what that
 *               costs.  Encryption, step j: E(X ^ P_j) and E(A_{j+1}).
 *               Decryption: the MAC takes the plaintext C_j ^ S_{j+1}, so the
 *               lane runs one block ahead -- E(X ^ P_j) travels with E(A_{j+2}),
 *               and the last step, with no block to prepare, makes S_0
 *               (ccm_ctr_of_step).  The last partial block is read and written
 *               by bytes inside the record, zero-padded for the MAC.
 *   tag         MSB_M(X ^ S_0).  Encryption stores it; decryption compares it
 *               with the expected one (OR of the XORs, no early exit), stores the
 *               verdict, and zeroes the tag row of a record that fails.
 *   wipe        the output of every record that failed is zeroed by the batched
 *               GCM's wipe kernel (aes_gcm_batch.hip), which reads the columns
 *               that otc_ccm_msg shares with otc_gcm_msg.
 *
 * Lane t takes record order[t]: the planner sorts the records by block count,
 * longest first (ccm_dev.h ccm_order_fill), so the lanes of a wave end together.
 * Consecutive waves of that order go to different workgroups (wave w to
 * workgroup w mod grid), so every CU gets records of every length.
 *
 * Nothing branches on, or addresses memory by, key material, data or MAC state
 * except the AES table lookups themselves (the T-table kernels' property,
 * docs/ARCHITECTURE.md); the branches are on lengths and on the call's shape.
 * Nothing reads or writes outside [in, in + n), [out, out + n), [aad, aad +
 * aad_bytes) and the arrays of the call.  A burst is read whole before any of it
 * is written, and by the same lane: in place is exact.  Every value is written
 * with ordinary vector stores.
 */
#include <hip/hip_runtime.h>

#include <cstddef>

#include "otc_device.h"
#include "otc_kernels.h"
#include "aes_tt_dev.h"
#include "ccm_dev.h"

using namespace otc_dev;

namespace {

constexpr int CB_THREADS = 1024;
constexpr int CB_G = (int)CCM_BURST;
constexpr uint32_t CB_WORDS = sizeof(otc_ccm_msg) / 8;
static_assert(sizeof(otc_ccm_msg) == sizeof(otc_gcm_msg) && offsetof(otc_ccm_msg, out) == offsetof(otc_gcm_msg, out) &&
                  offsetof(otc_ccm_msg, nbytes) == offsetof(otc_gcm_msg, nbytes),
              "the wipe kernel reads the columns otc_ccm_msg shares with otc_gcm_msg");
static_assert(OTC_CCM_BATCH_MAX_BYTES <= (1u << 20), "lengths and counters in 32 bits, the order's counting sort");

struct CcmParams {
    const uint64_t *msgs;
    const uint32_t *order;
    uint64_t nmsg;
    const uint8_t *nonces; /* nmsg x nonce_len */
    uint8_t *tags;         /* nmsg x tag_len */
    const uint8_t *expect; /* nmsg x tag_len, a decryption's */
    uint8_t *ok;           /* nmsg verdicts, a decryption's */
    uint32_t nonce_len, tag_len;
};

/* one record, both directions; t: the lane's place in the order */
template <int NR, bool DEC>
__device__ __forceinline__ void ccm_record(const CcmParams &P, const otc_aes_key &K, const uint32_t *tbl,
                                           const uint32_t (&lk)[4], uint64_t t)
{
    const bool live = t < P.nmsg; /* a lane past the last record runs record 0's start and touches nothing */
    const uint32_t m = live ? P.order[t] : 0u;
    const uint64_t *D = P.msgs + (uint64_t)m * CB_WORDS;
    const uint8_t *in = (const uint8_t *)D[0];
    uint8_t *out = (uint8_t *)D[1];
    const uint32_t nbytes = live ? (uint32_t)D[2] : 0u; /* <= 2^20 */
    const uint8_t *aad = (const uint8_t *)D[3];
    const uint32_t alen = live ? (uint32_t)D[4] : 0u; /* <= 2^16 */
    const uint32_t nfull = nbytes >> 4, r = nbytes & 15u, n = ccm_data_blocks(nbytes), nab = ccm_aad_blocks(alen);

    uint32_t nw[4] = {0, 0, 0, 0}, base[4];
    {
        const uint8_t *np = P.nonces + (uint64_t)m * P.nonce_len; /* any byte address */
#pragma unroll
        for (uint32_t i = 0; i < 13; ++i)
            if (i < P.nonce_len) nw[i >> 2] |= (uint32_t)np[i] << (8 * (i & 3u));
    }
    ccm_base(base, nw);
    const uint32_t fl = ccm_flags_ctr(P.nonce_len);

    /* ---- B0 and the AAD; beside them the first pad ---- */
    uint32_t X[4], S[4];
    ccm_block(X, base, ccm_flags_b0(alen != 0, P.tag_len, P.nonce_len), nbytes);
    {
        uint32_t A[4];
        ccm_block(A, base, fl, ccm_ctr_first(DEC, n));
#pragma unroll 1
        for (uint32_t k = 0; k <= nab; ++k) {
            uint32_t s[2][4];
            if (k) {
                uint32_t w[4];
                ccm_aad_block(w, aad, alen, k - 1u);
#pragma unroll
                for (int q = 0; q < 4; ++q) X[q] ^= w[q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) s[0][q] = X[q] ^ K.rk[q], s[1][q] = A[q] ^ K.rk[q];
            enc_rounds4_from<1, NR, 2>(tbl, lk, K, s);
#pragma unroll
            for (int q = 0; q < 4; ++q) X[q] = s[0][q], S[q] = s[1][q];
        }
    }

    /* ---- the data, a burst at a time ---- */
    const uint32_t mask[4] = {ccm_mask_word(r, 0), ccm_mask_word(r, 1), ccm_mask_word(r, 2), ccm_mask_word(r, 3)};
#pragma unroll 1
    for (uint32_t g0 = 0; g0 < n; g0 += CB_G) {
        uint4 cur[CB_G];
#pragma unroll
        for (int u = 0; u < CB_G; ++u)
            cur[u] = g0 + u < nfull ? ld_u4<false, true>(in + 16 * (uint64_t)(g0 + u)) : make_uint4(0, 0, 0, 0);
        const bool tail = r && nfull - g0 < (uint32_t)CB_G; /* g0 <= nfull: the partial block is this burst's */
        if (tail) {
            const uint8_t *tp = in + 16 * (uint64_t)nfull;
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t b = 0; b < 15; ++b)
                if (b < r) w[b >> 2] |= (uint32_t)tp[b] << (8 * (b & 3u));
#pragma unroll
            for (int u = 0; u < CB_G; ++u)
                if (nfull - g0 == (uint32_t)u) cur[u] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        const uint32_t cnt = n - g0 < (uint32_t)CB_G ? n - g0 : (uint32_t)CB_G;
#pragma unroll 1
        for (uint32_t u = 0; u < (uint32_t)CB_G; ++u) {
            uint4 res = make_uint4(0, 0, 0, 0);
            if (u < cnt) { /* the steps past a short last burst only turn the ring */
                const uint32_t j = g0 + u;
                uint32_t p[4] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w}, A[4], s[2][4];
                if constexpr (DEC) {
                    /* the plaintext; what lies past the record's end is zero for the MAC */
                    const bool part = j == nfull; /* only with r != 0 */
#pragma unroll
                    for (int q = 0; q < 4; ++q) p[q] = (p[q] ^ S[q]) & (part ? mask[q] : 0xFFFFFFFFu);
                }
                ccm_block(A, base, fl, ccm_ctr_of_step(DEC, j, n));
#pragma unroll
                for (int q = 0; q < 4; ++q) s[0][q] = X[q] ^ p[q] ^ K.rk[q], s[1][q] = A[q] ^ K.rk[q];
                enc_rounds4_from<1, NR, 2>(tbl, lk, K, s);
#pragma unroll
                for (int q = 0; q < 4; ++q) X[q] = s[0][q];
                if constexpr (DEC) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) S[q] = s[1][q];
                    res = make_uint4(p[0], p[1], p[2], p[3]);
                } else {
                    res = make_uint4(p[0] ^ s[1][0], p[1] ^ s[1][1], p[2] ^ s[1][2], p[3] ^ s[1][3]);
                }
            }
#pragma unroll
            for (int v = 0; v + 1 < CB_G; ++v) cur[v] = cur[v + 1];
            cur[CB_G - 1] = res;
        }
#pragma unroll
        for (int u = 0; u < CB_G; ++u)
            if (g0 + u < nfull) st_u4<false, true>(out + 16 * (uint64_t)(g0 + u), cur[u]);
        if (tail) {
            uint8_t *tp = out + 16 * (uint64_t)nfull;
            uint4 v = cur[0];
#pragma unroll
            for (int u = 1; u < CB_G; ++u)
                if (nfull - g0 == (uint32_t)u) v = cur[u];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t b = 0; b < 15; ++b)
                if (b < r) tp[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3u)));
        }
    }

    /* ---- the tag: X ^ S_0, its first tag_len bytes ---- */
    if (!live) return;
    uint32_t T[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) T[q] = X[q] ^ S[q];
    uint8_t *tg = P.tags + (uint64_t)m * P.tag_len;
    if constexpr (DEC) {
        /* the verdict is formed before anything is stored (the host also rejects expect overlapping the tags) */
        const uint8_t *e = P.expect + (uint64_t)m * P.tag_len;
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t b = 0; b < 16; ++b)
            if (b < P.tag_len) diff |= ((T[b >> 2] >> (8 * (b & 3u))) & 0xFFu) ^ (uint32_t)e[b];
        P.ok[m] = diff == 0 ? 1 : 0;
        /* the computed tag of a forged record is the valid tag of the forgery: not handed out */
        if (diff)
#pragma unroll
            for (int q = 0; q < 4; ++q) T[q] = 0;
    }
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b < P.tag_len) tg[b] = (uint8_t)(T[b >> 2] >> (8 * (b & 3u)));
}

/* One record per thread; the workgroup size is chosen at launch (a multiple of
 * 64 up to CB_THREADS), as for the segment chains (aes_tt.hip launch_seg): with
 * fewer records than CUs x CB_THREADS every CU still gets waves. */
template <int NR, bool DEC>
__global__ __launch_bounds__(CB_THREADS) void k_aes_ccm_batch(CcmParams P, otc_aes_key K)
{
    __shared__ __attribute__((aligned(16))) uint32_t tbl[2 * 256 * 64];
    const uint32_t nt = blockDim.x;
    if (nt == CB_THREADS)
        fill_tbl4<CB_THREADS>(tbl, g_tab.te0);
    else
        fill_tbl4(tbl, g_tab.te0, nt);
    __syncthreads();
    uint32_t lk[4];
    const uint32_t lane = threadIdx.x & 63u;
    tbl4_lane_consts(lane, lk);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = nt >> 6;
    /* wave w of the order goes to workgroup w mod grid */
    for (uint64_t w = blockIdx.x + (uint64_t)gridDim.x * wave; w * 64 < P.nmsg; w += (uint64_t)gridDim.x * nwaves)
        ccm_record<NR, DEC>(P, K, tbl, lk, w * 64 + lane);
}

/* the workgroup size for nmsg records on `cus` CUs */
inline uint32_t cb_threads(uint64_t nmsg, uint64_t cus)
{
    if (nmsg >= cus * CB_THREADS) return CB_THREADS;
    const uint64_t per = ((nmsg + cus - 1) / cus + 63) / 64 * 64;
    return (uint32_t)(per < 64 ? 64 : per);
}

} // namespace

/* ---- host entry points (otc_kernels.h) ------------------------------------- */
namespace otc_impl {

int ccm_batch_spans(uint64_t *spans, int max)
{
    const uint64_t s[] = {16,                                      /* a block, bytes */
                          CCM_BURST * 16,                          /* a lane's burst, bytes */
                          64,                                      /* a wave, records */
                          CB_THREADS,                              /* a workgroup, records */
                          (uint64_t)device_cus() * CB_THREADS};    /* the full grid's first step, records */
    const int n = (int)(sizeof s / sizeof s[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = s[i];
    return n;
}

hipError_t ccm_batch_run(const otc_ccm_msg *msgs, const uint32_t *order, uint64_t nmsg, const otc_aes_key &K, bool dec,
                         const uint8_t *nonces, int nonce_len, uint8_t *tags, int tag_len, const uint8_t *expect,
                         uint8_t *ok, hipStream_t st)
{
    CcmParams P{};
    P.msgs = (const uint64_t *)msgs;
    P.order = order;
    P.nmsg = nmsg;
    P.nonces = nonces;
    P.tags = tags;
    P.expect = expect;
    P.ok = ok;
    P.nonce_len = (uint32_t)nonce_len;
    P.tag_len = (uint32_t)tag_len;
    /* one workgroup per CU (the 128 KiB table image), wave-stride over the order */
    const uint64_t cus = (uint64_t)device_cus();
    const uint32_t nt = cb_threads(nmsg, cus);
    const uint64_t need = (nmsg + nt - 1) / nt;
    const dim3 grid((unsigned)(need < cus ? need : cus)), wg(nt);
    return with_rounds(K.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        if (dec) hipLaunchKernelGGL((k_aes_ccm_batch<NR, true>), grid, wg, 0, st, P, K);
        else hipLaunchKernelGGL((k_aes_ccm_batch<NR, false>), grid, wg, 0, st, P, K);
        return hipGetLastError();
    });
}

} // namespace otc_impl
