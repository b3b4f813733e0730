/*
 * aes_gcm_mk_batch.hip -- batched AES-GCM with a KEY PER RECORD
 * (otc_aes_gcm_mk_batch, "mk": many keys): record m is SP 800-38D GCM under
 * (keys[key_m], iv[m], aad[m]).  aes_gcm_batch.hip holds a whole batch to one key
 * because its positional hash tables are 64 KiB per constant; here the hash
 * multiplies on 256-byte NIBBLE TABLES, as aes_gcm_siv_batch.hip's does, and
 * reaches GHASH through RFC 8452 appendix A:
 *
 *   GHASH(H, X_1 .. X_n) = ByteReverse(POLYVAL(mulX_POLYVAL(ByteReverse(H)),
 *                                              ByteReverse(X_1), .., ByteReverse(X_n)))
 *
 * A GCM key lives for many records, so what the GCM-SIV batch pays per record --
 * log2 L squarings of 32 LDS steps each to get the tables of H^(2^s) -- is paid
 * here once per KEY, and a record only copies its key's tables.  Three kernels:
 *
 *   k_gmk_tables      once per plan and on rekey: per key, H = E_K(0^128) on the
 *                     constant tables in global memory (ocb_dev.h), the POLYVAL
 *                     key C_0 = mulX(ByteReverse(H)), its dot-powers C_s = C_0^(2^s),
 *                     s = 0 .. 6, by squaring, and the nibble tables of all seven
 *                     into the key's image: 7 x 256 B = 1792 B per key.  Sixteen
 *                     lanes per key, one table entry each; every lane squares
 *                     redundantly.
 *   k_ghash_mk_batch  S_m = GHASH_{H(key_m)}(pad16(AAD) || pad16(data) || [8 aad]_64
 *                     [8 n]_64), L lanes per record, L = 16 (four records per wave,
 *                     polyval_batch_dev.h sb_place) or 64 (one wave per record).
 *                     k_polyval_batch's decomposition -- lane j runs Horner under
 *                     H^L over the record's blocks L apart, aligned to the END of
 *                     the record; log2 L fold steps across lanes; a last product
 *                     by H -- with two differences: the record's lanes COPY the
 *                     tables of H^(2^s), s = 0 .. log2 L, from the key's image to the
 *                     record's LDS slot with 16-byte loads (the 16-lane form takes
 *                     the image's first five), and every block enters
 *                     byte-reversed, the result leaves byte-reversed.
 *   k_gmk_final       one lane per record: tag = S_m ^ E_{K_m}(J0_m), the schedule
 *                     read from keys[key_m]; on decryption the verdict over the
 *                     first tag_bytes bytes (OR of the XORs, no early exit) and a
 *                     zero tag row where it fails.
 *
 * The rest of the chain is aes_gcm_batch.hip's prep and wipe and the batched CTR
 * kernel (aes_tt.hip), which has always taken a key index per message.
 *
 * A record never leaves its wave: no workgroup barrier, no accumulator array.
 * LDS per workgroup of 4 waves: 16 records x 5 tables x 256 B = 20 KiB (L = 16),
 * 4 x 7 x 256 B = 7 KiB (L = 64).
 *
 * Nothing here reads at or past the end of a record's data or AAD: whole
 * 16-byte loads only where 16 bytes are inside, bytes otherwise.  The table
 * image and the schedule array are KEY MATERIAL.  Every value is written with
 * ordinary vector stores.
 */
#include <hip/hip_runtime.h>

#include <cstddef>

#include "otc_device.h"
#include "otc_kernels.h"
#include "aes_tt_dev.h"
#include "ocb_dev.h"
#include "polyval_batch_dev.h"

using namespace otc_dev;

namespace otc_impl {

namespace {

static_assert(sizeof(otc_gcm_mk_msg) == 48 && offsetof(otc_gcm_mk_msg, key) == 40, "the kernels read word 5 as the key index");
static_assert(GMK_NTAB == 7, "the tables of C^(2^s) up to s = log2 64");

constexpr uint32_t GMK_IMAGE = GMK_NTAB * 16; /* a key's image in table entries of 16 bytes */

__device__ __forceinline__ uint4 gmk_rev(uint4 v)
{
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    pv_rev(w, w);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* ---- the per-key tables -------------------------------------------------------- */
constexpr uint32_t GMK_TAB_KEYS = 4; /* keys of a workgroup of one wave: 16 lanes each */

template <int NR>
__global__ __launch_bounds__(64) void k_gmk_tables(const otc_aes_key *keys, uint64_t nkeys, uint4 *tab)
{
    __shared__ __attribute__((aligned(16))) uint4 lds[GMK_TAB_KEYS * GMK_IMAGE];
    const uint32_t kw = threadIdx.x >> 4, l = threadIdx.x & 15u;
    const uint64_t k = (uint64_t)blockIdx.x * GMK_TAB_KEYS + kw;
    const bool live = k < nkeys;
    uint4 *const T = lds + kw * GMK_IMAGE;
    /* a key past the end runs along with C = 0 and stores nothing */
    uint32_t c[4] = {0, 0, 0, 0};
    if (live) {
        uint32_t h[4] = {0, 0, 0, 0};
        enc_block_global<NR>(keys[k], h);
        gmk_key(c, h);
    }
    uint4 C = make_uint4(c[0], c[1], c[2], c[3]);
#pragma unroll 1
    for (uint32_t s = 0; s < GMK_NTAB; ++s) {
        const uint32_t cw[4] = {C.x, C.y, C.z, C.w};
        uint32_t e[4];
        pv4_entry(e, cw, l);
        const uint4 E = make_uint4(e[0], e[1], e[2], e[3]);
        T[s * 16 + l] = E;
        if (live) tab[k * GMK_IMAGE + s * 16 + l] = E;
        sb_wave_sync();
        if (s + 1 < GMK_NTAB) C = sb_mul(T + s * 16, C);
    }
}

/* ---- the batched hash ---------------------------------------------------------- */
struct GmkParams {
    const otc_gcm_mk_msg *msgs;
    uint64_t nmsg;
    const uint4 *tab;  /* nkeys x GMK_IMAGE entries: the keys' table images */
    uint4 *s;          /* nmsg x 16: GHASH of record m, in GCM's byte order */
    uint32_t hash_out; /* hash the record's `out` (an encryption's ciphertext), else its `in` */
};

/* block i (< na + nd + 1) of the record's hashed string, byte-reversed */
__device__ __forceinline__ uint4 gmk_block(const SbRec &R, uint64_t i)
{
    if (i < R.na + R.nd) return gmk_rev(sb_text_block(R, i));
    uint32_t x[4];
    gmk_len_block(x, R.aad_bytes, R.nbytes);
    return make_uint4(x[0], x[1], x[2], x[3]);
}

/* the passes kb .. kb + SB_BATCH - 1 of a record, one block per lane of its L */
template <uint32_t L>
__device__ __forceinline__ void gmk_load(uint4 (&X)[SB_BATCH], const SbRec &R, uint32_t kb, uint32_t npass, uint64_t pad,
                                         uint32_t l)
{
#pragma unroll
    for (uint32_t i = 0; i < SB_BATCH; ++i) {
        const uint64_t v = (uint64_t)(kb + i) * L + l;
        X[i] = (kb + i < npass && v >= pad) ? gmk_block(R, v - pad) : make_uint4(0, 0, 0, 0);
    }
}

/* L lanes per record (16 or 64), 64 / L records per wave */
template <uint32_t L>
__global__ __launch_bounds__(SB_THREADS) void k_ghash_mk_batch(GmkParams P)
{
    constexpr uint32_t LOG = L == 16 ? 4 : 6; /* fold steps; the tables are those of C^(2^s), s = 0 .. LOG */
    constexpr uint32_t NT = LOG + 1, NREC = SB_THREADS / L;
    static_assert(NT <= GMK_NTAB, "a record copies the front of its key's image");
    __shared__ __attribute__((aligned(16))) uint4 tab[NREC * NT * 16];
    const uint32_t tid = threadIdx.x;
    uint32_t rec, l; /* the record of the group this lane works on, and its lane there */
    sb_thread<L>(tid, rec, l);
    uint4 *const T = tab + rec * NT * 16;
    const uint64_t ngroups = (P.nmsg + NREC - 1) / NREC;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t m = g * NREC + rec;
        const bool live = m < P.nmsg;
        const uint64_t *D = (const uint64_t *)(P.msgs + m);
        /* the record's lanes copy its key's tables; a record past the end runs along on
         * zero tables (entry 0 of a table is zero, and its accumulator stays zero) */
        const uint4 *G = live ? P.tab + D[5] * GMK_IMAGE : nullptr;
#pragma unroll
        for (uint32_t i = l; i < NT * 16; i += L) T[i] = live ? ld_u4<false, true>(G + i) : make_uint4(0, 0, 0, 0);
        sb_wave_sync();
        uint4 A = make_uint4(0, 0, 0, 0);
        if (live) {
            const SbRec R = sb_record(D, P.hash_out);
            const uint64_t nb = R.na + R.nd + 1;
            const uint32_t npass = (uint32_t)((nb + L - 1) / L);
            const uint64_t pad = (uint64_t)npass * L - nb; /* zero blocks in front, < L */
            const uint4 *TL = T + LOG * 16;
            uint4 X[SB_BATCH], N[SB_BATCH];
            gmk_load<L>(X, R, 0, npass, pad, l);
            for (uint32_t kb = 0; kb < npass; kb += SB_BATCH) {
                /* the next batch's loads are in flight during this one's multiplications */
                gmk_load<L>(N, R, kb + SB_BATCH, npass, pad, l);
#pragma unroll
                for (uint32_t i = 0; i < SB_BATCH; ++i)
                    if (kb + i < npass) A = sb_xor(sb_mul(TL, A), X[i]);
#pragma unroll
                for (uint32_t i = 0; i < SB_BATCH; ++i) X[i] = N[i];
            }
        }
        /* the fold: after the step with d, lane j (a multiple of 2 d) holds
         * sum_{i < 2 d} A_{j+i} . C^(2 d - 1 - i); the other lanes' values are not used */
#pragma unroll 1
        for (uint32_t s = 0; s < LOG; ++s) {
            const uint4 B = sb_from_lane<L>(A, rec, l, 1u << s);
            A = sb_xor(sb_mul(T + s * 16, A), B);
        }
        A = sb_mul(T, A);
        if (live && l == 0) P.s[m] = gmk_rev(A);
        sb_wave_sync(); /* the next group's tables overwrite these */
    }
}

/* ---- the finisher -------------------------------------------------------------- */
template <int NR>
__global__ __launch_bounds__(64) void k_gmk_final(const otc_gcm_mk_msg *msgs, const otc_aes_key *keys, const uint4 *j0,
                                                  const uint4 *s, uint64_t nmsg, uint4 *tags, const uint8_t *expect,
                                                  uint32_t tag_bytes, uint8_t *ok)
{
    const uint64_t m = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (m >= nmsg) return;
    const uint4 J = j0[m], S = s[m];
    uint32_t y[4] = {J.x, J.y, J.z, J.w};
    enc_block_global<NR>(keys[((const uint64_t *)(msgs + m))[5]], y);
    y[0] ^= S.x;
    y[1] ^= S.y;
    y[2] ^= S.z;
    y[3] ^= S.w;
    if (ok) {
        /* the kept bytes against the expected tag: OR of the XORs, no early exit.  The verdict is
         * formed BEFORE anything is stored (the host also rejects expect overlapping tags or ok) */
        const uint8_t *e = expect + m * tag_bytes;
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t t = 0; t < 16; ++t)
            if (t < tag_bytes) diff |= ((y[t >> 2] >> (8 * (t & 3))) & 0xFFu) ^ (uint32_t)e[t];
        ok[m] = diff == 0 ? 1 : 0;
        /* the computed tag of a forged record is the valid tag of the forgery: not handed out */
        if (diff) y[0] = y[1] = y[2] = y[3] = 0;
    }
    tags[m] = make_uint4(y[0], y[1], y[2], y[3]);
}

} // namespace

/* ---- host entry points (otc_kernels.h) ------------------------------------- */
int gcm_mk_batch_spans(uint64_t *spans, int max)
{
    const uint64_t all[] = {GMK_LANES_SHORT,            /* a pass of the 16-lane form: one block per lane of a record */
                            GMK_LANES_LONG,             /* its batch of passes, and a pass of the 64-lane form */
                            SB_BATCH * GMK_LANES_LONG}; /* a batch of passes of the 64-lane form */
    static_assert(SB_BATCH * GMK_LANES_SHORT == GMK_LANES_LONG, "the middle span is both");
    const int n = (int)(sizeof all / sizeof all[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = all[i];
    return n;
}

size_t gcm_mk_batch_table_bytes(size_t nkeys) { return nkeys * (size_t)GMK_IMAGE * 16; }

hipError_t gcm_mk_batch_tables(const otc_aes_key *keys, uint64_t nkeys, int nr, void *tab, hipStream_t st)
{
    if (nkeys == 0) return hipSuccess;
    const dim3 g((unsigned)((nkeys + GMK_TAB_KEYS - 1) / GMK_TAB_KEYS)), b(64);
    return with_rounds(nr, [&](auto r) {
        constexpr int NR = decltype(r)::value;
        hipLaunchKernelGGL((k_gmk_tables<NR>), g, b, 0, st, keys, nkeys, (uint4 *)tab);
        return hipGetLastError();
    });
}

hipError_t ghash_mk_batch_run(const otc_gcm_mk_msg *msgs, uint64_t nmsg, const void *tab, void *s, bool hash_out,
                              int lanes, hipStream_t st)
{
    if (lanes != GMK_LANES_SHORT && lanes != GMK_LANES_LONG) return hipErrorInvalidValue;
    GmkParams P{};
    P.msgs = msgs;
    P.nmsg = nmsg;
    P.tab = (const uint4 *)tab;
    P.s = (uint4 *)s;
    P.hash_out = hash_out ? 1u : 0u;
    const uint64_t nrec = SB_THREADS / (unsigned)lanes; /* records of a workgroup */
    /* up to 8 workgroups per CU (20 KiB of LDS each at most), grid-stride over the groups of records */
    const uint64_t ngroups = (nmsg + nrec - 1) / nrec, cap = (uint64_t)device_cus() * 8;
    const dim3 g((unsigned)(ngroups < cap ? ngroups : cap)), b(SB_THREADS);
    if (lanes == GMK_LANES_SHORT)
        hipLaunchKernelGGL(k_ghash_mk_batch<16>, g, b, 0, st, P);
    else
        hipLaunchKernelGGL(k_ghash_mk_batch<64>, g, b, 0, st, P);
    return hipGetLastError();
}

hipError_t gcm_mk_batch_final(const otc_gcm_mk_msg *msgs, const otc_aes_key *keys, const void *j0, const void *s,
                              uint64_t nmsg, int nr, void *tags, const uint8_t *expect, int tag_bytes, uint8_t *ok,
                              hipStream_t st)
{
    const dim3 g((unsigned)((nmsg + 63) / 64)), b(64);
    return with_rounds(nr, [&](auto r) {
        constexpr int NR = decltype(r)::value;
        hipLaunchKernelGGL((k_gmk_final<NR>), g, b, 0, st, msgs, keys, (const uint4 *)j0, (const uint4 *)s, nmsg,
                           (uint4 *)tags, ok ? expect : nullptr, (uint32_t)tag_bytes, ok);
        return hipGetLastError();
    });
}

} // namespace otc_impl
