/*
 * aes_gcm_siv_batch.hip -- AES-GCM-SIV (RFC 8452) over MANY short records in
 * one linear chain of launches (otc_aes_gcm_siv_batch): every record has its own
 * nonce, and in this mode the nonce decides BOTH keys of the record -- the
 * POLYVAL key H_m and the cipher key K_m -- so nothing per key can be shared the
 * way aes_gcm_batch.hip shares its tables and the batched CTR kernel its one
 * schedule.  Four kernels, each over all records:
 *
 *   k_gsb_derive      one lane per record: the 4 (AES-128) or 6 (AES-256)
 *                     derivation blocks le32(i) || nonce under the key-generating
 *                     key (the cipher on the constant tables in global memory,
 *                     ocb_dev.h), their low halves -> H_m into the workspace and
 *                     K_m, expanded right there (polyval_dev.h siv_expand_key over
 *                     the S-box already on the device) into an otc_aes_key in the
 *                     workspace.  Nothing per record happens on the host.
 *   k_polyval_batch   S_m = POLYVAL_{H_m}(pad16(AAD) || pad16(data) || le64(8 aad)
 *                     le64(8 n)), L lanes per record, L = 16 (four records per
 *                     wave) or 64 (one wave per record); see below.
 *   k_gsb_final       one lane per record: tag = E_{K_m}((S_m ^ nonce) with bit
 *                     127 cleared), the schedule read from the workspace; on
 *                     decryption the verdict against the received tag (all 16
 *                     bytes, OR of the XORs) and a zero tag row where it fails.
 *   k_aes_ctr_le32_batch   the counter mode, a wave tile of 256 blocks of one
 *                     record from the host planner's tile map (the batched CTR
 *                     kernel's arrangement, aes_tt.hip).  Per tile the wave reads
 *                     the record's schedule and its counter block -- the tag, or a
 *                     decryption's received tag -- from DEVICE memory with scalar
 *                     loads; block i takes polyval_dev.h siv_ctr_block: word 0 + i
 *                     modulo 2^32 and bit 31 of word 3 forced on.  A record's last
 *                     tile takes 1, 2 or 4 blocks per lane, whatever covers it: a
 *                     1 KiB record costs 64 cipher calls, not 256 (measured: 375 ->
 *                     1110 GB/s for the kernel alone at 65536 x 1 KiB).  All rounds go
 *                     through the LDS tables (no round caching: a tile starts at a
 *                     counter nobody knows before the finisher has run).
 *
 * The hash.  A key per record rules out positional byte tables (64 KiB per
 * constant).  A lane multiplies by Shoup's 4-bit method on a NIBBLE TABLE of the
 * constant, 16 entries of 16 bytes, 256 bytes per record and constant in LDS
 * (polyval_dev.h: Horner over the accumulator's 32 nibbles from the lowest,
 * dividing by x^4 each step -- 32 LDS reads of 16 bytes whose addresses depend
 * only on the multiplicand, so they are all issued ahead of the serial chain of
 * 32 x (4 XOR, 4 funnel shifts, the reduction in 4 more)).  The decomposition is
 * aes_gcm_batch.hip's with another fold:
 *
 *   powers    C_s = H^(2^s), s = 0 .. log2 L, by squaring; the record's first 16
 *             lanes write one table entry each, every lane squares redundantly.
 *             (In the 16-lane form a record's lanes are one of the LDS's four
 *             service groups of a 16-byte read, not consecutive ones: sb_place,
 *             polyval_batch_dev.h, which holds what this hash kernel shares with
 *             aes_gcm_mk_batch.hip's.)
 *   lanes     lane j runs Horner under H^L over the record's blocks L apart,
 *             aligned to the END of the record (zero blocks in front).
 *   fold      log2 L steps across lanes, A_j = A_j . H^d ^ A_{j+d}, d = 1, 2, ..
 *             L / 2 -- every lane multiplies by the SAME constant in a step, so a
 *             step reads one table of the record -- and Y = A_0 . H.  (The serial
 *             fold of aes_gcm_batch.hip would be L + 1 of these costly products
 *             in one lane.)
 *
 * A record never leaves its wave, so there is no workgroup barrier and no
 * accumulator array: waves of a workgroup only share the launch.  LDS per
 * workgroup of 4 waves: 16 records x 5 tables x 256 B = 20 KiB (L = 16), 4 x 7 x
 * 256 B = 7 KiB (L = 64).
 *
 * Nothing here reads at or past the end of a record's data or AAD: whole
 * 16-byte loads only where 16 bytes are inside, bytes otherwise.  Every value
 * is written with ordinary vector stores.
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

typedef __attribute__((address_space(1))) uint8_t g_u8;
/* loads through the constant address space (wave-uniform address -> s_load), as aes_tt.hip's batch kernel */
typedef const __attribute__((address_space(4))) uint32_t *cptr32;
typedef const __attribute__((address_space(4))) uint64_t *cptr64;
__device__ __forceinline__ uint32_t cld32(const uint32_t *p) { return *(cptr32)p; }
__device__ __forceinline__ uint64_t cld64(const uint64_t *p) { return *(cptr64)p; }

static_assert(sizeof(otc_aes_key) == 256 && offsetof(otc_aes_key, rk) == 0 && offsetof(otc_aes_key, nr) == 240,
              "the derive kernel writes a schedule as 16 rows of 16 bytes");

/* the 12 bytes of nonce m as three words as loaded; the array has any alignment */
__device__ __forceinline__ void nonce_words(uint32_t (&n)[3], const uint8_t *nonces, uint64_t m)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        n[j] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) n[j] |= (uint32_t)nonces[m * 12 + 4 * j + b] << (8 * b);
    }
}

/* ---- derive ------------------------------------------------------------------ */
template <int NR>
__global__ __launch_bounds__(64) void k_gsb_derive(otc_aes_key KGK, const uint8_t *nonces, uint64_t nmsg, uint4 *h,
                                                   otc_aes_key *keys)
{
    static_assert(NR == 10 || NR == 14, "RFC 8452 has AES-128 and AES-256");
    constexpr int NK = NR == 10 ? 4 : 8, NB = 2 + NK / 2;
    const uint64_t m = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (m >= nmsg) return;
    uint32_t n[3], lo[NB][2];
    nonce_words(n, nonces, m);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        uint32_t b[4];
        siv_derive_block(b, n, (uint32_t)i);
        enc_block_global<NR>(KGK, b);
        lo[i][0] = b[0];
        lo[i][1] = b[1];
    }
    h[m] = make_uint4(lo[0][0], lo[0][1], lo[1][0], lo[1][1]);
    uint32_t rk[64];
#pragma unroll
    for (int j = 0; j < NK; ++j) rk[j] = lo[2 + j / 2][j & 1];
    siv_expand_key(rk, g_tab.sb, NK);
#pragma unroll
    for (int j = 4 * (NR + 1); j < 60; ++j) rk[j] = 0;
    rk[60] = NR;
    rk[61] = OTC_DIR_ENCRYPT;
    rk[62] = 32 * NK;
    rk[63] = 0;
    uint4 *K = (uint4 *)(keys + m);
#pragma unroll
    for (int q = 0; q < 16; ++q) K[q] = make_uint4(rk[4 * q], rk[4 * q + 1], rk[4 * q + 2], rk[4 * q + 3]);
}

/* ---- the batched hash -------------------------------------------------------- */
/* block i (< na + nd + 1) of the record's hashed string */
__device__ __forceinline__ uint4 sb_block(const SbRec &R, uint64_t i)
{
    if (i < R.na + R.nd) return sb_text_block(R, i);
    const uint64_t ab = R.aad_bytes * 8, db = R.nbytes * 8; /* le64(8 aad) le64(8 n) */
    return make_uint4((uint32_t)ab, (uint32_t)(ab >> 32), (uint32_t)db, (uint32_t)(db >> 32));
}

struct SbParams {
    const otc_gcm_msg *msgs;
    uint64_t nmsg;
    const uint4 *h;    /* nmsg x 16: H_m */
    uint4 *s;          /* nmsg x 16: S_m */
    uint32_t hash_out; /* hash the record's `out` (a decryption's plaintext), else its `in` */
};

/* the passes kb .. kb + SB_BATCH - 1 of a record, one block per lane of its L */
template <uint32_t L>
__device__ __forceinline__ void sb_load(uint4 (&X)[SB_BATCH], const SbRec &R, uint32_t kb, uint32_t npass, uint64_t pad,
                                        uint32_t l)
{
#pragma unroll
    for (uint32_t i = 0; i < SB_BATCH; ++i) {
        const uint64_t v = (uint64_t)(kb + i) * L + l;
        X[i] = (kb + i < npass && v >= pad) ? sb_block(R, v - pad) : make_uint4(0, 0, 0, 0);
    }
}

/* L lanes per record (16 or 64), 64 / L records per wave */
template <uint32_t L>
__global__ __launch_bounds__(SB_THREADS) void k_polyval_batch(SbParams P)
{
    constexpr uint32_t LOG = L == 16 ? 4 : 6; /* fold steps; the tables are those of H^(2^s), s = 0 .. LOG */
    constexpr uint32_t NT = LOG + 1, NREC = SB_THREADS / L;
    __shared__ __attribute__((aligned(16))) uint4 tab[NREC * NT * 16];
    const uint32_t tid = threadIdx.x;
    uint32_t rec, l; /* the record of the group this lane works on, and its lane there */
    sb_thread<L>(tid, rec, l);
    uint4 *const T = tab + rec * NT * 16;
    const uint64_t ngroups = (P.nmsg + NREC - 1) / NREC;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t m = g * NREC + rec;
        const bool live = m < P.nmsg;
        /* the powers of H_m and their tables; a record past the end runs along with H = 0 */
        uint4 C = live ? P.h[m] : make_uint4(0, 0, 0, 0);
#pragma unroll 1
        for (uint32_t s = 0; s <= LOG; ++s) {
            if (l < 16) {
                const uint32_t c[4] = {C.x, C.y, C.z, C.w};
                uint32_t e[4];
                pv4_entry(e, c, l);
                T[s * 16 + l] = make_uint4(e[0], e[1], e[2], e[3]);
            }
            sb_wave_sync();
            if (s < LOG) C = sb_mul(T + s * 16, C);
        }
        uint4 A = make_uint4(0, 0, 0, 0);
        if (live) {
            const SbRec R = sb_record((const uint64_t *)(P.msgs + m), P.hash_out);
            const uint64_t nb = R.na + R.nd + 1;
            const uint32_t npass = (uint32_t)((nb + L - 1) / L);
            const uint64_t pad = (uint64_t)npass * L - nb; /* zero blocks in front, < L */
            const uint4 *TL = T + LOG * 16;
            uint4 X[SB_BATCH], N[SB_BATCH];
            sb_load<L>(X, R, 0, npass, pad, l);
            for (uint32_t kb = 0; kb < npass; kb += SB_BATCH) {
                /* the next batch's loads are in flight during this one's multiplications */
                sb_load<L>(N, R, kb + SB_BATCH, npass, pad, l);
#pragma unroll
                for (uint32_t i = 0; i < SB_BATCH; ++i)
                    if (kb + i < npass) A = sb_xor(sb_mul(TL, A), X[i]);
#pragma unroll
                for (uint32_t i = 0; i < SB_BATCH; ++i) X[i] = N[i];
            }
        }
        /* the fold: after the step with d, lane j (a multiple of 2 d) holds
         * sum_{i < 2 d} A_{j+i} . H^(2 d - 1 - i); the other lanes' values are not used */
#pragma unroll 1
        for (uint32_t s = 0; s < LOG; ++s) {
            const uint32_t d = 1u << s;
            const uint4 B = sb_from_lane<L>(A, rec, l, d);
            A = sb_xor(sb_mul(T + s * 16, A), B);
        }
        A = sb_mul(T, A);
        if (live && l == 0) P.s[m] = A;
        sb_wave_sync(); /* the next group's tables overwrite these */
    }
}

/* ---- the finisher -------------------------------------------------------------- */
template <int NR>
__global__ __launch_bounds__(64) void k_gsb_final(const uint4 *s, const uint8_t *nonces, const otc_aes_key *keys,
                                                  uint64_t nmsg, uint4 *tags, const uint8_t *expect, uint8_t *ok)
{
    const uint64_t m = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (m >= nmsg) return;
    uint32_t n[3];
    nonce_words(n, nonces, m);
    const uint4 S = s[m];
    uint32_t y[4] = {S.x ^ n[0], S.y ^ n[1], S.z ^ n[2], S.w & 0x7FFFFFFFu};
    enc_block_global<NR>(keys[m], y);
    if (ok) {
        /* against the received tag: OR of the XORs, no early exit.  The verdict is formed BEFORE
         * anything is stored (the host also rejects expect overlapping tags or ok) */
        const uint8_t *e = expect + m * 16;
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t t = 0; t < 16; ++t) diff |= ((y[t >> 2] >> (8 * (t & 3))) & 0xFFu) ^ (uint32_t)e[t];
        ok[m] = diff == 0 ? 1 : 0;
        /* the computed tag of a forged record is the valid tag of the forgery: not handed out */
        if (diff) y[0] = y[1] = y[2] = y[3] = 0;
    }
    tags[m] = make_uint4(y[0], y[1], y[2], y[3]);
}

/* ---- the counter mode ----------------------------------------------------------- */
constexpr int SBC_THREADS = 1024;
constexpr int SBC_B = 4; /* blocks per lane: a tile is 64 x 4 blocks */
static_assert(64 * SBC_B == OTC_GCM_SIV_BATCH_TILE_BLOCKS, "the planner's tile");

struct SbCtrParams {
    const otc_gcm_msg *msgs;
    const otc_aes_key *keys; /* one schedule per record */
    const uint32_t *ctrs;    /* one counter block per record: nmsg x 16 bytes, 4-byte aligned */
    const uint32_t *tile_msg;
    const uint64_t *tile_first;
    uint64_t ntiles;
};

/* BB x 64 blocks of one record from block vb: BB = 4 is a whole tile; a record's last tile
 * takes 1, 2 or 4 loads' worth, so a 1 KiB record costs 64 cipher calls, not 256 */
template <int NR, int BB>
__device__ __forceinline__ void sbc_blocks(const uint32_t *tbl, const uint32_t (&lk)[4], const otc_aes_key &K,
                                           const uint32_t (&tg)[4], const uint8_t *in, uint8_t *out, uint64_t nfull,
                                           uint32_t tail, uint64_t vb, uint32_t lane)
{
    uint32_t s[BB][4];
    uint4 x[BB];
#pragma unroll
    for (int b = 0; b < BB; ++b) {
        const uint64_t i = vb + 64u * b + lane;
        x[b] = i < nfull ? ld16<M_BATCH>(in, i) : make_uint4(0, 0, 0, 0);
        uint32_t c[4];
        siv_ctr_block(c, tg, (uint32_t)i);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[b][j] = c[j] ^ K.rk[j];
    }
    enc_rounds4_from<1, NR, BB>(tbl, lk, K, s);
#pragma unroll
    for (int b = 0; b < BB; ++b) {
        const uint64_t i = vb + 64u * b + lane;
        if (i < nfull) {
            st16<M_BATCH>(out, i, make_uint4(x[b].x ^ s[b][0], x[b].y ^ s[b][1], x[b].z ^ s[b][2], x[b].w ^ s[b][3]));
        } else if (i == nfull && tail) {
            /* the partial last block, as in k_aes_ctr_batch_tt */
            const uint32_t ks[4] = {s[b][0], s[b][1], s[b][2], s[b][3]};
            const g_u8 *gi = (const g_u8 *)in;
            g_u8 *go = (g_u8 *)out;
            for (uint32_t n = 0; n < tail; ++n)
                go[16 * i + n] = gi[16 * i + n] ^ (uint8_t)(ks[n >> 2] >> (8 * (n & 3)));
        }
    }
}

template <int NR>
__global__ __launch_bounds__(SBC_THREADS) void k_aes_ctr_le32_batch(SbCtrParams P)
{
    constexpr uint64_t TILE = 64u * SBC_B;
    constexpr uint32_t WAVES = SBC_THREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t tbl[2 * 256 * 64];
    uint32_t lk[4];
    const uint32_t lane = tt_open<SBC_THREADS>(tbl, lk).lane;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    /* each wave walks a contiguous run of tiles, as k_aes_ctr_batch_tt does */
    const uint64_t nw = (uint64_t)gridDim.x * WAVES, wid = (uint64_t)blockIdx.x * WAVES + wave;
    const uint64_t t_end = (wid + 1) * P.ntiles / nw;
    for (uint64_t t = wid * P.ntiles / nw; t < t_end; ++t) {
        /* descriptor, schedule and counter block at wave-uniform addresses: scalar loads */
        const uint64_t m = cld32(P.tile_msg + t);
        const uint64_t *D = (const uint64_t *)(P.msgs + m);
        const uint8_t *in = (const uint8_t *)cld64(D + 0);
        uint8_t *out = (uint8_t *)cld64(D + 1);
        const uint64_t nbytes = cld64(D + 2);
        const uint32_t *Kg = P.keys[m].rk;
        otc_aes_key K;
#pragma unroll
        for (int q = 0; q < 4 * (NR + 1); ++q) K.rk[q] = cld32(Kg + q);
        const uint32_t *cg = P.ctrs + 4 * m;
        const uint32_t tg[4] = {cld32(cg), cld32(cg + 1), cld32(cg + 2), cld32(cg + 3)};
        const uint64_t nfull = nbytes >> 4;
        const uint32_t tail = (uint32_t)(nbytes & 15u);
        const uint64_t vb = (t - cld64(P.tile_first + m)) * TILE; /* the tile's first block */
        const uint64_t left = nfull + (tail ? 1u : 0u) - vb;      /* blocks from here to the record's end, >= 1 */
        if (left > 128)
            sbc_blocks<NR, 4>(tbl, lk, K, tg, in, out, nfull, tail, vb, lane);
        else if (left > 64)
            sbc_blocks<NR, 2>(tbl, lk, K, tg, in, out, nfull, tail, vb, lane);
        else
            sbc_blocks<NR, 1>(tbl, lk, K, tg, in, out, nfull, tail, vb, lane);
    }
}

} // namespace

/* ---- host entry points (otc_kernels.h) ------------------------------------- */
int gcm_siv_batch_spans(uint64_t *spans, int max)
{
    const uint64_t all[] = {GSB_LANES_SHORT,            /* a pass of the 16-lane form: one block per lane of a record */
                            GSB_LANES_LONG,             /* its batch of passes, and a pass of the 64-lane form */
                            SB_BATCH * GSB_LANES_LONG}; /* a batch of passes of the 64-lane form */
    static_assert(SB_BATCH * GSB_LANES_SHORT == GSB_LANES_LONG, "the middle span is both");
    const int n = (int)(sizeof all / sizeof all[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = all[i];
    return n;
}

hipError_t gcm_siv_batch_derive(const otc_aes_key &kgk, const uint8_t *nonces, uint64_t nmsg, void *h, otc_aes_key *keys,
                                hipStream_t st)
{
    const dim3 g((unsigned)((nmsg + 63) / 64)), b(64);
    if (kgk.nr == 10)
        hipLaunchKernelGGL(k_gsb_derive<10>, g, b, 0, st, kgk, nonces, nmsg, (uint4 *)h, keys);
    else if (kgk.nr == 14)
        hipLaunchKernelGGL(k_gsb_derive<14>, g, b, 0, st, kgk, nonces, nmsg, (uint4 *)h, keys);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t polyval_batch_run(const otc_gcm_msg *msgs, uint64_t nmsg, const void *h, void *s, bool hash_out, int lanes,
                             hipStream_t st)
{
    if (lanes != GSB_LANES_SHORT && lanes != GSB_LANES_LONG) return hipErrorInvalidValue;
    SbParams P{};
    P.msgs = msgs;
    P.nmsg = nmsg;
    P.h = (const uint4 *)h;
    P.s = (uint4 *)s;
    P.hash_out = hash_out ? 1u : 0u;
    const uint64_t nrec = SB_THREADS / (unsigned)lanes; /* records of a workgroup */
    /* up to 8 workgroups per CU (20 KiB of LDS each at most), grid-stride over the groups of records */
    const uint64_t ngroups = (nmsg + nrec - 1) / nrec, cap = (uint64_t)device_cus() * 8;
    const dim3 g((unsigned)(ngroups < cap ? ngroups : cap)), b(SB_THREADS);
    if (lanes == GSB_LANES_SHORT)
        hipLaunchKernelGGL(k_polyval_batch<16>, g, b, 0, st, P);
    else
        hipLaunchKernelGGL(k_polyval_batch<64>, g, b, 0, st, P);
    return hipGetLastError();
}

hipError_t gcm_siv_batch_final(const void *s, const uint8_t *nonces, const otc_aes_key *keys, uint64_t nmsg, int nr,
                               void *tags, const uint8_t *expect, uint8_t *ok, hipStream_t st)
{
    const dim3 g((unsigned)((nmsg + 63) / 64)), b(64);
    if (nr == 10)
        hipLaunchKernelGGL(k_gsb_final<10>, g, b, 0, st, (const uint4 *)s, nonces, keys, nmsg, (uint4 *)tags, expect, ok);
    else if (nr == 14)
        hipLaunchKernelGGL(k_gsb_final<14>, g, b, 0, st, (const uint4 *)s, nonces, keys, nmsg, (uint4 *)tags, expect, ok);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t ctr_le32_batch_run(const otc_gcm_msg *msgs, const otc_aes_key *keys, const void *ctrs,
                              const uint32_t *tile_msg, const uint64_t *tile_first, uint64_t ntiles, int nr,
                              hipStream_t st)
{
    if (ntiles == 0) return hipSuccess;
    SbCtrParams P{};
    P.msgs = msgs;
    P.keys = keys;
    P.ctrs = (const uint32_t *)ctrs;
    P.tile_msg = tile_msg;
    P.tile_first = tile_first;
    P.ntiles = ntiles;
    /* one workgroup per CU (the 128 KiB table image); a wave gets at least one tile where there are enough */
    const uint64_t need = (ntiles + SBC_THREADS / 64 - 1) / (SBC_THREADS / 64), cus = (uint64_t)device_cus();
    const dim3 grid((unsigned)(need < cus ? need : cus)), wg(SBC_THREADS);
    return with_rounds(nr, [&](auto r) {
        constexpr int NR = decltype(r)::value;
        hipLaunchKernelGGL((k_aes_ctr_le32_batch<NR>), grid, wg, 0, st, P);
        return hipGetLastError();
    });
}

} // namespace otc_impl
