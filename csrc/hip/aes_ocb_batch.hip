/*
 * aes_ocb_batch.hip -- AES-OCB3 (RFC 7253) over MANY short records in one
 * chain of launches (otc_aes_ocb_batch): one key per batch, every record with
 * its own 12-byte nonce, its own AAD and its own 16-byte tag.
 *
 * aes_ocb.hip spreads ONE message over the chip and computes Offset_0 and
 * HASH(K, A) on the host, which a 1-16 KiB record cannot carry.  Here both are
 * made on the device, and the data is read ONCE: the two other batched AEADs
 * read every record in the cipher pass and again in the hash pass.
 *
 *   prep      a 16-lane group per record, tables in global memory.  Lane 0
 *             builds the nonce block, Ktop = E_K(nonce block), Stretch and
 *             Offset_0 (ocb_dev.h) and stores it, and clears the record's
 *             checksum.  The group strides over the AAD's blocks -- block i has
 *             the offset XOR{ L_j : bit j of i ^ (i >> 1) }, read by bytes --
 *             and folds Sum by cross-lane XOR into the record's HASH.  (A
 *             version that made the nonce block one more item of that stride,
 *             so that it shared a short AAD's cipher call in another lane, was
 *             SLOWER: 382-386 against 463-467 GB/s at 65536 records of 1 KiB,
 *             docs/PERF.md "Batched AES-OCB3"; why was not found.)
 *   bulk      k_aes_ocb_batch on the LDS T-table rounds (aes_tt_dev.h: 128 KiB
 *             image to encrypt, 160 KiB to decrypt), 1024 threads, one
 *             workgroup per CU, grid-stride over the tiles.  A tile is 64
 *             consecutive whole blocks (1 KiB) of one record, aligned in the
 *             record's block numbering: tile k starts at 0-based block W = 64 k.
 *             A wave takes four consecutive tiles per pass as its four per-lane
 *             blocks (the b = 0..3 of aes_ocb.hip's ocb_run); each of the four
 *             slots has its own record and its own wave-uniform start
 *                 S = Offset_0[m] ^ XOR{ L_j : bit j of W ^ (W >> 1) }   (j = 5..15)
 *             Lane v - 1 (v = 1..63) holds index W + v with offset S ^ low(v),
 *             low(v) = XOR{ L_j : bit j of v ^ (v >> 1), j <= 5 }, computed once
 *             per lane; lane 63 holds W + 64 with S ^ L_5 ^ L_ntz(W + 64), ntz
 *             in 6..16 (the largest index is 2^16: L_0 .. L_16 travel by value).
 *             Lanes past the record's whole blocks do nothing.  Every access is
 *             a coalesced 1 KiB wave access, non-temporal; a block is read and
 *             written by the same lane, so in place is allowed.
 *   checksum  each slot's 64 lanes hold the plaintext of its blocks (the input
 *             of an encryption, the output of a decryption).  Slots are taken
 *             in order; neighbours of one record are XORed lane by lane first
 *             and share ONE fold (cross-lane XOR, no LDS memory: the decryption
 *             image fills it), then lane 0 issues one vector atomic XOR per
 *             word into the record's 16-byte accumulator.  A fold that comes
 *             out zero issues none.  XOR is exact: the order does not matter.
 *   finish    one lane per record: Offset_m by the closed form over the
 *             record's whole blocks, the trailing r < 16 bytes as
 *             P ^ E_K(Offset_*)[:r], the padded piece into the checksum,
 *             Tag = E_K(Checksum ^ Offset ^ L_$) ^ HASH.  On decryption the tag
 *             is compared with the expected one (OR of the XORs, no early
 *             exit), the verdict written, and the tag of a record that fails
 *             zeroed.
 *   wipe      the output of every record that failed is zeroed by the batched
 *             GCM's wipe kernel (aes_gcm_batch.hip), which reads the columns
 *             that otc_ocb_msg shares with otc_gcm_msg.
 *
 * Nothing branches on, or addresses memory by, key material, data or
 * checksums except the AES table lookups themselves (the T-table kernels'
 * property, docs/ARCHITECTURE.md); the other branches are on lengths and on
 * the call's shape.  Nothing reads or writes outside [in, in + n), [out, out +
 * n), [aad, aad + aad_bytes) and the arrays of the call.  Every value is
 * written with ordinary vector stores or vector atomics.
 */
#include <hip/hip_runtime.h>

#include <cstddef>

#include "otc_device.h"
#include "otc_kernels.h"
#include "aes_tt_dev.h"
#include "ocb_dev.h"

using namespace otc_dev;

namespace {

constexpr int OB_THREADS = 1024;
constexpr int OB_B = 4;                                         /* slots of a wave pass: blocks per lane */
constexpr uint32_t OB_TILE = 64;                                /* blocks of a tile */
constexpr uint32_t OB_WG_TILES = (OB_THREADS / 64) * OB_B;      /* tiles of a workgroup step */
constexpr int OB_NL = 17;                                       /* L_0 .. L_16 */
constexpr uint32_t OB_WORDS = sizeof(otc_ocb_msg) / 8;
constexpr uint32_t OB_PREP_LANES = 16;
static_assert(sizeof(otc_ocb_msg) == sizeof(otc_gcm_msg) && offsetof(otc_ocb_msg, out) == offsetof(otc_gcm_msg, out) &&
                  offsetof(otc_ocb_msg, nbytes) == offsetof(otc_gcm_msg, nbytes),
              "the wipe kernel reads the columns otc_ocb_msg shares with otc_gcm_msg");
static_assert(OTC_OCB_BATCH_MAX_BYTES / 16 <= (1u << 16), "block indices up to 2^16: L_0 .. L_16");
static_assert(OTC_OCB_BATCH_MAX_AAD / 16 < (1u << 16), "AAD block indices below 2^16: L_0 .. L_16");

typedef const __attribute__((address_space(1))) uint8_t *gptr8;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v); }

/* the key's constants the prep and finish kernels take by value */
struct ObConsts {
    uint32_t l[OB_NL][4];
    uint32_t l_star[4], l_dollar[4];
};

/* the 16 bytes at p + off as four words, those at or past `end` as zero; never reads them */
__device__ __forceinline__ void ob_bytes(uint32_t (&w)[4], gptr8 p, uint64_t off, uint64_t end)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = 0;
#pragma unroll
    for (uint32_t t = 0; t < 16; ++t) {
        const uint32_t v = off + t < end ? (uint32_t)p[off + t] : 0u;
        w[t >> 2] |= v << (8 * (t & 3));
    }
}

/* ---- prep: Offset_0, a clear checksum and HASH(K, A) per record ------------- */
template <int NR>
__global__ __launch_bounds__(256) void k_ocb_batch_prep(const uint64_t *msgs, uint64_t nmsg, const uint8_t *nonces,
                                                        uint4 *off0, uint4 *checksum, uint4 *hash, ObConsts C,
                                                        otc_aes_key K)
{
    const uint32_t j = threadIdx.x & (OB_PREP_LANES - 1);
    const uint64_t m = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / OB_PREP_LANES;
    const bool live = m < nmsg; /* every lane runs the cross-lane fold */
    uint32_t sum[4] = {0, 0, 0, 0};
    if (live) {
        if (j == 0) {
            auto p = (gptr8)(nonces + m * 12); /* any byte address */
            uint32_t n[3], nb[4], o[4];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                n[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
                       (uint32_t)p[4 * i + 3] << 24;
            const uint32_t bottom = ocb_nonce_block12(nb, n);
            enc_block_global<NR>(K, nb); /* Ktop */
            ocb_offset0_from_ktop(o, nb, bottom);
            off0[m] = make_uint4(o[0], o[1], o[2], o[3]);
            checksum[m] = make_uint4(0, 0, 0, 0);
        }
        const uint64_t *D = msgs + m * OB_WORDS;
        auto aad = (gptr8)D[3];
        const uint64_t abytes = D[4], nfull = abytes >> 4; /* <= 4096 */
        for (uint64_t i = j; i < nfull; i += OB_PREP_LANES) { /* block i + 1: on the length */
            uint32_t x[4], o[4] = {0, 0, 0, 0};
            ob_bytes(x, aad, i * 16, abytes);
            ocb_xor_gray(o, C.l, ocb_gray((uint32_t)i + 1u));
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] ^= o[q];
            enc_block_global<NR>(K, x);
#pragma unroll
            for (int q = 0; q < 4; ++q) sum[q] ^= x[q];
        }
        if ((abytes & 15u) && j == (nfull & (OB_PREP_LANES - 1))) { /* A_* || 1 || 0*, under Offset_nfull ^ L_* */
            uint32_t x[4], o[4];
            ob_bytes(x, aad, nfull * 16, abytes);
            const uint32_t r = (uint32_t)abytes & 15u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] |= (r >> 2) == (uint32_t)q ? 0x80u << (8 * (r & 3u)) : 0u;
                o[q] = C.l_star[q];
            }
            ocb_xor_gray(o, C.l, ocb_gray((uint32_t)nfull));
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] ^= o[q];
            enc_block_global<NR>(K, x);
#pragma unroll
            for (int q = 0; q < 4; ++q) sum[q] ^= x[q];
        }
    }
#pragma unroll
    for (int d = OB_PREP_LANES / 2; d; d >>= 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) sum[q] ^= (uint32_t)__shfl_xor((int)sum[q], d);
    if (live && j == 0) hash[m] = make_uint4(sum[0], sum[1], sum[2], sum[3]);
}

/* ---- bulk: four tiles per wave pass ------------------------------------------ */
struct ObParams {
    const uint64_t *msgs;
    const uint32_t *tile_msg;
    const uint64_t *tile_first;
    uint64_t ntiles;
    const uint32_t *off0; /* nmsg x 4 words */
    uint32_t *checksum;   /* nmsg x 4 words */
    uint32_t l[OB_NL][4];
};

/* fold the wave's 64 lanes and add the result to record m's accumulator */
__device__ __forceinline__ void ob_flush(uint32_t *checksum, uint32_t m, uint32_t lane, uint32_t (&acc)[4])
{
#pragma unroll
    for (int d = 32; d; d >>= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] ^= (uint32_t)__shfl_xor((int)acc[j], d);
    /* blocks that cancel add nothing */
    if (lane == 0 && (acc[0] | acc[1] | acc[2] | acc[3]))
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicXor(checksum + 4 * (uint64_t)m + j, acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 0;
}

template <int NR, bool DEC>
__global__ __launch_bounds__(OB_THREADS) void k_aes_ocb_batch(ObParams P, otc_aes_key K)
{
    /* encryption: Te0..Te3 (128 KiB); decryption: Td0..Td3 + inverse S-box (160 KiB) */
    __shared__ __attribute__((aligned(16))) uint32_t tbl[DEC ? 2 * 256 * 64 + 256 * 32 : 2 * 256 * 64];
    uint32_t lk[4];
    uint32_t lane;
    if constexpr (DEC) {
        fill_dtbl4<OB_THREADS>(tbl, g_tab.td0, g_tab.is4);
        __syncthreads();
        lane = threadIdx.x & 63u;
        tbl4_lane_consts(lane, lk);
    } else {
        lane = tt_open<OB_THREADS>(tbl, lk).lane;
    }
    const uint32_t lk_is2 = 0x40000u | ((lane & 31u) << 3);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int B = OB_B;

    uint32_t low[4] = {0, 0, 0, 0};
    ocb_low(low, P.l, ocb_lane_mask(lane + 1u));
    const bool carry = lane == 63u;

    const uint64_t step = (uint64_t)gridDim.x * OB_WG_TILES;
    for (uint64_t t0 = ((uint64_t)blockIdx.x * (OB_THREADS / 64) + wave) * B; t0 < P.ntiles; t0 += step) {
        uint32_t T[B][4], s[B][4], rec[B], acc[4] = {0, 0, 0, 0};
        const uint8_t *src[B];
        uint8_t *dst[B];
        bool ok[B];
        uint32_t cur = 0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            /* the slot's tile, its record and where it starts: the same for every lane.  A slot
             * past the last tile reads slot 0's (t0 < ntiles) and does nothing */
            const bool have = t0 + b < P.ntiles;
            const uint64_t t = have ? t0 + b : t0;
            const uint32_t m = uni(P.tile_msg[t]);
            const uint64_t *D = P.msgs + (uint64_t)m * OB_WORDS;
            const uint64_t nblk = uni64(D[2]) >> 4;                             /* whole blocks, <= 2^16 */
            const uint32_t W = (uint32_t)(t - uni64(P.tile_first[m])) * OB_TILE; /* < 2^16 */
            uint32_t S[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) S[j] = uni(P.off0[4 * (uint64_t)m + j]);
            ocb_xor_gray(S, P.l, ocb_gray(W)); /* bits 5 .. 15 */
            const int z = ocb_carry_ntz(W);    /* 6 .. 16 */
            const uint64_t a = (uint64_t)W + lane; /* the block's 0-based number: its index is a + 1 */
            ok[b] = have && a < nblk;
            src[b] = (const uint8_t *)uni64(D[0]) + 16 * a;
            dst[b] = (uint8_t *)uni64(D[1]) + 16 * a;
            rec[b] = have || b == 0 ? m : rec[b ? b - 1 : 0];
            const uint4 v = ok[b] ? ld_u4<MEM_NT<M_BATCH>, true>(src[b]) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) T[b][j] = low[j] ^ S[j] ^ (carry ? P.l[z][j] : 0u);
            if constexpr (!DEC) {
                if (b == 0) cur = rec[0];
                if (rec[b] != cur) { /* wave-uniform */
                    ob_flush(P.checksum, cur, lane, acc);
                    cur = rec[b];
                }
                acc[0] ^= v.x; acc[1] ^= v.y; acc[2] ^= v.z; acc[3] ^= v.w;
            }
            s[b][0] = v.x ^ T[b][0] ^ K.rk[0]; s[b][1] = v.y ^ T[b][1] ^ K.rk[1];
            s[b][2] = v.z ^ T[b][2] ^ K.rk[2]; s[b][3] = v.w ^ T[b][3] ^ K.rk[3];
        }
        if constexpr (!DEC) ob_flush(P.checksum, cur, lane, acc);
        if constexpr (DEC)
            dec_rounds4<NR, B>(tbl, lk, lk_is2, K, s);
        else
            enc_rounds4_from<1, NR, B>(tbl, lk, K, s);
        if constexpr (DEC) cur = rec[0];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if constexpr (DEC) {
                if (rec[b] != cur) {
                    ob_flush(P.checksum, cur, lane, acc);
                    cur = rec[b];
                }
            }
            if (ok[b]) {
                const uint4 o = make_uint4(s[b][0] ^ T[b][0], s[b][1] ^ T[b][1], s[b][2] ^ T[b][2], s[b][3] ^ T[b][3]);
                st_u4<MEM_NT<M_BATCH>, true>(dst[b], o);
                if constexpr (DEC) {
                    acc[0] ^= o.x; acc[1] ^= o.y; acc[2] ^= o.z; acc[3] ^= o.w;
                }
            }
        }
        if constexpr (DEC) ob_flush(P.checksum, cur, lane, acc);
    }
}

/* ---- finish: the trailing bytes, the tag, the verdict ------------------------ */
struct ObFinParams {
    const uint64_t *msgs;
    uint64_t nmsg;
    const uint4 *off0, *checksum, *hash;
    uint4 *tags;
    const uint8_t *expect; /* nmsg x 16 or null (with ok) */
    uint8_t *ok;           /* nmsg verdicts or null: an encryption */
    ObConsts C;
};

template <int NR>
__global__ __launch_bounds__(256) void k_ocb_batch_fin(ObFinParams P, otc_aes_key K)
{
    const uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= P.nmsg) return;
    const bool dec = P.ok != nullptr;
    const uint64_t *D = P.msgs + m * OB_WORDS;
    const uint64_t nbytes = D[2];
    const uint32_t nblk = (uint32_t)(nbytes >> 4), r = (uint32_t)nbytes & 15u;
    const uint4 o0 = P.off0[m], c0 = P.checksum[m], h = P.hash[m];
    const uint32_t o0w[4] = {o0.x, o0.y, o0.z, o0.w};
    uint32_t cs[4] = {c0.x, c0.y, c0.z, c0.w}, off[4];
    ocb_offset_at(off, o0w, P.C.l, nblk); /* Offset_m: bits 0 .. 16 */
    if (r) {
        auto in = (gptr8)((const uint8_t *)D[0] + 16 * (uint64_t)nblk);
        auto out = (__attribute__((address_space(1))) uint8_t *)((uint8_t *)D[1] + 16 * (uint64_t)nblk);
        uint32_t pad[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pad[j] = off[j] ^= P.C.l_star[j];
        enc_block_global<NR>(K, pad);
        /* every input byte is read before any is written: in place is exact */
        uint32_t x[4];
        ob_bytes(x, in, 0, r);
        uint32_t y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            /* the r bytes' mask, word by word */
            const uint32_t k = r > 4u * j ? r - 4u * j : 0u;
            y[j] = (x[j] ^ pad[j]) & (k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u);
        }
#pragma unroll
        for (uint32_t n = 0; n < 15; ++n)
            if (n < r) out[n] = (uint8_t)(y[n >> 2] >> (8 * (n & 3u)));
        /* the plaintext piece || 0x80 || 0* */
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] ^= dec ? y[j] : x[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] ^= (r >> 2) == (uint32_t)j ? 0x80u << (8 * (r & 3u)) : 0u;
    }
    uint32_t t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = cs[j] ^ off[j] ^ P.C.l_dollar[j];
    enc_block_global<NR>(K, t);
    t[0] ^= h.x; t[1] ^= h.y; t[2] ^= h.z; t[3] ^= h.w;
    uint4 Tg = make_uint4(t[0], t[1], t[2], t[3]);
    if (dec) {
        /* the tag against the expected one: OR of the XORs, no early exit.  The verdict is formed
         * before anything is stored (the host also rejects expect overlapping the tags) */
        auto e = (gptr8)(P.expect + m * 16);
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t b = 0; b < 16; ++b) diff |= ((t[b >> 2] >> (8 * (b & 3))) & 0xFFu) ^ (uint32_t)e[b];
        P.ok[m] = diff == 0 ? 1 : 0;
        /* the computed tag of a forged record is the valid tag of the forgery: not handed out */
        if (diff) Tg = make_uint4(0, 0, 0, 0);
    }
    P.tags[m] = Tg;
}

void consts_of(ObConsts &C, const otc_ocb_key &k)
{
    for (int j = 0; j < OB_NL; ++j) words(C.l[j], k.l[j]);
    words(C.l_star, k.l_star);
    words(C.l_dollar, k.l_dollar);
}

} // namespace

/* ---- host entry points (otc_kernels.h) ------------------------------------- */
namespace otc_impl {

int ocb_batch_spans(uint64_t *spans, int max)
{
    const uint64_t s[] = {16,                                  /* a lane's block */
                          OB_TILE * 16,                        /* a slot: one tile */
                          OB_B * OB_TILE * 16,                 /* a wave pass */
                          (uint64_t)OB_WG_TILES * OB_TILE * 16, /* a workgroup step */
                          (uint64_t)device_cus() * OB_WG_TILES * OB_TILE * 16}; /* the full grid's first step */
    const int n = (int)(sizeof s / sizeof s[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = s[i];
    return n;
}

hipError_t ocb_batch_prep(const otc_ocb_msg *msgs, uint64_t nmsg, const otc_ocb_key &k, const uint8_t *nonces, void *ws,
                          hipStream_t st)
{
    const uint64_t wgs = (nmsg * OB_PREP_LANES + 255) / 256;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    ObConsts C;
    consts_of(C, k);
    uint4 *off0 = (uint4 *)ws, *cs = off0 + nmsg, *hash = cs + nmsg;
    return with_rounds(k.enc.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        hipLaunchKernelGGL((k_ocb_batch_prep<NR>), dim3((unsigned)wgs), dim3(256), 0, st, (const uint64_t *)msgs, nmsg,
                           nonces, off0, cs, hash, C, k.enc);
        return hipGetLastError();
    });
}

hipError_t ocb_batch_bulk(const otc_ocb_msg *msgs, uint64_t nmsg, const uint32_t *tile_msg, const uint64_t *tile_first,
                          uint64_t ntiles, const otc_ocb_key &k, bool dec, void *ws, hipStream_t st)
{
    if (ntiles == 0) return hipSuccess;
    ObParams P{};
    P.msgs = (const uint64_t *)msgs;
    P.tile_msg = tile_msg;
    P.tile_first = tile_first;
    P.ntiles = ntiles;
    P.off0 = (const uint32_t *)ws;
    P.checksum = (uint32_t *)ws + 4 * nmsg;
    for (int j = 0; j < OB_NL; ++j) words(P.l[j], k.l[j]);
    /* one workgroup per CU (the 128 / 160 KiB table image), grid-stride over the tiles */
    const uint64_t need = (ntiles + OB_WG_TILES - 1) / OB_WG_TILES, cus = (uint64_t)device_cus();
    const dim3 grid((unsigned)(need < cus ? need : cus)), wg(OB_THREADS);
    return with_rounds(k.enc.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        if (dec) hipLaunchKernelGGL((k_aes_ocb_batch<NR, true>), grid, wg, 0, st, P, k.dec);
        else hipLaunchKernelGGL((k_aes_ocb_batch<NR, false>), grid, wg, 0, st, P, k.enc);
        return hipGetLastError();
    });
}

hipError_t ocb_batch_finish(const otc_ocb_msg *msgs, uint64_t nmsg, const otc_ocb_key &k, void *ws, void *tags,
                            const uint8_t *expect, uint8_t *ok, hipStream_t st)
{
    const uint64_t wgs = (nmsg + 255) / 256;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    ObFinParams P{};
    P.msgs = (const uint64_t *)msgs;
    P.nmsg = nmsg;
    P.off0 = (const uint4 *)ws;
    P.checksum = P.off0 + nmsg;
    P.hash = P.checksum + nmsg;
    P.tags = (uint4 *)tags;
    P.expect = ok ? expect : nullptr;
    P.ok = ok;
    consts_of(P.C, k);
    return with_rounds(k.enc.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        hipLaunchKernelGGL((k_ocb_batch_fin<NR>), dim3((unsigned)wgs), dim3(256), 0, st, P, k.enc);
        return hipGetLastError();
    });
}

} // namespace otc_impl
