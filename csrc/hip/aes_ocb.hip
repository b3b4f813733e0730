/*
 * aes_ocb.hip -- AES-OCB3 (RFC 7253) kernels for gfx950, on the LDS T-table
 * rounds of aes_tt.hip (aes_tt_dev.h): an AEAD in ONE pass over the data.
 *
 * Block i (1-based) of a message:  C_i = Offset_i ^ E_K(P_i ^ Offset_i)
 * (decryption: D_K), Offset_i = Offset_0 ^ XOR{ L_j : bit j of i ^ (i >> 1) },
 * Checksum = XOR of every P_i.  Offset_0, the table L_0 .. L_32 and the key
 * arrive by value; offsets are byte strings and XOR does not care about byte
 * order, so a block and an L_j are four little-endian words as loaded.
 *
 * Layout: aes_xts.hip's.  A wave takes a RUN of 2048 consecutive blocks as 8
 * passes of 256 (4 blocks per lane, block = pass base + 64 b + lane: every
 * access a coalesced 1 KiB wave access); a 1024-thread workgroup takes a chunk
 * of 16 runs (512 KiB) per grid step, one workgroup per CU.  Runs and passes
 * are aligned in the MESSAGE's block numbering (first_block counts), so a pass
 * is the indices W + 1 .. W + 256 with W a multiple of 256, also when a call
 * starts in the middle of a message; lanes outside the call's range do nothing.
 *  * Offsets.  i ^ (i >> 1) is linear over XOR, so for 1 <= v < 64 and
 *    b = 0..3:  Offset_{W + 64 b + v} = S_b ^ low(v),  S_b = Offset_{W + 64 b},
 *    low(v) = XOR{ L_j : bit j of v ^ (v >> 1) }, j <= 5.  low(lane + 1) is
 *    computed once per lane; S_0 .. S_3 are wave-uniform (S_1 = S_0 ^ L_5 ^
 *    L_6, S_2 = S_0 ^ L_6 ^ L_7, S_3 = S_0 ^ L_5 ^ L_7) and live in scalars.
 *  * The carry.  Indices are 1-based, so lane 63's blocks are W + 64 (b + 1):
 *    the NEXT S, which low() does not reach.  Lane 63 takes S_{b+1} with a zero
 *    low part; its last block is W + 256, the next pass's S_0 = S_0 ^ L_7 ^
 *    L_ntz(W + 256), which the pass computes anyway to step on.  That L is the
 *    one table entry fetched with a run-time index (a scalar load from the
 *    kernel arguments); a run's first S_0 is the closed form over bits 7 .. 32.
 *  * Checksum.  Each lane XORs the plaintext of its blocks (the input of an
 *    encryption, the output of a decryption) across the whole kernel; at the
 *    end a wave folds its 64 lanes with cross-lane reads (no LDS memory: the
 *    decryption image fills all 160 KiB) and lane 0 issues one vector atomic
 *    XOR per word into the 16-byte accumulator.  XOR is exact: the result does
 *    not depend on the order.
 *    otc_aes_ocb clears the accumulator with a four-lane kernel in front, so a
 *    call is three kernels in stream order (three kernel nodes in a graph).
 *  * The finisher k_aes_ocb_fin, one lane, tables in global memory, queued
 *    behind the bulk kernel: the trailing r < 16 bytes as P ^ E_K(Offset_*)[:r]
 *    (the forward cipher in both directions), the padded piece into the
 *    checksum, then Tag = E_K(Checksum ^ Offset ^ L_$) ^ HASH(K, A), truncated.
 * Loads and stores are the streaming (non-temporal) form; every block is read
 * and written by the same lane, so in place is allowed in both directions.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "otc_device.h"
#include "otc_kernels.h"
#include "aes_tt_dev.h"
#include "ocb_dev.h"

using namespace otc_dev;

namespace {

constexpr int OCB_THREADS = 1024;
constexpr int OCB_B = 4;                                          /* blocks per lane and pass */
constexpr uint32_t OCB_PASS = 64u * OCB_B;                        /* blocks per wave pass */
constexpr uint32_t OCB_PASSES = 8;
constexpr uint32_t OCB_RUN = OCB_PASS * OCB_PASSES;               /* 2048 blocks per wave */
constexpr uint64_t OCB_CHUNK = (uint64_t)(OCB_THREADS / 64) * OCB_RUN; /* 32768 blocks per workgroup step */
static_assert(OCB_PASS == 256, "the offsets' split into S_b and low(v) is written for passes of 256 blocks");

struct OcbParams {
    const uint8_t *in;
    uint8_t *out;      /* both address the call's first block, index first + 1 */
    uint64_t first;    /* blocks of the message before this call */
    uint64_t end;      /* first + the call's blocks, <= 2^32 */
    uint32_t *checksum;
    uint32_t off0[4];
    uint32_t l[33][4];
};

/* One wave's run: the message blocks with 0-based numbers [r0, r0 + OCB_RUN)
 * that lie in [P.first, P.end); r0 is wave-uniform and a multiple of OCB_PASS */
template <int NR, bool DEC>
__device__ __forceinline__ void ocb_run(const OcbParams &P, const otc_aes_key &K, const uint32_t *tbl,
                                        const uint32_t (&lk)[4], uint32_t lk_is2, uint32_t lane,
                                        const uint32_t (&low)[4], uint32_t (&acc)[4], uint64_t r0)
{
    constexpr int B = OCB_B;
    /* S[0] = Offset_{r0}: the closed form; bits 0..6 of r0 ^ (r0 >> 1) are zero */
    uint32_t S[B + 1][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) S[0][j] = P.off0[j];
#pragma unroll 1
    for (uint64_t g = r0 ^ (r0 >> 1); g; g &= g - 1) {
        const int q = __builtin_ctzll(g);
#pragma unroll
        for (int j = 0; j < 4; ++j) S[0][j] ^= P.l[q][j];
    }
    const bool carry = lane == 63u;

#pragma unroll 1
    for (uint32_t p = 0; p < OCB_PASSES; ++p) {
        const uint64_t W = r0 + (uint64_t)p * OCB_PASS;
        if (W >= P.end) break;
        const bool full = W >= P.first && W + OCB_PASS <= P.end;
        const int z = __builtin_ctzll(W + OCB_PASS); /* 8 .. 32 */
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            S[1][j] = S[0][j] ^ P.l[5][j] ^ P.l[6][j];
            S[2][j] = S[0][j] ^ P.l[6][j] ^ P.l[7][j];
            S[3][j] = S[0][j] ^ P.l[5][j] ^ P.l[7][j];
            S[4][j] = S[0][j] ^ P.l[7][j] ^ P.l[z][j];
        }

        uint32_t T[B][4], s[B][4];
        bool ok[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const uint64_t a = W + 64u * b + lane; /* the block's 0-based number: its index is a + 1 */
            ok[b] = full || (a >= P.first && a < P.end);
            const uint4 v = ok[b] ? ld16<M_STREAM>(P.in, a - P.first) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) T[b][j] = low[j] ^ (carry ? S[b + 1][j] : S[b][j]);
            if constexpr (!DEC) {
                acc[0] ^= v.x; acc[1] ^= v.y; acc[2] ^= v.z; acc[3] ^= v.w;
            }
            s[b][0] = v.x ^ T[b][0] ^ K.rk[0]; s[b][1] = v.y ^ T[b][1] ^ K.rk[1];
            s[b][2] = v.z ^ T[b][2] ^ K.rk[2]; s[b][3] = v.w ^ T[b][3] ^ K.rk[3];
        }
        if constexpr (DEC)
            dec_rounds4<NR, B>(tbl, lk, lk_is2, K, s);
        else
            enc_rounds4_from<1, NR, B>(tbl, lk, K, s);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (ok[b]) {
                const uint64_t a = W + 64u * b + lane;
                const uint4 o = make_uint4(s[b][0] ^ T[b][0], s[b][1] ^ T[b][1], s[b][2] ^ T[b][2], s[b][3] ^ T[b][3]);
                st16<M_STREAM>(P.out, a - P.first, o);
                if constexpr (DEC) {
                    acc[0] ^= o.x; acc[1] ^= o.y; acc[2] ^= o.z; acc[3] ^= o.w;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) S[0][j] = S[4][j];
    }
}

template <int NR, bool DEC>
__global__ __launch_bounds__(OCB_THREADS) void k_aes_ocb(OcbParams P, otc_aes_key K)
{
    /* encryption: Te0..Te3 (128 KiB); decryption: Td0..Td3 + inverse S-box (160 KiB) */
    __shared__ __attribute__((aligned(16))) uint32_t tbl[DEC ? 2 * 256 * 64 + 256 * 32 : 2 * 256 * 64];
    uint32_t lk[4];
    uint32_t lane;
    if constexpr (DEC) {
        fill_dtbl4<OCB_THREADS>(tbl, g_tab.td0, g_tab.is4);
        __syncthreads();
        lane = threadIdx.x & 63u;
        tbl4_lane_consts(lane, lk);
    } else {
        lane = tt_open<OCB_THREADS>(tbl, lk).lane;
    }
    const uint32_t lk_is2 = 0x40000u | ((lane & 31u) << 3);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    /* low(lane + 1); lane 63's blocks are the next S themselves */
    uint32_t low[4] = {0, 0, 0, 0};
    const uint32_t u = lane + 1u, gl = lane == 63u ? 0u : u ^ (u >> 1);
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) low[j] ^= (gl >> q) & 1u ? P.l[q][j] : 0u;

    uint32_t acc[4] = {0, 0, 0, 0};
    const uint64_t a0 = P.first & ~(uint64_t)(OCB_PASS - 1u);
    for (uint64_t base = a0 + (uint64_t)blockIdx.x * OCB_CHUNK; base < P.end; base += (uint64_t)gridDim.x * OCB_CHUNK) {
        const uint64_t r0 = base + (uint64_t)wave * OCB_RUN;
        if (r0 < P.end) ocb_run<NR, DEC>(P, K, tbl, lk, lk_is2, lane, low, acc, r0);
    }

    /* the wave's checksum: fold the lanes, then one atomic per word */
#pragma unroll
    for (int d = 32; d; d >>= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] ^= (uint32_t)__shfl_xor((int)acc[j], d);
    /* a wave that had no block, or whose blocks cancel, adds nothing */
    if (lane == 0 && (acc[0] | acc[1] | acc[2] | acc[3]))
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicXor(P.checksum + j, acc[j]);
}

/* zeroes the 16 bytes of a checksum accumulator in front of the bulk kernel */
__global__ __launch_bounds__(64) void k_aes_ocb_clear(uint32_t *p)
{
    if (threadIdx.x < 4) p[threadIdx.x] = 0;
}

struct OcbFinParams {
    const uint8_t *in;
    uint8_t *out;             /* the trailing piece: r bytes */
    const uint32_t *checksum; /* the whole blocks' checksum (may be the tag's own 16 bytes), or null: zero */
    uint32_t *tag;            /* 16 bytes: tag_bytes of tag, then zeros */
    uint32_t off[4];          /* Offset_m */
    uint32_t l_star[4], l_dollar[4], hash[4];
    uint32_t r, tag_bytes, dec;
};

template <int NR>
__global__ __launch_bounds__(64) void k_aes_ocb_fin(OcbFinParams P, otc_aes_key K)
{
    if (threadIdx.x != 0) return;
    uint32_t cs[4] = {0, 0, 0, 0}, off[4];
    if (P.checksum)
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] = P.checksum[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) off[j] = P.off[j];
    if (P.r) {
        uint32_t pad[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pad[j] = off[j] ^= P.l_star[j];
        enc_block_global<NR>(K, pad);
        /* every input byte is read before any is written: in place is exact */
        uint32_t x[4] = {0, 0, 0, 0};
        for (uint32_t n = 0; n < P.r; ++n) x[n >> 2] |= (uint32_t)P.in[n] << (8 * (n & 3u));
        uint32_t y[4], m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            /* the r bytes' mask, word by word */
            const uint32_t k = P.r > 4u * j ? P.r - 4u * j : 0u;
            m[j] = k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u;
            y[j] = (x[j] ^ pad[j]) & m[j];
        }
        for (uint32_t n = 0; n < P.r; ++n) P.out[n] = (uint8_t)(y[n >> 2] >> (8 * (n & 3u)));
        /* the plaintext piece || 0x80 || 0* */
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] ^= P.dec ? y[j] : x[j];
        cs[P.r >> 2] ^= 0x80u << (8 * (P.r & 3u));
    }
    uint32_t t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = cs[j] ^ off[j] ^ P.l_dollar[j];
    enc_block_global<NR>(K, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t k = P.tag_bytes > 4u * j ? P.tag_bytes - 4u * j : 0u;
        P.tag[j] = (t[j] ^ P.hash[j]) & (k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u);
    }
}

} // namespace

/* ---- host entry points (otc_kernels.h) ------------------------------------- */
namespace otc_impl {

int ocb_spans(uint64_t *spans, int max)
{
    const uint64_t s[] = {16,                        /* a lane's block */
                          64 * 16,                   /* one load of a wave */
                          OCB_PASS * 16,             /* a pass */
                          OCB_RUN * 16,              /* a wave's run */
                          OCB_CHUNK * 16,            /* a workgroup's chunk */
                          (uint64_t)device_cus() * OCB_CHUNK * 16}; /* the full grid's first step: past it a second begins */
    const int n = (int)(sizeof s / sizeof s[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = s[i];
    return n;
}

hipError_t ocb_clear(void *checksum, hipStream_t st)
{
    hipLaunchKernelGGL(k_aes_ocb_clear, dim3(1), dim3(64), 0, st, (uint32_t *)checksum);
    return hipGetLastError();
}

hipError_t ocb_bulk(const void *in, void *out, uint64_t first_block, uint64_t nblocks, const otc_aes_key &K,
                    const uint8_t offset0[16], const uint8_t (*l)[16], void *checksum, hipStream_t st)
{
    if (nblocks == 0) return hipSuccess;
    if (first_block > ((uint64_t)1 << 32) || nblocks > ((uint64_t)1 << 32) - first_block) return hipErrorInvalidValue;
    OcbParams P{};
    P.in = (const uint8_t *)in;
    P.out = (uint8_t *)out;
    P.first = first_block;
    P.end = first_block + nblocks;
    P.checksum = (uint32_t *)checksum;
    words(P.off0, offset0);
    for (int j = 0; j < 33; ++j) words(P.l[j], l[j]);
    /* one workgroup per CU (the 128 / 160 KiB table image), grid-stride over the chunks */
    const uint64_t a0 = first_block & ~(uint64_t)(OCB_PASS - 1u);
    const uint64_t need = (P.end - a0 + OCB_CHUNK - 1) / OCB_CHUNK, cus = (uint64_t)device_cus();
    const dim3 grid((unsigned)(need < cus ? need : cus)), wg(OCB_THREADS);
    const bool dec = K.dir == OTC_DIR_DECRYPT;
    return with_rounds(K.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        if (dec) hipLaunchKernelGGL((k_aes_ocb<NR, true>), grid, wg, 0, st, P, K);
        else hipLaunchKernelGGL((k_aes_ocb<NR, false>), grid, wg, 0, st, P, K);
        return hipGetLastError();
    });
}

hipError_t ocb_finish(const void *in, void *out, uint32_t r, bool dec, const otc_aes_key &Kenc,
                      const uint8_t offset_m[16], const uint8_t l_star[16], const uint8_t l_dollar[16],
                      const uint8_t hash[16], int tag_bytes, const void *checksum, void *tag, hipStream_t st)
{
    if (r > 15 || tag_bytes < 1 || tag_bytes > 16 || Kenc.dir != OTC_DIR_ENCRYPT) return hipErrorInvalidValue;
    OcbFinParams P{};
    P.in = (const uint8_t *)in;
    P.out = (uint8_t *)out;
    P.checksum = (const uint32_t *)checksum;
    P.tag = (uint32_t *)tag;
    words(P.off, offset_m);
    words(P.l_star, l_star);
    words(P.l_dollar, l_dollar);
    words(P.hash, hash);
    P.r = r;
    P.tag_bytes = (uint32_t)tag_bytes;
    P.dec = dec ? 1u : 0u;
    return with_rounds(Kenc.nr, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        hipLaunchKernelGGL((k_aes_ocb_fin<NR>), dim3(1), dim3(64), 0, st, P, Kenc);
        return hipGetLastError();
    });
}

} // namespace otc_impl
