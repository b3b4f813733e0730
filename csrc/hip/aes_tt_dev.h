/*
 * aes_tt_dev.h -- the device helpers of the LDS T-table kernels that more
 * than one kernel file uses (aes_tt.hip, aes_xts.hip): the constant tables,
 * the 4-table LDS images and their fill, the one-op lookup addressing, the
 * round loops of both directions, the 16-byte block accesses and the kernel
 * opening.  Everything is file-local (an unnamed namespace) and forced
 * inline: each kernel file carries its own copy of the tables.
 * The layout and its measurements: aes_tt.hip's header and docs/PERF.md.
 */
#ifndef OTC_AES_TT_DEV_H
#define OTC_AES_TT_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "otc_device.h"

namespace {

using namespace otc_dev;

__device__ const AesTables g_tab = make_tables();

/* second table (byte 2 of the address taken from lane word byte 2 = 1) */
constexpr uint32_t SEL_HI(int k) { return 0x0c020000u | ((uint32_t)(4 + k) << 8); }

__device__ __forceinline__ uint32_t lds_at(const uint32_t *tbl, uint32_t byte_addr)
{
    return *(const uint32_t *)((const char *)tbl + byte_addr);
}

/* The claim kernels' tables live in dynamic LDS (aes_tt.hip tt_lds), which starts
 * at address 0 -- those kernels declare no static LDS (tests/test_isa_cpu.py
 * checks their descriptors' fixed group segment size is 0).  hipcc learns the
 * dynamic base only after instruction selection, so addressing through the
 * extern array adds it to every lookup (v_add_u32 v, 0, v: +1792 VALU per
 * AES-256 ECB claim-loop iteration, +36% instructions, ~8-10% slower).  Their
 * lookups take the integer LDS address instead. */
struct DynTbl {
};
__device__ __forceinline__ uint32_t lds_at(DynTbl, uint32_t byte_addr)
{
    return *(const __attribute__((address_space(3))) uint32_t *)(uintptr_t)byte_addr;
}

/* LDS address of table k's entry for byte k of state word w: byte 1 <- that
 * byte, bytes 0 / 2 <- the per-lane, per-table constant lkk (whose bytes 1
 * and 3 are zero).  For k = 1 the byte is already in place, so the address is
 * one bit-field insert (v_bfi_b32, ~0.75 nJ per wave-instruction) instead of
 * a v_perm_b32 (~1.03 nJ, profiles/r3/energy/): a quarter of all lookups. */
__device__ __forceinline__ uint32_t tt_addr(uint32_t w, uint32_t lkk, int k)
{
    if (k == 1) {
        /* written out: hipcc turns the C form into v_and_or_b32 (0.83 nJ,
         * and a costlier VOP3 issue than v_perm) */
        uint32_t r;
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(0x0000FF00u), "v"(w), "v"(lkk));
        return r;
    }
    return __builtin_amdgcn_perm(w, lkk, SEL_HI(k));
}

/* 4-table layout (TBL4): T_k (k = 0..3, T_k = rotl(T0, 8k)) each replicated
 * 32 ways.  Row x of region r (r = k >> 1, 64 KiB each) holds T_{2r} for lanes
 * 0..31 in bytes 0..127 and T_{2r+1} in bytes 128..255:
 *   addr(k, x, lane) = (k >> 1) << 16 | x << 8 | (k & 1) << 7 | (lane & 31) << 2
 * so again one v_perm per lookup (byte 1 <- x, bytes 0/2 <- a per-lane,
 * per-table constant) and no rotations: 16 perm + 8 bitop3 per round instead
 * of 16 + 12 + 8.  Bank = lane & 31 for every lookup -> conflict free. */
/* the word that fills 16-byte row q (< 8192) of the image of T0 = t0 */
template <class Q>
__device__ __forceinline__ uint32_t tbl4_row(const uint32_t *t0, Q q)
{
    const Q r = q >> 12, x = (q >> 4) & 255, half = (q >> 3) & 1;
    const Q k = 2 * r + half;
    const uint32_t t = t0[x];
    return k ? ((t << (8 * k)) | (t >> (32 - 8 * k))) : t;
}
/* nt threads fill the image: nt is the workgroup size, a constant
 * (fill_tbl4<THREADS>) or blockDim.x where the launch chooses it */
template <class Q>
__device__ __forceinline__ void fill_tbl4(uint32_t *lds, const uint32_t *te0, Q nt)
{
    uint4 *l4 = reinterpret_cast<uint4 *>(lds);
    for (Q q = threadIdx.x; q < 8192; q += nt) {
        const uint32_t v = tbl4_row(te0, q);
        l4[q] = make_uint4(v, v, v, v);
    }
}
template <int THREADS>
__device__ __forceinline__ void fill_tbl4(uint32_t *lds, const uint32_t *te0)
{
    fill_tbl4(lds, te0, THREADS);
}

__device__ __forceinline__ void tbl4_lane_consts(uint32_t lane, uint32_t (&lk)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) lk[k] = ((uint32_t)(k >> 1) << 16) | ((uint32_t)(k & 1) << 7) | ((lane & 31u) << 2);
}

/* Per round, issue every lookup of all B blocks before combining any of
 * them (+0..1.6%, profiles/r1/otbench_issue_all_ab.jsonl).  hipcc otherwise consumes each ds_read right away (1-3 LDS ops
 * in flight per wave); with at most 16 waves per CU (the 128 KiB table allows
 * one workgroup) that starves the LDS pipe.  gfx9 lgkmcnt still caps a wave at
 * 15 outstanding LDS ops. */
template <int B, class TBL>
__device__ __forceinline__ void issue_lookups4(TBL tbl, const uint32_t (&lk)[4], const uint32_t (&s)[B][4],
                                               uint32_t (&a)[B][4][4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k) a[b][j][k] = lds_at(tbl, tt_addr(s[b][(j + k) & 3], lk[k], k));
}

template <int R0, int NR, int B, class TBL>
__device__ __forceinline__ void enc_rounds4_from(TBL tbl, const uint32_t (&lk)[4], const otc_aes_key &K,
                                                 uint32_t (&s)[B][4])
{
#pragma unroll
    for (int r = R0; r < NR; ++r) {
        uint32_t t[B][4];
        uint32_t a[B][4][4];
        issue_lookups4(tbl, lk, s, a);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < B; ++b)
                t[b][j] = xor3(xor3(a[b][j][0], a[b][j][1], a[b][j][2]), a[b][j][3], K.rk[4 * r + j]);
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[b][j] = t[b][j];
    }
    uint32_t t[B][4];
    uint32_t a[B][4][4];
    issue_lookups4(tbl, lk, s, a);
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            /* S[x] sits in byte 1 of T0, byte 2 of T1, byte 3 of T2, byte 0 of T3 */
            uint32_t lo = __builtin_amdgcn_perm(a[b][j][1], a[b][j][0], 0x0c0c0601u);
            uint32_t hi = __builtin_amdgcn_perm(a[b][j][3], a[b][j][2], 0x04030c0cu);
            t[b][j] = xor3(lo, hi, K.rk[4 * NR + j]);
        }
    }
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[b][j] = t[b][j];
}

/* Decryption 4-table layout: Td0..Td3 as above (128 KiB) plus the inverse
 * S-box replicated 32 ways as byte-splatted words at 0x20000 + x*128 + lane*4
 * (32 KiB): 160 KiB, the whole LDS of a CU.  The final-round address is one
 * v_perm + one shift: perm gives 0x40000 | x << 8 | lane*8, >> 1 gives the
 * row-128 address. */
template <int THREADS>
__device__ __forceinline__ void fill_dtbl4(uint32_t *lds, const uint32_t *td0, const uint32_t *is4)
{
    uint4 *l4 = reinterpret_cast<uint4 *>(lds);
    for (int q = threadIdx.x; q < 8192 + 2048; q += THREADS) {
        /* past the four tables: 8 uint4 (32 dwords) per 128-byte row */
        const uint32_t v = q < 8192 ? tbl4_row(td0, q) : is4[(q - 8192) >> 3];
        l4[q] = make_uint4(v, v, v, v);
    }
}

template <int NR, int B, class TBL>
__device__ __forceinline__ void dec_rounds4(TBL tbl, const uint32_t (&lk)[4], uint32_t lk_is2,
                                            const otc_aes_key &K, uint32_t (&s)[B][4])
{
#pragma unroll
    for (int r = 1; r < NR; ++r) {
        uint32_t t[B][4];
#pragma unroll
        for (int b = 0; b < B; ++b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t a0 = lds_at(tbl, tt_addr(s[b][j], lk[0], 0));
                uint32_t a1 = lds_at(tbl, tt_addr(s[b][(j + 3) & 3], lk[1], 1));
                uint32_t a2 = lds_at(tbl, tt_addr(s[b][(j + 2) & 3], lk[2], 2));
                uint32_t a3 = lds_at(tbl, tt_addr(s[b][(j + 1) & 3], lk[3], 3));
                t[b][j] = xor3(xor3(a0, a1, a2), a3, K.rk[4 * r + j]);
            }
        }
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[b][j] = t[b][j];
    }
    uint32_t t[B][4];
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t a0 = lds_at(tbl, tt_addr(s[b][j], lk_is2, 0) >> 1);
            uint32_t a1 = lds_at(tbl, tt_addr(s[b][(j + 3) & 3], lk_is2, 1) >> 1);
            uint32_t a2 = lds_at(tbl, tt_addr(s[b][(j + 2) & 3], lk_is2, 2) >> 1);
            uint32_t a3 = lds_at(tbl, tt_addr(s[b][(j + 1) & 3], lk_is2, 3) >> 1);
            uint32_t lo = __builtin_amdgcn_perm(a1, a0, 0x0c0c0400u);
            uint32_t hi = __builtin_amdgcn_perm(a3, a2, 0x04000c0cu);
            t[b][j] = xor3(lo, hi, K.rk[4 * NR + j]);
        }
    }
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[b][j] = t[b][j];
}

/* 16-byte block `blk` of a buffer (otc_device.h ld_u4 / st_u4), three ways:
 * M_CACHED plain; M_STREAM and M_BATCH with the non-temporal bit by their
 * build arms, M_BATCH also through the global address space.
 * M_STREAM (the streaming form) is for the kernels whose wave
 * loads / stores 1 KiB of consecutive blocks per instruction -- ECB, CTR, the
 * CFB / CBC decryptions and their claim forms: the non-temporal bit
 * (OTC_TT_NT, default 1).  Round 6 A/B (profiles/r6/ntall_ab/, AES-256, 2
 * reps): the splits +0.8-1.5% (CBC-dec 8 GiB 1205-1208 vs 1188-1194), ECB-dec
 * +1%, T-table CTR even.  NOT the serial segment chains: there each lane
 * walks its own segment 16 B at a time, the next block sits in the line just
 * read, and without the line in cache every block refetches it -- CBC
 * segment encryption fell from 1114-1120 to 472-476 GB/s with the bit.
 * M_BATCH is for the batch kernel's message buffers, which come from
 * descriptors as plain addresses (otc_device.h ld_u4 on GLOBAL); the
 * non-temporal bit (OTC_BATCH_NT, default 1) because each tile is read and
 * written once, lane-linear.  Round 6 A/B, 3 reps (profiles/r6/batch_nt/):
 * 1024 x 1 MiB packed 1484-1492 vs 1446-1460 GB/s, 16384 x 4 KiB packed
 * 1156-1164 vs 1136-1144, 262144 x 4 KiB 1191-1212 vs 1173-1192, 65536 x
 * 1504 B even. */
#ifndef OTC_TT_NT
#define OTC_TT_NT 1
#endif
#ifndef OTC_BATCH_NT
#define OTC_BATCH_NT 1
#endif
enum Mem : int { M_CACHED, M_STREAM, M_BATCH };
template <Mem M>
constexpr bool MEM_NT = M == M_STREAM ? OTC_TT_NT != 0 : M == M_BATCH && OTC_BATCH_NT != 0;
template <Mem M = M_CACHED>
__device__ __forceinline__ uint4 ld16(const uint8_t *p, uint64_t blk)
{
    return ld_u4<MEM_NT<M>, M == M_BATCH>(p + 16 * blk);
}
template <Mem M = M_CACHED>
__device__ __forceinline__ void st16(uint8_t *p, uint64_t blk, uint4 v)
{
    st_u4<MEM_NT<M>, M == M_BATCH>(p + 16 * blk, v);
}

/* How a kernel of THREADS threads opens: the workgroup fills the encryption
 * image, and each thread gets its lookup constants and its place.  (wave is
 * not wave-uniform to hipcc: the kernels that need that take it through
 * readfirstlane themselves.) */
struct Place {
    uint32_t lane, wave;
};
template <int THREADS>
__device__ __forceinline__ Place tt_open(uint32_t *tbl, uint32_t (&lk)[4])
{
    fill_tbl4<THREADS>(tbl, g_tab.te0);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    tbl4_lane_consts(lane, lk);
    return {lane, wave};
}

} // namespace

#endif
