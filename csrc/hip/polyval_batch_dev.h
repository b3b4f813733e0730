/*
 * polyval_batch_dev.h -- what the two batched hash kernels over per-record
 * NIBBLE TABLES share: k_polyval_batch (aes_gcm_siv_batch.hip, a POLYVAL key per
 * record, tables built per record) and k_ghash_mk_batch (aes_gcm_mk_batch.hip,
 * GHASH through RFC 8452 appendix A, tables copied from a per-key image).  The
 * record as the hash sees it, the loads that never read at or past a buffer's
 * end, the product on a table in LDS, the wave-level ordering of LDS accesses
 * and the placement of a 16-lane record on the lanes of a wave.  The field
 * arithmetic itself is polyval_dev.h's.
 */
#ifndef OTC_POLYVAL_BATCH_DEV_H
#define OTC_POLYVAL_BATCH_DEV_H

#include <hip/hip_runtime.h>

#include "otc_device.h"
#include "polyval_dev.h"

namespace {

using namespace otc_dev;

typedef const __attribute__((address_space(1))) uint8_t *gptr8;

constexpr uint32_t SB_THREADS = 256; /* 4 waves: they share nothing but the launch */
constexpr uint32_t SB_BATCH = 4;     /* passes loaded ahead */

/* one record as the hash sees it */
struct SbRec {
    gptr8 data, aad;
    uint64_t nbytes, aad_bytes;
    uint64_t na, nd; /* blocks of the AAD and of the data */
};

/* the 16 bytes at p + off, those at or past `end` as zero; never reads them
 * (aes_gcm_batch.hip's gb_bytes: that file's kernels stay as they are) */
__device__ __forceinline__ uint4 sb_bytes(gptr8 p, uint64_t off, uint64_t end)
{
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t t = 0; t < 16; ++t) {
        const uint32_t v = off + t < end ? (uint32_t)p[off + t] : 0u;
        w[t >> 2] |= v << (8 * (t & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* block i (< na + nd) of pad16(AAD) || pad16(data), as loaded */
__device__ __forceinline__ uint4 sb_text_block(const SbRec &R, uint64_t i)
{
    if (i < R.na) return sb_bytes(R.aad, i * 16, R.aad_bytes); /* any alignment: bytes */
    const uint64_t off = (i - R.na) * 16;
    if (off + 16 <= R.nbytes) return ld_u4<false, true>((const uint8_t *)R.data + off);
    return sb_bytes(R.data, off, R.nbytes);
}

/* record m's descriptor (six 64-bit words: in, out, nbytes, aad, aad_bytes, one more) */
__device__ __forceinline__ SbRec sb_record(const uint64_t *D, uint32_t hash_out)
{
    SbRec R;
    R.data = (gptr8)D[hash_out ? 1 : 0];
    R.nbytes = D[2];
    R.aad = (gptr8)D[3];
    R.aad_bytes = D[4];
    R.na = (R.aad_bytes + 15) >> 4;
    R.nd = (R.nbytes + 15) >> 4;
    return R;
}

/* dot(a, C) over C's nibble table T (LDS): every lookup's address comes from a alone */
__device__ __forceinline__ uint4 sb_mul(const uint4 *T, uint4 a)
{
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w};
    uint32_t z[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const uint4 e = T[pv4_nibble(aw, k)];
        const uint32_t t[4] = {e.x, e.y, e.z, e.w};
        pv4_step(z, t);
    }
    return make_uint4(z[0], z[1], z[2], z[3]);
}

__device__ __forceinline__ uint4 sb_xor(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }

/* what one lane of a wave wrote to LDS, the wave's other lanes read after this: a
 * wave's LDS accesses execute in order, so only the compiler must keep them so */
__device__ __forceinline__ void sb_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* The 16-lane form puts a record on one of the four 16-lane groups in which the LDS serves a
 * wave's ds_read_b128 -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- and not on
 * 16 consecutive lanes: lanes of one group then read ONE record's table, where two lanes either
 * take the same entry (one address, broadcast) or entries in different banks (an entry is 4 banks,
 * a table all 64).  On consecutive lanes a group mixes the tables of the wave's four records, which
 * lie on the same banks, and random nibbles collide about 3 deep.  sb_place: physical lane ->
 * record of the wave and lane of the record; sb_lane_of: its inverse. */
__device__ __forceinline__ void sb_place(uint32_t lane, uint32_t &rec, uint32_t &l)
{
    const uint32_t p = lane & 31u, q = p >> 2; /* q: the lane's quad, 0 .. 7 */
    const uint32_t g = (0x96u >> q) & 1u;      /* quads 1, 2, 4, 7 belong to the second group */
    rec = 2u * (lane >> 5) + g;
    l = g ? (p < 12 ? p - 4 : p < 20 ? p - 8 : p - 16) : (p < 4 ? p : p < 16 ? p - 8 : p - 12);
}
__device__ __forceinline__ uint32_t sb_lane_of(uint32_t rec, uint32_t l)
{
    const uint32_t p = rec & 1u ? (l < 8 ? l + 4 : l < 12 ? l + 8 : l + 16) : (l < 4 ? l : l < 8 ? l + 8 : l + 12);
    return 32u * (rec >> 1) + p;
}

/* the record of its workgroup's group that thread tid works on, and its lane there */
template <uint32_t L>
__device__ __forceinline__ void sb_thread(uint32_t tid, uint32_t &rec, uint32_t &l)
{
    static_assert(L == 16 || L == 64, "a record is a quarter of a wave or a whole one");
    rec = tid / L;
    l = tid % L;
    if constexpr (L == 16) {
        uint32_t r;
        sb_place(tid & 63u, r, l);
        rec = 4u * (tid >> 6) + r;
    }
}

/* one step of the fold: lane l's value from lane l + d of its record (a lane without one takes
 * its own value, which nobody uses) */
template <uint32_t L>
__device__ __forceinline__ uint4 sb_from_lane(uint4 A, uint32_t rec, uint32_t l, uint32_t d)
{
    const uint32_t ld = l + d < L ? l + d : l;
    const int src = (int)(L == 16 ? sb_lane_of(rec & 3u, ld) : ld);
    return make_uint4((uint32_t)__shfl((int)A.x, src), (uint32_t)__shfl((int)A.y, src), (uint32_t)__shfl((int)A.z, src),
                      (uint32_t)__shfl((int)A.w, src));
}

} // namespace

#endif
