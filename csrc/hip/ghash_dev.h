/*
 * ghash_dev.h -- the GF(2^128) device code of the GHASH kernels, in one copy
 * for both kernel files (aes_gcm.hip, aes_gcm_batch.hip): the multiplication
 * by a constant through its positional byte table, the doubling, and the
 * kernel that builds such tables.  Everything is file-local (an unnamed
 * namespace): each kernel file instantiates what it uses.  The chip-wide level
 * kernel over such tables is in ghash_levels_dev.h.
 *
 * Bit order: the leftmost bit of a block (bit 7 of byte 0) is x^0, "times x"
 * is a right shift of the byte string, reduction by 0xE1 || 0^120 -- the same
 * convention as csrc/cpu/aes.c, whose nibble tables are these byte tables in
 * small.  Blocks and table entries stay in memory byte order (little-endian
 * words); only the doubling works on big-endian words.  The tables themselves:
 * aes_gcm.hip's header.
 */
#ifndef OTC_GHASH_DEV_H
#define OTC_GHASH_DEV_H

#include <hip/hip_runtime.h>

namespace otc_impl {
namespace {

constexpr uint32_t GF_TAB = 16 * 256; /* entries of one constant's table */

__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }

/* x . C by the positional table of C (LDS): 16 reads of 16 B */
__device__ __forceinline__ uint4 gh_mul(const uint4 *T, uint4 x)
{
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    uint4 r = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int p = 0; p < 16; ++p) r = xor4(r, T[p * 256 + ((w[p >> 2] >> (8 * (p & 3))) & 0xFFu)]);
    return r;
}

/* big-endian words <-> memory-order words */
__device__ __forceinline__ uint4 gh_swap(uint4 v)
{
    return make_uint4(__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w));
}
/* v . x on big-endian words */
__device__ __forceinline__ uint4 gh_mulx(uint4 v)
{
    const uint32_t carry = v.w & 1u;
    return make_uint4((v.x >> 1) ^ (carry ? 0xE1000000u : 0u), (v.y >> 1) | (v.x << 31), (v.z >> 1) | (v.y << 31),
                      (v.w >> 1) | (v.z << 31));
}

/* N constants in memory order, by value */
template <int N>
struct GfConsts {
    uint4 c[N];
};

/* tab[t] = the table of K.c[t]: one workgroup per (table, byte position), one
 * thread per byte value -- a grid of 16 N workgroups of 256 threads */
template <int N>
__global__ __launch_bounds__(256) void k_gf128_tables(GfConsts<N> K, uint4 *tab)
{
    const uint32_t t = blockIdx.x >> 4, pos = blockIdx.x & 15u, b = threadIdx.x;
    uint4 v = gh_swap(K.c[t]);
    for (uint32_t i = 0; i < 8 * pos; ++i) v = gh_mulx(v);
    uint4 e = make_uint4(0, 0, 0, 0);
    for (uint32_t k = 0; k < 8; ++k) { /* the byte's leftmost bit is the lowest power */
        if (b & (0x80u >> k)) e = xor4(e, v);
        v = gh_mulx(v);
    }
    tab[(size_t)t * GF_TAB + pos * 256 + b] = gh_swap(e);
}

} // namespace
} // namespace otc_impl

#endif
