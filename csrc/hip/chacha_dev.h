/*
 * chacha_dev.h -- the device code that the two ChaCha20-Poly1305 kernel files
 * (chacha.hip: one message over the chip; chacha_batch.hip: many records per
 * launch) share, in one copy, the way ghash_dev.h serves the two GHASH files:
 * the ChaCha20 block function with its rotations and the quad transpose of
 * the bulk store layout, and the Poly1305 field arithmetic -- Fe / Mul /
 * fe_mac / fe_carry / fe_mul / fe_of_words and the final reduction.
 * Everything is file-local (an unnamed namespace).
 *
 * The field arithmetic is plain C++ and host-callable: the kernel files' host
 * code computes powers with it, and csrc/cpu/poly_batch_selftest.cpp includes
 * this header with an ordinary host compiler (no HIP) to check the batched
 * kernel's decomposition and carry bounds against csrc/cpu/chacha.c.  The
 * ChaCha20 part uses gfx950 builtins and exists under hipcc only.
 *
 * Layouts and carry bounds: chacha.hip's header.
 */
#ifndef OTC_CHACHA_DEV_H
#define OTC_CHACHA_DEV_H

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
#define __host__
#define __device__
#define __forceinline__ inline
#endif

namespace otc_impl {
namespace {

#ifdef __HIPCC__
/* ======================= ChaCha20 ========================================= */

/* rotations: 16 and 8 as byte permutes, 12 and 7 as v_alignbit_b32 */
__device__ __forceinline__ uint32_t cc_rot16(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x01000302u); }
__device__ __forceinline__ uint32_t cc_rot8(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x02010003u); }
__device__ __forceinline__ uint32_t cc_rot12(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 20); }
__device__ __forceinline__ uint32_t cc_rot7(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 25); }

__device__ __forceinline__ void cc_qr(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d)
{
    a += b; d = cc_rot16(d ^ a);
    c += d; b = cc_rot12(b ^ c);
    a += b; d = cc_rot8(d ^ a);
    c += d; b = cc_rot7(b ^ c);
}

/* the keystream block of counter `ctr` under the key and nonce words */
__device__ __forceinline__ void cc_block(const uint32_t (&key)[8], const uint32_t (&nonce)[3], uint32_t ctr,
                                         uint32_t (&x)[16])
{
    const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                            key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                            ctr, nonce[0], nonce[1], nonce[2]};
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        cc_qr(x[0], x[4], x[8], x[12]);
        cc_qr(x[1], x[5], x[9], x[13]);
        cc_qr(x[2], x[6], x[10], x[14]);
        cc_qr(x[3], x[7], x[11], x[15]);
        cc_qr(x[0], x[5], x[10], x[15]);
        cc_qr(x[1], x[6], x[11], x[12]);
        cc_qr(x[2], x[7], x[8], x[13]);
        cc_qr(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] += s[i];
}

/* One butterfly of the 4x4 transpose among the lanes of a quad: with the
 * partner lane q ^ D, exchange quarter e | D of the lane whose bit is clear
 * with quarter e of the lane whose bit is set (hi). */
template <int D>
__device__ __forceinline__ void cc_xchg(uint32_t (&x)[16], bool hi)
{
    constexpr int ctrl = D == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : 0x4E /* [2,3,0,1] */;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e & D) continue;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            uint32_t &lo = x[4 * e + w], &up = x[4 * (e | D) + w];
            const uint32_t send = hi ? lo : up;
            const uint32_t recv = (uint32_t)__builtin_amdgcn_update_dpp((int)send, (int)send, ctrl, 0xF, 0xF, false);
            lo = hi ? recv : lo;
            up = hi ? up : recv;
        }
    }
}
#endif /* __HIPCC__ */

/* ======================= Poly1305 ========================================= */

constexpr uint32_t PL_BATCH = 4;             /* passes per carry */
constexpr uint32_t M26 = 0x3FFFFFFu;

struct Fe {
    uint32_t l[5]; /* value = sum l[i] 2^(26 i) */
};
struct Mul {
    uint32_t r[5], s[4]; /* a multiplier's limbs and 5 * r[1..4] */
};

__host__ __device__ __forceinline__ Mul mul_of(const Fe &a)
{
    Mul m;
    for (int i = 0; i < 5; ++i) m.r[i] = a.l[i];
    for (int i = 0; i < 4; ++i) m.s[i] = a.l[i + 1] * 5u;
    return m;
}

/* d += a . m, unreduced (five multiply-adds per limb) */
__host__ __device__ __forceinline__ void fe_mac(uint64_t (&d)[5], const Fe &a, const Mul &m)
{
    const uint64_t a0 = a.l[0], a1 = a.l[1], a2 = a.l[2], a3 = a.l[3], a4 = a.l[4];
    d[0] += a0 * m.r[0] + a1 * m.s[3] + a2 * m.s[2] + a3 * m.s[1] + a4 * m.s[0];
    d[1] += a0 * m.r[1] + a1 * m.r[0] + a2 * m.s[3] + a3 * m.s[2] + a4 * m.s[1];
    d[2] += a0 * m.r[2] + a1 * m.r[1] + a2 * m.r[0] + a3 * m.s[3] + a4 * m.s[2];
    d[3] += a0 * m.r[3] + a1 * m.r[2] + a2 * m.r[1] + a3 * m.r[0] + a4 * m.s[3];
    d[4] += a0 * m.r[4] + a1 * m.r[3] + a2 * m.r[2] + a3 * m.r[1] + a4 * m.r[0];
}

/* one carry chain: limbs 0, 2, 3, 4 below 2^26, limb 1 below 2^26 + 2^13 */
__host__ __device__ __forceinline__ Fe fe_carry(uint64_t (&d)[5])
{
    d[1] += d[0] >> 26;
    d[2] += d[1] >> 26;
    d[3] += d[2] >> 26;
    d[4] += d[3] >> 26;
    const uint64_t t = (d[0] & M26) + (d[4] >> 26) * 5; /* 2^130 = 5 */
    Fe f;
    f.l[0] = (uint32_t)t & M26;
    f.l[1] = (uint32_t)((d[1] & M26) + (t >> 26));
    f.l[2] = (uint32_t)d[2] & M26;
    f.l[3] = (uint32_t)d[3] & M26;
    f.l[4] = (uint32_t)d[4] & M26;
    return f;
}

__host__ __device__ __forceinline__ Fe fe_mul(const Fe &a, const Mul &m)
{
    uint64_t d[5] = {0, 0, 0, 0, 0};
    fe_mac(d, a, m);
    return fe_carry(d);
}

/* a 16-byte block (little-endian words) plus hibit * 2^128 */
__host__ __device__ __forceinline__ Fe fe_of_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hibit)
{
    Fe f;
    f.l[0] = w0 & M26;
    f.l[1] = (w0 >> 26 | w1 << 6) & M26;
    f.l[2] = (w1 >> 20 | w2 << 12) & M26;
    f.l[3] = (w2 >> 14 | w3 << 18) & M26;
    f.l[4] = w3 >> 8 | hibit << 24;
    return f;
}

/* t = ((h mod p) + s) mod 2^128 as little-endian words, from a carried h and
 * the words of s: the full reduction, without a branch on the value */
__host__ __device__ __forceinline__ void fe_tag(const Fe &h, const uint32_t (&skey)[4], uint32_t (&t)[4])
{
    /* the full reduction: two carry chains bring h below 2^130 with every limb below 2^26 ... */
    uint32_t h0 = h.l[0], h1 = h.l[1], h2 = h.l[2], h3 = h.l[3], h4 = h.l[4], c;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        c = h0 >> 26; h0 &= M26; h1 += c;
        c = h1 >> 26; h1 &= M26; h2 += c;
        c = h2 >> 26; h2 &= M26; h3 += c;
        c = h3 >> 26; h3 &= M26; h4 += c;
        c = h4 >> 26; h4 &= M26; h0 += c * 5;
    }
    c = h0 >> 26; h0 &= M26; h1 += c;
    /* ... then g = h - p = h + 5 - 2^130, taken by a mask where it did not borrow: no branch on the value */
    uint32_t g0 = h0 + 5;
    c = g0 >> 26; g0 &= M26;
    uint32_t g1 = h1 + c;
    c = g1 >> 26; g1 &= M26;
    uint32_t g2 = h2 + c;
    c = g2 >> 26; g2 &= M26;
    uint32_t g3 = h3 + c;
    c = g3 >> 26; g3 &= M26;
    const uint32_t g4 = h4 + c - (1u << 26);
    const uint32_t take = (g4 >> 31) - 1u; /* all ones iff h >= p */
    h0 = (h0 & ~take) | (g0 & take);
    h1 = (h1 & ~take) | (g1 & take);
    h2 = (h2 & ~take) | (g2 & take);
    h3 = (h3 & ~take) | (g3 & take);
    h4 = (h4 & ~take) | (g4 & take);
    /* h mod 2^128, plus s mod 2^128 */
    const uint32_t w0 = h0 | h1 << 26, w1 = h1 >> 6 | h2 << 20, w2 = h2 >> 12 | h3 << 14, w3 = h3 >> 18 | h4 << 8;
    uint64_t f = (uint64_t)w0 + skey[0];
    t[0] = (uint32_t)f;
    f = (uint64_t)w1 + skey[1] + (f >> 32);
    t[1] = (uint32_t)f;
    f = (uint64_t)w2 + skey[2] + (f >> 32);
    t[2] = (uint32_t)f;
    f = (uint64_t)w3 + skey[3] + (f >> 32);
    t[3] = (uint32_t)f;
}

} // namespace
} // namespace otc_impl

#endif
