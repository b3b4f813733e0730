/*
 * poly_batch_selftest.cpp -- the batched Poly1305 kernel's decomposition
 * (csrc/hip/chacha_batch.hip, k_poly1305_batch<L>) run on the host, lane by
 * lane, with the very arithmetic the kernel uses (csrc/hip/chacha_dev.h), and
 * compared with poly1305_mac of csrc/cpu/chacha.c:
 *
 *   powers   r^(j+1) in lane j by the parallel prefix (log2 L steps), C = r^L
 *            from lane L - 1, then C^2 .. C^4;
 *   Horner   blocks aligned to the END in whole batches of PL_BATCH passes of L,
 *            A = A C^4 + X0 C^3 + X1 C^2 + X2 C + X3, one carry per batch;
 *   fold     A_j . r^(L-j), the L lanes summed limb by limb in 64 bits, one
 *            carry, the full reduction, + s.
 *
 * For L = 16 and 64, every hashed block count 1 .. 300 and 4096 .. 4100, with
 * random inputs and with the worst case of the carry bound: all-0xFF blocks
 * under the clamped all-ones r (and s all ones).  Every 64-bit accumulator is
 * checked against the bound the kernel file states (< 2^61.7 < 2^62) before it
 * is carried, and every multiplier limb against 2^27.
 *
 * A program of its own: `make bin/poly_batch_selftest`; the test suite also
 * builds it with -fsanitize=address,undefined.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chacha.h"
#include "chacha_dev.h"

using namespace otc_impl;

static int g_fail = 0;

static void expect(bool ok, const char *what, unsigned L, size_t nb)
{
    if (ok) return;
    if (g_fail++ < 10) fprintf(stderr, "FAIL: %s (L = %u, %zu blocks)\n", what, L, nb);
}

static uint32_t ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

static Mul mul_checked(const Fe &a, unsigned L, size_t nb)
{
    for (int k = 0; k < 5; ++k) expect(a.l[k] < (1u << 27), "a multiplier limb reaches 2^27", L, nb);
    return mul_of(a);
}

static Fe carry_checked(uint64_t (&d)[5], unsigned L, size_t nb)
{
    for (int k = 0; k < 5; ++k) expect(d[k] < ((uint64_t)1 << 62), "an accumulator limb reaches 2^62", L, nb);
    return fe_carry(d);
}

/* the kernel's computation over nb full blocks (16 nb bytes), L lanes */
static void tag_by_lanes(unsigned L, const uint8_t key[32], const uint8_t *data, size_t nb, uint8_t tag[16])
{
    const uint32_t rw[4] = {ld32(key) & 0x0FFFFFFFu, ld32(key + 4) & 0x0FFFFFFCu, ld32(key + 8) & 0x0FFFFFFCu,
                            ld32(key + 12) & 0x0FFFFFFCu};
    const uint32_t sw[4] = {ld32(key + 16), ld32(key + 20), ld32(key + 24), ld32(key + 28)};
    std::vector<Fe> pw(L, fe_of_words(rw[0], rw[1], rw[2], rw[3], 0));
    for (unsigned d = 1; d < L; d <<= 1) {
        const std::vector<Fe> old = pw; /* every lane reads its neighbour's value of before the step */
        for (unsigned j = d; j < L; ++j) pw[j] = fe_mul(old[j], mul_checked(old[j - d], L, nb));
    }
    Mul M[PL_BATCH];
    M[0] = mul_checked(pw[L - 1], L, nb);
    Fe c = pw[L - 1];
    for (unsigned i = 1; i < PL_BATCH; ++i) {
        c = fe_mul(c, M[0]);
        M[i] = mul_checked(c, L, nb);
    }
    const size_t nbat = (nb + PL_BATCH * L - 1) / (PL_BATCH * L), pad = nbat * PL_BATCH * L - nb;
    uint64_t sum[5] = {0, 0, 0, 0, 0};
    for (unsigned j = 0; j < L; ++j) {
        Fe A = {{0, 0, 0, 0, 0}};
        for (size_t kb = 0; kb < nbat; ++kb) {
            Fe X[PL_BATCH];
            for (unsigned i = 0; i < PL_BATCH; ++i) {
                const size_t v = (kb * PL_BATCH + i) * L + j;
                if (v >= pad) {
                    const uint8_t *p = data + (v - pad) * 16;
                    X[i] = fe_of_words(ld32(p), ld32(p + 4), ld32(p + 8), ld32(p + 12), 1);
                } else {
                    X[i] = Fe{{0, 0, 0, 0, 0}};
                }
            }
            uint64_t d[5];
            for (int k = 0; k < 5; ++k) d[k] = X[PL_BATCH - 1].l[k];
            fe_mac(d, A, M[PL_BATCH - 1]);
            for (unsigned i = 0; i + 1 < PL_BATCH; ++i) fe_mac(d, X[i], M[PL_BATCH - 2 - i]);
            A = carry_checked(d, L, nb);
        }
        uint64_t d[5] = {0, 0, 0, 0, 0};
        fe_mac(d, A, mul_checked(pw[L - 1 - j], L, nb)); /* r^(L-j) */
        A = carry_checked(d, L, nb);
        for (int k = 0; k < 5; ++k) sum[k] += A.l[k];
    }
    const Fe h = carry_checked(sum, L, nb);
    uint32_t t[4];
    fe_tag(h, sw, t);
    for (int i = 0; i < 16; ++i) tag[i] = (uint8_t)(t[i >> 2] >> (8 * (i & 3)));
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint8_t rnd8()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint8_t)(g_rng >> 32);
}

static void run(unsigned L, size_t nb, bool worst)
{
    std::vector<uint8_t> data(nb * 16);
    uint8_t key[32], want[16], got[16];
    if (worst) {
        memset(data.data(), 0xFF, data.size());
        memset(key, 0xFF, 32);
    } else {
        for (auto &b : data) b = rnd8();
        for (auto &b : key) b = rnd8();
    }
    poly1305_mac(key, data.data(), data.size(), want);
    tag_by_lanes(L, key, data.data(), nb, got);
    expect(memcmp(want, got, 16) == 0, worst ? "worst-case tag differs" : "random tag differs", L, nb);
}

int main()
{
    size_t cases = 0;
    for (unsigned L : {16u, 64u}) {
        std::vector<size_t> counts;
        for (size_t nb = 1; nb <= 300; ++nb) counts.push_back(nb);
        for (size_t nb = 4096; nb <= 4100; ++nb) counts.push_back(nb);
        for (size_t nb : counts) {
            run(L, nb, false);
            run(L, nb, true);
            cases += 2;
        }
    }
    if (g_fail) {
        fprintf(stderr, "poly_batch_selftest: %d failures\n", g_fail);
        return 1;
    }
    printf("poly_batch_selftest: OK (%zu cases)\n", cases);
    return 0;
}
