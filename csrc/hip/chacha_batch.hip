/*
 * chacha_batch.hip -- ChaCha20-Poly1305 (RFC 8439 section 2.8) over MANY short
 * records in one chain of launches (otc_chacha20_poly1305_batch): every record
 * with its own key, its own nonce, its own AAD and its own 16-byte tag.
 *
 * chacha.hip spreads ONE message over the chip and computes what depends on
 * the key -- block 0, the powers of r -- on the host, which a 1-4 KiB record
 * cannot carry.  Here r is bytes 0..15 of a record's block 0 and never exists
 * on the host: the one-time keys and the powers are made on the device.
 *
 *   prep      one lane per record: block 0 under the record's key and nonce;
 *             r (clamped) and s go to the caller's workspace, 32 bytes each.
 *   cipher    the unit is a tile: one 4 KiB pass (64 blocks) of one record,
 *             found through the host-built tile map (tile_msg[t],
 *             tile_first[m]).  A wave reads its record's descriptor, key and
 *             nonce from memory -- wave-uniform, held in SGPRs -- and computes
 *             block 1 + 64 p + lb per lane.  A whole pass uses k_chacha20_bulk's
 *             transposed layout (chacha.hip's header: 16-byte non-temporal
 *             accesses, two quad_perm butterflies, 1 KiB per instruction); the
 *             record's last, partial pass keeps the layout with every 16-byte
 *             piece guarded by the length, and the one piece that holds the
 *             record's end moved byte by byte (a first version moved the whole
 *             partial pass byte by byte like k_chacha20_edge: 122 GB/s for
 *             1 KiB records, docs/PERF.md "Batched ChaCha20-Poly1305").  The plaintext of a pass is loaded before its
 *             keystream is stored, so in place is safe.  A wave takes CB_RUN = 4
 *             consecutive tiles and a workgroup is CB_WAVES = 4 waves, the grid
 *             one workgroup per 16 tiles: chacha.hip's numbers, NOT measured for
 *             the batch.
 *   hash      k_poly1305_batch<L>, L = 16 or 64 lanes per record (64 / L
 *             records per wave).  Record m hashes
 *                 pad16(AAD) || pad16(data) || le64(aad_bytes) le64(nbytes),
 *             nb = ceil(aad/16) + ceil(n/16) + 1 full blocks, each with its 2^128
 *             bit, the length block formed from the descriptor.  The blocks are
 *             aligned to the END of the record in whole batches of PL_BATCH = 4
 *             passes of L blocks; zero blocks in front change nothing.  Lane j
 *             runs Horner under C = r^L over the blocks L apart,
 *                 A = A C^4 + X0 C^3 + X1 C^2 + X2 C + X3      per batch,
 *             a batch loaded while the one before it is multiplied, carried
 *             once per batch.  Then lane j multiplies its accumulator by
 *             r^(L-j), the L lanes are summed limb by limb by cross-lane moves
 *             (log2 L steps), and the same lanes do the full reduction mod
 *             2^130 - 5, add s and write the tag; on decryption they compare it
 *             with the expected tag (OR of the XORs, no early exit), write the
 *             verdict and zero the tag of a record that fails.
 *   powers    r^1 .. r^L of a record are built in the kernel by a parallel
 *             prefix over its lanes: at step d = 1, 2, 4, .. lane j >= d
 *             multiplies its power by lane j - d's, so lane j ends with r^(j+1)
 *             after log2 L multiplications.  C^2 .. C^4 cost three more.  The
 *             multipliers are per record: VGPRs when L = 16.  No LDS.
 *   wipe      the output of every record that failed is zeroed by the batched
 *             GCM's wipe kernel (aes_gcm_batch.hip), which reads the columns
 *             that otc_chacha_msg shares with otc_gcm_msg.
 *   grid      the hash runs one workgroup of 4 waves per 16 (L = 16) or 4
 *             (L = 64) records, no stride loop: not measured against a
 *             persistent grid.
 *
 * Carry bounds (chacha.hip's argument, chacha_dev.h's arithmetic).  An operand
 * limb is below 2^28: a raw block limb is below 2^26, a carried value below
 * 2^26 + 2^13.  A MULTIPLIER limb must be a carried value below 2^27 so that
 * 5 b_j < 2^29.33 and one term stays below 2^57.33.  Every multiplier here is
 * the result of fe_carry: r itself (clamped, raw limbs below 2^26), the prefix
 * products, C^2 .. C^4 -- all below 2^26 + 2^13.  One multiplication adds five
 * terms, < 2^59.66; a batch accumulates PL_BATCH = 4 of them plus one added
 * block before it carries: < 2^61.7 in 64 bits.  The prefix, the fold and the
 * powers of C are single multiplications.  The lane sum adds at most 64
 * carried limbs: < 2^33 in 64 bits.  csrc/cpu/poly_batch_selftest.cpp runs this
 * decomposition on the host with all-0xFF data under the all-ones clamped r.
 *
 * Nothing branches on, or addresses memory by, key, keystream, data or hash
 * state; branches are on lengths and on the call's shape.  Nothing reads or
 * writes outside [in, in + n), [out, out + n), [aad, aad + aad_bytes) and the
 * arrays of the call: whole 16-byte accesses only where 16 bytes are inside,
 * bytes otherwise.  Every value is written with ordinary vector stores.
 */
#include <hip/hip_runtime.h>

#include "chacha_dev.h"
#include "otc_device.h"
#include "otc_kernels.h"

namespace otc_impl {

using otc_dev::lane_id;
using otc_dev::ld_u4;
using otc_dev::st_u4;

namespace {

constexpr uint32_t CB_WAVES = 4;       /* waves of a cipher workgroup */
constexpr uint32_t CB_RUN = 4;         /* consecutive tiles of a wave */
constexpr uint32_t CB_PASS = 64 * 64;  /* bytes of a tile: one pass */
constexpr uint32_t PB_WAVES = 4;       /* waves of a hash workgroup */
constexpr uint32_t DESC_WORDS = sizeof(otc_chacha_msg) / 8;
static_assert(sizeof(otc_chacha_msg) == 48, "six 64-bit columns: in, out, nbytes, aad, aad_bytes, key");

typedef const __attribute__((address_space(1))) uint8_t *gptr8;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v); }

/* the three little-endian words of nonce m: the array may sit at any byte address */
__device__ __forceinline__ void cb_nonce(const uint8_t *nonces, uint64_t m, uint32_t (&w)[3])
{
    auto p = (gptr8)(nonces + m * 12);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
}

/* the 16 bytes at p + off, those at or past `end` as zero; never reads them */
__device__ __forceinline__ uint4 pb_bytes(gptr8 p, uint64_t off, uint64_t end)
{
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t t = 0; t < 16; ++t) {
        const uint32_t v = off + t < end ? (uint32_t)p[off + t] : 0u;
        w[t >> 2] |= v << (8 * (t & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* ---- prep: the one-time keys ------------------------------------------------ */
__global__ __launch_bounds__(256) void k_chacha_batch_prep(const uint64_t *msgs, uint64_t nmsg, const uint32_t *keys,
                                                           const uint8_t *nonces, uint4 *otk)
{
    const uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= nmsg) return;
    const uint64_t ki = msgs[m * DESC_WORDS + 5]; /* an index the planner checked, not key material */
    uint32_t key[8], nonce[3], x[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = keys[ki * 8 + i];
    cb_nonce(nonces, m, nonce);
    cc_block(key, nonce, 0, x);
    /* r clamped (RFC 8439 section 2.5), then s */
    otk[2 * m] = make_uint4(x[0] & 0x0FFFFFFFu, x[1] & 0x0FFFFFFCu, x[2] & 0x0FFFFFFCu, x[3] & 0x0FFFFFFCu);
    otk[2 * m + 1] = make_uint4(x[4], x[5], x[6], x[7]);
}

/* ---- the cipher: one tile per wave step ------------------------------------- */
struct CbParams {
    const uint64_t *msgs;
    const uint32_t *keys;   /* nkeys x 8 words */
    const uint8_t *nonces;  /* nmsg x 12 */
    const uint32_t *tile_msg;
    const uint64_t *tile_first;
    uint64_t ntiles;
};

__global__ __launch_bounds__(64 * CB_WAVES) void k_chacha20_batch(CbParams P)
{
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * CB_WAVES + uni(threadIdx.x >> 6);
    for (uint32_t k = 0; k < CB_RUN; ++k) {
        const uint64_t t = wave * CB_RUN + k;
        if (t >= P.ntiles) break; /* wave-uniform */
        /* the record of the tile, its descriptor, key and nonce: the same for every lane */
        const uint32_t m = uni(P.tile_msg[t]);
        const uint64_t *D = P.msgs + (uint64_t)m * DESC_WORDS;
        const uint8_t *in = (const uint8_t *)uni64(D[0]);
        uint8_t *out = (uint8_t *)uni64(D[1]);
        const uint64_t nbytes = uni64(D[2]);
        const uint32_t ki = uni((uint32_t)D[5]);
        const uint32_t pass = (uint32_t)(t - uni64(P.tile_first[m])); /* < 256: a record has at most 1 MiB */
        uint32_t key[8], nonce[3];
#pragma unroll
        for (int i = 0; i < 8; ++i) key[i] = uni(P.keys[(uint64_t)ki * 8 + i]);
        cb_nonce(P.nonces, m, nonce);
#pragma unroll
        for (int i = 0; i < 3; ++i) nonce[i] = uni(nonce[i]);
        const uint64_t at = (uint64_t)pass * CB_PASS;
        /* lane 4g + q computes block 16q + g of the pass; its 16-byte piece j is at (64 j + lane) * 16 */
        const uint32_t lb = (lane & 3u) << 4 | lane >> 2;
        uint32_t x[16];
        if (at + CB_PASS <= nbytes) { /* a whole pass: on the length */
            const uint8_t *src = in + at + lane * 16;
            uint8_t *dst = out + at + lane * 16;
            uint4 d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = ld_u4<true, true>(src + j * 1024);
            /* counters 1 .. 16384: no wrap */
            cc_block(key, nonce, 1u + pass * 64u + lb, x);
            cc_xchg<1>(x, (lane & 1u) != 0);
            cc_xchg<2>(x, (lane & 2u) != 0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                st_u4<true, true>(dst + j * 1024, make_uint4(d[j].x ^ x[4 * j], d[j].y ^ x[4 * j + 1], d[j].z ^ x[4 * j + 2],
                                                             d[j].w ^ x[4 * j + 3]));
        } else {
            /* the record's last, partial pass, in the same layout (every lane computes: the exchange
             * needs all four of a quad).  A 16-byte piece that lies inside the record moves whole; the
             * one piece that holds the record's end moves byte by byte, every byte guarded by the
             * length; a piece past the end is not touched.  Only lengths decide. */
            const uint32_t rem = (uint32_t)(nbytes - at); /* 1 .. 4095 */
            /* the ragged piece, if the record does not end on a multiple of 16: piece jr of one lane */
            const uint32_t last = (rem - 1) >> 4, jr = last >> 6, roff = last * 16;
            const bool ragged = (rem & 15u) != 0 && (last & 63u) == lane;
            uint4 d[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t off = j * 1024 + lane * 16;
                d[j] = make_uint4(0, 0, 0, 0);
                if (off + 16 <= rem) d[j] = ld_u4<true, true>(in + at + off);
            }
            if (ragged) {
                const uint4 r = pb_bytes((gptr8)(in + at), roff, rem);
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (j == jr) d[j] = r;
            }
            cc_block(key, nonce, 1u + pass * 64u + lb, x);
            cc_xchg<1>(x, (lane & 1u) != 0);
            cc_xchg<2>(x, (lane & 2u) != 0);
            uint4 e[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t off = j * 1024 + lane * 16;
                e[j] = make_uint4(d[j].x ^ x[4 * j], d[j].y ^ x[4 * j + 1], d[j].z ^ x[4 * j + 2], d[j].w ^ x[4 * j + 3]);
                if (off + 16 <= rem) st_u4<true, true>(out + at + off, e[j]);
            }
            if (ragged) {
                uint4 r = e[0];
#pragma unroll
                for (uint32_t j = 1; j < 4; ++j)
                    if (j == jr) r = e[j];
                const uint32_t w[4] = {r.x, r.y, r.z, r.w};
                auto dst = (__attribute__((address_space(1))) uint8_t *)(out + at + roff);
#pragma unroll
                for (uint32_t t = 0; t < 15; ++t)
                    if (t < (rem & 15u)) dst[t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
            }
        }
    }
}

/* ---- the hash ---------------------------------------------------------------- */
struct PbParams {
    const uint64_t *msgs;
    uint64_t nmsg;
    const uint32_t *otk;   /* nmsg x 8 words: r (clamped here again: a no-op on prep's), s */
    uint4 *tags;           /* nmsg x 16 (zero where ok[m] becomes 0) */
    const uint8_t *expect; /* nmsg x 16 or null (with ok) */
    uint8_t *ok;           /* nmsg verdicts or null */
    uint32_t hash_out;     /* hash the record's `out` (an encryption's ciphertext), else its `in` */
};

/* one record as the hash sees it */
struct PbRec {
    gptr8 data, aad;
    uint64_t nbytes, aad_bytes;
    uint64_t na, nd; /* blocks of the AAD and of the data */
};

/* block i (< na + nd + 1) of the record's hashed string, with its 2^128 bit */
__device__ __forceinline__ Fe pb_block(const PbRec &R, uint64_t i)
{
    uint4 w;
    if (i < R.na) {
        w = pb_bytes(R.aad, i * 16, R.aad_bytes); /* any alignment: bytes */
    } else if (i < R.na + R.nd) {
        const uint64_t off = (i - R.na) * 16;
        if (off + 16 <= R.nbytes)
            w = ld_u4<false, true>((const uint8_t *)R.data + off);
        else
            w = pb_bytes(R.data, off, R.nbytes);
    } else { /* le64(aad_bytes) le64(nbytes) */
        w = make_uint4((uint32_t)R.aad_bytes, (uint32_t)(R.aad_bytes >> 32), (uint32_t)R.nbytes, (uint32_t)(R.nbytes >> 32));
    }
    return fe_of_words(w.x, w.y, w.z, w.w, 1);
}

/* the batch kb of a record: PL_BATCH passes of L blocks, one block per lane;
 * slots in front of the record (v < pad) and batches past its last are zero */
template <uint32_t L>
__device__ __forceinline__ void pb_load(Fe (&X)[PL_BATCH], const PbRec &R, uint32_t kb, uint32_t nbat, uint64_t pad, uint32_t j)
{
#pragma unroll
    for (uint32_t i = 0; i < PL_BATCH; ++i) {
        const uint64_t v = ((uint64_t)kb * PL_BATCH + i) * L + j;
        X[i] = (kb < nbat && v >= pad) ? pb_block(R, v - pad) : Fe{{0, 0, 0, 0, 0}};
    }
}

/* lane `src` of this lane's record (src < L) */
template <uint32_t L>
__device__ __forceinline__ Fe pb_from(const Fe &a, uint32_t lane, uint32_t src)
{
    Fe f;
#pragma unroll
    for (int k = 0; k < 5; ++k) f.l[k] = (uint32_t)__shfl((int)a.l[k], (int)((lane & ~(L - 1)) | src), 64);
    return f;
}

/* L lanes per record (16 or 64), 64 / L records per wave.  Every lane runs
 * every cross-lane step: a record past the batch's end has no blocks and
 * stores nothing. */
template <uint32_t L>
__global__ __launch_bounds__(64 * PB_WAVES) void k_poly1305_batch(PbParams P)
{
    const uint32_t lane = lane_id(), j = lane & (L - 1);
    const uint64_t m = ((uint64_t)blockIdx.x * (64 * PB_WAVES) + threadIdx.x) / L;
    const bool live = m < P.nmsg;
    PbRec R{};
    uint32_t rw[4] = {0, 0, 0, 0}, sw[4] = {0, 0, 0, 0};
    uint32_t nbat = 0;
    uint64_t pad = 0;
    if (live) { /* on the call's shape */
        const uint64_t *D = P.msgs + m * DESC_WORDS;
        R.data = (gptr8)D[P.hash_out ? 1 : 0];
        R.nbytes = D[2];
        R.aad = (gptr8)D[3];
        R.aad_bytes = D[4];
        R.na = (R.aad_bytes + 15) >> 4;
        R.nd = (R.nbytes + 15) >> 4;
        const uint64_t nb = R.na + R.nd + 1;
        nbat = (uint32_t)((nb + PL_BATCH * L - 1) / (PL_BATCH * L));
        pad = (uint64_t)nbat * (PL_BATCH * L) - nb; /* zero blocks in front, < PL_BATCH * L */
        const uint32_t *k = P.otk + m * 8;
        rw[0] = k[0] & 0x0FFFFFFFu, rw[1] = k[1] & 0x0FFFFFFCu, rw[2] = k[2] & 0x0FFFFFFCu, rw[3] = k[3] & 0x0FFFFFFCu;
#pragma unroll
        for (int i = 0; i < 4; ++i) sw[i] = k[4 + i];
    }
    Fe X[PL_BATCH], N[PL_BATCH];
    pb_load<L>(X, R, 0, nbat, pad, j); /* in flight during the powers */

    /* r^(j+1) by a parallel prefix: the multiplier is the neighbour's carried power */
    Fe pw = fe_of_words(rw[0], rw[1], rw[2], rw[3], 0);
#pragma unroll
    for (uint32_t d = 1; d < L; d <<= 1) {
        const Fe q = fe_mul(pw, mul_of(pb_from<L>(pw, lane, (j - d) & (L - 1))));
        const bool take = j >= d; /* on the lane's number */
#pragma unroll
        for (int k = 0; k < 5; ++k) pw.l[k] = take ? q.l[k] : pw.l[k];
    }
    const Fe fold = pb_from<L>(pw, lane, L - 1 - j); /* r^(L-j) */
    const Fe c1 = pb_from<L>(pw, lane, L - 1);       /* C = r^L */
    Mul M[PL_BATCH];                                 /* C, C^2, C^3, C^4 */
    M[0] = mul_of(c1);
    Fe c = c1;
#pragma unroll
    for (uint32_t i = 1; i < PL_BATCH; ++i) {
        c = fe_mul(c, M[0]);
        M[i] = mul_of(c);
    }

    Fe A = {{0, 0, 0, 0, 0}};
    for (uint32_t kb = 0; kb < nbat; ++kb) { /* on the length */
        /* the next batch's loads are in flight during this one's multiplications */
        pb_load<L>(N, R, kb + 1, nbat, pad, j);
        uint64_t d[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) d[k] = X[PL_BATCH - 1].l[k];
        fe_mac(d, A, M[PL_BATCH - 1]);
#pragma unroll
        for (uint32_t i = 0; i + 1 < PL_BATCH; ++i) fe_mac(d, X[i], M[PL_BATCH - 2 - i]);
        A = fe_carry(d);
#pragma unroll
        for (uint32_t i = 0; i < PL_BATCH; ++i) X[i] = N[i];
    }

    /* fold: lane j's last block is L - 1 - j short of the record's last, which is multiplied by r */
    A = fe_mul(A, mul_of(fold));
    uint64_t d[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint64_t v = A.l[k];
#pragma unroll
        for (uint32_t o = L / 2; o >= 1; o >>= 1) v += __shfl_xor(v, (int)o, 64);
        d[k] = v;
    }
    const Fe h = fe_carry(d);
    uint32_t t[4];
    fe_tag(h, sw, t);
    if (live && j == 0) {
        uint4 T = make_uint4(t[0], t[1], t[2], t[3]);
        if (P.ok) {
            /* the tag against the expected one: OR of the XORs, no early exit.  The verdict is
             * formed BEFORE anything is stored, so the expected bytes are never this kernel's own
             * output (the host also rejects expect overlapping the tags) */
            auto e = (gptr8)(P.expect + m * 16);
            uint32_t diff = 0;
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b) diff |= ((t[b >> 2] >> (8 * (b & 3))) & 0xFFu) ^ (uint32_t)e[b];
            P.ok[m] = diff == 0 ? 1 : 0;
            /* the computed tag of a forged record is the valid tag of the forgery: not handed out */
            if (diff) T = make_uint4(0, 0, 0, 0);
        }
        P.tags[m] = T;
    }
}

} // namespace

int chacha_batch_spans(uint64_t *spans, int max)
{
    const uint64_t all[] = {CB_LANES_SHORT,                       /* a pass of the 16-lane form */
                            CB_LANES_LONG,                        /* its batch of passes, and a pass of the 64-lane form */
                            (uint64_t)PL_BATCH * CB_LANES_LONG};  /* a batch of passes of the 64-lane form */
    static_assert(PL_BATCH * CB_LANES_SHORT == CB_LANES_LONG, "the middle span is both");
    const int n = (int)(sizeof all / sizeof all[0]);
    for (int i = 0; i < n && i < max; ++i) spans[i] = all[i];
    return n;
}

hipError_t chacha_batch_prep(const otc_chacha_msg *msgs, uint64_t nmsg, const uint8_t *keys, const uint8_t *nonces,
                             void *otk, hipStream_t st)
{
    hipLaunchKernelGGL(k_chacha_batch_prep, dim3((unsigned)((nmsg + 255) / 256)), dim3(256), 0, st,
                       (const uint64_t *)msgs, nmsg, (const uint32_t *)keys, nonces, (uint4 *)otk);
    return hipGetLastError();
}

hipError_t chacha20_batch_run(const otc_chacha_msg *msgs, const uint8_t *keys, const uint8_t *nonces,
                              const uint32_t *tile_msg, const uint64_t *tile_first, uint64_t ntiles, hipStream_t st)
{
    if (ntiles == 0) return hipSuccess;
    const uint64_t per = (uint64_t)CB_WAVES * CB_RUN, wgs = (ntiles + per - 1) / per;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const CbParams P{(const uint64_t *)msgs, (const uint32_t *)keys, nonces, tile_msg, tile_first, ntiles};
    hipLaunchKernelGGL(k_chacha20_batch, dim3((unsigned)wgs), dim3(64 * CB_WAVES), 0, st, P);
    return hipGetLastError();
}

hipError_t poly1305_batch_run(const otc_chacha_msg *msgs, uint64_t nmsg, const void *otk, void *tags,
                              const uint8_t *expect, uint8_t *ok, bool hash_out, int lanes, hipStream_t st)
{
    if (lanes != CB_LANES_SHORT && lanes != CB_LANES_LONG) return hipErrorInvalidValue;
    PbParams P{};
    P.msgs = (const uint64_t *)msgs;
    P.nmsg = nmsg;
    P.otk = (const uint32_t *)otk;
    P.tags = (uint4 *)tags;
    P.expect = ok ? expect : nullptr;
    P.ok = ok;
    P.hash_out = hash_out ? 1u : 0u;
    const uint64_t nrec = (uint64_t)PB_WAVES * (64 / (unsigned)lanes), wgs = (nmsg + nrec - 1) / nrec;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 g((unsigned)wgs), b(64 * PB_WAVES);
    if (lanes == CB_LANES_SHORT)
        hipLaunchKernelGGL(k_poly1305_batch<16>, g, b, 0, st, P);
    else
        hipLaunchKernelGGL(k_poly1305_batch<64>, g, b, 0, st, P);
    return hipGetLastError();
}

} // namespace otc_impl
