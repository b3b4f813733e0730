"""The bitsliced claim kernel with work to do, alone and inside a real split.

split.cpp split_run hands the first claim units out from the host: the last
``pb = min(nunits, 16 * CUs)`` units to the T-table waves, the first
``pf = min(nunits - pb, 4 * bs_wgs)`` to the bitsliced waves, and only the
units between them go through the claim word.  An ``impl="split"`` call of
fewer than 16 units per CU (128 MiB on 256 CUs) therefore has ``pf = 0``: the
bitsliced kernel is launched, takes nothing, and the T-table does the whole
buffer while ``last_impl()`` still says "split".  The split tests of the other
modules mostly sit below that line (the degenerate split); this module runs

1. every ``k_aes_bs_claim<NR, MODE>`` segment instantiation alone
   (``impl="bitslice"``), small, the whole output against the CPU oracle, at
   segment shifts 0, 1, 5, 6, 7, 8, 11 and 12 -- aes_bs.hip seg_prev behaves
   differently under 64 blocks per segment (every slot of every wave holds
   segment starts) and at one block per segment (every lane is a start, and
   IV_s = iv0 + i carries out of the low 64 bits per block);
2. ``impl="split"`` at the smallest shape with a pre-assigned front, a claimed
   middle and a pre-assigned back all non-empty, where the split's accounting
   (otc_split_stats) must report ``front >= pf > 0`` -- the assertion that
   keeps these cases from going hollow if the pre-assignment changes;
3. ``impl="bitslice"`` at a size where its waves claim through the word.

Every comparison is byte-exact: against the C oracle (cpu_ref, csrc/cpu) or
the T-table grid kernel (itself oracle-tested in test_gpu_kernels.py).  Sizes
derive from the device's CU count (otc_device_cus); the thresholds are the
shipped ones.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref

gpu_test = pytest.mark.gpu  # per test: test_shape_helpers_mirror_split_run needs no GPU

UNIT = 2048 * 16  # bytes of one claim unit (otc_device.h CLAIM_UNIT blocks)


# ---- 0. shapes ---------------------------------------------------------------

def split_shape(cus, middle):
    """(nunits, pf, pb) of an impl="split" call with 16 units per CU
    pre-assigned to the T-table waves (back), 4 per CU to the bitsliced waves
    (front: one workgroup of 4 waves per CU) and ``middle`` units claimed."""
    pf, pb = 4 * cus, 16 * cus
    return pf + middle + pb, pf, pb


def bs_alone_shape(cus, middle):
    """The same for impl="bitslice": no T-table units, three bitsliced
    workgroups per CU."""
    pf = 4 * 3 * cus
    return pf + middle, pf, 0


def claimed_middle(cus):
    return 2 * cus + 5


def test_shape_helpers_mirror_split_run():
    """The helpers against split_run's two min() expressions; front, claimed
    middle and back are all non-empty at every CU count."""
    for cus in range(1, 513):
        nunits, pf, pb = split_shape(cus, claimed_middle(cus))
        bs_wgs = cus
        want_pb = min(nunits, 16 * cus)  # preassigned_back
        want_pf = min(nunits - want_pb, 4 * bs_wgs)
        assert (pf, pb) == (want_pf, want_pb), cus
        assert pf > 0 and pb > 0 and nunits - pf - pb == claimed_middle(cus) > 0, cus
        assert nunits == 20 * cus + claimed_middle(cus)
        nunits, pf, pb = bs_alone_shape(cus, 7)
        bs_wgs = 3 * cus
        want_pb = 0  # bs_only
        want_pf = min(nunits - want_pb, 4 * bs_wgs)
        assert (pf, pb) == (want_pf, want_pb), cus
        assert pf == 12 * cus and nunits - pf == 7, cus


def _cus():
    return _native.require_gpu_lib().otc_device_cus(0)


# ---- helpers -----------------------------------------------------------------

def _host(t):
    return t.cpu().numpy().tobytes()


def _where(y, t):
    """first / last differing claim unit, for the assertion message"""
    d = (y != t).nonzero()
    return f"{d.numel()} bytes differ, units {int(d[0]) // UNIT}..{int(d[-1]) // UNIT} of {y.numel() // UNIT}"


class _Mode:
    """One claimed mode: call(x, impl, out) on the device and the CPU oracle
    of output bytes [a, b) (a, b multiples of 16).  Names: "ecb", "ecb-dec",
    "cbc-dec", "cfb-dec", and "cbc-dec-seg<bytes>" / "cfb-dec-seg<bytes>"."""

    def __init__(self, name, bits):
        self.name, self.bits, self.seg = name, bits, 0
        rng = np.random.default_rng([zlib.crc32(name.encode()), bits])  # seeded: a failure reproduces
        self.key = rng.integers(0, 256, bits // 8, dtype=np.uint8).tobytes()
        # IV_s = iv0 + s carries into the high half at segment 3
        self.iv = rng.integers(0, 256, 8, dtype=np.uint8).tobytes() + (2**64 - 3).to_bytes(8, "big")
        self.base, _, seg = name.partition("-seg")
        if seg:
            self.seg = int(seg)
        self.inplace = self.base in ("ecb", "ecb-dec")  # the chained decryptions read block i-1: never in == out

    def trim(self, n):
        return n - n % self.seg if self.seg else n

    def call(self, x, impl, out=None):
        k, iv = self.key, self.iv
        if self.base == "ecb":
            return ops.ecb_encrypt(x, k, out=out, impl=impl)
        if self.base == "ecb-dec":
            return ops.ecb_decrypt(x, k, out=out, impl=impl)
        if self.base == "cbc-dec":
            if self.seg:
                return ops.cbc_decrypt_segments(x, k, iv, self.seg, out=out, impl=impl)
            return ops.cbc_decrypt(x, k, iv, out=out, impl=impl)
        assert self.base == "cfb-dec", self.name
        if self.seg:
            return ops.cfb128_decrypt_segments(x, k, iv, self.seg, out=out, impl=impl)
        return ops.cfb128_decrypt(x, k, iv, out=out, impl=impl)

    def oracle(self, x, a, b):
        if self.base in ("ecb", "ecb-dec"):
            return cpu_ref.ecb(self.key, _host(x[a:b]), decrypt=self.base == "ecb-dec")
        chain = cpu_ref.cbc if self.base == "cbc-dec" else cpu_ref.cfb128
        if self.seg and a % self.seg == 0:  # from a segment start: the segment oracle itself
            segs = cpu_ref.cbc_segments if self.base == "cbc-dec" else cpu_ref.cfb128_segments
            return segs(self.key, cpu_ref.ctr128_add(self.iv, a // self.seg), _host(x[a:b]), self.seg, decrypt=True)
        seg = self.seg or x.numel()
        out = bytearray()
        while a < b:  # piecewise: each piece chains from the block before it, or from its segment's IV
            s, off = divmod(a, seg)
            e = min(b, (s + 1) * seg)
            if off:
                iv = _host(x[a - 16:a])
            else:
                iv = cpu_ref.ctr128_add(self.iv, s) if self.seg else self.iv
            out += chain(self.key, iv, _host(x[a:e]), decrypt=True)
            a = e
        return bytes(out)


def _random_input(n, seed, gpu):
    x = torch.empty(n, dtype=torch.uint8, device=gpu)
    ops.fill_random_(x, seed=seed)
    return x


def _with_stats(run):
    """run() under otc_split_stats(1) (the call then waits for its kernels and
    keeps its claim word).  Returns (run's result, last_impl, fallback reason,
    front, back, nunits)."""
    lib = _native.require_gpu_lib()
    fr, bk, nu = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.otc_split_stats(1)
    try:
        y = run()
        torch.cuda.synchronize()
        ran, why = ops.last_impl(), ops.split_fallback_reason()
        assert lib.otc_split_last_units(ctypes.byref(fr), ctypes.byref(bk), ctypes.byref(nu)) == 0
    finally:
        lib.otc_split_stats(0)
    return y, ran, why, fr.value, bk.value, nu.value


# ---- 1. the bitsliced claim kernel alone, every instantiation, small -----------

ALONE_BYTES = (5 * 2048 + 300) * 16  # 5 pre-assigned tasks + a remainder run by the T-table's workgroup 0
# shifts 0, 1, 5, 6 (64 blocks: the ballot in seg_prev stops being always true), 7, 8, 11 (one unit), 12
ALONE_SEGS = [16, 32, 512, 1024, 2048, 4096, 32768, 65536]


def _alone(gpu, m):
    n = m.trim(ALONE_BYTES)
    assert n >= 4 * UNIT
    x = _random_input(n, m.bits + m.seg + len(m.name), gpu)
    y = m.call(x, "bitslice")
    torch.cuda.synchronize()
    assert ops.last_impl() == "bitslice", ops.split_fallback_reason()
    t = m.call(x, "ttable")
    torch.cuda.synchronize()
    assert ops.last_impl() == "ttable"
    ref = m.oracle(x, 0, n)
    got = _host(y)
    if got != ref:
        bad = [i for i in range(0, n, 16) if got[i:i + 16] != ref[i:i + 16]]
        pytest.fail(f"{m.name}-{m.bits}: {len(bad)} of {n // 16} blocks differ from the oracle, "
                    f"blocks {bad[0]}..{bad[-1]}, first {bad[:8]}")
    assert torch.equal(y, t), _where(y, t)


@gpu_test
@pytest.mark.parametrize("seg", ALONE_SEGS)
@pytest.mark.parametrize("base", ["cbc-dec", "cfb-dec"])
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_bitslice_alone_segments_match_oracle(gpu, bits, base, seg):
    """k_aes_bs_claim<NR, BS_CBC_DEC_SEG | BS_CFB_DEC_SEG> alone over five
    units and a remainder: the whole output equals the CPU oracle and the
    T-table kernel, at every key size and every segment size at which
    seg_prev takes another path."""
    _alone(gpu, _Mode(f"{base}-seg{seg}", bits))


@gpu_test
@pytest.mark.parametrize("name", ["ecb", "ecb-dec", "cbc-dec", "cfb-dec"])
def test_bitslice_alone_aes192_matches_oracle(gpu, name):
    """The four whole-stream modes at AES-192, the key size with the least
    coverage elsewhere, in the same way."""
    _alone(gpu, _Mode(name, 192))


# ---- 2. a real split: front, claimed middle and back all non-empty ------------

BIG = "big"  # one segment longer than the pf pre-assigned front units: the next power of two above 4 units per CU

SPLIT_CASES = [(name, bits) for name in ("ecb", "ecb-dec", "cbc-dec", "cfb-dec") for bits in (128, 192, 256)] + [
    # every segment size in both modes; every (mode, key size) at two segment sizes
    ("cbc-dec-seg16", 128), ("cbc-dec-seg65536", 128),
    ("cbc-dec-seg512", 192), ("cbc-dec-seg" + BIG, 192),
    ("cbc-dec-seg4096", 256), ("cbc-dec-seg16", 256),
    ("cfb-dec-seg512", 128), ("cfb-dec-seg" + BIG, 128),
    ("cfb-dec-seg4096", 192), ("cfb-dec-seg65536", 192),
    ("cfb-dec-seg16", 256), ("cfb-dec-seg512", 256),
]


def _split_case(name, bits, cus):
    """(mode, bytes) of a claimed case: split_shape(cus, 2 * cus + 5) and 3
    blocks past the last unit, cut to whole segments -- rounded up for the big
    segment (cut down, its units would all be the T-table's)."""
    nunits, pf, _ = split_shape(cus, claimed_middle(cus))
    n = nunits * UNIT + 48
    if name.endswith(BIG):
        seg = (1 << (4 * cus).bit_length()) * UNIT
        assert seg > pf * UNIT
        m = _Mode(name[:-len(BIG)] + str(seg), bits)
        return m, -(-n // seg) * seg
    m = _Mode(name, bits)
    return m, m.trim(n)


def _regions(n, cus):
    """(nunits, pf, pb) of an impl="split" call of n bytes through split_shape;
    all three regions non-empty."""
    nunits = n // UNIT
    middle = nunits - 20 * cus
    assert middle > 0, (n, cus)
    shape = split_shape(cus, middle)
    assert shape[0] == nunits
    return shape


def _windows(n, pf, pb, front, nunits):
    """Byte ranges across every place a unit can be lost or done twice."""
    w = [(0, 65536)]
    for u in (pf, front, nunits - pb):
        w.append((max(0, u - 1) * UNIT, min(n, (u + 1) * UNIT)))
    w.append(((n - 65536) & ~15, n))
    return sorted(set(w))


@gpu_test
@pytest.mark.parametrize("name,bits", SPLIT_CASES, ids=[f"{m}-{b}" for m, b in SPLIT_CASES])
def test_split_front_middle_back(gpu, name, bits):
    """impl="split" with pf = 4 per CU units pre-assigned to the bitsliced
    waves, 2 per CU + 5 claimed through the word and 16 per CU pre-assigned to
    the T-table waves: it splits (2a), the bitsliced half took at least its
    pre-assigned units and the T-table its own, every unit once (2b), the
    output equals the T-table's everywhere (2c) and the CPU oracle around unit
    pf, the meeting point, unit nunits - pb, the head and the tail (2d); ECB
    in place gives the same bytes -- no unit enciphered twice (2e).  Who wins
    the claimed middle is timing and not asserted.  front >= pf fails whenever
    the bitsliced half did less than its 4 units per CU -- always in a shape
    whose units are all the T-table's (front 0).  It cannot tell pre-assigned
    front units from claimed ones: with pf forced to 0 in split_run the
    bitsliced waves usually win that many by claim."""
    cus = _cus()
    m, n = _split_case(name, bits, cus)
    nunits, pf, pb = _regions(n, cus)
    x = _random_input(n, nunits + bits, gpu)
    t = m.call(x, "ttable")
    torch.cuda.synchronize()
    assert ops.last_impl() == "ttable"
    y, ran, why, front, back, nu = _with_stats(lambda: m.call(x, "split"))
    print(f"{m.name}-{bits}: cus {cus} nunits {nu} pf {pf} pb {pb} front {front} back {back}")
    assert ran == "split" and why == "", (ran, why)  # 2a
    assert nu == nunits and front + back == nunits, (front, back, nu, nunits)  # 2b
    assert front >= pf > 0 and back >= pb > 0, (front, pf, back, pb)
    assert torch.equal(y, t), _where(y, t)  # 2c
    for a, b in _windows(n, pf, pb, front, nunits):  # 2d
        assert _host(y[a:b]) == m.oracle(x, a, b), (m.name, a, b, a // UNIT)
    if m.inplace:  # 2e
        w = x.clone()
        m.call(w, "split", out=w)
        torch.cuda.synchronize()
        assert ops.last_impl() == "split", ops.split_fallback_reason()
        assert torch.equal(w, y), _where(w, y)


# ---- 3. impl="bitslice" claiming through the word -------------------------------

@gpu_test
@pytest.mark.parametrize("name", ["ecb", "cbc-dec-seg512"])
def test_bitslice_alone_claims_through_the_word(gpu, name):
    """impl="bitslice" over 12 units per CU + 7 (and 3 blocks): every wave of
    its three workgroups per CU has a pre-assigned unit and the last 7 go
    through the claim word.  Whole buffer against the T-table; ECB in place."""
    cus = _cus()
    nunits, pf, pb = bs_alone_shape(cus, 7)
    m = _Mode(name, 256)
    n = m.trim(nunits * UNIT + 48)
    assert n // UNIT == nunits > pf and pb == 0
    x = _random_input(n, nunits, gpu)
    t = m.call(x, "ttable")
    if m.inplace:
        y = x.clone()
        m.call(y, "bitslice", out=y)
    else:
        y = m.call(x, "bitslice")
    torch.cuda.synchronize()
    assert ops.last_impl() == "bitslice", ops.split_fallback_reason()
    assert torch.equal(y, t), _where(y, t)
    for a, b in ((0, 65536), ((pf - 1) * UNIT, n)):  # the claimed units and the tail
        assert _host(y[a:b]) == m.oracle(x, a, b), (m.name, a, b)
