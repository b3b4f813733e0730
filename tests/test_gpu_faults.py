"""Allocation-failure injection on a healthy GPU ("Failure
detection / fault injection"): ``otc_fault_inject_alloc(n)`` makes the
(n+1)-th runtime allocation from now fail once -- device chunk buffers,
NUMA-pinned host windows, RCCL job buffers, the bitsliced kernel's per-call
tables.  Every entry point must then fail cleanly with an error (or, for the
bitsliced CTR tables, fall back to the uncached kernel, and for the claimed
kernels to the T-table, with identical output), release what it had built,
and work again on the next call."""
import os

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref
from our_tree_amd.parallel import stream as pstream

pytestmark = pytest.mark.gpu


@pytest.fixture
def inject(gpu):
    lib = _native.require_gpu_lib()
    yield lib.otc_fault_inject_alloc
    lib.otc_fault_inject_alloc(-1)


def _pending():
    """The hook's countdown (otc_fault_inject_pending): -1 once the injected
    failure has fired, >= 0 while it is still armed -- a fault that never
    landed would leave the test checking the ordinary path."""
    return _native.require_gpu_lib().otc_fault_inject_pending()


def _rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def test_engine_create_and_run_under_alloc_faults(inject):
    key, ctr = os.urandom(16), os.urandom(16)
    x = _rnd((3 << 20) + 5, 1)
    ref = cpu_ref.ctr(key, ctr, x.tobytes())
    failed = 0
    for k in range(12):
        inject(k)
        try:
            with pstream.StreamEngine(0, chunk_bytes=1 << 20, depth=3) as eng:
                y = np.zeros_like(x)
                eng.run("ctr", x, y, key, ctr)
                assert y.tobytes() == ref  # the fault landed after this call's allocations
        except RuntimeError as e:
            failed += 1
            assert "otc_engine" in str(e)
        finally:
            inject(-1)
    assert failed >= 6  # 3 x (d_in, d_out) device buffers at least
    with pstream.StreamEngine(0, chunk_bytes=1 << 20, depth=3) as eng:
        y = np.zeros_like(x)
        eng.run("ctr", x, y, key, ctr)
    assert y.tobytes() == ref


def test_multi_rccl_job_under_alloc_faults(inject):
    key, iv = os.urandom(32), os.urandom(16)
    x = pstream.pinned_empty((2 << 20) + 48)
    x[:] = _rnd(x.nbytes, 2)
    ref = cpu_ref.cbc(key, iv, x.tobytes(), decrypt=True)
    failed = 0
    y = pstream.pinned_empty(x.nbytes)  # before arming: the injected faults are the job's own
    for k in range(8):
        y[:] = 0
        inject(k)
        try:
            pstream.multi_gpu_run("cbc-dec", x, y, key, iv, ngpus=1, strategy="rccl", chunk_bytes=256 << 10)
            assert y.tobytes() == ref
        except RuntimeError as e:
            failed += 1
            assert "otc_multi_run" in str(e)
        finally:
            inject(-1)
        _native.require_gpu_lib().otc_release_resources()  # next attempt builds the job afresh
    assert failed >= 4  # 2 x (pin, pout) + 2 x (root_in, root_out)
    y = pstream.pinned_empty(x.nbytes)
    pstream.multi_gpu_run("cbc-dec", x, y, key, iv, ngpus=1, strategy="rccl", chunk_bytes=256 << 10)
    assert y.tobytes() == ref


@pytest.mark.parametrize("bits", [128, 256])
def test_bitslice_ctr_falls_back_without_group_table(inject, gpu, bits):
    """No room for the counter-caching tables: the uncached kernel runs."""
    key, ctr = os.urandom(bits // 8), os.urandom(8) + (2**64 - 50000).to_bytes(8, "big")
    x = torch.from_numpy(_rnd(16 * 100000 + 3, 3)).to(gpu)
    inject(0)
    y = ops.ctr(x, key, ctr, impl="bitslice")
    torch.cuda.synchronize()
    assert _pending() == -1  # the table allocation did fail: the uncached kernel ran
    assert y.cpu().numpy().tobytes() == cpu_ref.ctr(key, ctr, x.cpu().numpy().tobytes())


@pytest.mark.parametrize("k", [0, 1])
def test_bitslice_ecb_alloc_failure_falls_back(inject, gpu, k):
    """impl="bitslice" ECB is the bitsliced claim kernel alone (split_run,
    bs_only).  If its work counter (allocation 0) or key table (allocation 1)
    cannot be allocated, the T-table runs the call instead -- complete output,
    and last_impl() says so -- and the next call runs bitsliced again."""
    key = os.urandom(16)
    x = torch.from_numpy(_rnd(16 * 4096 * 3 + 32, 4)).to(gpu)
    ref = cpu_ref.ecb(key, x.cpu().numpy().tobytes())
    inject(k)
    y = ops.ecb_encrypt(x, key, impl="bitslice")
    torch.cuda.synchronize()
    assert _pending() == -1
    assert ops.last_impl() == "ttable"
    assert y.cpu().numpy().tobytes() == ref
    inject(-1)
    y = ops.ecb_encrypt(x, key, impl="bitslice")
    torch.cuda.synchronize()
    assert ops.last_impl() == "bitslice"
    assert y.cpu().numpy().tobytes() == ref


@pytest.mark.parametrize("k,want", [(0, "ttable"), (1, "ttable")])
def test_split_under_alloc_faults(inject, gpu, k, want):
    """The claimed split's work counter (allocation 0) or the bitsliced half's
    key table (allocation 1) cannot be allocated: the T-table runs every unit
    (plain, or as the split's only claimant) and the output is complete."""
    key, iv = os.urandom(32), os.urandom(16)
    x = torch.from_numpy(_rnd(16 * 2048 * 40 + 48, 5)).to(gpu)
    ref_ecb = cpu_ref.ecb(key, x.cpu().numpy().tobytes())
    inject(k)
    y = ops.ecb_encrypt(x, key, impl="split")
    torch.cuda.synchronize()
    assert _pending() == -1
    assert ops.last_impl() == want
    assert y.cpu().numpy().tobytes() == ref_ecb
    inject(-1)
    inject(k)
    z = ops.cbc_decrypt(x, key, iv, impl="split")
    torch.cuda.synchronize()
    assert _pending() == -1
    assert z.cpu().numpy().tobytes() == cpu_ref.cbc(key, iv, x.cpu().numpy().tobytes(), decrypt=True)
    inject(-1)
    y = ops.ecb_encrypt(x, key, impl="split")
    torch.cuda.synchronize()
    assert ops.last_impl() == "split" and y.cpu().numpy().tobytes() == ref_ecb


# ---- every claimed mode with its bitsliced half not launched ----------------
# split.cpp split_run queues the T-table claim kernel first, told that
# units [0, pf) are the bitsliced waves' (impl "bitslice": every unit).  When
# the bitsliced half's key table (allocation 1; allocation 0 is the claim
# counter) cannot be allocated those units are still owed, and the host reruns
# exactly them.  pf > 0 needs more than 16 units per CU.

UNIT = 2048 * 16  # bytes of one claim unit (otc_device.h CLAIM_UNIT blocks)
HALF_FAILED = "the bitsliced half failed to launch"


def _host(t):
    return t.cpu().numpy().tobytes()


class _Mode:
    """One claimed mode: call(x, impl, out) on the device and the CPU oracle
    of output bytes [a, b) (a, b multiples of 16)."""

    def __init__(self, name, bits=256):
        self.name, self.seg = name, 0
        rng = np.random.default_rng(bits + len(name))
        self.key = rng.integers(0, 256, bits // 8, dtype=np.uint8).tobytes()
        # segment IVs carry out of the low 64 bits inside every shape used here
        self.iv = rng.integers(0, 256, 8, dtype=np.uint8).tobytes() + (2**64 - 3).to_bytes(8, "big")
        base, _, seg = name.partition("-seg")
        if seg:
            self.seg = int(seg)
        self.base = base
        self.inplace = base in ("ecb", "ecb-dec")  # the native API refuses in == out for the chained decryptions

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


CLAIMED_MODES = ["ecb", "ecb-dec", "cbc-dec", "cfb-dec", "cbc-dec-seg4096", "cfb-dec-seg4096", "cbc-dec-seg65536",
                 "cfb-dec-seg65536"]
CLAIMED_CASES = [(m, 256) for m in CLAIMED_MODES] + [("ecb", 128)]


def _where(y, t):
    """first / last differing claim unit, for the assertion message"""
    d = (y != t).nonzero()
    return f"{d.numel()} bytes differ, units {int(d[0]) // UNIT}..{int(d[-1]) // UNIT} of {y.numel() // UNIT}"


def _split_front(n, cus):
    """split_run's pre-assignment for an impl="split" call of n bytes"""
    nunits = n // UNIT
    pb = min(nunits, 16 * cus)
    return nunits, min(nunits - pb, 4 * cus)


def _faulted_split(m, x, n, pf, inject):
    """impl="split" over x with the bitsliced half's key table failing: the
    asserts of every such case.  Returns (faulted output, T-table output)."""
    t = m.call(x, "ttable")
    y = x.clone()  # a prefix left unwritten is plaintext, not whatever the allocator held
    inject(1)
    m.call(x, "split", out=y)
    torch.cuda.synchronize()
    assert _pending() == -1
    assert ops.last_impl() == "ttable"
    assert ops.split_fallback_reason() == HALF_FAILED
    inject(-1)
    assert torch.equal(y, t), _where(y, t)
    for a, b in ((0, (pf + 1) * UNIT), (n - 65536, n)):
        assert _host(y[a:b]) == m.oracle(x, a, b), (m.name, a, b)
    z = x.clone()
    m.call(x, "split", out=z)
    torch.cuda.synchronize()
    assert ops.last_impl() == "split", ops.split_fallback_reason()
    assert torch.equal(z, t), _where(z, t)
    return y, t


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("name,bits", CLAIMED_CASES, ids=[f"{m}-{b}" for m, b in CLAIMED_CASES])
def test_split_bitsliced_half_fails(inject, gpu, name, bits, shape):
    """impl="split" with pf > 0 units pre-assigned to bitsliced waves that never
    launch.  A: 16 CUs' worth of units + 8, and 3 blocks past the last unit
    (pf = 8); B: 20 per CU + 5 (pf at its cap of 4 per CU).  The call reports
    the T-table and why, equals the T-table run everywhere and the CPU oracle
    over units [0, pf] and the last 64 KiB, and the same call without the
    fault splits and gives the same bytes.  ECB also in place: nothing is
    enciphered twice."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = _Mode(name, bits)
    n = m.trim((16 * cus + 8) * UNIT + 48 if shape == "A" else (20 * cus + 5) * UNIT)
    nunits, pf = _split_front(n, cus)
    assert nunits > 16 * cus and pf == (8 if shape == "A" else 4 * cus)
    x = torch.empty(n, dtype=torch.uint8, device=gpu)
    ops.fill_random_(x, seed=nunits + bits)
    y, _ = _faulted_split(m, x, n, pf, inject)
    if m.inplace:
        w = x.clone()
        inject(1)
        m.call(w, "split", out=w)
        torch.cuda.synchronize()
        assert _pending() == -1
        assert ops.last_impl() == "ttable" and ops.split_fallback_reason() == HALF_FAILED
        inject(-1)
        assert torch.equal(w, y), _where(w, y)


@pytest.mark.parametrize("base", ["cbc-dec", "cfb-dec"])
def test_split_bitsliced_half_fails_inside_a_segment(inject, gpu, base):
    """The owed prefix ends inside a segment: three segments of at least 8
    units per CU each, so pf = 4 per CU lies within segment 0 (segments of two
    units cannot show this: pf and the T-table's 16 per CU are both even)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    seg_units = 1 << (8 * cus - 1).bit_length()
    m = _Mode(f"{base}-seg{seg_units * UNIT}")
    n = 3 * seg_units * UNIT
    nunits, pf = _split_front(n, cus)
    assert 0 < pf < seg_units
    x = torch.empty(n, dtype=torch.uint8, device=gpu)
    ops.fill_random_(x, seed=seg_units)
    y, _ = _faulted_split(m, x, n, pf, inject)
    a = m.seg - UNIT  # across the first segment boundary
    assert _host(y[a:a + 2 * UNIT]) == m.oracle(x, a, a + 2 * UNIT)


@pytest.mark.parametrize("name,bits", CLAIMED_CASES, ids=[f"{m}-{b}" for m, b in CLAIMED_CASES])
def test_bitslice_alone_key_table_fails(inject, gpu, name, bits):
    """impl="bitslice" (bs_only) with the key table failing: the T-table claim
    kernel has run only the blocks past the last unit, the host owes every
    unit.  Whole output against the CPU oracle; ECB also in place, where a
    rerun of the whole call would encipher those last blocks twice."""
    m = _Mode(name, bits)
    n = m.trim((5 * 2048 + 300) * 16)
    x = torch.empty(n, dtype=torch.uint8, device=gpu)
    ops.fill_random_(x, seed=bits + len(name))
    ref = m.oracle(x, 0, n)
    y = x.clone()
    inject(1)
    m.call(x, "bitslice", out=y)
    torch.cuda.synchronize()
    assert _pending() == -1
    assert ops.last_impl() == "ttable"
    assert ops.split_fallback_reason() == HALF_FAILED
    inject(-1)
    assert _host(y) == ref
    z = m.call(x, "bitslice")
    torch.cuda.synchronize()
    assert ops.last_impl() == "bitslice", ops.split_fallback_reason()
    assert torch.equal(z, y), _where(z, y)
    if m.inplace:
        w = x.clone()
        inject(1)
        m.call(w, "bitslice", out=w)
        torch.cuda.synchronize()
        assert _pending() == -1
        assert ops.last_impl() == "ttable" and ops.split_fallback_reason() == HALF_FAILED
        inject(-1)
        assert torch.equal(w, y), _where(w, y)


# ---- the persistent T-table forms without their claim counter ---------------
# ECB and the decryptions from 512 MiB, CTR from 512 MiB, segment encryption
# from 1 GiB and batches from 65536 tiles run the T-table as a claim kernel by
# itself (split.cpp claim_alone); allocation 0, the counter, failing sends them
# to the grid kernel.

def _windows(n, size=16384):
    return [(a, min(n, a + size)) for a in (0, (n // 2) & ~(size - 1), (n - size + 15) & ~15)]


def test_persistent_ecb_without_claim_counter(inject, gpu):
    key = _rnd(32, 11).tobytes()
    n = (512 << 20) + 3 * UNIT + 5 * 16
    x = torch.empty(n, dtype=torch.uint8, device=gpu)
    ops.fill_random_(x, seed=11)
    inject(0)
    y = ops.ecb_encrypt(x, key, impl="auto")
    torch.cuda.synchronize()
    assert _pending() == -1
    assert ops.last_impl() == "ttable"
    inject(-1)
    z = ops.ecb_encrypt(x, key, impl="auto")
    assert torch.equal(y, z), _where(y, z)
    for a, b in _windows(n):
        assert _host(y[a:b]) == cpu_ref.ecb(key, _host(x[a:b])), (a, b)


def test_persistent_ctr_without_claim_counter(inject, gpu):
    key = _rnd(32, 12).tobytes()
    ctr = _rnd(8, 13).tobytes() + (2**64 - 4096 * 40 - 77).to_bytes(8, "big")
    off = 1234567
    n = (512 << 20) + 16 * 9 + 11
    x = torch.empty(n, dtype=torch.uint8, device=gpu)
    ops.fill_random_(x, seed=12)
    inject(0)
    y = ops.ctr(x, key, ctr, block_offset=off, impl="ttable")
    torch.cuda.synchronize()
    assert _pending() == -1
    inject(-1)
    z = ops.ctr(x, key, ctr, block_offset=off, impl="ttable")
    assert torch.equal(y, z), _where(y, z)
    for a, b in _windows(n):
        assert _host(y[a:b]) == cpu_ref.ctr(key, ctr, _host(x[a:b]), block_offset=off + a // 16), (a, b)


@pytest.mark.parametrize("mode", ["cbc", "cfb"])
def test_persistent_segment_encrypt_without_claim_counter(inject, gpu, mode):
    key = _rnd(32, 14).tobytes()
    iv0 = _rnd(8, 15).tobytes() + (2**64 - 1000).to_bytes(8, "big")
    seg = 512
    n = ((1 << 30) // seg + 64 * 7 + 5) * seg
    run = ops.cbc_encrypt_segments if mode == "cbc" else ops.cfb128_encrypt_segments
    oracle = cpu_ref.cbc_segments if mode == "cbc" else cpu_ref.cfb128_segments
    x = torch.empty(n, dtype=torch.uint8, device=gpu)
    ops.fill_random_(x, seed=14)
    inject(0)
    y = run(x, key, iv0, seg)
    torch.cuda.synchronize()
    assert _pending() == -1
    inject(-1)
    z = run(x, key, iv0, seg)
    assert torch.equal(y, z), _where(y, z)
    for a, b in _windows(n):  # 16 KiB windows on segment boundaries: n and the window are multiples of 512
        assert a % seg == 0
        assert _host(y[a:b]) == oracle(key, cpu_ref.ctr128_add(iv0, a // seg), _host(x[a:b]), seg), (a, b)


def test_claimed_batch_without_claim_counter(inject, gpu):
    """The batch of test_gpu_batch.py::test_claimed_batch_matches_oracle (its
    AES-256 launch has >= 65536 tiles and runs claimed tile runs; the small
    AES-128 launch before it consults no allocation): without the counter the
    static kernel runs, with the same output."""
    rng = np.random.default_rng(21)
    big = [int(v) | 1 for v in rng.integers(3 << 19, (3 << 19) + (1 << 16), 43)]
    lens = big + [0, 1, 15, 16, 17, 1023, 1025, 0, 4097, 100001]
    buf = torch.empty(sum((n + 15) // 16 * 16 for n in lens), dtype=torch.uint8, device=gpu)
    ops.fill_random_(buf, seed=22)
    keys = [_rnd(32, 23).tobytes(), _rnd(16, 24).tobytes()]
    kidx = [0] * len(big) + [1, 0, 1, 1, 0, 1, 1, 1, 0, 1]
    ctrs = rng.integers(0, 256, (len(lens), 16), dtype=np.uint8)
    ctrs[2, 8:] = np.frombuffer((2**64 - 1000).to_bytes(8, "big"), dtype=np.uint8)
    b = ops.CtrBatch.packed(buf, lens, keys, ctrs, key_index=kidx, tile_blocks=64)
    tiles = {nr: t for *_, t, nr in b._launches}
    assert tiles[14] >= 65536 > tiles[10] > 0, tiles
    b.out.zero_()  # the slots' padding is not written
    inject(0)
    b.run()
    torch.cuda.synchronize()
    assert _pending() == -1
    y = b.out.clone()
    inject(-1)
    b.out.zero_()
    b.run()
    torch.cuda.synchronize()
    assert torch.equal(y, b.out), _where(y, b.out)
