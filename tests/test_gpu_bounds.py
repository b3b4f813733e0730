"""Guard bands around every device op's buffers: no kernel of ``aes_tt.hip``,
``aes_bs.hip`` or ``stream_ops.hip`` writes outside its output, changes its
input, or lets bytes outside its input reach the result.

Every case runs inside arenas::

    [ GUARD bytes 0xA5 | shift | n bytes of output | GUARD bytes 0xA5 ]
    [ GUARD bytes fill | shift | n bytes of input  | GUARD bytes fill ]   fill = 0x00, then 0xFF

and ``run_guarded`` asserts that (1) the output equals a reference that does
not run the kernel under test, (2) the output's guards still hold 0xA5, (3) the
whole input arena is what it was before the call, (4) the outputs under the two
fills are equal, and (5) in place, where the mode allows it, the one arena's
guards hold.  The guards are wider than one store step of any kernel, so a
wrong range check shows as a changed guard byte and never as a fault.

The helper takes the device as an argument; its own tests at the top of the
file run it on the CPU against fake ops in plain torch and carry no ``gpu``
mark."""
import ctypes

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref

# The widest store step of any kernel: a 1024-thread T-table workgroup moving
# 4 blocks per lane (aes_tt.hip OTC_TT_CTR_B / OTC_TT_ENC_B / OTC_TT_DEC_B = 4)
# covers 4096 blocks = 64 KiB per step.  A bitsliced task and a claim unit
# (otc_device.h CLAIM_UNIT) are 2048 blocks, a claimed batch unit 8 tiles of at
# most 4 KiB, an RC4 store 16 bytes.  64 more bytes for the edge stores of a
# step that starts one block off.
GUARD = 1024 * 4 * 16 + 64
A5 = 0xA5
CHUNK = 64 << 20  # inputs are generated, and compared again, this many bytes at a time
UNIT = 2048 * 16  # bytes of one claim unit (otc_device.h CLAIM_UNIT blocks)


def host(t):
    return t.cpu().numpy().tobytes()


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _as_tensor(v, device):
    if isinstance(v, torch.Tensor):
        return v.reshape(-1).view(torch.uint8)
    v = bytes(v)
    if not v:
        return torch.empty(0, dtype=torch.uint8, device=device)
    return torch.frombuffer(bytearray(v), dtype=torch.uint8).to(device)


def _assert_same(got, exp, what):
    """Byte equality on the device; the first and last differing offsets on failure."""
    assert got.numel() == exp.numel(), f"{what}: {got.numel()} bytes, expected {exp.numel()}"
    if torch.equal(got, exp):
        return
    idx = (got != exp).nonzero()
    raise AssertionError(f"{what}: {idx.numel()} of {got.numel()} bytes differ, from +{int(idx[0])} to +{int(idx[-1])}")


class Arena:
    """One uint8 buffer ``[GUARD | shift | region 0 | gap | region 1 | ... | GUARD]``
    filled with ``fill``.  Every region starts ``shift`` bytes past a multiple
    of 16 (torch aligns the buffer itself far beyond that; GUARD and the gaps
    are multiples of 16)."""

    def __init__(self, lengths, device, fill=A5, shift=0, gap=0):
        lengths = [lengths] if isinstance(lengths, int) else list(lengths)
        assert GUARD % 16 == 0 and gap % 16 == 0 and 0 <= shift < 16
        self.fill, self.device, self.spans = fill, torch.device(device), []
        at = GUARD
        for n in lengths:
            self.spans.append((at + shift, at + shift + n))
            at += (shift + n + 15) // 16 * 16 + gap
        self.buf = torch.full((self.spans[-1][1] + GUARD,), fill, dtype=torch.uint8, device=device)

    def region(self, r=0):
        a, b = self.spans[r]
        return self.buf[a:b]

    def packed(self):
        """(view, offsets): the regions as messages packed in one 16-byte aligned buffer."""
        end = (self.spans[-1][1] + 15) // 16 * 16
        return self.buf[GUARD:end], [a - GUARD for a, _ in self.spans]

    def where(self, i):
        """Offset ``i`` of the buffer relative to the nearest region edge: ``start-1``, ``end+0``."""
        best = None
        for r, (a, b) in enumerate(self.spans):
            for name, d in (("start", i - a), ("end", i - b)):
                if (d < 0) == (name == "start") and (best is None or abs(d) < abs(best[2])):
                    best = (r, name, d)
        r, name, d = best
        return (f"region {r} " if len(self.spans) > 1 else "") + f"{name}{d:+d}"

    def assert_guards(self, what):
        """Every byte outside the regions still holds the fill (compared on the device)."""
        count, first, last = 0, None, None
        edges = [0] + [e for span in self.spans for e in span] + [self.buf.numel()]
        for a, b in zip(edges[0::2], edges[1::2]):
            idx = (self.buf[a:b] != self.fill).nonzero()
            if idx.numel():
                count += idx.numel()
                first = a + int(idx[0]) if first is None else first
                last = a + int(idx[-1])
        assert count == 0, (f"{what}: {count} guard bytes changed, from {self.where(first)} to {self.where(last)} "
                            f"(fill 0x{self.fill:02X})")

    def _chunks(self, seed):
        for r in range(len(self.spans)):
            for k, c in enumerate(self.region(r).split(CHUNK)):
                g = torch.Generator(device=self.device).manual_seed(seed * 1_000_003 + r * 4099 + k)
                yield r, k, c, g

    def fill_random(self, seed):
        """Seeded random bytes in every region, generated on the device."""
        for _, _, c, g in self._chunks(seed):
            c.random_(0, 256, generator=g)

    def assert_input_intact(self, seed, what):
        """The arena is bit-identical to what it held after ``fill_random(seed)``:
        the guards by their fill, the regions by generating them again chunk by
        chunk -- what a clone taken before the call would show, without holding
        a second copy of a 1 GiB input."""
        self.assert_guards(f"{what}: input arena")
        for r, k, c, g in self._chunks(seed):
            again = torch.empty_like(c).random_(0, 256, generator=g)
            if not torch.equal(again, c):
                idx = (again != c).nonzero()
                raise AssertionError(f"{what}: input changed, {idx.numel()} bytes of region {r} from "
                                     f"+{k * CHUNK + int(idx[0])} to +{k * CHUNK + int(idx[-1])}")


def run_guarded(op, device, n, *, n_in=None, ref=None, check=None, seed=1, shift=0, also_inplace=False,
                compare_fills=True, what="op"):
    """Run ``op(*xs, out)`` inside arenas and assert the five properties of the
    module docstring.  ``xs`` are uint8 views of ``n_in`` bytes each (default:
    one input of ``n`` bytes; ``()`` for an op that only writes) with seeded
    random contents, ``out`` a view of ``n`` bytes; in place ``out`` is
    ``xs[0]``.  ``ref(*xs)`` gives the expected output as bytes or a tensor; it
    is evaluated once, before the first call (the inputs are the same in
    every run).  ``check(*xs, out)`` runs after each call for what a reference
    cannot express (in place ``xs[0]`` is the output by then).
    ``compare_fills=False`` leaves property 4 to the reference (two outputs
    that both equal it are equal) where a second copy of the output is too
    large to keep."""
    n_in = (n,) if n_in is None else tuple(n_in)
    expect = first = None
    for inplace in ((False, True) if also_inplace else (False,)):
        for fill in ((A5,) if inplace else (0x00, 0xFF) if n_in else (0x00,)):
            tag = f"{what} [{'in place' if inplace else f'input fill 0x{fill:02X}'}, shift {shift}]"
            ins = [Arena(m, device, fill, shift) for m in n_in]
            for i, a in enumerate(ins):
                a.fill_random(seed + i)
            xs = [a.region() for a in ins]
            if expect is None and ref is not None:
                expect = _as_tensor(ref(*xs), device)
            outa = ins[0] if inplace else Arena(n, device, A5, shift)
            out = xs[0] if inplace else outa.region()
            op(*xs, out)
            _sync(device)
            if expect is not None:
                _assert_same(out, expect, f"{tag}: output against the reference")
            outa.assert_guards(f"{tag}: output arena")
            for i, a in enumerate(ins[1 if inplace else 0:], 1 if inplace else 0):
                a.assert_input_intact(seed + i, tag)
            if check is not None:
                check(*xs, out)
            if not inplace:
                if compare_fills and first is None:
                    first = out.clone()
                elif compare_fills:
                    _assert_same(out, first, f"{tag}: output depends on bytes outside the input: against fill 0x00")
            del ins, xs, outa, out


# ---- the helper's own tests: fake ops in plain torch, on the CPU ---------------

CPU = torch.device("cpu")


def _past(t, lo, hi):
    """View of ``t``'s storage from ``lo`` bytes before its start to ``hi`` bytes past its end."""
    return torch.as_strided(t, (t.numel() + lo + hi,), (1,), t.storage_offset() - lo)


def _fake_good(x, out):
    out.copy_(x ^ 0x5C)


def _fake_ref(x):
    return x ^ 0x5C


@pytest.mark.parametrize("n", [0, 1, 17, 4099])
@pytest.mark.parametrize("shift", [0, 3])
def test_helper_accepts_a_correct_op(n, shift, device=CPU):
    run_guarded(_fake_good, device, n, ref=_fake_ref, shift=shift, also_inplace=True)
    run_guarded(lambda out: out.fill_(7), device, n, n_in=(), ref=lambda: bytes([7]) * n, shift=shift)
    run_guarded(lambda a, b, out: out.copy_(a ^ b), device, n, n_in=(n, n), ref=lambda a, b: a ^ b, shift=shift)


@pytest.mark.parametrize("shift", [0, 3])
def test_helper_rejects_a_write_after_the_region(shift, device=CPU):
    def op(x, out):
        _fake_good(x, out)
        _past(out, 0, 1)[-1] = 0

    with pytest.raises(AssertionError, match=r"output arena: 1 guard bytes changed, from end\+0 to end\+0"):
        run_guarded(op, device, 100, ref=_fake_ref, shift=shift)
    with pytest.raises(AssertionError, match=r"in place.*output arena: 1 guard bytes changed, from end\+0 to end\+0"):
        run_guarded(lambda x, out: op(x, out) if out is x else _fake_good(x, out), device, 100, ref=_fake_ref,
                    shift=shift, also_inplace=True)


def test_helper_rejects_a_write_before_the_region(device=CPU):
    def op(x, out):
        _fake_good(x, out)
        _past(out, 1, 0)[0] = 0

    with pytest.raises(AssertionError, match=r"1 guard bytes changed, from start-1 to start-1"):
        run_guarded(op, device, 100, ref=_fake_ref)

    def wide(x, out):  # a 16-byte store one block early and one 15 bytes late
        _fake_good(x, out)
        _past(out, 16, 15)[:16] = 0
        _past(out, 16, 15)[-15:] = 0

    with pytest.raises(AssertionError, match=r"31 guard bytes changed, from start-16 to end\+14"):
        run_guarded(wide, device, 64, ref=_fake_ref, shift=3)


def test_helper_rejects_an_altered_input(device=CPU):
    def op(x, out):
        _fake_good(x, out)
        x[5] ^= 1

    with pytest.raises(AssertionError, match=r"input changed, 1 bytes of region 0 from \+5 to \+5"):
        run_guarded(op, device, 100, ref=_fake_ref)

    def beside(x, out):  # not the input itself but the byte in front of it
        _fake_good(x, out)
        _past(x, 1, 0)[0] ^= 1

    with pytest.raises(AssertionError, match=r"input arena: 1 guard bytes changed, from start-1 to start-1"):
        run_guarded(beside, device, 100, ref=_fake_ref)


def test_helper_rejects_a_read_past_the_input(device=CPU):
    def op(x, out):
        _fake_good(x, out)
        out[-1] ^= _past(x, 0, 1)[-1]

    with pytest.raises(AssertionError, match=r"depends on bytes outside the input.*1 of 100 bytes differ, from \+99"):
        run_guarded(op, device, 100)
    with pytest.raises(AssertionError, match=r"fill 0xFF.*against the reference: 1 of 100 bytes differ, from \+99"):
        run_guarded(op, device, 100, ref=_fake_ref)


def test_helper_rejects_a_wrong_output_and_names_regions(device=CPU):
    with pytest.raises(AssertionError, match=r"against the reference: 100 of 100 bytes differ"):
        run_guarded(lambda x, out: out.copy_(x), device, 100, ref=_fake_ref)
    a = Arena([5, 0, 40], device, gap=64)
    buf, offs = a.packed()
    assert offs == [0, 16 + 64, 16 + 64 + 64] and buf.numel() == 16 + 64 + 64 + 48
    a.assert_guards("untouched")
    buf[5] = 0  # the slot padding right behind message 0
    buf[offs[2] - 2] = 0
    with pytest.raises(AssertionError, match=r"2 guard bytes changed, from region 0 end\+0 to region 2 start-2"):
        a.assert_guards("packed")


@pytest.mark.gpu
def test_helper_rejects_the_same_on_the_device(gpu):
    """The same fake torch ops (no kernel of the project's) with the arenas in
    device memory: the guard comparison and the regenerated input behave
    there as on the CPU."""
    test_helper_accepts_a_correct_op(4099, 3, device=gpu)
    test_helper_rejects_a_write_after_the_region(3, device=gpu)
    test_helper_rejects_a_write_before_the_region(device=gpu)
    test_helper_rejects_an_altered_input(device=gpu)
    test_helper_rejects_a_read_past_the_input(device=gpu)
    test_helper_rejects_a_wrong_output_and_names_regions(device=gpu)


# ---- the GPU cases ------------------------------------------------------------

KEYS = {128: bytes(range(0x10, 0x20)), 192: bytes(range(0x30, 0x48)), 256: bytes(range(0x60, 0x80))}
IV = bytes(range(0xA0, 0xB0))
CTR_HI = bytes.fromhex("0123456789abcdef")
# lo % 4096 and lo % 2048 are both non-zero: the T-table's virtual range and
# the first bitsliced task both begin with a masked head in front of block 0
LO_HEAD = 0x5A5A5A5A00000FFD
LO_FLAT = 0x5A5A5A5A00001000
SHIFTS = [0, 3]


def _ctr0(lo):
    return CTR_HI + lo.to_bytes(8, "big")


def _windows(n, w=4096, align=16):
    """Three 4 KiB windows of an n-byte buffer on block (segment) boundaries:
    the first, one in the middle, and the last one with the tail."""
    mid = n // 2 // align * align
    return [(0, min(w, n)), (mid, mid + w), ((n - w) // align * align, n)]


def _claim_stats(run):
    """run() under otc_split_stats(1): (front, back, nunits) of the claimed
    call it made, as tests/test_gpu_kernels.py split_units."""
    lib = _native.require_gpu_lib()
    fr, bk, nu = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.otc_split_stats(1)
    try:
        run()
        torch.cuda.synchronize()
        assert lib.otc_split_last_units(ctypes.byref(fr), ctypes.byref(bk), ctypes.byref(nu)) == 0
    finally:
        lib.otc_split_stats(0)
    return fr.value, bk.value, nu.value


CTR_SHAPES = [  # (bytes, low 64 bits of the counter)
    (1, LO_HEAD), (15, LO_HEAD), (16, LO_HEAD), (17, LO_HEAD),
    (16 * 100 + 3, LO_HEAD),            # one partial task with a head
    (2 * UNIT, LO_FLAT),                # no edge launch, no head
    ((1 << 20) + 5, LO_HEAD),           # just past the 256 x 1 shape
    ((4 << 20) + 19, LO_HEAD),          # just past 1024 x 1
    ((5 << 20) + 3, LO_HEAD),           # the grid-stride bulk shape
    (9 * UNIT + 16 * 77 + 3, LO_HEAD),  # partial first and last task, the tail at out + full
]
CTR_CASES = [pytest.param(bits, n, lo, id=f"{bits}-{n}")
             for bits, shapes in ((128, CTR_SHAPES), (256, CTR_SHAPES), (192, CTR_SHAPES[:3])) for n, lo in shapes]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("bits,n,lo", CTR_CASES)
@pytest.mark.parametrize("impl", ["ttable", "bitslice"])
def test_ctr_guarded(gpu, impl, bits, n, lo, shift):
    key, ctr0 = KEYS[bits], _ctr0(lo)

    def op(x, out):
        ops.ctr(x, key, ctr0, out=out, impl=impl)
        assert ops.last_impl() == impl

    run_guarded(op, gpu, n, ref=lambda x: cpu_ref.ctr(key, ctr0, host(x), threads=4), seed=n % 1009, shift=shift,
                also_inplace=True, what=f"ctr {impl} AES-{bits} {n} bytes")


@pytest.mark.gpu
def test_ctr_persistent_ttable_guarded(gpu):
    """512 MiB is the persistent claim kernel's threshold (split.cpp
    tt_ctr_persistent_min): the claim units cover the virtual range that
    starts lo % 4096 blocks in front of block 0 (aes_tt.hip
    tt_ctr_claim_units).  The whole output against the bitsliced kernel on
    plain buffers, three windows of that against the oracle."""
    n = (512 << 20) + 3 * UNIT + 16 * 9 + 11
    key, ctr0 = KEYS[128], _ctr0(LO_HEAD)
    units = ((n + 15) // 16 + LO_HEAD % 4096 + 2047) // 2048

    def op(x, out):
        _, _, nunits = _claim_stats(lambda: ops.ctr(x, key, ctr0, out=out, impl="ttable"))
        assert ops.last_impl() == "ttable" and nunits == units, (nunits, units)

    def ref(x):
        r = ops.ctr(x.clone(), key, ctr0, impl="bitslice")
        assert ops.last_impl() == "bitslice"
        for lo, hi in _windows(n):
            assert host(r[lo:hi]) == cpu_ref.ctr(key, ctr0, host(x[lo:hi]), block_offset=lo // 16), lo
        return r

    run_guarded(op, gpu, n, ref=ref, also_inplace=True, what="persistent T-table ctr")
    torch.cuda.empty_cache()


def _block_modes(key_bits):
    """name -> (op(x, out, impl), oracle(iv, bytes), in place allowed natively)"""
    k = KEYS[key_bits]
    return {
        "ecb_encrypt": (lambda x, out, impl: ops.ecb_encrypt(x, k, out=out, impl=impl),
                        lambda iv, h: cpu_ref.ecb(k, h, threads=4), True),
        "ecb_decrypt": (lambda x, out, impl: ops.ecb_decrypt(x, k, out=out, impl=impl),
                        lambda iv, h: cpu_ref.ecb(k, h, decrypt=True, threads=4), True),
        "cbc_decrypt": (lambda x, out, impl: ops.cbc_decrypt(x, k, IV, out=out, impl=impl),
                        lambda iv, h: cpu_ref.cbc(k, iv, h, decrypt=True), False),
        "cfb128_decrypt": (lambda x, out, impl: ops.cfb128_decrypt(x, k, IV, out=out, impl=impl),
                           lambda iv, h: cpu_ref.cfb128(k, iv, h, decrypt=True), False),
    }


BLOCK_MODES = ["ecb_encrypt", "ecb_decrypt", "cbc_decrypt", "cfb128_decrypt"]
INPLACE_COPY_BLOCKS = 65537  # the one shape at which CBC / CFB decryption run in place (through ops' copy)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("blocks", [1, 2, 65536, 65537, 262145, (5 << 20) // 16 + 3])
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("mode", BLOCK_MODES)
def test_block_modes_ttable_guarded(gpu, mode, bits, blocks, shift):
    """The grid T-table kernels: one block, two, the 1 MiB and 4 MiB launch
    shapes' last and first sizes, the grid-stride shape."""
    f, oracle, native_inplace = _block_modes(bits)[mode]

    def op(x, out):
        f(x, out, "ttable")
        assert ops.last_impl() == "ttable"

    run_guarded(op, gpu, 16 * blocks, ref=lambda x: oracle(IV, host(x)), seed=blocks % 1009, shift=shift,
                also_inplace=native_inplace or blocks == INPLACE_COPY_BLOCKS,
                what=f"{mode} ttable AES-{bits} {blocks} blocks")


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("blocks", [4 * 2048 + 300, 2 * 2048])
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("mode", BLOCK_MODES)
def test_block_modes_bitslice_guarded(gpu, mode, bits, blocks, shift):
    """impl="bitslice": the bitsliced claim kernel takes every unit, one
    T-table workgroup the blocks past the last unit (300, or none)."""
    f, oracle, native_inplace = _block_modes(bits)[mode]

    def op(x, out):
        f(x, out, "bitslice")
        assert ops.last_impl() == "bitslice", ops.split_fallback_reason()

    run_guarded(op, gpu, 16 * blocks, ref=lambda x: oracle(IV, host(x)), seed=blocks % 1009, shift=shift,
                also_inplace=native_inplace, what=f"{mode} bitslice AES-{bits} {blocks} blocks")


def _big_block_ref(mode, bits, n, other_impl):
    """The whole output from another kernel family on plain buffers; three
    windows of that against the oracle (a window's IV is the block in front)."""
    f, oracle, _ = _block_modes(bits)[mode]

    def ref(x):
        r = torch.empty(n, dtype=torch.uint8, device=x.device)
        f(x.clone(), r, other_impl)
        assert ops.last_impl() == other_impl
        for lo, hi in _windows(n):
            iv = IV if lo == 0 else host(x[lo - 16:lo])
            assert host(r[lo:hi]) == oracle(iv, host(x[lo:hi])), (mode, lo)
        return r

    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ecb_encrypt", "cbc_decrypt"])
def test_claimed_split_guarded(gpu, mode):
    """impl="split" at the smallest shape whose pre-assigned front, claimed
    middle and pre-assigned back are all non-empty (tests/test_gpu_kernels.py
    claimed_split): both kernels store into one guarded buffer."""
    cus = _native.require_gpu_lib().otc_device_cus(0)
    n, pf = (22 * cus + 5) * UNIT + 48, 4 * cus
    f = _block_modes(256)[mode][0]

    def op(x, out):
        front, back, nunits = _claim_stats(lambda: f(x, out, "split"))
        assert ops.last_impl() == "split", ops.split_fallback_reason()
        assert nunits == n // UNIT and front + back == nunits and front >= pf > 0, (front, back, nunits, pf)

    run_guarded(op, gpu, n, ref=_big_block_ref(mode, 256, n, "ttable"), also_inplace=mode == "ecb_encrypt",
                what=f"{mode} claimed split")
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ecb_encrypt", "cbc_decrypt"])
def test_block_modes_persistent_ttable_guarded(gpu, mode):
    """impl="auto" from 512 MiB: the persistent T-table claim kernel alone
    (split.cpp split_form), workgroup 0 finishing the 5 blocks past the last
    unit."""
    blocks = (512 << 20) // 16 + 3 * 2048 + 5
    n = 16 * blocks
    f = _block_modes(128)[mode][0]

    def op(x, out):
        _, _, nunits = _claim_stats(lambda: f(x, out, "auto"))
        assert ops.last_impl() == "ttable" and nunits == blocks // 2048, (nunits, blocks // 2048)

    run_guarded(op, gpu, n, ref=_big_block_ref(mode, 128, n, "bitslice"), also_inplace=mode == "ecb_encrypt",
                what=f"{mode} persistent T-table")
    torch.cuda.empty_cache()


IV0_CARRY = CTR_HI + (2**64 - 700).to_bytes(8, "big")  # IV_s = iv0 + s carries out of the low 64 bits at s = 700
NSEG = 64 * 19 + 37  # a partial last wave of chains


def _seg_modes(bits):
    """name -> (op(x, out, seg, impl), oracle(bytes, seg), in place allowed)"""
    k = KEYS[bits]
    return {
        "cbc_encrypt_segments": (lambda x, out, seg, impl: ops.cbc_encrypt_segments(x, k, IV0_CARRY, seg, out=out, impl=impl),
                                 lambda h, seg: cpu_ref.cbc_segments(k, IV0_CARRY, h, seg), True),
        "cfb128_encrypt_segments": (lambda x, out, seg, impl: ops.cfb128_encrypt_segments(x, k, IV0_CARRY, seg, out=out, impl=impl),
                                    lambda h, seg: cpu_ref.cfb128_segments(k, IV0_CARRY, h, seg), True),
        "cbc_decrypt_segments": (lambda x, out, seg, impl: ops.cbc_decrypt_segments(x, k, IV0_CARRY, seg, out=out, impl=impl),
                                 lambda h, seg: cpu_ref.cbc_segments(k, IV0_CARRY, h, seg, decrypt=True), False),
        "cfb128_decrypt_segments": (lambda x, out, seg, impl: ops.cfb128_decrypt_segments(x, k, IV0_CARRY, seg, out=out, impl=impl),
                                    lambda h, seg: cpu_ref.cfb128_segments(k, IV0_CARRY, h, seg, decrypt=True), False),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("seg", [16, 48, 512, 528, 4096])
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("mode", ["cbc_encrypt_segments", "cfb128_encrypt_segments", "cbc_decrypt_segments",
                                  "cfb128_decrypt_segments"])
def test_segment_modes_ttable_guarded(gpu, mode, bits, seg, shift):
    """One chain per lane (encryption) and the parallel decryption on the
    T-table: segments under 4 blocks, the 4- and 8-block burst loops and
    their remainders, 64 x 19 + 37 segments."""
    f, oracle, inplace = _seg_modes(bits)[mode]

    def op(x, out):
        f(x, out, seg, "ttable")
        assert ops.last_impl() == "ttable"

    run_guarded(op, gpu, seg * NSEG, ref=lambda x: oracle(host(x), seg), seed=seg, shift=shift,
                also_inplace=inplace or seg == 512, what=f"{mode} ttable AES-{bits} {NSEG} x {seg} bytes")


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("seg", [512, 4096])
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("mode", ["cbc_decrypt_segments", "cfb128_decrypt_segments"])
def test_segment_decrypt_bitslice_guarded(gpu, mode, bits, seg, shift):
    """Segment decryption on the bitsliced claim kernel alone: 4 units and 300
    blocks, rounded down to whole segments."""
    f, oracle, _ = _seg_modes(bits)[mode]
    n = (4 * 2048 + 300) * 16 // seg * seg

    def op(x, out):
        f(x, out, seg, "bitslice")
        assert ops.last_impl() == "bitslice", ops.split_fallback_reason()

    run_guarded(op, gpu, n, ref=lambda x: oracle(host(x), seg), seed=seg, shift=shift,
                what=f"{mode} bitslice AES-{bits} {n // seg} x {seg} bytes")


@pytest.mark.gpu
def test_segment_encrypt_persistent_guarded(gpu):
    """CBC encryption of 2^21 + 64 x 7 + 5 segments of 512 bytes, just over the
    1 GiB from which the persistent claim kernel runs (split.cpp
    segenc_persistent): 64-segment units, the 5 segments past the last unit in
    workgroup 0.  Every impl runs this kernel at this size, so the whole
    output is compared with the grid kernel run on 128 MiB pieces (IV
    iv0 + s0) in plain buffers, and three windows with the oracle.  The two
    outputs (input fills 0x00 and 0xFF) are not compared with each other:
    each equals the grid kernel's in full, and a third GiB is not held."""
    seg, nseg, key = 512, (1 << 21) + 64 * 7 + 5, KEYS[256]
    n = seg * nseg
    piece = (128 << 20) // seg

    def op(x, out):
        _, _, nunits = _claim_stats(lambda: ops.cbc_encrypt_segments(x, key, IV0_CARRY, seg, out=out))
        assert ops.last_impl() == "ttable" and nunits == nseg // 64, (nunits, nseg // 64)

    def check(x, out):
        for s0 in range(0, nseg, piece):
            lo, hi = s0 * seg, min(nseg, s0 + piece) * seg
            g = ops.cbc_encrypt_segments(x[lo:hi].clone(), key, cpu_ref.ctr128_add(IV0_CARRY, s0), seg)
            _assert_same(out[lo:hi], g, f"persistent segment encryption against the grid kernel, segment {s0} on")
            del g
        for lo, hi in _windows(n, align=seg):
            exp = cpu_ref.cbc_segments(key, cpu_ref.ctr128_add(IV0_CARRY, lo // seg), host(x[lo:hi]), seg)
            assert host(out[lo:hi]) == exp, lo

    run_guarded(op, gpu, n, check=check, compare_fills=False, what="persistent segment encryption")
    torch.cuda.empty_cache()


def _batch_messages(tile):
    """(lengths, key index, counters) for the CtrBatch cases: the edge
    lengths, then a short message directly in front of one of more than 6
    tiles whose counter is not tile-aligned (the counter-aligned tile form,
    which starts lo % tile blocks in front of the message)."""
    lens = [0, 1, 15, 16, 17, 4095, 4096, 4097, 33, 16 * (6 * 256 + 70) + 9]
    kidx = [0, 1, 0, 1, 0, 1, 0, 1, 1, 1]
    ctrs = [_ctr0(LO_HEAD + 977 * i) for i in range(len(lens))]
    ctrs[7] = CTR_HI + (2**64 - 3).to_bytes(8, "big")  # the 2^64 carry inside the message
    assert int.from_bytes(ctrs[-1][8:], "big") % tile and lens[-1] >= 6 * tile * 16
    return lens, kidx, ctrs


def _run_batch(gpu, lens, keys, kidx, ctrs, tile, form, gap, refs, expect_tiles=None, what="batch"):
    """Out of place under both input fills, then in place; every region
    against its reference, every other byte of the arenas unchanged."""
    first = None
    for inplace in (False, True):
        for fill in ((A5,) if inplace else (0x00, 0xFF)):
            tag = f"{what} [{'in place' if inplace else f'input fill 0x{fill:02X}'}]"
            ina = Arena(lens, gpu, fill, gap=gap)
            ina.fill_random(3)
            outa = ina if inplace else Arena(lens, gpu, A5, gap=gap)
            if not refs:
                refs.extend(_as_tensor(cpu_ref.ctr(keys[kidx[i]], ctrs[i], host(ina.region(i)), threads=8), gpu)
                            for i in range(len(lens)))
            if form == "list":
                b = ops.CtrBatch([ina.region(i) for i in range(len(lens))], keys, ctrs,
                                 outs=[outa.region(i) for i in range(len(lens))], key_index=kidx, tile_blocks=tile)
            else:
                (buf, offs), (obuf, _) = ina.packed(), outa.packed()
                b = ops.CtrBatch.packed(buf, lens, keys, ctrs, out=obuf, offsets=offs, key_index=kidx,
                                        tile_blocks=tile)
            if expect_tiles is not None:
                expect_tiles({nr: t for *_, t, nr in b._launches})
            else:
                assert b.aligned_msgs == 1
            b.run()
            torch.cuda.synchronize()
            for i in range(len(lens)):
                _assert_same(outa.region(i), refs[i], f"{tag}: message {i} ({lens[i]} bytes)")
            outa.assert_guards(f"{tag}: output arena")
            if not inplace:
                ina.assert_input_intact(3, tag)
                if first is None:
                    first = outa.buf.clone()
                else:
                    _assert_same(outa.buf, first, f"{tag}: output depends on bytes outside the input")
            del ina, outa, b


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [64, 128, 256])
@pytest.mark.parametrize("form", ["list", "packed"])
def test_ctr_batch_guarded(gpu, form, tile):
    """List form: every message a guarded region of its own.  Packed form:
    explicit offsets that leave 64 bytes between the slots, every byte of
    ``out`` outside the messages still 0xA5."""
    lens, kidx, ctrs = _batch_messages(tile)
    _run_batch(gpu, lens, [KEYS[128], KEYS[256]], kidx, ctrs, tile, form, GUARD if form == "list" else 64, [],
               what=f"CtrBatch {form} tile {tile}")


@pytest.mark.gpu
def test_ctr_batch_claimed_guarded(gpu):
    """A launch of at least 65536 tiles runs claimed tile runs: the shape of
    tests/test_gpu_batch.py test_claimed_batch_matches_oracle (43 AES-256
    messages of about 1.5 MiB in 1 KiB tiles, small AES-128 ones beside them)
    packed with 64-byte gaps."""
    rng = np.random.default_rng(21)
    big = [int(v) | 1 for v in rng.integers(3 << 19, (3 << 19) + (1 << 16), 43)]
    lens = big + [0, 1, 15, 16, 17, 1023, 1025, 0, 4097, 100001]
    kidx = [0] * len(big) + [1, 0, 1, 1, 0, 1, 1, 1, 0, 1]
    ctrs = [_ctr0(LO_HEAD + 7919 * i) for i in range(len(lens))]
    ctrs[2] = CTR_HI + (2**64 - 1000).to_bytes(8, "big")  # carry inside a big message

    def tiles_ok(tiles):
        assert tiles[14] >= 65536 > tiles[10] > 0, tiles

    _run_batch(gpu, lens, [KEYS[256], KEYS[128]], kidx, ctrs, 64, "packed", 64, [], expect_tiles=tiles_ok,
               what="claimed CtrBatch")
    torch.cuda.empty_cache()


def _rc4_keys(ns, gpu):
    g = torch.Generator().manual_seed(ns)
    return torch.randint(0, 256, (ns, 16), dtype=torch.uint8, generator=g).to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [0, 3, 16])
@pytest.mark.parametrize("length", [1, 15, 16, 17, 35, 64, 4096])
@pytest.mark.parametrize("ns", [200, 64])
def test_rc4_multi_guarded(gpu, ns, length, drop):
    """``out`` and ``x`` as views at both alignments (the kernel takes any; ops
    does not stage them): a partial and a full last workgroup, lengths around
    the 16-byte stores, every stream against the oracle."""
    keys = _rc4_keys(ns, gpu)
    kh = keys.cpu().numpy()
    ks = b"".join(cpu_ref.arc4_keystream(bytes(kh[s]), length, drop=drop) for s in range(ns))
    ksn = np.frombuffer(ks, dtype=np.uint8)
    for shift in SHIFTS:
        what = f"rc4_multi {ns} x {length} drop {drop}"
        run_guarded(lambda out: ops.rc4_multi(keys, length, drop=drop, out=out.view(ns, length)), gpu, ns * length,
                    n_in=(), ref=lambda: ks, shift=shift, what=what + " keystream")
        run_guarded(lambda x, out: ops.rc4_multi(keys, length, x=x.view(ns, length), drop=drop,
                                                 out=out.view(ns, length)), gpu, ns * length,
                    ref=lambda x: (x.cpu().numpy() ^ ksn).tobytes(), shift=shift, what=what + " x ^ keystream")
    assert torch.equal(keys.cpu(), torch.from_numpy(kh))


RC4_STATE = 264  # sizeof(struct rc4_state): perm[256], index1, index2


def _host_rc4(key, data):
    """rc4_init + rc4_crypt on the host: (output, the struct rc4_state afterwards)."""
    lib = _native.cpu_lib()
    st = _native.Rc4State()
    lib.rc4_init(ctypes.byref(st), key, len(key))
    o = ctypes.create_string_buffer(max(len(data), 1))
    lib.rc4_crypt(ctypes.byref(st), data, o, len(data))
    return o.raw[:len(data)], bytes(st)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [1, 15, 16, 17, 35, 64, 4096])
@pytest.mark.parametrize("ns", [200, 64])
def test_rc4_crypt_batch_guarded(gpu, ns, length):
    """The data as for ``rc4_multi``; the states in an arena of their own: the
    write-back of perm, index1 and index2 stays within 264 bytes per stream.
    Every stream's output and state against the host ``rc4_crypt``."""
    keys = [bytes((7 * r + 13 * i + 1) & 0xFF for i in range(1 + r % 32)) for r in range(ns)]
    st0 = ops.rc4_states(keys).reshape(-1).to(gpu)
    held = {}

    def ref(x):
        xh = x.cpu().numpy().reshape(ns, length)
        res = [_host_rc4(keys[r], xh[r].tobytes()) for r in range(ns)]
        held["states"] = _as_tensor(b"".join(s for _, s in res), gpu)
        return b"".join(o for o, _ in res)

    def op(x, out):
        held["arena"] = sa = Arena(ns * RC4_STATE, gpu)
        sa.region().copy_(st0)
        ops.rc4_crypt_batch(sa.region().view(ns, RC4_STATE), x.view(ns, length), out=out.view(ns, length))

    def check_states(x, out):
        sa = held.pop("arena")
        sa.assert_guards(f"rc4_crypt_batch {ns} x {length}: states arena")
        _assert_same(sa.region(), held["states"], f"rc4_crypt_batch {ns} x {length}: states written back")

    for shift in SHIFTS:
        run_guarded(op, gpu, ns * length, ref=ref, check=check_states, shift=shift, also_inplace=True,
                    what=f"rc4_crypt_batch {ns} x {length}")


STREAM_SIZES = [0, 1, 15, 16, 17, 4096 + 5, (1 << 20) + 13]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", STREAM_SIZES)
def test_xor_guarded(gpu, n, shift):
    run_guarded(lambda a, b, out: ops.xor(a, b, out=out), gpu, n, n_in=(n, n),
                ref=lambda a, b: (a.cpu().numpy() ^ b.cpu().numpy()).tobytes(), seed=n % 1009, shift=shift,
                also_inplace=True, what=f"xor {n} bytes")


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", STREAM_SIZES)
def test_fill_random_guarded(gpu, n, shift):
    """The splitmix64 layout is not pinned bytewise, so the fill is compared
    with itself: the same seed in an unguarded buffer of the same length and
    alignment gives the same bytes."""
    plain = torch.empty(n + 16, dtype=torch.uint8, device=gpu)[shift:shift + n]
    ops.fill_random_(plain, seed=77)
    run_guarded(lambda out: ops.fill_random_(out, seed=77), gpu, n, n_in=(), ref=lambda: plain, shift=shift,
                what=f"fill_random_ {n} bytes")
    if n >= 16:
        assert len(set(host(plain))) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 11, 12, 27, 4099])
def test_ctr_stream_update_guarded(gpu, n):
    """One ``update`` after 5 consumed bytes (nc_off = 5), at each of the 16
    alignments, input and output aligned alike so that nothing is staged: the
    head from the kept keystream block (11 bytes), the funnel-shift body and
    the partial tail, against the oracle over the whole stream."""
    key, ctr0 = KEYS[128], _ctr0(LO_HEAD)
    head = bytes(range(1, 6))
    head_dev = _as_tensor(head, gpu)

    def op(x, out):
        s = ops.CtrStream(key, ctr0)
        s.update(head_dev)
        assert s.nc_off == 5
        assert x.data_ptr() % 16 == out.data_ptr() % 16
        s.update(x, out=out)
        assert s.nc_off == (5 + n) % 16

    for a in range(16):
        run_guarded(op, gpu, n, ref=lambda x: cpu_ref.ctr(key, ctr0, head + host(x))[5:], seed=n, shift=a,
                    also_inplace=True, what=f"CtrStream.update {n} bytes at alignment {a}")
