"""Every persistent claim kernel against the C oracle, byte for byte, at sizes
small enough to check whole: the child program of tests/test_gpu_claim_forms.py
(and, for its plan, of tests/test_claim_forms_cpu.py).

    python tests/claim_forms_child.py --out FILE [--set NAME] [--only CASE ...]
    python tests/claim_forms_child.py --plan --cus N [--set NAME]

The persistent kernels (one workgroup per CU; the last pb = min(nunits, 16 CUs)
units handed to the waves by the host, the units before them taken from one
atomic word, the blocks past the last unit run by workgroup 0: otc_device.h
SplitClaim, split.cpp claim_alone) are routed to from 512 MiB or 1 GiB.  The
thresholds are read once per process from OTC_TT_PERSISTENT_MIN_MIB,
OTC_TT_CTR_PERSISTENT_MIN_MIB and OTC_SEGENC_PERSISTENT_MIN_MIB, so a process
STARTED with them at 0 reaches every claim path between 64 KiB and about
130 MiB.  This program never sets them: the set "thresholds" expects them to
be 0 in its environment, the sets "forms" and "envcheck" expect the defaults.

Each case: seeded input, fixed key / IV / counter; the oracle's output for the
whole buffer, uploaded; torch.equal on every byte of the device output, out of
place and (where the mode allows) in place; and the proof of path -- the claim
accounting (otc_split_stats / otc_split_last_units) read around each call.  A
claimed call must report the planned unit count (a one-unit marker call runs
before it, so the count is this call's), a call planned to run the grid kernel
must leave the accounting of the call before it untouched (which is why
consecutive cases never plan the same unit count).

One JSON record per case is appended to FILE as the case ends (oracle_s: an
oracle output shared by several cases is charged to the first of them).  Exit status 0:
ran to the end, whatever the cases found; 3: an exception stopped the run
(nothing more is started on the GPU after one).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
import traceback
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

UNIT_BLOCKS = 2048           # otc_device.h CLAIM_UNIT
UNIT = UNIT_BLOCKS * 16      # bytes of one claim unit of the whole-buffer modes
SEG_UNIT = 64                # otc_device.h SEG_UNIT: segments per unit of the persistent segment encryption
CTR_PER = 4096               # aes_tt.hip CTR_BULK_PER: the persistent CTR kernel's counter alignment, blocks
MIN_UNITS = 2                # split.cpp job_run / engine.cpp ctr_common: claim_alone's minimum
SEGENC_MIN_UNITS = 16        # engine.cpp seg_enc_run
SETS = ("thresholds", "forms", "envcheck")
SEED = 0x0C1A1F02            # the input bytes of every case: one seeded buffer, each case a prefix of it

# ---- fixed keys, IVs and counters ------------------------------------------
IV = bytes.fromhex("f0e1d2c3b4a5968778695a4b3c2d1e0f")
IV0_SEG = bytes.fromhex("0123456789abcdef") + (2**64 - 3).to_bytes(8, "big")  # IV_s carries into the high half at s = 3
# CTR: the counter's low half is 2^64 - CTR_K0 and block_offset is odd, so the
# first block's counter is 2^64 - CTR_K: not a multiple of 4096 (a masked head
# of CTR_SHIFT blocks in front of the virtual range) and the low half wraps at
# virtual block CTR_SHIFT + CTR_K = 4096, the first block of unit 2.
CTR_BLOCK_OFFSET = 1234567
CTR_K = 2861
CTR_K0 = CTR_K + CTR_BLOCK_OFFSET
CTR_SHIFT = (-CTR_K) % CTR_PER  # 1235
COUNTER = bytes.fromhex("00112233445566ff") + (2**64 - CTR_K0).to_bytes(8, "big")
RFC_NONCE = bytes.fromhex("a1b2c3d4")
RFC_IVEC = bytes.fromhex("5e6f7081") + b"\xff" * 4  # nonce | ivec | 00000001: the low half is 0xffffffff00000001 ...
RFC_BLOCK_OFFSET = 2**32 - 1 - CTR_K                # ... + this = 2^64 - CTR_K; the 64-bit wrap leaves the high half alone


def key_of(bits: int) -> bytes:
    return bytes((37 * i + bits) & 0xFF for i in range(bits // 8))


def tt_waves(cus: int) -> int:
    """The waves of a persistent T-table kernel: 16 per workgroup, one workgroup per CU."""
    return 16 * cus


def claimed_split_bytes(cus: int) -> int:
    """tests/test_gpu_kernels.py claimed_split(): the smallest impl="split"
    shape whose pre-assigned front (4 per CU), claimed middle (2 per CU + 5)
    and pre-assigned back (16 per CU) are all non-empty, 3 blocks past the last unit."""
    return (22 * cus + 5) * UNIT + 48


# ---- the plan ---------------------------------------------------------------
# A case is a plain dict (it is printed and recorded as JSON):
#   name, set, kind (whole | segdec | ctr | rfc3686 | segenc), mode, bits,
#   nbytes, seg (bytes of a segment, 0: none), impls (the out-of-place calls),
#   inplace, form (claim | grid | bitslice | split: the kernels planned),
#   units (the claim units of the call -- for "grid", what a claimed run would
#   report), unit_of (blocks, or segments, per unit), head (blocks in front of
#   the virtual range: CTR), pf / pb (units handed to the bitsliced / the
#   T-table waves without a claim), claimed (units taken from the claim word),
#   past (blocks, or segments, past the last unit), idle (T-table waves without
#   a unit), reaches (what the shape is there for; checked from the plan alone
#   by tests/test_claim_forms_cpu.py).

def _claim_fields(form: str, units: int, total: int, unit_of: int, cus: int, exact_units: bool) -> dict:
    w = tt_waves(cus)
    if form == "grid":
        return dict(pf=0, pb=0, claimed=0, past=0, idle=0)
    pb = 0 if form == "bitslice" else min(units, w)  # split.cpp preassigned_back
    # split.cpp split_run: 4 waves per bitsliced workgroup, one workgroup per CU beside the T-table, three alone
    pf = {"split": min(units - pb, 4 * cus), "bitslice": min(units, 12 * cus)}.get(form, 0)
    past = 0 if exact_units else total - units * unit_of
    return dict(pf=pf, pb=pb, claimed=units - pb - pf, past=past, idle=0 if form == "bitslice" else w - pb)


def _case(cset, name, kind, mode, bits, nbytes, form, units, cus, reaches, seg=0, impls=("ttable",), inplace=False,
          unit_of=UNIT_BLOCKS, head=0, note=""):
    total = nbytes // seg if kind == "segenc" else (nbytes + 15) // 16
    c = dict(name=name, set=cset, kind=kind, mode=mode, bits=bits, nbytes=nbytes, seg=seg, impls=list(impls),
             inplace=inplace, form=form, units=units, unit_of=unit_of, head=head, reaches=list(reaches), note=note)
    # CTR counts its units over the virtual range, rounded up: nothing lies past them
    c.update(_claim_fields(form, units, total, unit_of, cus, exact_units=kind in ("ctr", "rfc3686")))
    return c


WHOLE_MODES = ("ecb-enc", "ecb-dec", "cbc-dec", "cfb-dec")
WHOLE_INPLACE = {"ecb-enc": True, "ecb-dec": True, "cbc-dec": False, "cfb-dec": False}
CLAIMED_BITS = {"ecb-enc": 128, "ecb-dec": 192, "cbc-dec": 256, "cfb-dec": 128}  # every NR instantiation gets one
FORMS_BITS = {"ecb-enc": 256, "ecb-dec": 128, "cbc-dec": 192, "cfb-dec": 256}


def whole_shapes(cus: int) -> dict:
    w = tt_waves(cus)
    return {"one-unit": 1 * UNIT + 48, "two-units": 2 * UNIT + 48, "waves-minus-1": (w - 1) * UNIT,
            "all-preassigned": w * UNIT, "claimed": (w + 5) * UNIT + 48}


WHOLE_REACHES = {
    "one-unit": ("fallback",),
    "two-units": ("idle-waves", "past", "no-claimed"),
    "waves-minus-1": ("one-idle-wave", "no-past", "no-claimed"),
    "all-preassigned": ("no-idle-waves", "no-claimed", "no-past"),
    "claimed": ("claimed", "past", "no-idle-waves"),
}


def _whole(cset, mode, bits, shape, cus, form, impls):
    n = whole_shapes(cus)[shape]
    units = n // UNIT
    if form == "claim" and units < MIN_UNITS:
        form = "grid"
    reaches = {"claim": WHOLE_REACHES[shape], "grid": ("fallback",) if units < MIN_UNITS else ("default-threshold",),
               "bitslice": ("front-only", "past"),
               "split": ("back-only", "past")}[form]  # a two-unit split: both units the T-table's, pre-assigned
    return _case(cset, f"{mode}-{bits}/{shape}/{form}", "whole", mode, bits, n, form, units, cus, reaches,
                 impls=impls, inplace=WHOLE_INPLACE[mode])


def plan_thresholds(cus: int) -> list:
    w = tt_waves(cus)
    cases = []
    both = ("ttable", "auto")
    # -- ECB both ways, CBC / CFB128 decryption: job_run -> FORM_TT -> claim_alone(blocks / 2048, 2)
    for mode in WHOLE_MODES:
        for bits in (128, 192, 256):
            cases.append(_whole("thresholds", mode, bits, "two-units", cus, "claim", both))
            cases.append(_whole("thresholds", mode, bits, "one-unit", cus, "claim", both))
        cases.append(_whole("thresholds", mode, CLAIMED_BITS[mode], "claimed", cus, "claim", both))
        if mode in ("ecb-enc", "cbc-dec"):
            cases.append(_whole("thresholds", mode, CLAIMED_BITS[mode], "waves-minus-1", cus, "claim", both))
            cases.append(_whole("thresholds", mode, CLAIMED_BITS[mode], "all-preassigned", cus, "claim", both))
    # -- segment decryption on the same path, IV_s = iv0 + s computed in the kernel
    for mode in ("cbc-dec-seg", "cfb-dec-seg"):
        n = 2 * UNIT + 48
        cases.append(_case("thresholds", f"{mode}-256/seg16/two-units/claim", "segdec", mode, 256, n, "claim", n // UNIT,
                           cus, ("idle-waves", "past", "no-claimed"), seg=16, impls=both))
        # the `claimed` shape's 48 trailing bytes are no whole 4 KiB segment: one whole segment instead,
        # so workgroup 0's blocks past the last unit begin a segment (IV_s there)
        n = (w + 5) * UNIT + 4096
        cases.append(_case("thresholds", f"{mode}-256/seg4096/claimed/claim", "segdec", mode, 256, n, "claim", n // UNIT,
                           cus, ("claimed", "past", "no-idle-waves"), seg=4096, impls=both,
                           note="8 segments per unit; 256 blocks (one segment) past the last unit"))
        # `claimed` rounded down to whole 64 KiB segments: W + 5 is odd, so W + 4 units and no block past the last
        n = ((w + 5) * UNIT + 48) // 65536 * 65536
        cases.append(_case("thresholds", f"{mode}-256/seg65536/claimed/claim", "segdec", mode, 256, n, "claim", n // UNIT,
                           cus, ("claimed", "no-past", "no-idle-waves", "segment-spans-units"), seg=65536, impls=both,
                           note="each segment spans two claim units; 0 blocks past the last unit"))
    # -- CTR on the T-table: units over the virtual range (the masked head counts), tt_ctr_claim_units
    def ctr_case(kind, bits, shape, blocks, tail):
        n = blocks * 16 + tail
        units = -(-(blocks + (1 if tail else 0) + CTR_SHIFT) // UNIT_BLOCKS)
        form = "claim" if units >= MIN_UNITS else "grid"
        reaches = {"claimed": ("claimed", "no-idle-waves", "carry-in-claimed-unit", "masked-head", "partial-block"),
                   "two-units": ("idle-waves", "no-claimed", "masked-head", "partial-block"),
                   "one-unit": ("fallback",)}[shape]
        return _case("thresholds", f"{kind}-{bits}/{shape}/{form}", kind, kind, bits, n, form, units, cus, reaches,
                     impls=("ttable",), inplace=True, head=CTR_SHIFT)
    claimed_blocks = (w + 5) * UNIT_BLOCKS - CTR_SHIFT - 100 - 1  # + the partial block: 100 blocks short of W + 5 units
    for bits in (128, 192, 256):
        cases.append(ctr_case("ctr", bits, "two-units", 2000, 11))
        cases.append(ctr_case("ctr", bits, "one-unit", 500, 11))
        if bits != 192:
            cases.append(ctr_case("ctr", bits, "claimed", claimed_blocks, 11))
    cases.append(ctr_case("rfc3686", 256, "two-units", 2000, 11))
    cases.append(ctr_case("rfc3686", 128, "claimed", claimed_blocks, 11))
    # -- segment encryption: 64-segment units, claim_alone's minimum 16 units, the < 64 segments past the
    #    last unit in wave 0 of workgroup 0
    def segenc(mode, bits, seg, shape, nseg, reaches):
        units = nseg // SEG_UNIT
        form = "claim" if units >= SEGENC_MIN_UNITS else "grid"
        return _case("thresholds", f"{mode}-{bits}/seg{seg}/{shape}/{form}", "segenc", mode, bits, seg * nseg, form,
                     units, cus, reaches, seg=seg, impls=("auto",), inplace=True, unit_of=SEG_UNIT)
    big, few = (w + 5) * SEG_UNIT + 37, 16 * SEG_UNIT + 37
    for mode in ("cbc-enc-seg", "cfb-enc-seg"):
        cases.append(segenc(mode, 256, 512, "preassigned-only", few, ("no-claimed", "past")))
        cases.append(segenc(mode, 256, 16, "claimed", big, ("claimed", "past", "no-idle-waves")))
        cases.append(segenc(mode, 256, 512, "no-remainder", w * SEG_UNIT, ("no-claimed", "no-past", "no-idle-waves")))
        cases.append(segenc(mode, 128, 16, "claimed", big, ("claimed", "past", "no-idle-waves")))
        cases.append(segenc(mode, 256, 4096, "preassigned-only", few, ("no-claimed", "past")))
        cases.append(segenc(mode, 256, 48, "claimed", big, ("claimed", "past", "no-idle-waves")))  # no power of two
        cases.append(segenc(mode, 256, 512, "below-minimum", 15 * SEG_UNIT + 63, ("fallback",)))
    return cases


def plan_forms(cus: int) -> list:
    """The claimed forms that need no variable -- the bitsliced claim kernel
    alone (FORM_BS), the co-resident split (FORM_SPLIT) -- and the grid
    T-table kernel, on the same shapes, each against the oracle."""
    cases = []
    for mode in WHOLE_MODES:
        bits = FORMS_BITS[mode]
        cases.append(_whole("forms", mode, bits, "claimed", cus, "bitslice", ("bitslice",)))
        cases.append(_whole("forms", mode, bits, "two-units", cus, "grid", ("ttable", "auto")))
        n = claimed_split_bytes(cus)
        cases.append(_case("forms", f"{mode}-{bits}/claimed-split/split", "whole", mode, bits, n, "split", n // UNIT, cus,
                           ("split-front-middle-back", "past"), impls=("split",), inplace=WHOLE_INPLACE[mode]))
        cases.append(_whole("forms", mode, bits, "two-units", cus, "bitslice", ("bitslice",)))
        cases.append(_whole("forms", mode, bits, "claimed", cus, "grid", ("ttable", "auto")))
        cases.append(_whole("forms", mode, bits, "two-units", cus, "split", ("split",)))
    return cases


def plan_envcheck(cus: int) -> list:
    """One call for a process started with an unparsable threshold: the
    default must hold, so the grid kernel runs."""
    return [_whole("envcheck", "ecb-enc", 256, "two-units", cus, "grid", ("ttable", "auto"))]


def plan(cus: int, which: str = "thresholds") -> list:
    if cus < 1:
        raise ValueError("cus must be at least 1")
    return {"thresholds": plan_thresholds, "forms": plan_forms, "envcheck": plan_envcheck}[which](cus)


def print_plan(cus: int, which: str, out=None):
    out = out or sys.stdout
    print(f"# set {which}, {cus} CUs: {tt_waves(cus)} T-table waves, unit {UNIT} B ({UNIT_BLOCKS} blocks; "
          f"segment encryption: {SEG_UNIT} segments)", file=out)
    print(f"{'case':<50} {'bytes':>11} {'form':<8} {'units':>6} {'pf':>5} {'pb':>5} {'claimed':>7} {'past':>5} {'idle':>5}", file=out)
    for c in plan(cus, which):
        print(f"{c['name']:<50} {c['nbytes']:>11} {c['form']:<8} {c['units']:>6} {c['pf']:>5} {c['pb']:>5} {c['claimed']:>7} "
              f"{c['past']:>5} {c['idle']:>5}" + (f"  # {c['note']}" if c["note"] else ""), file=out)


# ---- the oracle -------------------------------------------------------------
def seg_oracle(mode: str, key: bytes, iv0: bytes, data, seg: int, decrypt: bool, threads: int = 8):
    """CBC ("cbc") or CFB128 ("cfb") over independent segments of ``seg`` bytes
    with IV_s = iv0 + s (128-bit big-endian): one aes_crypt_cbc /
    aes_crypt_cfb128 call of the C oracle per segment -- what
    cpu_ref.cbc_segments / cfb128_segments compute, without their per-segment
    copies, and the segments shared among threads (the C calls drop the GIL).
    ``data``: a writable numpy uint8 array; returns one of the same size."""
    import numpy as np

    from our_tree_amd import _native
    from our_tree_amd.models import cpu_ref

    n = int(data.size)
    if seg <= 0 or seg % 16 or n % seg or not data.flags.c_contiguous:
        raise ValueError("whole segments of whole blocks, contiguous")
    nseg = n // seg
    out = np.empty(n, dtype=np.uint8)
    lib = _native.cpu_lib()
    base = int.from_bytes(iv0, "big")
    direction = cpu_ref.AES_DECRYPT if decrypt else cpu_ref.AES_ENCRYPT
    # the two C functions once more, with plain addresses for their buffers: a segment is an offset, not an object
    vp = ctypes.c_void_p
    cbc = ctypes.CFUNCTYPE(ctypes.c_int, vp, ctypes.c_int, ctypes.c_size_t, vp, vp, vp)(("aes_crypt_cbc", lib))
    cfb = ctypes.CFUNCTYPE(ctypes.c_int, vp, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp)(("aes_crypt_cfb128", lib))
    src, dst = data.ctypes.data, out.ctypes.data

    def work(lo, hi):
        ctx = cpu_ref._ctx(key, decrypt and mode == "cbc")  # CFB runs the forward cipher both ways
        pctx = ctypes.byref(ctx)
        ivb = (ctypes.c_uint8 * 16)()
        off = ctypes.c_int(0)
        poff = ctypes.byref(off)
        for s in range(lo, hi):
            ctypes.memmove(ivb, ((base + s) % (1 << 128)).to_bytes(16, "big"), 16)
            if mode == "cbc":
                rc = cbc(pctx, direction, seg, ivb, src + s * seg, dst + s * seg)
            else:
                off.value = 0
                rc = cfb(pctx, direction, seg, poff, ivb, src + s * seg, dst + s * seg)
            if rc:
                raise RuntimeError(f"oracle call failed: {rc}")

    threads = max(1, min(threads, nseg))
    step = -(-nseg // threads)
    if threads == 1:
        work(0, nseg)
        return out
    with ThreadPoolExecutor(threads) as pool:
        for f in [pool.submit(work, lo, min(nseg, lo + step)) for lo in range(0, nseg, step)]:
            f.result()
    return out


def oracle_key(c: dict) -> tuple:
    """Cases with the same key compute prefixes of one oracle output (every
    mode here is prefix-stable: a shorter call is the longer one cut short)."""
    return (c["kind"], c["mode"], c["bits"], c["seg"])


def oracle(c: dict, data, threads: int):
    """The oracle's output for the input bytes ``data`` (numpy uint8) of case c's call."""
    import numpy as np

    from our_tree_amd.models import cpu_ref

    key, kind, mode = key_of(c["bits"]), c["kind"], c["mode"]
    if kind in ("segdec", "segenc"):
        return seg_oracle("cbc" if mode.startswith("cbc") else "cfb", key, IV0_SEG, data, c["seg"],
                          decrypt=kind == "segdec", threads=threads if c["seg"] >= 2048 else 1)  # short calls: the GIL
    b = data.tobytes()
    if kind == "ctr":
        r = cpu_ref.ctr(key, COUNTER, b, CTR_BLOCK_OFFSET, threads=threads)
    elif kind == "rfc3686":
        r = cpu_ref.aesni_ctr(key, RFC_NONCE, RFC_IVEC, b, RFC_BLOCK_OFFSET)
    elif mode == "ecb-enc":
        r = cpu_ref.ecb(key, b, threads=threads)
    elif mode == "ecb-dec":
        r = cpu_ref.ecb(key, b, decrypt=True, threads=threads)
    elif mode == "cbc-dec":
        r = cpu_ref.cbc(key, IV, b, decrypt=True)
    elif mode == "cfb-dec":
        r = cpu_ref.cfb128(key, IV, b, decrypt=True)
    else:
        raise ValueError(mode)
    return np.frombuffer(r, dtype=np.uint8).copy()  # writable, as torch.from_numpy wants it


# ---- the device side --------------------------------------------------------
def device_call(c: dict, x, impl: str, out=None):
    from our_tree_amd import ops

    key, mode, seg = key_of(c["bits"]), c["mode"], c["seg"]
    if c["kind"] == "ctr":
        return ops.ctr(x, key, COUNTER, out=out, block_offset=CTR_BLOCK_OFFSET, impl=impl)
    if c["kind"] == "rfc3686":
        return ops.ctr_rfc3686(x, key, RFC_NONCE, RFC_IVEC, out=out, block_offset=RFC_BLOCK_OFFSET, impl=impl)
    f = {"ecb-enc": lambda: ops.ecb_encrypt(x, key, out=out, impl=impl),
         "ecb-dec": lambda: ops.ecb_decrypt(x, key, out=out, impl=impl),
         "cbc-dec": lambda: ops.cbc_decrypt(x, key, IV, out=out, impl=impl),
         "cfb-dec": lambda: ops.cfb128_decrypt(x, key, IV, out=out, impl=impl),
         "cbc-dec-seg": lambda: ops.cbc_decrypt_segments(x, key, IV0_SEG, seg, out=out, impl=impl),
         "cfb-dec-seg": lambda: ops.cfb128_decrypt_segments(x, key, IV0_SEG, seg, out=out, impl=impl),
         "cbc-enc-seg": lambda: ops.cbc_encrypt_segments(x, key, IV0_SEG, seg, out=out, impl=impl),
         "cfb-enc-seg": lambda: ops.cfb128_encrypt_segments(x, key, IV0_SEG, seg, out=out, impl=impl)}[mode]
    return f()


def unit_of_offset(c: dict, off: int) -> int:
    """The claim unit that byte ``off`` of case c's buffer belongs to (>= units: past the last unit)."""
    if c["kind"] == "segenc":
        return off // c["seg"] // SEG_UNIT
    return (off // 16 + c["head"]) // UNIT_BLOCKS


MARKER = (1, 0, 1)  # (front, back, nunits) of a one-unit impl="bitslice" call: the bitsliced claim kernel alone


class Stats:
    """otc_split_stats(1) for the life of the run; read(): (front, back, nunits) of the thread's last claimed call."""

    def __init__(self):
        from our_tree_amd import _native

        self.lib = _native.require_gpu_lib()
        self.lib.otc_split_stats(1)

    def read(self):
        fr, bk, nu = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        if self.lib.otc_split_last_units(ctypes.byref(fr), ctypes.byref(bk), ctypes.byref(nu)) != 0:
            raise RuntimeError("otc_split_last_units failed")
        return fr.value, bk.value, nu.value

    def close(self):
        self.lib.otc_split_stats(0)


def path_problem(c: dict, cus: int, before, after, ran: str):
    """None, or why the accounting around one call is not what case c plans."""
    form, units = c["form"], c["units"]
    fr, bk, nu = after
    want_impl = {"claim": "ttable", "grid": "ttable", "bitslice": "bitslice", "split": "split"}[form]
    if ran != want_impl:
        return f"ran {ran!r}, planned {want_impl!r}"
    if form == "grid":
        if before[2] == units:
            return f"undecidable: the call before also had {units} units"
        return None if after == before else f"planned the grid kernel, but a claimed run reported {after} (before: {before})"
    if nu != units:
        return f"planned a claimed run of {units} units, the accounting says {after} (before: {before})"
    if form == "claim" and (fr, bk) != (0, units):
        return f"front {fr} back {bk}, planned 0 / {units}"
    if form == "bitslice" and (fr, bk) != (units, 0):
        return f"front {fr} back {bk}, planned {units} / 0"
    if form == "split":
        pb = min(units, 16 * cus)
        pf = min(units - pb, 4 * cus)  # split.cpp split_run: one 4-wave bitsliced workgroup per CU
        if fr + bk != units or fr < pf or bk < pb:
            return f"front {fr} back {bk} of {units}, planned front >= {pf}, back >= {pb}"
    return None


def run_cases(cases: list, which: str, out_path: str) -> int:
    import numpy as np
    import torch

    from our_tree_amd import _native, ops
    from our_tree_amd.models import cpu_ref

    lib = _native.require_gpu_lib()
    cus = lib.otc_device_cus(0)
    dev = torch.device("cuda", 0)
    threads = max(1, min(16, os.cpu_count() or 1))
    # cases are planned for THIS device's CU count: re-plan, keep the selection
    names = [c["name"] for c in cases]
    by_name = {c["name"]: c for c in plan(cus, which)}
    cases = [by_name[n] for n in names]
    need = {}
    for c in cases:
        need[oracle_key(c)] = max(need.get(oracle_key(c), 0), c["nbytes"])
    host_in = np.random.default_rng(SEED).integers(0, 256, size=max(c["nbytes"] for c in cases), dtype=np.uint8)
    dev_in = torch.from_numpy(host_in).to(dev)
    refs = {}
    stats = Stats()
    status = 0
    with open(out_path, "w") as fh:
        for c in cases:
            rec = dict(name=c["name"], set=c["set"], passed=False, skipped=None, first_diff=None, diff_unit=None, ran=None,
                       units=None, planned=dict(form=c["form"], units=c["units"], pf=c["pf"], pb=c["pb"],
                                                claimed=c["claimed"], past=c["past"]), nbytes=c["nbytes"], cus=cus, device_s=0.0, oracle_s=0.0,
                       problems=[], calls=[])
            try:
                if c["kind"] == "rfc3686" and not cpu_ref.aesni_supported():
                    rec["skipped"] = "no AES-NI on this host (cpu_ref.aesni_ctr is the oracle of ctr_rfc3686)"
                    continue
                n, k = c["nbytes"], oracle_key(c)
                if k not in refs:
                    t0 = time.perf_counter()
                    refs[k] = torch.from_numpy(oracle(c, host_in[:need[k]], threads)).to(dev)
                    rec["oracle_s"] = round(time.perf_counter() - t0, 3)
                ref, x = refs[k][:n], dev_in[:n]
                before = stats.read()
                runs = [(impl, False) for impl in c["impls"]] + ([(c["impls"][0], True)] if c["inplace"] else [])
                for impl, inplace in runs:
                    if c["form"] != "grid":
                        # the calls of one case plan the same unit count: a one-unit claimed call in between,
                        # so that a call which claimed nothing cannot pass for the one before it
                        ops.ecb_encrypt(dev_in[:UNIT], key_of(128), impl="bitslice")
                        torch.cuda.synchronize()
                        before = stats.read()
                        if before != MARKER:
                            rec["problems"].append(f"the one-unit marker call reported {before}, not {MARKER}")
                    t0 = time.perf_counter()
                    if inplace:
                        y = x.clone()
                        device_call(c, y, impl, out=y)
                    else:
                        y = device_call(c, x, impl)
                    torch.cuda.synchronize()
                    rec["device_s"] = round(rec["device_s"] + time.perf_counter() - t0, 4)
                    ran, after = ops.last_impl(), stats.read()
                    call = dict(impl=impl, inplace=inplace, ran=ran, front=after[0], back=after[1], nunits=after[2],
                                equal=bool(torch.equal(y, ref)), first_diff=None)
                    if not call["equal"]:
                        off = int((y != ref).to(torch.uint8).argmax())
                        call["first_diff"] = off
                        if rec["first_diff"] is None:
                            rec["first_diff"], rec["diff_unit"] = off, unit_of_offset(c, off)
                        rec["problems"].append(f"impl {impl}{' in place' if inplace else ''}: first differing byte {off}, "
                                               f"unit {unit_of_offset(c, off)} of {c['units']}")
                    why = path_problem(c, cus, before, after, ran)
                    if why:
                        extra = ops.split_fallback_reason()
                        rec["problems"].append(f"impl {impl}{' in place' if inplace else ''}: {why}" +
                                               (f" ({extra})" if extra else ""))
                    rec["calls"].append(call)
                    rec["ran"] = f"{ran}/{'unplanned' if why else c['form']}"
                    rec["units"] = dict(front=after[0], back=after[1], nunits=after[2])
                    del y
                rec["passed"] = not rec["problems"]
            except Exception:  # nothing more on the GPU after an error: the record says why
                rec["problems"].append(traceback.format_exc())
                traceback.print_exc()
                status = 3
            finally:
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
                print(f"{'SKIP' if rec['skipped'] else 'ok  ' if rec['passed'] else 'FAIL'} {rec['name']:<50} "
                      f"{rec['ran'] or '-':<18} units {rec['units']} device {rec['device_s']:.3f}s oracle "
                      f"{rec['oracle_s']:.3f}s" + "".join("\n     " + p.splitlines()[-1] for p in rec["problems"]),
                      flush=True)
            if status:
                break
    if not status:
        stats.close()
    return status


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="the JSON-lines file of records")
    ap.add_argument("--set", default="thresholds", choices=SETS)
    ap.add_argument("--only", nargs="+", default=None, metavar="CASE", help="run (or plan) only these cases")
    ap.add_argument("--plan", action="store_true", help="print the plan for --cus CUs; no GPU is touched")
    ap.add_argument("--cus", type=int, default=256)
    a = ap.parse_args(argv)
    cases = plan(a.cus, a.set)
    if a.only:
        unknown = sorted(set(a.only) - {c["name"] for c in cases})
        if unknown:
            ap.error(f"no such case in set {a.set}: {unknown}")
        cases = [c for c in cases if c["name"] in a.only]
    if a.plan:
        if a.only:
            print(json.dumps(cases, indent=1))
        else:
            print_plan(a.cus, a.set)
        return 0
    if not a.out:
        ap.error("--out FILE is required to run")
    return run_cases(cases, a.set, a.out)


if __name__ == "__main__":
    sys.exit(main())
