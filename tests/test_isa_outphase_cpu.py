"""Static check of what the depth-first CTR output phase is for (no GPU
needed): in the built bulk kernels every plaintext load is issued far ahead of
the wait that needs it (tools/isa_load_distance.py: VALU instructions between
the youngest load an ``s_waitcnt vmcnt(N)`` covers and the wait).

The parent of this change (all four transposes, then the slots in order with
loads 8 slots ahead), measured once with the same tool on its aes_bs.o, for
AES-128 / 192 / 256 alike:

    min_distance 2            the conservative vmcnt(0) in front of the first
                              staged-LDS read, 2 VALU after the loads of slots
                              10 and 11 (late_under_first_vmcnt0 2)
    min_after_first 35        the smallest distance of every other wait
                              (35-56 VALU over 15-16 waits)

The issue sets the bound at twice the parent's minimum; both of the parent's
figures are held to it.  With OTC_BS_OUT_DFS=1 the tool gives 222 for both and
0 late loads."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "build", "obj", "hip", "aes_bs.o")
LLVM = "/opt/rocm/lib/llvm/bin"

PARENT_MIN_DISTANCE = 2
PARENT_MIN_AFTER_FIRST = 35


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"):
        pytest.skip("no built aes_bs.o (make) or no ROCm LLVM tools")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_load_distance.py"), OBJ], check=True,
                         capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.search(r": ([\w-]+) (AES-\d+) waits (\d+) min_distance (-?\d+) min_after_first (-?\d+) "
                      r"late_under_first_vmcnt0 (\d+)", line)
        if m:
            rows[(m.group(1), m.group(2))] = tuple(int(m.group(i)) for i in (3, 4, 5, 6))
    return rows


def test_every_ctr_bulk_kernel_analysed(rows):
    for mode in ("CTR", "CTR-nocache"):
        for bits in ("AES-128", "AES-192", "AES-256"):
            assert (mode, bits) in rows, (mode, bits, sorted(rows))
            # 22 register slots, retired by more than a handful of waits
            assert rows[(mode, bits)][0] >= 8, (mode, bits, rows[(mode, bits)])


def test_no_late_load_under_the_first_vmcnt0(rows):
    """no load issued after the byte stages of the output transposes is
    covered by the first vmcnt(0) of the phase"""
    for key, (waits, dist, rest, late) in rows.items():
        assert late == 0, (key, late)


def test_load_distance_at_least_twice_the_parents(rows):
    for key, (waits, dist, rest, late) in rows.items():
        assert dist >= 2 * PARENT_MIN_DISTANCE, (key, dist)
        assert rest >= 2 * PARENT_MIN_AFTER_FIRST, (key, rest)
