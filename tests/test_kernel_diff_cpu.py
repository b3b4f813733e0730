"""tools/kernel_diff.py, the per-kernel device-code comparison a refactor of
the kernel files is checked with (no GPU needed): run on the built T-table
object against itself it finds every kernel and calls each one the same."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "build", "obj", "hip", "aes_tt.o")
TOOL = os.path.join(ROOT, "tools", "kernel_diff.py")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_count import LLVM  # noqa: E402  (where the ROCm LLVM tools live)


@pytest.fixture(scope="module")
def self_diff():
    if not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"):
        pytest.skip("no built aes_tt.o (make) or no ROCm LLVM tools")
    return subprocess.run([sys.executable, TOOL, OBJ, OBJ], capture_output=True, text=True)


def test_object_against_itself_is_all_same(self_diff):
    assert self_diff.returncode == 0, self_diff.stderr
    rows = [l.split() for l in self_diff.stdout.splitlines() if l.startswith(("same ", "differs ", "only-"))]
    assert len(rows) == 116, len(rows)
    assert all(r[0] == "same" for r in rows), [r for r in rows if r[0] != "same"][:3]
    assert "116 kernels in both, 116 same, 0 differ, 0 only in OLD, 0 only in NEW" in self_diff.stdout


def test_rows_carry_counts_and_resources(self_diff):
    """every row: both instruction counts (a kernel is hundreds of
    instructions) and both (vgpr, sgpr, scratch, allocated VGPRs, static LDS)
    tuples, read from the notes and the kernel descriptor"""
    pat = re.compile(r"^same (\d+) (\d+) \((\d+), (\d+), (\d+), (\d+), (\d+)\) \((\d+), (\d+), (\d+), (\d+), (\d+)\) \S+$")
    seen_lds = set()
    for line in self_diff.stdout.splitlines()[:-1]:
        m = pat.match(line)
        assert m, line
        n_old, n_new, vg, sg, scratch, alloc, lds = (int(x) for x in m.groups()[:7])
        assert n_old == n_new > 0 and 0 < vg <= alloc <= 512 and alloc % 8 == 0 and sg > 0, line
        assert m.groups()[2:7] == m.groups()[7:12], line
        seen_lds.add(lds)
    # the grid kernels' static tables (128 / 160 KiB) and the claim kernels' dynamic ones (0)
    assert {0, 128 << 10, 160 << 10} <= seen_lds, seen_lds
