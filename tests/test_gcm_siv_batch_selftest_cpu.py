"""csrc/cpu/gcmsiv_batch_selftest.c with csrc/cpu/aes.c as a stand-alone
executable, plain and under AddressSanitizer and UBSan: the host-callable
arithmetic of the batched AES-GCM-SIV kernels (csrc/hip/polyval_dev.h: the
nibble-table product, the lane decomposition of both forms with its fold, the
derivation, the key expansion, the little-endian counter) agrees with the
oracle over RFC 8452's vectors and the lengths of the GPU tests.  Nothing is
loaded into Python, and the program runs in the environment the test inherits."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=["plain", "san"])
def selftest(request, tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path_factory.mktemp("gcmsiv_batch") / f"gcmsiv_batch_selftest_{request.param}")
    subprocess.run([cc, "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "csrc", "include"),
                    *(SAN if request.param == "san" else []),
                    os.path.join(ROOT, "csrc", "cpu", "gcmsiv_batch_selftest.c"), os.path.join(ROOT, "csrc", "cpu", "aes.c"),
                    "-o", exe, "-lpthread"], check=True, cwd=ROOT)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_runs_clean(selftest):
    assert selftest.returncode == 0, selftest.stdout[-2000:] + selftest.stderr[-4000:]
    assert "ERROR" not in selftest.stderr and "runtime error" not in selftest.stderr, selftest.stderr[-4000:]
    assert "FAIL" not in selftest.stdout


def test_every_part_reports(selftest):
    lines = selftest.stdout.splitlines()
    assert any(ln.startswith("MUL ok ") for ln in lines)
    assert "EXPAND ok" in lines and "WRAP ok" in lines
    # both lane forms over the vectors' shapes and 25 lengths x 4 AAD lengths, per key size
    assert "OK AES-128 220 records" in lines and "OK AES-256 220 records" in lines


def test_the_makefile_builds_it():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "bin/gcmsiv_batch_selftest:" in mk and "csrc/hip/aes_gcm_siv_batch.hip" in mk
    for target in ("all:", "cpu:"):
        line = next(ln for ln in mk.splitlines() if ln.startswith(target))
        assert "bin/gcmsiv_batch_selftest" in line
    assert "bin/gcmsiv_batch_selftest" in mk[mk.index("\nclean:"):]
