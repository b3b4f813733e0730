"""csrc/cpu/gcm_mk_batch_selftest.c with csrc/cpu/aes.c as a stand-alone
executable, plain and under AddressSanitizer and UBSan: the host-callable
arithmetic of the many-key batched AES-GCM kernels (csrc/hip/polyval_dev.h: a
key's seven nibble tables from E_K(0), GHASH through RFC 8452 appendix A with
byte-reversed blocks, the lane decomposition of both forms with its fold)
agrees with the oracle's GHASH and GCM.  Nothing is loaded into Python, and the
program runs in the environment the test inherits."""
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
    exe = str(tmp_path_factory.mktemp("gcm_mk_batch") / f"gcm_mk_batch_selftest_{request.param}")
    subprocess.run([cc, "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "csrc", "include"),
                    *(SAN if request.param == "san" else []),
                    os.path.join(ROOT, "csrc", "cpu", "gcm_mk_batch_selftest.c"), os.path.join(ROOT, "csrc", "cpu", "aes.c"),
                    "-o", exe, "-lpthread"], check=True, cwd=ROOT)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_runs_clean(selftest):
    assert selftest.returncode == 0, selftest.stdout[-2000:] + selftest.stderr[-4000:]
    assert "ERROR" not in selftest.stderr and "runtime error" not in selftest.stderr, selftest.stderr[-4000:]
    assert "FAIL" not in selftest.stdout


def test_every_part_reports(selftest):
    lines = selftest.stdout.splitlines()
    # RFC 8452 appendix A: GHASH(H, X_1, X_2) through the POLYVAL tables
    assert "APPENDIX-A bd9b3997046731fb96251b91f9c99d7a" in lines
    # both lane forms x 12 hashed-block counts x 4 AAD lengths, less the 8 where the AAD alone has more blocks
    for bits in (128, 192, 256):
        assert f"OK AES-{bits} 88 records" in lines


def test_the_makefile_builds_it():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "bin/gcm_mk_batch_selftest:" in mk and "csrc/hip/aes_gcm_mk_batch.hip" in mk
    for target in ("all:", "cpu:"):
        line = next(ln for ln in mk.splitlines() if ln.startswith(target))
        assert "bin/gcm_mk_batch_selftest" in line
    assert "bin/gcm_mk_batch_selftest" in mk[mk.index("\nclean:"):]
