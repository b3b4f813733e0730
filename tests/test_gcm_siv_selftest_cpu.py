"""csrc/cpu/gcmsiv_selftest.c with csrc/cpu/aes.c as a stand-alone executable,
plain and under AddressSanitizer and UBSan: the GCM-SIV oracle's vectors, the
counter's wrap, the tamper checks and the POLYVAL kernels' decomposition (with
the device's own field arithmetic, csrc/hip/polyval_dev.h) run clean and print
RFC 8452's results.  Nothing is loaded into Python, and the program runs in the
environment the test inherits."""
import os
import shutil
import subprocess

import pytest

from test_gcm_siv_cpu import SEALED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=["plain", "san"])
def selftest(request, tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path_factory.mktemp("gcmsiv") / f"gcmsiv_selftest_{request.param}")
    subprocess.run([cc, "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "csrc", "include"),
                    *(SAN if request.param == "san" else []),
                    os.path.join(ROOT, "csrc", "cpu", "gcmsiv_selftest.c"), os.path.join(ROOT, "csrc", "cpu", "aes.c"),
                    "-o", exe, "-lpthread"], check=True, cwd=ROOT)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_runs_clean(selftest):
    assert selftest.returncode == 0, selftest.stdout[-2000:] + selftest.stderr[-4000:]
    assert "ERROR" not in selftest.stderr and "runtime error" not in selftest.stderr, selftest.stderr[-4000:]
    assert "FAIL" not in selftest.stdout
    lines = selftest.stdout.splitlines()
    assert "WRAP ok" in lines and "TAMPER ok" in lines and "DECOMP ok" in lines


def test_prints_the_rfc_results(selftest):
    lines = selftest.stdout.splitlines()
    assert "POLYVAL f7a3b47b846119fae5b7866cf5e5b77e" in lines
    assert "DERIVE 310728d9911f1f3837b24316c3fab9a0 a4c5ae6249963279c100be4d7e2c6edd" in lines
    want = [f"V {len(key) * 8} {len(aad)} {len(pt)} {sealed}" for key, _, aad, pt, sealed in SEALED]
    assert [ln for ln in lines if ln.startswith("V ")] == want
