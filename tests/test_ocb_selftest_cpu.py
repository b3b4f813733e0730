"""csrc/cpu/ocb_selftest.c with csrc/cpu/aes.c as a stand-alone executable under
AddressSanitizer and UBSan: the OCB3 oracle's vectors, iterated check, tamper
checks and chained pieces run clean, and print the RFC's results.  Nothing is
loaded into Python, and the program runs in the environment the test inherits."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ocb_vectors.json")) as f:
    VEC = json.load(f)["ocb"]

ITERATED = """ITER 128 128 67E944D23256C5E0B6C61FA22FDF1EA2
ITER 128 96 77A3D8E73589158D25D01209
ITER 128 64 192C9B7BD90BA06A
ITER 192 128 F673F2C3E7174AAE7BAE986CA9F29E17
ITER 192 96 05D56EAD2752C86BE6932C5E
ITER 192 64 0066BC6E0EF34E24
ITER 256 128 D90EB8E9C977C88B79DD793D7FFA161C
ITER 256 96 5458359AC23B0CBA9E6330DD
ITER 256 64 7D4EA5D445501CBE""".splitlines()


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path_factory.mktemp("ocb") / "ocb_selftest_san")
    subprocess.run([cc, "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "csrc", "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "csrc", "cpu", "ocb_selftest.c"), os.path.join(ROOT, "csrc", "cpu", "aes.c"),
                    "-o", exe, "-lpthread"], check=True, cwd=ROOT)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_runs_clean_under_the_sanitizers(selftest):
    assert selftest.returncode == 0, selftest.stdout[-2000:] + selftest.stderr[-4000:]
    assert "ERROR" not in selftest.stderr and "runtime error" not in selftest.stderr, selftest.stderr[-4000:]
    assert "FAIL" not in selftest.stdout
    assert "TAMPER ok" in selftest.stdout.splitlines()


def test_prints_the_anchors_and_the_iterated_results(selftest):
    lines = selftest.stdout.splitlines()
    assert "V 128 BBAA99887766554433221100 0 0 16 - 785407BFFFC8AD9EDCC5520AC9111EE6" in lines
    assert "V 128 BBAA99887766554433221101 8 8 16 6820B3657B6F615A 5725BDA0D3B4EB3A257C9AF1F8F03009" in lines
    assert [ln for ln in lines if ln.startswith("ITER")] == ITERATED


def test_prints_every_golden_vector(selftest):
    """The program builds the golden file's inputs itself; its outputs are libcrypto's."""
    want = [f"V {len(v['key']) * 4} {v['nonce'].upper()} {len(v['aad']) // 2} {len(v['pt']) // 2} {v['tag_bytes']} "
            f"{v['ct'].upper() or '-'} {v['tag'].upper()}" for v in VEC]
    assert [ln for ln in selftest.stdout.splitlines() if ln.startswith("V ")] == want
