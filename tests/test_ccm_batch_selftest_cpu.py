"""csrc/cpu/ccm_batch_selftest.c: the batched CCM kernel's lane on the host, with
the kernel's own block formatting (csrc/hip/ccm_dev.h), against aes_crypt_ccm of
aes.c -- the program `make` builds, and the same source with csrc/cpu/aes.c as a
stand-alone executable under AddressSanitizer and UBSan.  Nothing is loaded
into Python, and the programs run in the environment the test inherits."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = 989  # 7 nonce x 7 tag lengths x 13 edge lengths + 301 lengths + 12 AAD lengths x 4 offsets + 3 large


def check(r):
    assert r.returncode == 0, r.stdout + r.stderr
    for bits in (128, 192, 256):
        assert f"OK AES-{bits} {RECORDS} records" in r.stdout
    assert "FAIL" not in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_the_built_program_passes():
    exe = os.path.join(ROOT, "bin", "ccm_batch_selftest")
    assert os.path.exists(exe), "bin/ccm_batch_selftest was not built (make)"
    check(subprocess.run([exe], capture_output=True, text=True, timeout=300))


def test_the_record_count_is_what_the_program_covers():
    assert RECORDS == 7 * 7 * 13 + 301 + 12 * 4 + 3


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "address-undefined"])
def test_ccm_batch_selftest(tmp_path, flags):
    """A program of its own with its own main: B0 and A_i from the nonce's words, the encoded AAD's
    blocks at every misalignment and either side of the encodings' switch, the pipelined decryption
    order, the counter's carry at block 256, the bursts' ring, the tail mask, the order array; every
    record in place between guard bytes."""
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("gcc not available")
    inc = ["-I", os.path.join(ROOT, "csrc/include"), "-I", os.path.join(ROOT, "csrc/hip")]
    exe = tmp_path / "ccm_batch_selftest"
    b = subprocess.run([cc, "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", *inc, *flags,
                        os.path.join(ROOT, "csrc/cpu/ccm_batch_selftest.c"), os.path.join(ROOT, "csrc/cpu/aes.c"),
                        "-o", str(exe), "-lpthread"], capture_output=True, text=True)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr
    check(subprocess.run([str(exe)], capture_output=True, text=True, timeout=300))
