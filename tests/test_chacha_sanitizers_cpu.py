"""Host sanitizers over the ChaCha20 / Poly1305 / AEAD oracle (csrc/cpu/chacha.c):
csrc/cli/san_driver.c built stand-alone with -DOTC_SAN_CHACHA and chacha.c, as
``make san-check`` builds it, with ThreadSanitizer and with AddressSanitizer +
UBSan; it must run clean.  (tests/test_sanitizers_cpu.py builds the same driver
without the macro: the AES / ARC4 part alone.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = ["csrc/cpu/aes.c", "csrc/cpu/arc4.c", "csrc/cpu/chacha.c", "csrc/cli/san_driver.c"]


@pytest.mark.parametrize("flags,env", [
    (["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1"}),
    (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], {"ASAN_OPTIONS": "detect_leaks=1"}),
], ids=["thread", "address-undefined"])
def test_san_driver_with_chacha(tmp_path, flags, env):
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "san_driver"
    cmd = [cc, "-O1", "-g", "-std=gnu99", "-DOTC_SAN_CHACHA", "-I", os.path.join(ROOT, "csrc/include"), *flags,
           *[os.path.join(ROOT, s) for s in SRCS], "-o", str(exe), "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "san_driver: OK" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
