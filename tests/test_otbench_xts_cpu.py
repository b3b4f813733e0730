"""bin/otbench's xts-enc / xts-dec modes on the CPU (bin/otbench_hostsim, as
tests/test_otbench_cpu.py): both verify against the C oracle in place and out
of place, and a corrupted output byte in any sample turns the verdict false
with exit code 3."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "otbench_hostsim")

MODES = ["xts-enc", "xts-dec"]


@pytest.fixture(scope="module", autouse=True)
def built():
    # one make at a time (pytest-xdist workers each run this fixture; two
    # concurrent links of the same binary race) -- the lock of test_otbench_cpu.py
    import fcntl

    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".hostsim.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", ROOT, "-s", "bin/otbench_hostsim"], check=True, capture_output=True)


def run(*args):
    p = subprocess.run([BIN, "--iters", "1", "--warmup", "1", *map(str, args)], capture_output=True, text=True,
                       timeout=300)
    line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else "{}"
    return p.returncode, json.loads(line), p.stderr


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("bits", [128, 256])
def test_xts_modes_verify(mode, inplace, bits):
    rc, d, err = run("--mode", mode, "--bits", bits, "--bytes", 1000000, *(["--inplace"] if inplace else []), "--verify")
    assert rc == 0, err
    assert d["verified"] is True and d["inplace"] is inplace and d["mode"] == mode
    assert d["bytes"] == 1000000 // 4096 * 4096  # whole default units


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", ["head", "mid", "tail"])
def test_corrupted_sample_fails(mode, where):
    n = 1000000 // 4096 * 4096
    off = {"head": 5, "mid": n // 2 + 3, "tail": n - 2}[where]
    rc, d, err = run("--mode", mode, "--bytes", 1000000, "--verify", "--corrupt-at", off)
    assert rc == 3, err
    assert d["verified"] is False
    assert "mismatch" in err


def test_unit_option():
    rc, d, err = run("--mode", "xts-enc", "--bytes", 1000000, "--unit", 512, "--verify")
    assert rc == 0 and d["verified"] is True and d["bytes"] == 1000000 // 512 * 512, err
    rc, _, err = run("--mode", "xts-enc", "--bytes", 1000000, "--unit", 24)
    assert rc == 2 and "multiple of 16" in err
    rc, _, err = run("--mode", "xts-dec", "--bits", 192, "--bytes", 1000000)
    assert rc == 2 and "128 or 256" in err
