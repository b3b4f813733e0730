"""bin/otbench's chacha20 / poly1305 / chachapoly-enc / chachapoly-dec modes on
the CPU (bin/otbench_hostsim, as tests/test_otbench_gcm_cpu.py): output samples
and the tag are verified against the C oracle, in place and out of place; a
corrupted output byte in any sample, or a wrong tag alone, turns the verdict
false with exit code 3."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "otbench_hostsim")

CIPHER_MODES = ["chacha20", "chachapoly-enc", "chachapoly-dec"]  # the modes that write an output buffer
TAG_MODES = ["poly1305", "chachapoly-enc", "chachapoly-dec"]
N = 1000003  # no multiple of 64, 16 or 4: every mode takes any byte count


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


@pytest.mark.parametrize("mode", CIPHER_MODES)
@pytest.mark.parametrize("inplace", [False, True])
def test_cipher_modes_verify(mode, inplace):
    rc, d, err = run("--mode", mode, "--bytes", N, *(["--inplace"] if inplace else []), "--verify")
    assert rc == 0, err
    assert d["verified"] is True and d["inplace"] is inplace and d["mode"] == mode
    assert d["bytes"] == N  # not rounded down to whole blocks
    if mode in TAG_MODES:
        assert d["tag_ok"] is True and len(bytes.fromhex(d["tag"])) == 16


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096, N])
def test_poly1305_verifies(n):
    rc, d, err = run("--mode", "poly1305", "--bytes", n, "--verify")
    assert rc == 0, err
    assert d["verified"] is True and d["tag_ok"] is True and d["bytes"] == n
    assert len(bytes.fromhex(d["tag"])) == 16


@pytest.mark.parametrize("mode", CIPHER_MODES)
@pytest.mark.parametrize("where", ["head", "mid", "tail"])
def test_corrupted_sample_fails(mode, where):
    off = {"head": 5, "mid": N // 2 + 3, "tail": N - 2}[where]
    rc, d, err = run("--mode", mode, "--bytes", N, "--verify", "--corrupt-at", off)
    assert rc == 3, err
    assert d["verified"] is False
    assert "mismatch" in err


@pytest.mark.parametrize("off", [0, 15, 16 + 7])
def test_corrupted_poly1305_tag_fails(off):
    rc, d, err = run("--mode", "poly1305", "--bytes", N, "--verify", "--corrupt-at", off)
    assert rc == 3, err
    assert d["verified"] is False and d["tag_ok"] is False
    assert "tag mismatch" in err


def test_wrong_tag_alone_fails():
    """A ciphertext byte outside every sample (they are 64 KiB at the head, the
    middle and the tail): the samples match, the tag over the whole ciphertext does not."""
    rc, d, err = run("--mode", "chachapoly-enc", "--bytes", N, "--verify", "--corrupt-at", 200000)
    assert rc == 3, err
    assert d["verified"] is False and d["tag_ok"] is False
    assert "tag mismatch" in err and "at byte" not in err


def test_aad_is_honoured():
    tags = {}
    for aad in (0, 13, 4097):
        rc, d, err = run("--mode", "chachapoly-enc", "--bytes", 4111, "--verify", "--aad", aad)
        assert rc == 0 and d["verified"] is True and d["tag_ok"] is True, err
        assert d["aad"] == aad
        tags[aad] = d["tag"]
    assert len(set(tags.values())) == len(tags)


def test_argument_errors():
    rc, _, err = run("--mode", "poly1305", "--bytes", 4096, "--inplace")
    assert rc == 2 and "inplace" in err
    rc, _, err = run("--mode", "chacha21", "--bytes", 4096)
    assert rc == 2 and "unknown mode" in err
