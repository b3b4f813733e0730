"""Batched ChaCha20-Poly1305 without a GPU: the host planner
(otc_chacha_batch_plan), what the kernels report about themselves, the argument
checks of otc_poly1305_batch / otc_chacha20_poly1305_batch -- which must answer
OTC_ERR_ARG with a message *before* any HIP call: the device addresses below
are fake and never dereferenced --, the Python layer's checks, and the host
program that runs the batched Poly1305 kernel's decomposition with the
kernel's own arithmetic (csrc/cpu/poly_batch_selftest.cpp), plain and under
AddressSanitizer + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models.chacha import ChaCha20Poly1305

ERR_ARG = -1
ENC, DEC = 1, 0
A = 0x7F0000000000  # fake, 16-byte aligned device addresses (never touched)
MAX_BYTES, MAX_AAD = 1 << 20, 1 << 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not _native.gpu_lib_available():
        pytest.skip("libotc.so not built")
    return _native.require_gpu_lib()


def err(lib) -> str:
    return lib.otc_last_error().decode()


def descs(rows):
    """rows of (in, out, nbytes, aad, aad_bytes[, key]) -> otc_chacha_msg[] as uint64 [n, 6]"""
    d = np.zeros((len(rows), 6), dtype=np.uint64)
    for i, r in enumerate(rows):
        d[i, :len(r)] = r
    return d


def plan(lib, d, nkeys=1, fill=True):
    n = d.shape[0]
    nt = lib.otc_chacha_batch_plan(d.ctypes.data, n, nkeys, None, None)
    if nt < 0 or not fill:
        return nt, None, None
    first = np.full(n, 0xEE, dtype=np.uint64)
    tmap = np.zeros(max(nt, 1), dtype=np.uint32)
    assert lib.otc_chacha_batch_plan(d.ctypes.data, n, nkeys, tmap.ctypes.data, first.ctypes.data) == nt
    return nt, tmap[:nt], first


# ---- the planner ----------------------------------------------------------------
@pytest.mark.parametrize("n,tiles", [(0, 0), (1, 1), (4095, 1), (4096, 1), (4097, 2), (MAX_BYTES, 256)])
def test_planner_tile_counts(lib, n, tiles):
    assert plan(lib, descs([(A, A, n, 0, 0)]), fill=False)[0] == tiles


def test_planner_tile_map_of_a_mixed_batch(lib):
    lens = [0, 1, 4096, 0, 4097, 0, 0, 12289, 64]
    rows, at = [], A
    for i, n in enumerate(lens):
        rows.append((at, at if i % 2 else at + (8 << 20), n, A + (32 << 20) + 3 + 64 * i, (i * 7) % 40, i % 3))
        at += (n + 15) // 16 * 16
    nt, tmap, first = plan(lib, descs(rows), nkeys=3)
    tiles = [(n + 4095) // 4096 for n in lens]
    assert tiles == [0, 1, 1, 0, 2, 0, 0, 4, 1] and nt == sum(tiles)
    assert first.tolist() == np.cumsum([0] + tiles[:-1]).tolist()
    assert tmap.tolist() == [m for m, t in enumerate(tiles) for _ in range(t)]
    for m, n in enumerate(lens):
        if n == 0:
            assert m not in tmap  # empty records have no tiles


def test_planner_counts_without_output_arrays(lib):
    d = descs([(A, A, 4097, 0, 0), (A + 8192, A + 8192, 0, 0, 0)])
    assert plan(lib, d, fill=False)[0] == 2
    assert lib.otc_chacha_batch_plan(None, 0, 1, None, None) == 0
    # either array alone
    first = np.zeros(2, dtype=np.uint64)
    tmap = np.zeros(2, dtype=np.uint32)
    assert lib.otc_chacha_batch_plan(d.ctypes.data, 2, 1, None, first.ctypes.data) == 2 and first.tolist() == [0, 2]
    assert lib.otc_chacha_batch_plan(d.ctypes.data, 2, 1, tmap.ctypes.data, None) == 2 and tmap.tolist() == [0, 0]
    assert lib.otc_chacha_batch_plan(None, 3, 1, None, None) == ERR_ARG and "null descriptors" in err(lib)


@pytest.mark.parametrize("row,what", [
    ((A, A, MAX_BYTES + 1, 0, 0), "1 MiB"),
    ((A, A, 16, A + 4096, MAX_AAD + 1), "64 KiB"),
    ((A, A, 0, 0, 5), "null aad"),
    ((0, A, 64, 0, 0), "null buffer"),
    ((A, 0, 64, 0, 0), "null buffer"),
    ((A + 4, A + 4096, 64, 0, 0), "aligned"),
    ((A, A + 4096 + 8, 64, 0, 0), "aligned"),
    ((A, A, 64, 0, 0, 2), "key index"),
    ((A, A, 0, 0, 0, 2), "key index"),            # an empty record has a key too
    ((A, A + 16, 64, 0, 0), "overlap partially"),
    ((A + 32, A, 64, 0, 0), "overlap partially"),
])
def test_planner_rejects_a_bad_record(lib, row, what):
    good = (A + (1 << 24), A + (1 << 24), 100, 0, 0, 1)
    nt = plan(lib, descs([good, row]), nkeys=2)[0]
    assert nt == ERR_ARG and what in err(lib) and "chacha_batch: record 1: " in err(lib), err(lib)


def test_planner_accepts_the_caps(lib):
    d = descs([(A, A, MAX_BYTES, A + (4 << 20) + 1, MAX_AAD, 6)])
    assert plan(lib, d, nkeys=7, fill=False)[0] == 256


def test_planner_rejects_records_that_overlap(lib):
    B = A + (1 << 24)
    # two outputs share bytes
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 96, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "output overlaps another record" in err(lib)
    # record 1 reads what record 0 writes
    assert plan(lib, descs([(A, B, 100, 0, 0), (B + 64, B + 4096, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "input overlaps another record's output" in err(lib)
    # an AAD inside an output -- its own record's or another's -- would be overwritten before it is hashed
    assert plan(lib, descs([(A, B, 100, B + 50, 13)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, A, 100, A + 99, 1)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 4096, 100, B - 3, 4)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "AAD overlaps" in err(lib)
    # next to an output, or inside an out-of-place record's input, it is fine; so are empty records anywhere
    assert plan(lib, descs([(A, B, 100, B + 100, 13), (A + 4096, B + 4096, 100, B - 4, 4),
                            (A + 8192, B + 8192, 64, A + 8192, 64), (A, B, 0, 0, 0)]), fill=False)[0] == 3


# ---- what the kernels report about themselves -----------------------------------
def test_ws_bytes(lib):
    assert lib.otc_chacha_batch_ws_bytes(0) == 0 and lib.otc_chacha_batch_ws_bytes(1000) == 32 * 1000


def test_spans_are_positive_and_increasing(lib):
    buf = (ctypes.c_uint64 * 16)()
    n = lib.otc_chacha_batch_spans(buf, 16)
    spans = [int(v) for v in buf[:n]]
    assert 16 in spans and 64 in spans
    assert all(s > 0 for s in spans) and all(a < b for a, b in zip(spans, spans[1:]))
    assert lib.otc_chacha_batch_spans(None, 0) == n
    one = (ctypes.c_uint64 * 2)(0, 0xDEAD)
    assert lib.otc_chacha_batch_spans(one, 1) == n and one[0] == spans[0] and one[1] == 0xDEAD  # max is honoured
    assert ops.chacha_batch_ops.chacha_batch_spans() == spans


def test_lanes_follow_the_record_sizes(lib):
    """64 lanes per record when the records hash more than 512 blocks on average
    (AAD blocks + data blocks + the length block), else 16: the measured sizes on
    both sides of the rule, and its edge."""
    lanes = lambda rows: lib.otc_chacha_batch_lanes(descs(rows).ctypes.data, len(rows))
    for size in (256, 1024, 4096):      # measured: 16 lanes win
        assert lanes([(A, A, size, A, 13)] * 4) == 16
    for size in (16384, 65536):         # measured: 64 lanes win
        assert lanes([(A, A, size, A, 13)] * 4) == 64
    assert lanes([(A, A, 16 * 511, 0, 0)]) == 16          # 512 blocks with the length block
    assert lanes([(A, A, 16 * 511 + 1, 0, 0)]) == 64      # 513
    assert lanes([(A, A, 16 * 510, A, 1)]) == 16          # the AAD block counts: 512
    assert lanes([(A, A, 16 * 510 + 1, A, 16)]) == 64
    assert lanes([(A, A, 16384, 0, 0), (A, A, 0, 0, 0), (A, A, 0, A, 13)]) == 16   # the mean, not the longest
    assert lanes([(A, A, 64, 0, 0)] * 50 + [(A, A, 1 << 20, 0, 0)]) == 64          # mean 1291
    assert lanes([(A, A, 64, 0, 0)] * 200 + [(A, A, 1 << 20, 0, 0)]) == 16         # mean 331
    assert lib.otc_chacha_batch_lanes(None, 0) == 16


# ---- the run entry points -------------------------------------------------------
def aead_batch(lib, **kw):
    a = dict(msgs=A, tmap=A + 0x2000, first=A + 0x3000, ntiles=4, nmsg=4, keys=A + 0x4000, dir=ENC, nonces=A + 0x5000,
             tags=A + 0x6000, expect=None, ok=None, ws=A + 0x7000, lanes=16)
    a.update(kw)
    return lib.otc_chacha20_poly1305_batch(a["msgs"], a["tmap"], a["first"], a["ntiles"], a["nmsg"], a["keys"], a["dir"],
                                           a["nonces"], a["tags"], a["expect"], a["ok"], a["ws"], a["lanes"], None)


@pytest.mark.parametrize("kw,what", [
    (dict(msgs=None), "null"),
    (dict(tmap=None), "null tile map"),
    (dict(first=None), "null tile map"),
    (dict(keys=None), "null"),
    (dict(nonces=None), "null nonces"),
    (dict(tags=None), "null"),
    (dict(ws=None), "null"),
    (dict(msgs=A + 4), "misaligned"),
    (dict(first=A + 0x3004), "misaligned"),
    (dict(tmap=A + 0x2002), "misaligned"),
    (dict(keys=A + 0x4002), "misaligned"),
    (dict(tags=A + 0x6004), "16-byte aligned"),
    (dict(ws=A + 0x7008), "16-byte aligned"),
    (dict(dir=2), "direction"),
    (dict(dir=-1), "direction"),
    (dict(lanes=32), "lanes"),
    (dict(lanes=-1), "lanes"),
    (dict(dir=DEC), "decryption needs"),
    (dict(dir=DEC, expect=A + 0x8000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000), "expected tags overlap"),        # the tag array itself
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 + 63), "expected tags overlap"),   # its last byte
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 - 63), "expected tags overlap"),   # its first
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 - 63), "expected tags overlap"),   # the verdicts
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 + 3), "expected tags overlap"),
])
def test_aead_batch_rejects_bad_arguments(lib, kw, what):
    assert aead_batch(lib, **kw) == ERR_ARG and what in err(lib), err(lib)


def test_aead_batch_accepts_expected_tags_next_to_its_own(lib):
    """Adjacent is not overlapping: the checks above do not fire, and the next one in line does."""
    for exp in (A + 0x6000 + 64, A + 0x6000 - 64, A + 0x9000 + 4):
        assert aead_batch(lib, dir=DEC, ok=A + 0x9000, expect=exp, nonces=None) == ERR_ARG
        assert "null nonces" in err(lib)


def test_all_empty_records_need_no_tile_map(lib):
    """ntiles == 0 skips the cipher: the missing map is not an error; the next check in line fires."""
    assert aead_batch(lib, ntiles=0, tmap=None, first=None, nonces=None) == ERR_ARG and "null nonces" in err(lib)


@pytest.mark.parametrize("args,what", [
    ((None, 4, A + 0x4000, A + 0x6000, 16), "null"),
    ((A, 4, None, A + 0x6000, 16), "null"),
    ((A, 4, A + 0x4000, None, 16), "null"),
    ((A + 4, 4, A + 0x4000, A + 0x6000, 16), "misaligned"),
    ((A, 4, A + 0x4002, A + 0x6000, 64), "misaligned"),
    ((A, 4, A + 0x4000, A + 0x6008, 64), "16-byte aligned"),
    ((A, 4, A + 0x4000, A + 0x6000, 17), "lanes"),
])
def test_poly1305_batch_rejects_bad_arguments(lib, args, what):
    assert lib.otc_poly1305_batch(*args, None) == ERR_ARG and what in err(lib), err(lib)


def test_an_empty_batch_launches_nothing(lib):
    assert aead_batch(lib, nmsg=0, ntiles=0, msgs=None, tmap=None, first=None, keys=None, nonces=None, tags=None,
                      ws=None) == 0
    assert aead_batch(lib, nmsg=0, ntiles=0, dir=DEC) == 0
    assert aead_batch(lib, nmsg=0, dir=7) == ERR_ARG  # the direction is checked even then
    assert lib.otc_poly1305_batch(None, 0, None, None, 0, None) == 0


# ---- the Python layer -----------------------------------------------------------
CB = ops.chacha_batch_ops


def test_the_module_is_reachable_but_not_exported():
    assert ops.chacha_batch_ops.ChaChaBatch is CB.ChaChaBatch
    for name in ("ChaChaBatch", "chacha20_poly1305_encrypt_batch", "chacha20_poly1305_decrypt_batch", "poly1305_batch",
                 "chacha_batch_spans"):
        assert hasattr(CB, name) and name not in ops.__all__
    assert hasattr(ChaCha20Poly1305, "encrypt_batch") and hasattr(ChaCha20Poly1305, "decrypt_batch")


@pytest.mark.parametrize("keys", [bytes(31), bytes(33), [bytes(32), bytes(16)], []])
def test_a_key_has_32_bytes(keys):
    with pytest.raises(ValueError):
        CB.ChaChaBatch([], keys)
    with pytest.raises(ValueError):
        ChaCha20Poly1305(bytes(16))


def test_lanes_are_16_or_64():
    with pytest.raises(ValueError, match="lanes"):
        CB.ChaChaBatch([], bytes(32), lanes=32)


def test_an_empty_batch_needs_no_device():
    b = CB.ChaChaBatch([], [bytes(32), bytes(32)], key_index=[])
    n0, t0 = torch.zeros((0, 12), dtype=torch.uint8), torch.zeros((0, 16), dtype=torch.uint8)
    outs, tags = b.encrypt(n0)
    assert outs == [] and tuple(tags.shape) == (0, 16) and tags.dtype == torch.uint8
    outs, ok = b.decrypt(n0, t0)
    assert outs == [] and tuple(ok.shape) == (0,) and ok.dtype == torch.bool
    assert tuple(b.poly1305([]).shape) == (0, 16)
    assert CB.chacha20_poly1305_encrypt_batch([], bytes(32), n0)[0] == []
    assert ChaCha20Poly1305(bytes(32)).decrypt_batch([], n0, t0)[0] == []
    # the shapes are checked even then
    for bad in (torch.zeros((0, 8), dtype=torch.uint8), torch.zeros((0, 12), dtype=torch.int32),
                torch.zeros((1, 12), dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8), b"", None):
        with pytest.raises(ValueError, match="nonce"):
            b.encrypt(bad)
    for bad in (torch.zeros((0, 15), dtype=torch.uint8), torch.zeros((0, 16), dtype=torch.int8),
                torch.zeros((2, 16), dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="tags"):
            b.decrypt(n0, bad)
    with pytest.raises(ValueError, match="one-time key"):
        b.poly1305([bytes(32)])


def planned(n=2):
    """A batch of n records as the constructor leaves it, without a device: what the run methods check first."""
    b = CB.ChaChaBatch.__new__(CB.ChaChaBatch)
    b._init_common(bytes(32), 16)
    b.n, b.device, b.outs = n, torch.device("cuda:0"), []
    b.tags, b.ok = torch.zeros((n, 16), dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
    return b


def test_nonces_and_tags_must_be_on_the_device():
    b = planned()
    with pytest.raises(ValueError, match="nonces must be a GPU tensor"):
        b.encrypt(torch.zeros((2, 12), dtype=torch.uint8))
    with pytest.raises(ValueError, match="nonces must be a GPU tensor"):
        b.decrypt(torch.zeros((2, 12), dtype=torch.uint8), torch.zeros((2, 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="nonces must be a GPU tensor"):
        b.encrypt([bytes(12)] * 2)


def test_decrypt_refuses_the_batchs_own_tensors():
    b = planned()
    for own in (b.tags, b.tags[1:], b.ok.view(1, 2)):
        with pytest.raises(ValueError, match="own tags"):
            b.decrypt(torch.zeros((2, 12), dtype=torch.uint8), own)


def test_the_new_functions_are_declared():
    src = open(os.path.join(ROOT, "our_tree_amd", "_native.py")).read()
    declared = set(re.findall(r'"(otc_\w+)": \(', src))
    assert {"otc_chacha_batch_plan", "otc_chacha_batch_ws_bytes", "otc_chacha_batch_lanes", "otc_chacha_batch_spans",
            "otc_poly1305_batch", "otc_chacha20_poly1305_batch"} <= declared
    # pointers as pointers, sizes as 64-bit: the planner's result is an int64 (a tile count or an error)
    assert re.search(r'"otc_chacha_batch_plan": \(ctypes\.c_int64, \[c_vp, c_sz, c_sz, c_vp, c_vp\]\)', src)
    assert re.search(r'"otc_chacha20_poly1305_batch": \(c_int, \[c_vp, c_vp, c_vp, c_u64, c_sz, c_vp, c_int, c_vp, c_vp, '
                     r'c_vp, c_vp,\s+c_vp, c_int, c_vp\]\)', src)
    assert ctypes.sizeof(_native.c_sz) == 8


# ---- the kernel's decomposition on the host ---------------------------------------
SELFTEST = ["csrc/cpu/poly_batch_selftest.cpp"]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "address-undefined"])
def test_poly_batch_selftest(tmp_path, flags):
    """A program of its own with its own main: prefix powers, Horner under r^L with a carry per
    batch, fold, final reduction, for L = 16 and 64, 1 .. 300 and 4096 .. 4100 blocks, random and
    worst-case inputs, against poly1305_mac of chacha.c."""
    cxx, cc = shutil.which("g++"), shutil.which("gcc")
    if cxx is None or cc is None:
        pytest.skip("g++ / gcc not available")
    inc = ["-I", os.path.join(ROOT, "csrc/include"), "-I", os.path.join(ROOT, "csrc/hip")]
    obj, exe = tmp_path / "chacha.o", tmp_path / "poly_batch_selftest"
    b = subprocess.run([cc, "-O1", "-g", "-std=gnu99", *inc, *flags, "-c", os.path.join(ROOT, "csrc/cpu/chacha.c"), "-o",
                        str(obj)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *inc, *flags,
                        os.path.join(ROOT, SELFTEST[0]), str(obj), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poly_batch_selftest: OK" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
