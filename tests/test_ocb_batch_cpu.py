"""Batched AES-OCB3 without a GPU: the host planner (otc_ocb_batch_plan), what
the kernels report about themselves, the argument checks of otc_aes_ocb_batch
-- which must answer OTC_ERR_ARG with a message *before* any HIP call: the
device addresses below are fake and never dereferenced --, the Python layer's
checks, the batch oracle, and the host program that runs the batched kernels'
decomposition with the kernels' own closed forms (csrc/cpu/ocb_batch_selftest.c
over csrc/hip/ocb_dev.h), plain and under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref
from our_tree_amd.models.aes import AES

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


@pytest.fixture(scope="module")
def key(lib):
    k = _native.OtcOcbKey()
    assert lib.otc_ocb_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(16))), 128) == 0
    return k


def err(lib) -> str:
    return lib.otc_last_error().decode()


def descs(rows):
    """rows of (in, out, nbytes, aad, aad_bytes) -> otc_ocb_msg[] as uint64 [n, 6]"""
    d = np.zeros((len(rows), 6), dtype=np.uint64)
    for i, r in enumerate(rows):
        d[i, :len(r)] = r
    return d


def plan(lib, d, fill=True):
    n = d.shape[0]
    nt = lib.otc_ocb_batch_plan(d.ctypes.data, n, None, None)
    if nt < 0 or not fill:
        return nt, None, None
    first = np.full(n, 0xEE, dtype=np.uint64)
    tmap = np.zeros(max(nt, 1), dtype=np.uint32)
    assert lib.otc_ocb_batch_plan(d.ctypes.data, n, tmap.ctypes.data, first.ctypes.data) == nt
    return nt, tmap[:nt], first


def tiles_of(n):
    return (n // 16 + 63) // 64


# ---- the planner ----------------------------------------------------------------
@pytest.mark.parametrize("n,tiles", [(0, 0), (15, 0), (16, 1), (1024, 1), (1039, 1), (1040, 2), (MAX_BYTES, 1024)])
def test_planner_tile_counts(lib, n, tiles):
    """A tile is 64 WHOLE blocks: the trailing bytes are the finisher's and have no tile."""
    assert plan(lib, descs([(A, A, n, 0, 0)]), fill=False)[0] == tiles == tiles_of(n)


def test_planner_tile_map_of_a_mixed_batch(lib):
    lens = [0, 1, 1024, 15, 1040, 0, 16, 4097, 64]
    rows, at = [], A
    for i, n in enumerate(lens):
        rows.append((at, at if i % 2 else at + (8 << 20), n, A + (32 << 20) + 3 + 64 * i, (i * 7) % 40))
        at += (n + 15) // 16 * 16
    nt, tmap, first = plan(lib, descs(rows))
    tiles = [tiles_of(n) for n in lens]
    assert tiles == [0, 0, 1, 0, 2, 0, 1, 4, 1] and nt == sum(tiles)
    assert first.tolist() == np.cumsum([0] + tiles[:-1]).tolist()
    assert tmap.tolist() == [m for m, t in enumerate(tiles) for _ in range(t)]
    for m, n in enumerate(lens):
        if n < 16:
            assert m not in tmap  # records without a whole block have no tiles


def test_planner_counts_without_output_arrays(lib):
    d = descs([(A, A, 1040, 0, 0), (A + 8192, A + 8192, 0, 0, 0)])
    assert plan(lib, d, fill=False)[0] == 2
    assert lib.otc_ocb_batch_plan(None, 0, None, None) == 0
    # either array alone
    first = np.zeros(2, dtype=np.uint64)
    tmap = np.zeros(2, dtype=np.uint32)
    assert lib.otc_ocb_batch_plan(d.ctypes.data, 2, None, first.ctypes.data) == 2 and first.tolist() == [0, 2]
    assert lib.otc_ocb_batch_plan(d.ctypes.data, 2, tmap.ctypes.data, None) == 2 and tmap.tolist() == [0, 0]
    assert lib.otc_ocb_batch_plan(None, 3, None, None) == ERR_ARG and "null descriptors" in err(lib)


@pytest.mark.parametrize("row,what", [
    ((A, A, MAX_BYTES + 1, 0, 0), "1 MiB"),
    ((A, A, 16, A + 4096, MAX_AAD + 1), "64 KiB"),
    ((A, A, 0, 0, 5), "null aad"),
    ((0, A, 64, 0, 0), "null buffer"),
    ((A, 0, 64, 0, 0), "null buffer"),
    ((0, A, 5, 0, 0), "null buffer"),             # no whole block, but trailing bytes
    ((A + 4, A + 4096, 64, 0, 0), "aligned"),
    ((A, A + 4096 + 8, 64, 0, 0), "aligned"),
    ((A, A + 16, 64, 0, 0), "overlap partially"),
    ((A + 32, A, 64, 0, 0), "overlap partially"),
])
def test_planner_rejects_a_bad_record(lib, row, what):
    good = (A + (1 << 24), A + (1 << 24), 100, 0, 0)
    nt = plan(lib, descs([good, row]))[0]
    assert nt == ERR_ARG and what in err(lib) and "ocb_batch: record 1: " in err(lib), err(lib)


def test_planner_accepts_the_caps(lib):
    d = descs([(A, A, MAX_BYTES, A + (4 << 20) + 1, MAX_AAD)])
    assert plan(lib, d, fill=False)[0] == 1024


def test_planner_rejects_records_that_overlap(lib):
    B = A + (1 << 24)
    # two outputs share bytes
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 96, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "output overlaps another record" in err(lib)
    # record 1 reads what record 0 writes
    assert plan(lib, descs([(A, B, 100, 0, 0), (B + 64, B + 4096, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "input overlaps another record's output" in err(lib)
    # an AAD inside an output -- its own record's or another's
    assert plan(lib, descs([(A, B, 100, B + 50, 13)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, A, 100, A + 99, 1)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 4096, 100, B - 3, 4)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "AAD overlaps" in err(lib)
    # next to an output, or inside an out-of-place record's input, it is fine; so are empty records anywhere
    assert plan(lib, descs([(A, B, 100, B + 100, 13), (A + 4096, B + 4096, 100, B - 4, 4),
                            (A + 8192, B + 8192, 64, A + 8192, 64), (A, B, 0, 0, 0)]), fill=False)[0] == 3


# ---- what the kernels report about themselves -----------------------------------
def test_ws_bytes(lib):
    """Offset_0, checksum and HASH: three 16-byte rows per record."""
    assert lib.otc_ocb_batch_ws_bytes(0) == 0 and lib.otc_ocb_batch_ws_bytes(1000) == 48 * 1000
    assert lib.otc_ocb_batch_ws_bytes(7) % 16 == 0


def test_spans_are_positive_and_increasing(lib):
    buf = (ctypes.c_uint64 * 16)()
    n = lib.otc_ocb_batch_spans(buf, 16)
    spans = [int(v) for v in buf[:n]]
    assert n == 5 and spans[0] == 16  # a block, a slot, a wave pass, a workgroup step, the grid's first step
    assert all(s > 0 for s in spans) and all(a < b for a, b in zip(spans, spans[1:]))
    assert all(s % 16 == 0 for s in spans)
    assert lib.otc_ocb_batch_spans(None, 0) == n
    one = (ctypes.c_uint64 * 2)(0, 0xDEAD)
    assert lib.otc_ocb_batch_spans(one, 1) == n and one[0] == spans[0] and one[1] == 0xDEAD  # max is honoured
    assert ops.ocb_batch_ops.OcbBatch.spans() == spans == ops.ocb_batch_ops.ocb_batch_spans()


# ---- the run entry point --------------------------------------------------------
def aead_batch(lib, k, **kw):
    a = dict(msgs=A, tmap=A + 0x2000, first=A + 0x3000, ntiles=4, nmsg=4, key=ctypes.byref(k), dir=ENC,
             nonces=A + 0x5000, tags=A + 0x6000, expect=None, ok=None, ws=A + 0x7000)
    a.update(kw)
    return lib.otc_aes_ocb_batch(a["msgs"], a["tmap"], a["first"], a["ntiles"], a["nmsg"], a["key"], a["dir"],
                                 a["nonces"], a["tags"], a["expect"], a["ok"], a["ws"], None)


@pytest.mark.parametrize("kw,what", [
    (dict(msgs=None), "null"),
    (dict(tmap=None), "null tile map"),
    (dict(first=None), "null tile map"),
    (dict(key=None), "null key"),
    (dict(nonces=None), "null nonces"),
    (dict(tags=None), "null"),
    (dict(ws=None), "null"),
    (dict(msgs=A + 4), "misaligned"),
    (dict(first=A + 0x3004), "misaligned"),
    (dict(tmap=A + 0x2002), "misaligned"),
    (dict(tags=A + 0x6004), "16-byte aligned"),
    (dict(ws=A + 0x7008), "16-byte aligned"),
    (dict(dir=2), "direction"),
    (dict(dir=-1), "direction"),
    (dict(dir=DEC), "decryption needs"),
    (dict(dir=DEC, expect=A + 0x8000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000), "expected tags overlap"),        # the tag array itself
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 + 63), "expected tags overlap"),   # its last byte
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 - 63), "expected tags overlap"),   # its first
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 - 63), "expected tags overlap"),   # the verdicts
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 + 3), "expected tags overlap"),
])
def test_aead_batch_rejects_bad_arguments(lib, key, kw, what):
    assert aead_batch(lib, key, **kw) == ERR_ARG and what in err(lib), err(lib)


def test_aead_batch_rejects_a_broken_key(lib, key):
    k = _native.OtcOcbKey.from_buffer_copy(bytes(key))
    k.dec.nr = 12  # the two schedules are of different keys
    assert aead_batch(lib, k) == ERR_ARG and "schedules" in err(lib)
    assert aead_batch(lib, _native.OtcOcbKey()) == ERR_ARG  # never initialised


def test_aead_batch_accepts_expected_tags_next_to_its_own(lib, key):
    """Adjacent is not overlapping: the checks above do not fire, and the next one in line does."""
    for exp in (A + 0x6000 + 64, A + 0x6000 - 64, A + 0x9000 + 4):
        assert aead_batch(lib, key, dir=DEC, ok=A + 0x9000, expect=exp, nonces=None) == ERR_ARG
        assert "null nonces" in err(lib)


def test_records_without_whole_blocks_need_no_tile_map(lib, key):
    """ntiles == 0 skips the bulk kernel: the missing map is not an error; the next check in line fires."""
    assert aead_batch(lib, key, ntiles=0, tmap=None, first=None, nonces=None) == ERR_ARG and "null nonces" in err(lib)


def test_an_empty_batch_launches_nothing(lib, key):
    assert aead_batch(lib, key, nmsg=0, ntiles=0, msgs=None, tmap=None, first=None, nonces=None, tags=None, ws=None) == 0
    assert aead_batch(lib, key, nmsg=0, ntiles=0, dir=DEC) == 0
    assert aead_batch(lib, key, nmsg=0, dir=7) == ERR_ARG  # the direction is checked even then
    assert aead_batch(lib, key, nmsg=0, key=None) == ERR_ARG  # and the key


# ---- the Python layer -----------------------------------------------------------
OB = ops.ocb_batch_ops


def test_the_module_is_reachable_but_not_exported():
    assert ops.ocb_batch_ops.OcbBatch is OB.OcbBatch
    for name in ("OcbBatch", "ocb_encrypt_batch", "ocb_decrypt_batch", "ocb_batch_spans"):
        assert hasattr(OB, name) and name not in ops.__all__
    assert hasattr(AES, "ocb_encrypt_batch") and hasattr(AES, "ocb_decrypt_batch")
    assert hasattr(OB.OcbBatch, "packed") and hasattr(OB.OcbBatch, "spans")


@pytest.mark.parametrize("key", [bytes(15), bytes(17), bytes(33), b""])
def test_a_key_has_16_24_or_32_bytes(key):
    with pytest.raises(ValueError, match="16, 24 or 32"):
        OB.OcbBatch([], key)


def test_an_empty_batch_needs_no_device(lib):
    b = OB.OcbBatch([], bytes(24))
    n0, t0 = torch.zeros((0, 12), dtype=torch.uint8), torch.zeros((0, 16), dtype=torch.uint8)
    outs, tags = b.encrypt(n0)
    assert outs == [] and tuple(tags.shape) == (0, 16) and tags.dtype == torch.uint8
    outs, ok = b.decrypt(n0, t0)
    assert outs == [] and tuple(ok.shape) == (0,) and ok.dtype == torch.bool
    assert OB.ocb_encrypt_batch([], bytes(16), n0)[0] == []
    assert AES(bytes(32)).ocb_decrypt_batch([], n0, t0)[0] == []
    # the shapes are checked even then
    for bad in (torch.zeros((0, 8), dtype=torch.uint8), torch.zeros((0, 12), dtype=torch.int32),
                torch.zeros((1, 12), dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8), b"", None):
        with pytest.raises(ValueError, match="nonce"):
            b.encrypt(bad)
    for bad in (torch.zeros((0, 15), dtype=torch.uint8), torch.zeros((0, 16), dtype=torch.int8),
                torch.zeros((2, 16), dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="tags"):
            b.decrypt(n0, bad)


def planned(n=2):
    """A batch of n records as the constructor leaves it, without a device: what the run methods check first."""
    b = OB.OcbBatch.__new__(OB.OcbBatch)
    b._init_common(bytes(16))
    b.n, b.device, b.outs = n, torch.device("cuda:0"), []
    b.tags, b.ok = torch.zeros((n, 16), dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
    return b


def test_nonces_and_tags_must_be_on_the_device(lib):
    b = planned()
    with pytest.raises(ValueError, match="nonces must be a GPU tensor"):
        b.encrypt(torch.zeros((2, 12), dtype=torch.uint8))
    with pytest.raises(ValueError, match="nonces must be a GPU tensor"):
        b.decrypt(torch.zeros((2, 12), dtype=torch.uint8), torch.zeros((2, 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="nonces must be a GPU tensor"):
        b.encrypt([bytes(12)] * 2)


def test_decrypt_refuses_the_batchs_own_tensors(lib):
    b = planned()
    for own in (b.tags, b.tags[1:], b.ok.view(1, 2)):
        with pytest.raises(ValueError, match="own tags"):
            b.decrypt(torch.zeros((2, 12), dtype=torch.uint8), own)


def test_the_new_functions_are_declared():
    src = open(os.path.join(ROOT, "our_tree_amd", "_native.py")).read()
    declared = set(re.findall(r'"(otc_\w+)": \(', src))
    assert {"otc_ocb_batch_plan", "otc_ocb_batch_ws_bytes", "otc_ocb_batch_spans", "otc_aes_ocb_batch"} <= declared
    # pointers as pointers, sizes as 64-bit: the planner's result is an int64 (a tile count or an error)
    assert re.search(r'"otc_ocb_batch_plan": \(ctypes\.c_int64, \[c_vp, c_sz, c_vp, c_vp\]\)', src)
    assert re.search(r'"otc_aes_ocb_batch": \(c_int, \[c_vp, c_vp, c_vp, c_u64, c_sz, P\(OtcOcbKey\), c_int, c_vp, c_vp, '
                     r'c_vp, c_vp, c_vp,\s+c_vp\]\)', src)
    hdr = open(os.path.join(ROOT, "csrc", "include", "otc.h")).read()
    for name in ("otc_ocb_msg", "OTC_OCB_BATCH_MAX_BYTES", "OTC_OCB_BATCH_MAX_AAD", "otc_ocb_batch_plan",
                 "otc_ocb_batch_ws_bytes", "otc_ocb_batch_spans", "otc_aes_ocb_batch"):
        assert name in hdr


def test_the_batch_oracle_is_a_loop_over_the_single_message_one():
    key = bytes(range(32))
    nonces = [bytes([i] * 12) for i in range(3)]
    datas, aads = [b"", b"x" * 17, bytes(range(100))], [b"a", b"", b"header"]
    got = cpu_ref.ocb_batch(key, nonces, datas, aads)
    assert got == [cpu_ref.ocb(key, n, d, a) for n, d, a in zip(nonces, datas, aads)]
    back = cpu_ref.ocb_batch(key, nonces, [c for c, _ in got], aads, decrypt=True)
    assert [p for p, _ in back] == datas and [t for _, t in back] == [t for _, t in got]
    with pytest.raises(ValueError, match="12 bytes"):
        cpu_ref.ocb_batch(key, [bytes(11)], [b""])
    with pytest.raises(ValueError, match="one nonce"):
        cpu_ref.ocb_batch(key, nonces, datas[:2])


# ---- the kernels' decomposition on the host ---------------------------------------
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "address-undefined"])
def test_ocb_batch_selftest(tmp_path, flags):
    """A program of its own with its own main: prep's Offset_0 and 16-lane HASH, the slot start,
    low(v), the lane-63 carry, the finisher's Offset_m, for every length 0 .. 4200, around the 1 MiB
    cap and for all three key sizes, against aes_crypt_ocb of aes.c."""
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("gcc not available")
    inc = ["-I", os.path.join(ROOT, "csrc/include"), "-I", os.path.join(ROOT, "csrc/hip")]
    exe = tmp_path / "ocb_batch_selftest"
    b = subprocess.run([cc, "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Wno-unknown-pragmas", *inc, *flags,
                        os.path.join(ROOT, "csrc/cpu/ocb_batch_selftest.c"), os.path.join(ROOT, "csrc/cpu/aes.c"),
                        "-o", str(exe), "-lpthread"], capture_output=True, text=True)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for bits in (128, 192, 256):
        assert f"OK AES-{bits} 4212 records" in r.stdout
    assert "FAIL" not in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
