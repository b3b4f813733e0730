"""Batched AES-GCM-SIV without a GPU: the host planner
(otc_gcm_siv_batch_plan), what the kernels report about themselves, the
argument checks of otc_aes_gcm_siv_batch and of the two halves -- which must
answer OTC_ERR_ARG with a message *before* any HIP call: the device addresses
below are fake and never dereferenced --, the Python layer's checks and the
batch oracle."""
import ctypes
import os
import re

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
TILE = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not _native.gpu_lib_available():
        pytest.fail("libotc.so not built")
    return _native.require_gpu_lib()


@pytest.fixture(scope="module")
def key(lib):
    k = _native.OtcGcmSivKey()
    assert lib.otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(16))), 128) == 0
    return k


def err(lib) -> str:
    return lib.otc_last_error().decode()


def descs(rows):
    """rows of (in, out, nbytes, aad, aad_bytes) -> otc_gcm_msg[] as uint64 [n, 6]"""
    d = np.zeros((len(rows), 6), dtype=np.uint64)
    for i, r in enumerate(rows):
        d[i, :len(r)] = r
    return d


def plan(lib, d, fill=True):
    n = d.shape[0]
    nt = lib.otc_gcm_siv_batch_plan(d.ctypes.data, n, None, None)
    if nt < 0 or not fill:
        return nt, None, None
    first = np.full(n, 0xEE, dtype=np.uint64)
    tmap = np.zeros(max(nt, 1), dtype=np.uint32)
    assert lib.otc_gcm_siv_batch_plan(d.ctypes.data, n, tmap.ctypes.data, first.ctypes.data) == nt
    return nt, tmap[:nt], first


def tiles_of(n):
    return (n + TILE - 1) // TILE


# ---- the planner ----------------------------------------------------------------
@pytest.mark.parametrize("n,tiles", [(0, 0), (1, 1), (15, 1), (TILE, 1), (TILE + 1, 2), (MAX_BYTES, 256)])
def test_planner_tile_counts(lib, n, tiles):
    """A tile is 256 blocks of one record, the trailing bytes included."""
    assert plan(lib, descs([(A, A, n, 0, 0)]), fill=False)[0] == tiles == tiles_of(n)


def test_planner_tile_map_of_a_mixed_batch(lib):
    lens = [0, 1, 4096, 15, 4097, 0, 16, 3 * 4096 + 17, 64]
    rows, at = [], A
    for i, n in enumerate(lens):
        rows.append((at, at if i % 2 else at + (8 << 20), n, A + (32 << 20) + 3 + 64 * i, (i * 7) % 40))
        at += (n + 15) // 16 * 16
    nt, tmap, first = plan(lib, descs(rows))
    tiles = [tiles_of(n) for n in lens]
    assert tiles == [0, 1, 1, 1, 2, 0, 1, 4, 1] and nt == sum(tiles)
    assert first.tolist() == np.cumsum([0] + tiles[:-1]).tolist()
    assert tmap.tolist() == [m for m, t in enumerate(tiles) for _ in range(t)]


def test_planner_counts_without_output_arrays(lib):
    d = descs([(A, A, 4097, 0, 0), (A + 8192, A + 8192, 0, 0, 0)])
    assert plan(lib, d, fill=False)[0] == 2
    assert lib.otc_gcm_siv_batch_plan(None, 0, None, None) == 0
    first = np.zeros(2, dtype=np.uint64)
    tmap = np.zeros(2, dtype=np.uint32)
    assert lib.otc_gcm_siv_batch_plan(d.ctypes.data, 2, None, first.ctypes.data) == 2 and first.tolist() == [0, 2]
    assert lib.otc_gcm_siv_batch_plan(d.ctypes.data, 2, tmap.ctypes.data, None) == 2 and tmap.tolist() == [0, 0]
    assert lib.otc_gcm_siv_batch_plan(None, 3, None, None) == ERR_ARG and "null descriptors" in err(lib)


@pytest.mark.parametrize("row,what", [
    ((A, A, MAX_BYTES + 1, 0, 0), "1 MiB"),                 # a record over 1 MiB
    ((A, A, 16, A + 4096, MAX_AAD + 1), "64 KiB"),          # AAD over 64 KiB
    ((A, A, 0, 0, 5), "null aad"),
    ((0, A, 64, 0, 0), "null buffer"),
    ((A, 0, 5, 0, 0), "null buffer"),
    ((A + 4, A + 4096, 64, 0, 0), "aligned"),               # a misaligned buffer
    ((A, A + 4096 + 8, 64, 0, 0), "aligned"),
    ((A, A + 16, 64, 0, 0), "overlap partially"),           # partial in/out overlap
    ((A + 32, A, 64, 0, 0), "overlap partially"),
])
def test_planner_rejects_a_bad_record(lib, row, what):
    good = (A + (1 << 24), A + (1 << 24), 100, 0, 0)
    nt = plan(lib, descs([good, row]))[0]
    assert nt == ERR_ARG and what in err(lib) and "gcm_siv_batch: record 1: " in err(lib), err(lib)


def test_planner_accepts_the_caps(lib):
    d = descs([(A, A, MAX_BYTES, A + (4 << 20) + 1, MAX_AAD)])
    assert plan(lib, d, fill=False)[0] == 256


def test_planner_rejects_records_that_overlap(lib):
    B = A + (1 << 24)
    # two records overlapping
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 96, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "output overlaps another record" in err(lib)
    assert plan(lib, descs([(A, B, 100, 0, 0), (B + 64, B + 4096, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "input overlaps another record's output" in err(lib)
    # an AAD overlapping an output -- its own record's or another's
    assert plan(lib, descs([(A, B, 100, B + 50, 13)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, A, 100, A + 99, 1)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 4096, 100, B - 3, 4)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "AAD overlaps" in err(lib)
    # next to an output it is fine; so are empty records anywhere
    assert plan(lib, descs([(A, B, 100, B + 100, 13), (A + 4096, B + 4096, 100, B - 4, 4), (A, B, 0, 0, 0)]),
                fill=False)[0] == 2


# ---- what the kernels report about themselves -----------------------------------
def test_ws_bytes_hold_two_rows_and_a_schedule_per_record(lib):
    per = 32 + ctypes.sizeof(_native.OtcAesKey)
    assert per == 288
    assert lib.otc_gcm_siv_batch_ws_bytes(0) == 0 and lib.otc_gcm_siv_batch_ws_bytes(1000) == per * 1000
    assert lib.otc_gcm_siv_batch_ws_bytes(7) % 16 == 0
    hdr = open(os.path.join(ROOT, "csrc", "include", "otc.h")).read()
    assert "KEY MATERIAL" in hdr[hdr.index("otc_gcm_siv_batch_plan"):hdr.index("size_t otc_gcm_siv_batch_ws_bytes")]


def test_spans_and_lanes(lib):
    buf = (ctypes.c_uint64 * 8)()
    n = lib.otc_gcm_siv_batch_spans(buf, 8)
    assert [int(v) for v in buf[:n]] == [16, 64, 256] == ops.gcm_siv_batch_ops.GcmSivBatch.spans()
    assert lib.otc_gcm_siv_batch_spans(None, 0) == n
    short = descs([(A + 8192 * i, A + 8192 * i, 4096, 0, 0) for i in range(8)])
    long_ = descs([(A + (1 << 20) * i, A + (1 << 20) * i, 16384, 0, 0) for i in range(8)])
    assert lib.otc_gcm_siv_batch_lanes(short.ctypes.data, 8) == 16
    assert lib.otc_gcm_siv_batch_lanes(long_.ctypes.data, 8) == 64
    assert lib.otc_gcm_siv_batch_lanes(None, 0) == 16


# ---- the run entry points -------------------------------------------------------
def aead_batch(lib, k, **kw):
    a = dict(msgs=A, tmap=A + 0x2000, first=A + 0x3000, ntiles=4, nmsg=4, key=ctypes.byref(k), dir=ENC,
             nonces=A + 0x5000, tags=A + 0x6000, expect=None, ok=None, ws=A + 0x7000, lanes=16)
    a.update(kw)
    return lib.otc_aes_gcm_siv_batch(a["msgs"], a["tmap"], a["first"], a["ntiles"], a["nmsg"], a["key"], a["dir"],
                                     a["nonces"], a["tags"], a["expect"], a["ok"], a["ws"], a["lanes"], None)


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
    (dict(lanes=32), "lanes"),
    (dict(dir=2), "direction"),
    (dict(dir=DEC), "decryption needs"),
    (dict(dir=DEC, expect=A + 0x8000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000), "expected tags overlap"),        # the tag array itself
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 + 63), "expected tags overlap"),   # its last byte
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 - 63), "expected tags overlap"),   # the verdicts
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x8002), "4-byte aligned"),               # the counter kernel reads them
])
def test_aead_batch_rejects_bad_arguments(lib, key, kw, what):
    assert aead_batch(lib, key, **kw) == ERR_ARG and what in err(lib), err(lib)


def test_aead_batch_rejects_aes192_and_a_blank_key(lib):
    k = _native.OtcGcmSivKey()
    assert lib.otc_aes_key_init(ctypes.byref(k.kgk), _native.as_u8p(bytes(24)), 192, ENC) == 0
    assert aead_batch(lib, k) == ERR_ARG and "128 or 256" in err(lib)
    assert aead_batch(lib, _native.OtcGcmSivKey()) == ERR_ARG  # never initialised
    assert lib.otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(bytes(24)), 192) == ERR_ARG


def test_an_empty_batch_launches_nothing(lib, key):
    assert aead_batch(lib, key, nmsg=0, ntiles=0, msgs=None, tmap=None, first=None, nonces=None, tags=None, ws=None) == 0
    assert aead_batch(lib, key, nmsg=0, dir=7) == ERR_ARG  # the direction is checked even then
    assert aead_batch(lib, key, nmsg=0, key=None) == ERR_ARG  # and the key


def test_all_empty_records_need_no_tile_map(lib, key):
    """ntiles == 0 skips the counter kernel only: the next check in line still fires."""
    assert aead_batch(lib, key, ntiles=0, tmap=None, first=None, nonces=None) == ERR_ARG and "null nonces" in err(lib)


def test_the_halves_reject_bad_arguments(lib):
    pv = lambda **kw: lib.otc_polyval_batch(*[{**dict(m=A, n=4, h=A + 0x1000, s=A + 0x2000, lanes=16), **kw}[k]
                                              for k in ("m", "n", "h", "s", "lanes")], None)
    assert pv(n=0, m=None) == 0
    for kw, what in [(dict(m=None), "null"), (dict(h=None), "null"), (dict(s=A + 0x2008), "16-byte aligned"),
                     (dict(h=A + 0x1004), "16-byte aligned"), (dict(lanes=8), "lanes"), (dict(m=A + 2), "misaligned")]:
        assert pv(**kw) == ERR_ARG and what in err(lib), (kw, err(lib))
    ct = lambda **kw: lib.otc_aes_ctr_le32_batch(*[{**dict(m=A, k=A + 0x1000, c=A + 0x2000, t=A + 0x3000, f=A + 0x4000,
                                                           nt=4, n=4, nr=10), **kw}[k]
                                                   for k in ("m", "k", "c", "t", "f", "nt", "n", "nr")], None)
    assert ct(nt=0) == 0 and ct(n=0) == 0
    for kw, what in [(dict(nr=11), "nr"), (dict(k=None), "null"), (dict(c=None), "null"), (dict(t=None), "tile map"),
                     (dict(k=A + 0x1008), "16-byte aligned"), (dict(c=A + 0x2002), "4-byte aligned"),
                     (dict(f=A + 0x4004), "misaligned")]:
        assert ct(**kw) == ERR_ARG and what in err(lib), (kw, err(lib))


# ---- the Python layer -----------------------------------------------------------
SB = ops.gcm_siv_batch_ops
NAMES = ("GcmSivBatch", "gcm_siv_encrypt_batch", "gcm_siv_decrypt_batch", "gcm_siv_batch_spans", "polyval_batch",
         "ctr_le32_batch")


def test_the_module_is_reachable_but_not_exported():
    assert ops.gcm_siv_batch_ops.GcmSivBatch is SB.GcmSivBatch
    for name in NAMES:
        assert hasattr(SB, name) and name not in ops.__all__
    assert hasattr(AES, "gcm_siv_encrypt_batch") and hasattr(AES, "gcm_siv_decrypt_batch")
    assert hasattr(SB.GcmSivBatch, "packed") and hasattr(SB.GcmSivBatch, "spans")
    assert issubclass(SB.GcmSivBatch, ops.ocb_batch_ops.OcbBatch)  # the contract and its checks are reused
    src = open(SB.__file__).read()
    assert "from .batch_ops import _Blob, _packed_buffers, _packed_layout, _set_aads, _tensor_descs" in src
    assert not re.search(r"^(class|def) (_Blob|_tensor_descs|_set_aads|_packed_layout|_packed_buffers)\b", src, re.M)


@pytest.mark.parametrize("key", [bytes(24), bytes(15), bytes(33), b""])
def test_a_key_has_16_or_32_bytes(key):
    with pytest.raises(ValueError, match="16 or 32"):
        SB.GcmSivBatch([], key)
    with pytest.raises(ValueError, match="16 or 32"):
        SB.GcmSivBatch.packed(torch.zeros(16, dtype=torch.uint8), [16], key)


def test_a_cpu_tensor_is_refused_before_any_device_call():
    x = torch.zeros(64, dtype=torch.uint8)
    n1 = torch.zeros((1, 12), dtype=torch.uint8)
    with pytest.raises(ValueError):
        SB.GcmSivBatch([x], bytes(16))
    with pytest.raises(ValueError):
        SB.GcmSivBatch.packed(x, [64], bytes(32))
    with pytest.raises(ValueError):
        SB.gcm_siv_encrypt_batch([x], bytes(16), n1)
    with pytest.raises(ValueError):
        SB.polyval_batch([x], torch.zeros((1, 16), dtype=torch.uint8))
    with pytest.raises(ValueError):
        SB.ctr_le32_batch([x], [bytes(16)], torch.zeros((1, 16), dtype=torch.uint8))


def test_an_empty_batch_needs_no_device():
    b = SB.GcmSivBatch([], bytes(32))
    n0, t0 = torch.zeros((0, 12), dtype=torch.uint8), torch.zeros((0, 16), dtype=torch.uint8)
    outs, tags = b.encrypt(n0)
    assert outs == [] and tuple(tags.shape) == (0, 16) and tags.dtype == torch.uint8
    outs, ok = b.decrypt(n0, t0)
    assert outs == [] and tuple(ok.shape) == (0,) and ok.dtype == torch.bool
    assert SB.gcm_siv_encrypt_batch([], bytes(16), n0)[0] == []
    assert AES(bytes(32)).gcm_siv_decrypt_batch([], n0, t0)[0] == []
    # the shapes are checked even then: nonces are [n, 12] uint8 contiguous
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
    b = SB.GcmSivBatch.__new__(SB.GcmSivBatch)
    b._init_common(bytes(16))
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
    names = {"otc_gcm_siv_batch_plan", "otc_gcm_siv_batch_ws_bytes", "otc_gcm_siv_batch_lanes", "otc_gcm_siv_batch_spans",
             "otc_polyval_batch", "otc_aes_ctr_le32_batch", "otc_aes_gcm_siv_batch"}
    assert names <= declared
    assert re.search(r'"otc_gcm_siv_batch_plan": \(ctypes\.c_int64, \[c_vp, c_sz, c_vp, c_vp\]\)', src)
    hdr = open(os.path.join(ROOT, "csrc", "include", "otc.h")).read()
    for name in names | {"OTC_GCM_SIV_BATCH_MAX_BYTES", "OTC_GCM_SIV_BATCH_MAX_AAD"}:
        assert name in hdr


def test_the_batch_oracle_is_a_loop_over_the_single_message_one():
    key = bytes(range(32))
    nonces = [bytes([i] * 12) for i in range(3)]
    datas, aads = [b"", b"x" * 17, bytes(range(100))], [b"a", b"", b"header"]
    got = cpu_ref.gcm_siv_batch(key, nonces, datas, aads)
    assert got == [cpu_ref.gcm_siv(key, n, d, a) for n, d, a in zip(nonces, datas, aads)]
    back = cpu_ref.gcm_siv_batch(key, nonces, [c for c, _ in got], aads, decrypt=True, tags=[t for _, t in got])
    assert [p for p, _ in back] == datas and [t for _, t in back] == [t for _, t in got]
    with pytest.raises(ValueError, match="12 bytes"):
        cpu_ref.gcm_siv_batch(key, [bytes(11)], [b""])
    with pytest.raises(ValueError, match="one nonce"):
        cpu_ref.gcm_siv_batch(key, nonces, datas[:2])
