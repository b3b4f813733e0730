"""Batched AES-GCM with a key per record, without a GPU: the host planner
(otc_gcm_mk_batch_plan), what the kernels report about themselves, the argument
checks of otc_aes_gcm_mk_batch, otc_ghash_mk_batch and otc_gcm_mk_batch_tables
-- which must answer OTC_ERR_ARG with a message *before* any HIP call: the
device addresses below are fake and never dereferenced --, the Python layer's
checks and the batch oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref

ERR_ARG = -1
ENC, DEC = 1, 0
A = 0x7F0000000000  # fake, 16-byte aligned device addresses (never touched)
MAX_BYTES, MAX_AAD = 1 << 20, 1 << 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not _native.gpu_lib_available():
        pytest.fail("libotc.so not built")
    return _native.require_gpu_lib()


def err(lib) -> str:
    return lib.otc_last_error().decode()


def descs(rows):
    """rows of (in, out, nbytes, aad, aad_bytes, key) -> otc_gcm_mk_msg[] as uint64 [n, 6]"""
    d = np.zeros((len(rows), 6), dtype=np.uint64)
    for i, r in enumerate(rows):
        d[i, :len(r)] = r
    return d


def plan(lib, d, nkeys=4, tile=256, fill=True):
    n = d.shape[0]
    nt = lib.otc_gcm_mk_batch_plan(d.ctypes.data, n, nkeys, tile, None, None, None)
    if nt < 0 or not fill:
        return nt, None, None, None
    ctr = np.full((n, 6), 0xEE, dtype=np.uint64)
    first = np.full(n, 0xEE, dtype=np.uint64)
    tmap = np.zeros(max(nt, 1), dtype=np.uint32)
    assert lib.otc_gcm_mk_batch_plan(d.ctypes.data, n, nkeys, tile, ctr.ctypes.data, tmap.ctypes.data,
                                     first.ctypes.data) == nt  # both passes agree
    return nt, ctr, tmap[:nt], first


# ---- the planner ----------------------------------------------------------------
@pytest.mark.parametrize("tile", [64, 128, 256])
def test_planner_tile_map_and_ctr_descriptors(lib, tile):
    lens = [0, 1, 4096, 15, 4097, 0, 16, 3 * 4096 + 17, 64]
    keys = [3, 0, 1, 2, 3, 0, 1, 2, 3]
    rows, at = [], A
    for i, n in enumerate(lens):
        rows.append((at, at if i % 2 else at + (8 << 20), n, A + (32 << 20) + 3 + 64 * i, (i * 7) % 40, keys[i]))
        at += (n + 15) // 16 * 16
    d = descs(rows)
    nt, ctr, tmap, first = plan(lib, d, tile=tile)
    tiles = [(n + 16 * tile - 1) // (16 * tile) for n in lens]
    assert nt == sum(tiles)
    assert first.tolist() == np.cumsum([0] + tiles[:-1]).tolist()
    assert tmap.tolist() == [m for m, t in enumerate(tiles) for _ in range(t)]
    # the CTR half's descriptors: buffers and length, counters left to prep, the key index, no alignment word
    assert (ctr[:, :3] == d[:, :3]).all() and (ctr[:, 3:5] == 0).all() and ctr[:, 5].tolist() == keys


def test_planner_counts_without_output_arrays(lib):
    d = descs([(A, A, 4097, 0, 0, 1), (A + 8192, A + 8192, 0, 0, 0, 0)])
    assert plan(lib, d, fill=False)[0] == 2
    assert lib.otc_gcm_mk_batch_plan(None, 0, 0, 256, None, None, None) == 0
    first = np.zeros(2, dtype=np.uint64)
    tmap = np.zeros(2, dtype=np.uint32)
    assert lib.otc_gcm_mk_batch_plan(d.ctypes.data, 2, 2, 256, None, None, first.ctypes.data) == 2
    assert first.tolist() == [0, 2]
    assert lib.otc_gcm_mk_batch_plan(d.ctypes.data, 2, 2, 256, None, tmap.ctypes.data, None) == 2 and tmap.tolist() == [0, 0]
    assert lib.otc_gcm_mk_batch_plan(None, 3, 1, 256, None, None, None) == ERR_ARG and "null descriptors" in err(lib)
    assert lib.otc_gcm_mk_batch_plan(d.ctypes.data, 2, 2, 100, None, None, None) == ERR_ARG and "tile_blocks" in err(lib)


@pytest.mark.parametrize("row,what", [
    ((A, A, 64, 0, 0, 4), "key index out of range"),           # key >= nkeys
    ((A, A, 0, 0, 0, 1 << 40), "key index out of range"),      # an empty record has a key too
    ((A, A, MAX_BYTES + 1, 0, 0, 0), "1 MiB"),                 # the caps
    ((A, A, 16, A + 4096, MAX_AAD + 1, 0), "64 KiB"),
    ((A, A, 0, 0, 5, 0), "null aad"),
    ((0, A, 64, 0, 0, 0), "null buffer"),
    ((A + 4, A + 4096, 64, 0, 0, 0), "aligned"),               # misalignment
    ((A, A + 4096 + 8, 64, 0, 0, 0), "aligned"),
    ((A, A + 16, 64, 0, 0, 0), "overlap partially"),           # each overlap kind
    ((A + (1 << 24) + 4096, A + (1 << 24) + 96, 100, 0, 0, 0), "output overlaps another record"),
    ((A + (1 << 24) + 64, A + 4096, 100, 0, 0, 0), "input overlaps another record's output"),
    ((A + 4096, A + 8192, 100, A + (1 << 24) + 50, 13, 0), "AAD overlaps"),
])
def test_planner_rejects_a_bad_record(lib, row, what):
    good = (A + (1 << 24), A + (1 << 24), 100, 0, 0, 3)
    nt = plan(lib, descs([good, row]))[0]
    assert nt == ERR_ARG and what in err(lib) and "gcm_mk_batch: record 1: " in err(lib), err(lib)


def test_planner_accepts_the_caps(lib):
    d = descs([(A, A, MAX_BYTES, A + (4 << 20) + 1, MAX_AAD, 0)])
    assert plan(lib, d, nkeys=1, fill=False)[0] == 256


# ---- what the kernels report about themselves -----------------------------------
def test_ws_and_table_bytes_are_linear(lib):
    assert lib.otc_gcm_mk_batch_ws_bytes(0) == 0 and lib.otc_gcm_mk_batch_ws_bytes(1000) == 32 * 1000  # J0 and the hash
    assert lib.otc_gcm_mk_batch_table_bytes(0) == 0 and lib.otc_gcm_mk_batch_table_bytes(1000) == 7 * 256 * 1000
    for n in (1, 3, 7):
        assert lib.otc_gcm_mk_batch_ws_bytes(n) % 16 == 0 and lib.otc_gcm_mk_batch_table_bytes(n) % 16 == 0
    hdr = open(os.path.join(ROOT, "csrc", "include", "otc.h")).read()
    sect = hdr[hdr.index("batched AES-GCM, a key per record"):hdr.index("} otc_gcm_mk_msg;")]
    assert "KEY MATERIAL" in sect and "the caller's job" in sect


def test_spans_and_lanes(lib):
    buf = (ctypes.c_uint64 * 8)()
    n = lib.otc_gcm_mk_batch_spans(buf, 8)
    assert [int(v) for v in buf[:n]] == [16, 64, 256] == ops.gcm_mk_batch_ops.GcmMkBatch.spans()
    assert ops.gcm_mk_batch_ops.gcm_mk_batch_spans() == [16, 64, 256]
    assert lib.otc_gcm_mk_batch_spans(None, 0) == n
    short = descs([(A + 8192 * i, A + 8192 * i, 1024, 0, 0, i) for i in range(8)])
    long_ = descs([(A + (1 << 20) * i, A + (1 << 20) * i, 65536, 0, 0, i) for i in range(8)])
    assert lib.otc_gcm_mk_batch_lanes(short.ctypes.data, 8) == 16
    assert lib.otc_gcm_mk_batch_lanes(long_.ctypes.data, 8) == 64
    assert lib.otc_gcm_mk_batch_lanes(None, 0) == 16


# ---- the run entry points -------------------------------------------------------
def aead_batch(lib, **kw):
    a = dict(msgs=A, ctr=A + 0x1000, tmap=A + 0x2000, first=A + 0x3000, ntiles=4, tile=256, nmsg=4, keys=A + 0x4000,
             nkeys=2, nr=10, tab=A + 0xA000, dir=ENC, ivs=A + 0x5000, tags=A + 0x6000, expect=None, tag_bytes=16,
             ok=None, ws=A + 0x7000, lanes=16)
    a.update(kw)
    return lib.otc_aes_gcm_mk_batch(a["msgs"], a["ctr"], a["tmap"], a["first"], a["ntiles"], a["tile"], a["nmsg"],
                                    a["keys"], a["nkeys"], a["nr"], a["tab"], a["dir"], a["ivs"], a["tags"], a["expect"],
                                    a["tag_bytes"], a["ok"], a["ws"], a["lanes"], None)


@pytest.mark.parametrize("kw,what", [
    (dict(msgs=None), "null"),                                   # a null argument
    (dict(ctr=None), "null"),
    (dict(tmap=None), "null tile map"),
    (dict(first=None), "null tile map"),
    (dict(keys=None), "null"),
    (dict(tab=None), "null"),
    (dict(ivs=None), "null IVs"),
    (dict(tags=None), "null"),
    (dict(ws=None), "null"),
    (dict(nkeys=0), "no keys"),
    (dict(msgs=A + 4), "misaligned"),                            # a misaligned argument
    (dict(ctr=A + 0x1004), "misaligned"),
    (dict(keys=A + 0x4004), "misaligned"),
    (dict(first=A + 0x3004), "misaligned"),
    (dict(tmap=A + 0x2002), "misaligned"),
    (dict(tab=A + 0xA008), "16-byte aligned"),
    (dict(tags=A + 0x6004), "16-byte aligned"),
    (dict(ws=A + 0x7008), "16-byte aligned"),
    (dict(lanes=32), "lanes"),                                   # bad lanes
    (dict(lanes=-16), "lanes"),
    (dict(tag_bytes=3), "4 to 16"),                              # bad tag_bytes
    (dict(tag_bytes=17), "4 to 16"),
    (dict(tile=100), "tile_blocks"),
    (dict(nr=11), "nr"),
    (dict(dir=2), "direction"),
    (dict(dir=DEC), "decryption needs"),
    (dict(dir=DEC, expect=A + 0x8000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000), "expected tags overlap"),        # the tag array itself
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 + 63), "expected tags overlap"),   # its last byte
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 - 63), "expected tags overlap"),   # the verdicts
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 - 15, tag_bytes=4), "expected tags overlap"),  # 4 x 4 bytes
])
def test_aead_batch_rejects_bad_arguments(lib, kw, what):
    assert aead_batch(lib, **kw) == ERR_ARG and what in err(lib), err(lib)


def test_short_expected_tags_next_to_the_tag_array_are_fine_as_far_as_the_checks_go(lib):
    """4 records x 4 bytes end where the tag array begins: no overlap; the next check in line fires."""
    assert aead_batch(lib, dir=DEC, ok=A + 0x9000, expect=A + 0x6000 - 16, tag_bytes=4, ivs=None) == ERR_ARG
    assert "null IVs" in err(lib)


def test_an_empty_batch_launches_nothing(lib):
    assert aead_batch(lib, nmsg=0, ntiles=0, msgs=None, ctr=None, tmap=None, first=None, keys=None, tab=None, ivs=None,
                      tags=None, ws=None) == 0
    assert aead_batch(lib, nmsg=0, dir=7) == ERR_ARG  # the direction is checked even then
    assert aead_batch(lib, nmsg=0, tag_bytes=2) == ERR_ARG
    assert aead_batch(lib, nmsg=0, nr=13) == ERR_ARG


def test_the_hash_and_the_table_call_reject_bad_arguments(lib):
    gh = lambda **kw: lib.otc_ghash_mk_batch(*[{**dict(m=A, n=4, t=A + 0x1000, s=A + 0x2000, lanes=16), **kw}[k]
                                               for k in ("m", "n", "t", "s", "lanes")], None)
    for kw, what in [(dict(m=None), "null"), (dict(t=None), "null"), (dict(s=None), "null"),
                     (dict(s=A + 0x2008), "16-byte aligned"), (dict(t=A + 0x1004), "16-byte aligned"),
                     (dict(lanes=8), "lanes"), (dict(m=A + 2), "misaligned")]:
        assert gh(**kw) == ERR_ARG and what in err(lib), (kw, err(lib))
    assert gh(n=0) == 0
    tb = lambda **kw: lib.otc_gcm_mk_batch_tables(*[{**dict(k=A, n=4, nr=14, t=A + 0x1000), **kw}[k]
                                                    for k in ("k", "n", "nr", "t")], None)
    for kw, what in [(dict(k=None), "schedules"), (dict(t=None), "tables"), (dict(k=A + 4), "8-byte aligned"),
                     (dict(t=A + 0x1008), "16-byte aligned"), (dict(nr=9), "nr")]:
        assert tb(**kw) == ERR_ARG and what in err(lib), (kw, err(lib))
    assert tb(n=0, k=None, t=None) == 0


# ---- the Python layer -----------------------------------------------------------
MK = ops.gcm_mk_batch_ops
NAMES = ("GcmMkBatch", "gcm_mk_encrypt_batch", "gcm_mk_decrypt_batch", "ghash_mk_batch", "gcm_mk_batch_spans")


def test_the_module_is_reachable_but_not_exported():
    for name in NAMES:
        assert hasattr(MK, name) and name not in ops.__all__
    for m in ("packed", "encrypt", "decrypt", "ghash", "rekey", "spans"):
        assert hasattr(MK.GcmMkBatch, m)
    assert issubclass(MK.GcmMkBatch, ops.GcmBatch)  # the contract, the IV checks and their texts are reused
    assert MK.GcmMkBatch._check_ivs is ops.GcmBatch._check_ivs and MK.GcmMkBatch.decrypt is ops.GcmBatch.decrypt
    src = open(MK.__file__).read()
    assert not re.search(r"^(class|def) (_Blob|_tensor_descs|_set_aads|_packed_layout|_packed_buffers|_key_index)\b", src, re.M)


def test_mixed_key_sizes_are_refused():
    for keys in ([bytes(16), bytes(32)], [bytes(24), bytes(16), bytes(24)]):
        with pytest.raises(ValueError, match="one size"):
            MK.GcmMkBatch([], keys, key_index=[])
        with pytest.raises(ValueError, match="one size"):
            MK.GcmMkBatch.packed(torch.zeros(16, dtype=torch.uint8), [16], keys, key_index=[0])
    for keys in ([bytes(15)], [bytes(16), b""], []):
        with pytest.raises(ValueError):
            MK.GcmMkBatch([], keys, key_index=[])


def test_a_key_index_out_of_range_is_refused():
    x = torch.zeros(64, dtype=torch.uint8)
    for kidx in ([2], [-1]):
        with pytest.raises(ValueError, match="key_index out of range"):
            MK.GcmMkBatch([x], [bytes(16), bytes(16)], key_index=kidx)
        with pytest.raises(ValueError, match="key_index out of range"):
            MK.GcmMkBatch.packed(x, [64], [bytes(16), bytes(16)], key_index=kidx)
    with pytest.raises(ValueError, match="one key index"):
        MK.GcmMkBatch([x], [bytes(16)], key_index=[0, 0])
    with pytest.raises(ValueError, match="one key per message"):
        MK.GcmMkBatch([x], [bytes(16), bytes(16)])  # no key_index: as many keys as records


def test_a_cpu_tensor_is_refused_before_any_device_call():
    x = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        MK.GcmMkBatch([x], [bytes(16)])
    with pytest.raises(ValueError):
        MK.GcmMkBatch.packed(x, [64], [bytes(32)])
    with pytest.raises(ValueError):
        MK.ghash_mk_batch([x], [bytes(16)])


def planned(n=2, tag_bytes=16):
    """A batch of n records as the constructor leaves it, without a device: what the run methods check first."""
    b = MK.GcmMkBatch.__new__(MK.GcmMkBatch)
    b._init_common([bytes(16)], tag_bytes, None)
    b.n, b.device, b.outs = n, torch.device("cuda:0"), []
    b.tags, b.ok = torch.zeros((n, 16), dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
    return b


def test_an_empty_batch_and_the_iv_shape():
    b = MK.GcmMkBatch([], [bytes(32)], key_index=[])
    assert b.n == 0 and b.nkeys == 1 and b.nr == 14
    # a wrong IV shape is a ValueError whatever else holds
    for bad in (torch.zeros((0, 8), dtype=torch.uint8), torch.zeros((2, 16), dtype=torch.uint8),
                torch.zeros(24, dtype=torch.uint8), [bytes(12)] * 2, None):
        with pytest.raises(ValueError):
            b.encrypt(bad)
        with pytest.raises(ValueError):
            planned().encrypt(bad)


def test_rekey_keeps_the_count_and_the_size():
    b = MK.GcmMkBatch([], [bytes(16), bytes(16)], key_index=[])
    b.rekey([bytes([1]) * 16, bytes([2]) * 16])  # an empty batch: nothing to upload
    for keys in ([bytes(16)], [bytes(32), bytes(32)], [bytes(16), bytes(24)]):
        with pytest.raises(ValueError):
            b.rekey(keys)


def test_the_new_functions_are_declared():
    src = open(os.path.join(ROOT, "our_tree_amd", "_native.py")).read()
    declared = set(re.findall(r'"(otc_\w+)": \(', src))
    names = {"otc_gcm_mk_batch_plan", "otc_gcm_mk_batch_table_bytes", "otc_gcm_mk_batch_tables", "otc_gcm_mk_batch_ws_bytes",
             "otc_gcm_mk_batch_lanes", "otc_gcm_mk_batch_spans", "otc_ghash_mk_batch", "otc_aes_gcm_mk_batch"}
    assert names <= declared
    hdr = open(os.path.join(ROOT, "csrc", "include", "otc.h")).read()
    for name in names | {"otc_gcm_mk_msg"}:
        assert name in hdr
    assert "many-key batches are out of scope" not in hdr and "otc_aes_gcm_mk_batch" in hdr[:hdr.index("} otc_gcm_msg;")]


def test_the_batch_oracle_is_a_loop_over_the_single_message_one():
    keys = [bytes(range(32)), bytes(range(1, 33))]
    ivs = [bytes([i] * 12) for i in range(3)]
    datas, aads = [b"", b"x" * 17, bytes(range(100))], [b"a", b"", b"header"]
    got = cpu_ref.gcm_mk_batch(keys, [1, 0, 1], ivs, datas, aads)
    assert got == [cpu_ref.gcm(keys[k], v, d, a) for k, v, d, a in zip([1, 0, 1], ivs, datas, aads)]
    back = cpu_ref.gcm_mk_batch(keys, [1, 0, 1], ivs, [c for c, _ in got], aads, decrypt=True)
    assert [p for p, _ in back] == datas and [t for _, t in back] == [t for _, t in got]
    assert cpu_ref.gcm_mk_batch(keys, None, ivs[:2], datas[:2]) == [cpu_ref.gcm(keys[i], ivs[i], datas[i]) for i in range(2)]
    with pytest.raises(ValueError, match="out of range"):
        cpu_ref.gcm_mk_batch(keys, [2], ivs[:1], datas[:1])
    with pytest.raises(ValueError, match="one key index"):
        cpu_ref.gcm_mk_batch(keys, [0, 1], ivs, datas)
