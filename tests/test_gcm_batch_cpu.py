"""Batched AES-GCM without a GPU: the host planner (otc_gcm_batch_plan)
against a pure-Python recount, and the argument checks of otc_ghash_batch /
otc_aes_gcm_batch, which must answer OTC_ERR_ARG with a message *before* any
HIP call -- the device addresses below are fake and never dereferenced."""
import ctypes
import os
import re

import numpy as np
import pytest

from our_tree_amd import _native

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


def gkey(lib, nbytes=16):
    k = _native.OtcGcmKey()
    assert lib.otc_gcm_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(nbytes))), nbytes * 8) == 0
    return k


def descs(rows):
    """rows of (in, out, nbytes, aad, aad_bytes) -> otc_gcm_msg[] as uint64 [n, 6]"""
    d = np.zeros((len(rows), 6), dtype=np.uint64)
    for i, r in enumerate(rows):
        d[i, :5] = r
    return d


def plan(lib, d, tile_blocks=256, fill=True):
    n = d.shape[0]
    nt = lib.otc_gcm_batch_plan(d.ctypes.data, n, tile_blocks, None, None, None)
    if nt < 0 or not fill:
        return nt, None, None, None
    ctr = np.full((n, 6), 0xEE, dtype=np.uint64)
    first = np.zeros(n, dtype=np.uint64)
    tmap = np.zeros(max(nt, 1), dtype=np.uint32)
    assert lib.otc_gcm_batch_plan(d.ctypes.data, n, tile_blocks, ctr.ctypes.data, tmap.ctypes.data,
                                  first.ctypes.data) == nt
    return nt, ctr, tmap[:nt], first


# ---- the planner ----------------------------------------------------------------
LENS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 0, 65541, MAX_BYTES, 5]


@pytest.mark.parametrize("tile_blocks", [64, 128, 256])
def test_planner_matches_a_python_recount(lib, tile_blocks):
    rows, at = [], A
    for i, n in enumerate(LENS):
        inplace = i % 2 == 0
        rows.append((at, at if inplace else at + (8 << 20), n, A + (32 << 20) + 3 + i, (i * 7) % 40))
        at += (n + 15) // 16 * 16
    d = descs(rows)
    nt, ctr, tmap, first = plan(lib, d, tile_blocks)
    tb = 16 * tile_blocks
    tiles = [(n + tb - 1) // tb for n in LENS]
    assert nt == sum(tiles)
    want_first = np.cumsum([0] + tiles[:-1])
    assert first.tolist() == want_first.tolist()
    assert tmap.tolist() == [m for m, t in enumerate(tiles) for _ in range(t)]
    for m, n in enumerate(LENS):
        if n == 0:
            assert tiles[m] == 0 and m not in tmap  # zero-length records have no tiles
    # the CTR half's descriptors: buffers and lengths copied, counters left zero, key 0, no alignment word
    assert (ctr[:, :3] == d[:, :3]).all() and (ctr[:, 3:] == 0).all()


def test_planner_counts_without_output_arrays(lib):
    d = descs([(A, A, 4097, 0, 0), (A + 8192, A + 8192, 0, 0, 0)])
    assert plan(lib, d, 256, fill=False)[0] == 2
    assert lib.otc_gcm_batch_plan(None, 0, 256, None, None, None) == 0


@pytest.mark.parametrize("row,what", [
    ((A, A, MAX_BYTES + 1, 0, 0), "1 MiB"),
    ((A, A, 16, A + 4096, MAX_AAD + 1), "64 KiB"),
    ((A, A, 0, 0, 5), "null aad"),
    ((A + 4, A + 4096, 64, 0, 0), "aligned"),
    ((A, A + 4096 + 8, 64, 0, 0), "aligned"),
    ((0, A, 64, 0, 0), "null"),
    ((A, A + 16, 64, 0, 0), "overlap partially"),
    ((A + 32, A, 64, 0, 0), "overlap partially"),
])
def test_planner_rejects_a_bad_record(lib, row, what):
    good = (A + (1 << 24), A + (1 << 24), 100, 0, 0)
    nt = plan(lib, descs([good, row]), 256)[0]
    assert nt == ERR_ARG and what in err(lib) and "record 1" in err(lib), err(lib)


def test_planner_accepts_the_caps(lib):
    d = descs([(A, A, MAX_BYTES, A + (4 << 20) + 1, MAX_AAD)])
    assert plan(lib, d, 256, fill=False)[0] == MAX_BYTES // 4096


def test_planner_rejects_records_that_overlap(lib):
    B = A + (1 << 24)
    # two outputs share bytes
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 96, 100, 0, 0)]))[0] == ERR_ARG
    assert "overlaps another record" in err(lib)
    # record 1 reads what record 0 writes
    assert plan(lib, descs([(A, B, 100, 0, 0), (B + 64, B + 4096, 100, 0, 0)]))[0] == ERR_ARG
    assert "overlaps another record" in err(lib)
    # an AAD inside an output -- its own record's or another's -- would be overwritten before it is hashed
    assert plan(lib, descs([(A, B, 100, B + 50, 13)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, A, 100, A + 99, 1)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 4096, 100, B - 3, 4)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "AAD overlaps" in err(lib)
    # next to an output, or inside an out-of-place record's input, it is fine
    assert plan(lib, descs([(A, B, 100, B + 100, 13), (A + 4096, B + 4096, 100, B - 4, 4), (A + 8192, B + 8192, 64, A + 8192, 64)]),
                fill=False)[0] == 3
    # back to back is fine, and so are empty records anywhere
    assert plan(lib, descs([(A, B, 112, 0, 0), (A + 112, B + 112, 100, 0, 0), (A, B, 0, 0, 0)]), fill=False)[0] == 2


def test_planner_rejects_bad_tile_blocks(lib):
    assert plan(lib, descs([(A, A, 64, 0, 0)]), 100)[0] == ERR_ARG and "tile_blocks" in err(lib)


# ---- entry points ---------------------------------------------------------------
def gcm_batch(lib, k, **kw):
    a = dict(msgs=A, ctr=A + 0x1000, tmap=A + 0x2000, first=A + 0x3000, ntiles=4, tile_blocks=256, nmsg=4,
             key=ctypes.byref(k), key_dev=A + 0x4000, tab=A + 0x10000, dir=ENC, ivs=A + 0x5000, tags=A + 0x6000,
             expect=None, tag_bytes=16, ok=None, ws=A + 0x7000, lanes=16)
    a.update(kw)
    return lib.otc_aes_gcm_batch(a["msgs"], a["ctr"], a["tmap"], a["first"], a["ntiles"], a["tile_blocks"], a["nmsg"],
                                 a["key"], a["key_dev"], a["tab"], a["dir"], a["ivs"], a["tags"], a["expect"],
                                 a["tag_bytes"], a["ok"], a["ws"], a["lanes"], None)


@pytest.mark.parametrize("kw,what", [
    (dict(msgs=None), "null"),
    (dict(ctr=None), "null"),
    (dict(tmap=None), "null"),
    (dict(first=None), "null"),
    (dict(key_dev=None), "null"),
    (dict(tab=None), "null"),
    (dict(ivs=None), "null IVs"),
    (dict(tags=None), "null"),
    (dict(ws=None), "null"),
    (dict(key=None), "null key"),
    (dict(msgs=A + 4), "misaligned"),
    (dict(ctr=A + 0x1004), "misaligned"),
    (dict(first=A + 0x3004), "misaligned"),
    (dict(tmap=A + 0x2002), "misaligned"),
    (dict(tab=A + 0x10008), "16-byte aligned"),
    (dict(tags=A + 0x6004), "16-byte aligned"),
    (dict(ws=A + 0x7008), "16-byte aligned"),
    (dict(tag_bytes=3), "4 to 16"),
    (dict(tag_bytes=17), "4 to 16"),
    (dict(dir=2), "direction"),
    (dict(tile_blocks=100), "tile_blocks"),
    (dict(lanes=32), "lanes"),
    (dict(lanes=-1), "lanes"),
    (dict(dir=DEC), "decryption needs"),
    (dict(dir=DEC, expect=A + 0x8000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000), "expected tags overlap"),             # the tag array itself
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 + 63), "expected tags overlap"),        # its last byte
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 - 15, tag_bytes=4), "expected tags overlap"),   # 4 x 4 bytes reach its first
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 - 63), "expected tags overlap"),        # the verdicts
])
def test_gcm_batch_rejects_bad_arguments(lib, kw, what):
    assert gcm_batch(lib, gkey(lib), **kw) == ERR_ARG and what in err(lib), err(lib)


def test_gcm_batch_accepts_expected_tags_next_to_its_own(lib):
    """Adjacent is not overlapping: the checks above do not fire, and the next one in line does."""
    k = gkey(lib)
    for exp, tb in ((A + 0x6000 + 64, 16), (A + 0x6000 - 16, 4), (A + 0x9000 + 4, 16)):
        assert gcm_batch(lib, k, dir=DEC, ok=A + 0x9000, expect=exp, tag_bytes=tb, ivs=None) == ERR_ARG
        assert "null IVs" in err(lib)


def test_gcm_batch_rejects_a_decryption_schedule(lib):
    k = gkey(lib)
    k.enc.dir = DEC
    assert gcm_batch(lib, k) == ERR_ARG and "encryption schedule" in err(lib)


@pytest.mark.parametrize("args,what", [
    ((None, 4, A + 0x10000, A + 0x6000), "null"),
    ((A, 4, None, A + 0x6000), "null"),
    ((A, 4, A + 0x10000, None), "null"),
    ((A + 4, 4, A + 0x10000, A + 0x6000), "misaligned"),
    ((A, 4, A + 0x10008, A + 0x6000), "16-byte aligned"),
    ((A, 4, A + 0x10000, A + 0x6008), "16-byte aligned"),
])
def test_ghash_batch_rejects_bad_arguments(lib, args, what):
    assert lib.otc_ghash_batch(*args, 64, None) == ERR_ARG and what in err(lib), err(lib)
    assert lib.otc_ghash_batch(A, 4, A + 0x10000, A + 0x6000, 17, None) == ERR_ARG and "lanes" in err(lib)


def test_tables_reject_bad_arguments(lib):
    k = gkey(lib)
    assert lib.otc_gcm_batch_tables(None, A, None) == ERR_ARG and "null key" in err(lib)
    assert lib.otc_gcm_batch_tables(ctypes.byref(k), None, None) == ERR_ARG and "16-byte aligned" in err(lib)
    assert lib.otc_gcm_batch_tables(ctypes.byref(k), A + 8, None) == ERR_ARG and "16-byte aligned" in err(lib)


def test_an_empty_batch_launches_nothing(lib):
    k = gkey(lib, 32)
    assert gcm_batch(lib, k, nmsg=0, ntiles=0, msgs=None, ctr=None, tmap=None, first=None, ivs=None, tags=None,
                     ws=None, tab=None, key_dev=None) == 0
    assert gcm_batch(lib, k, nmsg=0, ntiles=0, dir=DEC) == 0
    assert lib.otc_ghash_batch(None, 0, None, None, 0, None) == 0


# ---- what the kernel reports about itself -----------------------------------------
def test_spans_are_positive_and_increasing(lib):
    buf = (ctypes.c_uint64 * 16)()
    n = lib.otc_gcm_batch_spans(buf, 16)
    spans = [int(v) for v in buf[:n]]
    assert n >= 1 and spans[0] == 16  # at least the pass: one block per lane of the 16-lane form
    assert 64 in spans                # and the 64-lane form's
    assert all(s > 0 for s in spans) and all(a < b for a, b in zip(spans, spans[1:]))
    assert lib.otc_gcm_batch_spans(None, 0) == n
    one = (ctypes.c_uint64 * 2)(0, 0xDEAD)
    assert lib.otc_gcm_batch_spans(one, 1) == n and one[0] == 16 and one[1] == 0xDEAD  # max is honoured


def test_table_and_workspace_bytes(lib):
    assert lib.otc_gcm_batch_table_bytes() == 3 * 64 * 1024  # H^16, H^64 and H, 16 x 256 x 16 B each
    assert lib.otc_gcm_batch_ws_bytes(0) == 0 and lib.otc_gcm_batch_ws_bytes(1000) == 32 * 1000  # J0[], E_K(J0)[]


def test_lanes_follow_the_record_sizes(lib):
    """64 lanes per record when the records hash more than 768 blocks on average
    (AAD blocks + data blocks + the length block) or one more than 4096, else 16."""
    lanes = lambda rows: lib.otc_gcm_batch_lanes(descs(rows).ctypes.data, len(rows))
    assert lanes([(A, A, 4096, 0, 0)] * 8) == 16
    assert lanes([(A, A, 16 * 767, 0, 0)]) == 16          # 768 blocks with the length block
    assert lanes([(A, A, 16 * 767 + 1, 0, 0)]) == 64      # 769
    assert lanes([(A, A, 16 * 766, A, 1)]) == 16          # the AAD block counts: 768
    assert lanes([(A, A, 16 * 766 + 1, A, 16)]) == 64
    assert lanes([(A, A, 8192, A, 13)] * 4) == 16 and lanes([(A, A, 16384, A, 13)] * 4) == 64   # the measured shapes
    assert lanes([(A, A, 16384, 0, 0), (A, A, 0, 0, 0), (A, A, 0, A, 13)]) == 16   # the mean, not the longest ...
    assert lanes([(A, A, 64, 0, 0)] * 50 + [(A, A, 16 * 4095, 0, 0)]) == 16        # ... up to 4096 blocks
    assert lanes([(A, A, 64, 0, 0)] * 50 + [(A, A, 16 * 4095 + 1, 0, 0)]) == 64
    assert lib.otc_gcm_batch_lanes(None, 0) == 16


def test_the_new_functions_are_declared():
    src = open(os.path.join(ROOT, "our_tree_amd", "_native.py")).read()
    declared = set(re.findall(r'"(otc_\w+)": \(', src))
    assert {"otc_gcm_batch_spans", "otc_gcm_batch_table_bytes", "otc_gcm_batch_ws_bytes", "otc_gcm_batch_tables",
            "otc_gcm_batch_plan", "otc_gcm_batch_lanes", "otc_ghash_batch", "otc_aes_gcm_batch"} <= declared
    # pointers as pointers, sizes as 64-bit: the planner's result is an int64 (a tile count or an error)
    assert re.search(r'"otc_gcm_batch_plan": \(ctypes\.c_int64, \[c_vp, c_sz, c_int, c_vp, c_vp, c_vp\]\)', src)
