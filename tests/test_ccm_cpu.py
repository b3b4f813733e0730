"""AES-CCM (NIST SP 800-38C, RFC 3610) without a GPU: the C oracle
(csrc/cpu/aes.c) against the golden vectors and against a pure-Python CCM
written here over the oracle's ECB, its tamper handling and refusals; the host
planner (otc_ccm_batch_plan) and the argument checks of otc_aes_ccm_batch --
which must answer OTC_ERR_ARG with a message *before* any HIP call: the device
addresses below are fake and never dereferenced --, and the Python layer's
checks."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref
from our_tree_amd.models.aes import AES
from our_tree_amd.models.cpu_ref import CcmTagError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ccm_vectors.json")) as f:
    VEC = json.load(f)
H = bytes.fromhex
CB = ops.ccm_batch_ops

ERR_ARG = -1
ENC, DEC = 1, 0
A = 0x7F0000000000  # fake, 16-byte aligned device addresses (never touched)
MAX_BYTES, MAX_AAD = 1 << 20, 1 << 16


def count(n):
    return bytes(i & 255 for i in range(n))


def fields(v):
    """(key, nonce, aad, pt, ct or None, ct_tail or None, tag) of a golden vector"""
    aad = count(v["aad_count"]) if "aad_count" in v else H(v["aad"])
    pt = count(v["pt_count"]) if "pt_count" in v else H(v["pt"])
    return (H(v["key"]), H(v["nonce"]), aad, pt, H(v["ct"]) if "ct" in v else None,
            H(v["ct_tail"]) if "ct_tail" in v else None, H(v["tag"]))


ALL_VECTORS = VEC["published"] + VEC["cross_checks"]


# ---- the golden vectors ---------------------------------------------------------
def test_golden_says_what_is_published():
    assert "NOT published" in VEC["about"] and "SP 800-38C" in VEC["about"] and "RFC 3610" in VEC["about"]
    assert len(VEC["published"]) == 5 and len(VEC["cross_checks"]) == 7
    assert {len(H(v["key"])) for v in ALL_VECTORS} == {16, 24, 32}
    assert {len(H(v["tag"])) for v in VEC["published"]} == {4, 6, 8, 14}
    assert {v.get("aad_count") for v in ALL_VECTORS} >= {65279, 65280, 65536}


@pytest.mark.parametrize("v", ALL_VECTORS, ids=[v["name"] for v in ALL_VECTORS])
def test_vector_both_directions(v):
    key, nonce, aad, pt, ct, tail, tag = fields(v)
    c, t = cpu_ref.ccm(key, nonce, pt, aad, tag_bytes=len(tag))
    assert t == tag and len(c) == len(pt)
    if ct is not None:
        assert c == ct
    if tail is not None:
        assert c[-len(tail):] == tail
    p, t2 = cpu_ref.ccm(key, nonce, c, aad, decrypt=True, tag_bytes=len(tag))
    assert p == pt and t2 == tag
    assert cpu_ref.ccm_auth_decrypt(key, nonce, c, tag, aad) == pt


# ---- a pure-Python CCM over the oracle's ECB --------------------------------------
def py_ccm(key, nonce, pt, aad, m):
    """SP 800-38C appendix A, byte by byte: (ciphertext, tag)"""
    ell = 15 - len(nonce)
    E = lambda b: cpu_ref.ecb(key, bytes(b))
    xor = lambda a, b: bytes(x ^ y for x, y in zip(a, b))
    b0 = bytes([64 * (len(aad) > 0) + 8 * ((m - 2) // 2) + (ell - 1)]) + nonce + len(pt).to_bytes(ell, "big")
    stream = b""
    if aad:
        enc = len(aad).to_bytes(2, "big") if len(aad) < 0xFF00 else b"\xff\xfe" + len(aad).to_bytes(4, "big")
        stream = enc + aad
        stream += bytes(-len(stream) % 16)
    stream += pt + bytes(-len(pt) % 16)
    x = E(b0)
    for i in range(0, len(stream), 16):
        x = E(xor(x, stream[i:i + 16]))
    a = lambda i: bytes([ell - 1]) + nonce + i.to_bytes(ell, "big")
    ct = b"".join(xor(pt[i:i + 16], E(a(i // 16 + 1))) for i in range(0, len(pt), 16))
    return ct, xor(x, E(a(0)))[:m]


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_oracle_against_the_python_ccm(bits):
    rng = random.Random(bits)
    key = rng.randbytes(bits // 8)
    cases = [(nl, m) for nl in cpu_ref.CCM_NONCE_BYTES for m in cpu_ref.CCM_TAG_BYTES]
    assert len(cases) == 49
    for nl, m in cases:
        n, alen = rng.randint(0, 600), rng.choice([0, 0, 1, 13, 14, 15, 16, 30, rng.randint(0, 300)])
        nonce, pt, aad = rng.randbytes(nl), rng.randbytes(n), rng.randbytes(alen)
        want = py_ccm(key, nonce, pt, aad, m)
        assert cpu_ref.ccm(key, nonce, pt, aad, tag_bytes=m) == want, (nl, m, n, alen)
        assert cpu_ref.ccm(key, nonce, want[0], aad, decrypt=True, tag_bytes=m) == (pt, want[1])
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 600):  # the block edges under one shape
        nonce, pt = rng.randbytes(12), rng.randbytes(n)
        assert cpu_ref.ccm(key, nonce, pt, b"hdr", tag_bytes=16) == py_ccm(key, nonce, pt, b"hdr", 16)


def test_python_ccm_agrees_with_a_published_vector():
    """The model above is checked too, not only trusted."""
    key, nonce, aad, pt, ct, _, tag = fields(VEC["published"][2])
    assert py_ccm(key, nonce, pt, aad, len(tag)) == (ct, tag)


def test_in_place_is_exact():
    lib = _native.cpu_lib()
    key, nonce, aad = bytes(range(16)), bytes(range(12)), b"in place"
    pt = random.Random(5).randbytes(333)
    want = cpu_ref.ccm(key, nonce, pt, aad)
    ctx = cpu_ref._ctx(key)
    buf = (ctypes.c_uint8 * len(pt)).from_buffer_copy(pt)
    tag = (ctypes.c_uint8 * 16)()
    assert lib.aes_crypt_ccm(ctypes.byref(ctx), 1, len(pt), _native.as_u8p(nonce), 12, _native.as_u8p(aad), len(aad),
                             buf, buf, tag, 16) == 0
    assert (bytes(buf), bytes(tag)) == want


# ---- tampering ------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 16])
@pytest.mark.parametrize("what", ["ciphertext", "tag", "aad", "nonce"])
def test_auth_decrypt_fails_and_zeroes(what, m):
    key, nonce, aad = bytes(range(32)), bytes(range(13)), bytes(range(20))
    pt = random.Random(m).randbytes(100)
    ct, tag = cpu_ref.ccm(key, nonce, pt, aad, tag_bytes=m)
    assert cpu_ref.ccm_auth_decrypt(key, nonce, ct, tag, aad) == pt
    flip = lambda b, i, bit=1: b[:i] + bytes([b[i] ^ bit]) + b[i + 1:]
    if what == "ciphertext":
        ct = flip(ct, 57, 0x10)
    elif what == "tag":
        tag = flip(tag, m - 1, 0x80)
    elif what == "aad":
        aad = flip(aad, 3)
    else:
        nonce = flip(nonce, 12)
    with pytest.raises(CcmTagError) as e:
        cpu_ref.ccm_auth_decrypt(key, nonce, ct, tag, aad)
    assert e.value.output == bytes(100)  # zeroed by the C side, not left at the wrapper's 0xA5 fill
    assert issubclass(CcmTagError, ValueError)


# ---- refusals -------------------------------------------------------------------
def c_ccm(nonce_len, tag_len, length, aad_len=0):
    lib = _native.cpu_lib()
    ctx = cpu_ref._ctx(bytes(16))
    buf = (ctypes.c_uint8 * max(length, 1))()
    tag = (ctypes.c_uint8 * 16)()
    return lib.aes_crypt_ccm(ctypes.byref(ctx), 1, length, _native.as_u8p(bytes(16)), nonce_len,
                             _native.as_u8p(bytes(max(aad_len, 1))), aad_len, buf, buf, tag, tag_len)


@pytest.mark.parametrize("nl", [6, 14, 0, 16])
def test_nonce_lengths_refused(nl):
    assert c_ccm(nl, 16, 10) != 0
    with pytest.raises(ValueError, match="7 to 13"):
        cpu_ref.ccm(bytes(16), bytes(nl), b"x")
    with pytest.raises(ValueError, match="7 to 13"):
        cpu_ref.ccm_auth_decrypt(bytes(16), bytes(nl), b"x", bytes(16))


@pytest.mark.parametrize("m", [2, 3, 5, 18, 0, 15])
def test_tag_lengths_refused(m):
    assert c_ccm(12, m, 10) != 0
    with pytest.raises(ValueError, match="4, 6, 8"):
        cpu_ref.ccm(bytes(16), bytes(12), b"x", tag_bytes=m)
    with pytest.raises(ValueError, match="4, 6, 8"):
        cpu_ref.ccm_auth_decrypt(bytes(16), bytes(12), b"x", bytes(m))


def test_length_must_fit_the_length_field():
    """L = 15 - nonce length bytes: with a 13-byte nonce 65535 bytes pass and 65536 do not."""
    assert c_ccm(13, 16, 65535) == 0 and c_ccm(13, 16, 65536) != 0
    assert c_ccm(12, 16, 65536) == 0
    cpu_ref.ccm_check(13, 16, 65535)
    with pytest.raises(ValueError, match="fewer than"):
        cpu_ref.ccm_check(13, 16, 65536)
    with pytest.raises(ValueError, match="fewer than"):
        cpu_ref.ccm(bytes(16), bytes(13), bytes(65536))
    with pytest.raises(ValueError, match="fewer than"):
        cpu_ref.ccm_check(12, 16, 1 << 24)
    cpu_ref.ccm_check(7, 16, 1 << 40)


def test_the_batch_oracle_is_a_loop_over_the_single_message_one():
    key = bytes(range(32))
    nonces = [bytes([i] * 11) for i in range(3)]
    datas, aads = [b"", b"x" * 17, bytes(range(100))], [b"a", b"", b"header"]
    got = cpu_ref.ccm_batch(key, nonces, datas, aads, tag_bytes=8)
    assert got == [cpu_ref.ccm(key, n, d, a, tag_bytes=8) for n, d, a in zip(nonces, datas, aads)]
    back = cpu_ref.ccm_batch(key, nonces, [c for c, _ in got], aads, decrypt=True, tag_bytes=8)
    assert [p for p, _ in back] == datas and [t for _, t in back] == [t for _, t in got]
    with pytest.raises(ValueError, match="one nonce length"):
        cpu_ref.ccm_batch(key, [bytes(11), bytes(12)], [b"", b""])
    with pytest.raises(ValueError, match="one nonce"):
        cpu_ref.ccm_batch(key, nonces, datas[:2])


# ---- the planner ----------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _native.require_gpu_lib()


@pytest.fixture(scope="module")
def key(lib):
    return ops.expand_key(bytes(range(16)))


def err(lib) -> str:
    return lib.otc_last_error().decode()


def descs(rows):
    """rows of (in, out, nbytes, aad, aad_bytes) -> otc_ccm_msg[] as uint64 [n, 6]"""
    d = np.zeros((len(rows), 6), dtype=np.uint64)
    for i, r in enumerate(rows):
        d[i, :len(r)] = r
    return d


def plan(lib, d, nonce_len=12, fill=True):
    n = d.shape[0]
    order = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    rc = lib.otc_ccm_batch_plan(d.ctypes.data, n, nonce_len, order.ctypes.data if fill else None)
    return rc, order


def test_planner_orders_by_block_count_longest_first(lib):
    lens = [0, 1, 1024, 15, 1040, 0, 16, 4097, 64, 17, 32, 4097, 1025]
    rows, at = [], A
    for i, n in enumerate(lens):
        rows.append((at, at if i % 2 else at + (8 << 20), n, A + (32 << 20) + 3 + 64 * i, (i * 7) % 40))
        at += (n + 15) // 16 * 16
    rc, order = plan(lib, descs(rows))
    assert rc == 0
    blocks = [(n + 15) // 16 for n in lens]
    # a stable sort, descending: records of one block count keep their order
    assert order.tolist() == sorted(range(len(lens)), key=lambda m: -blocks[m])
    assert order.tolist()[:2] == [7, 11] and sorted(order.tolist()) == list(range(len(lens)))


def test_planner_checks_without_an_order_array(lib):
    d = descs([(A, A, 1040, 0, 0), (A + 8192, A + 8192, 0, 0, 0)])
    assert plan(lib, d, fill=False)[0] == 0
    assert lib.otc_ccm_batch_plan(None, 0, 12, None) == 0
    assert lib.otc_ccm_batch_plan(None, 3, 12, None) == ERR_ARG and "null descriptors" in err(lib)


@pytest.mark.parametrize("row,what", [
    ((A, A, MAX_BYTES + 1, 0, 0), "1 MiB"),
    ((A, A, 16, A + 4096, MAX_AAD + 1), "64 KiB"),
    ((A, A, 0, 0, 5), "null aad"),
    ((0, A, 64, 0, 0), "null buffer"),
    ((A, 0, 64, 0, 0), "null buffer"),
    ((0, A, 5, 0, 0), "null buffer"),
    ((A + 4, A + 4096, 64, 0, 0), "aligned"),
    ((A, A + 4096 + 8, 64, 0, 0), "aligned"),
    ((A, A + 16, 64, 0, 0), "overlap partially"),
    ((A + 32, A, 64, 0, 0), "overlap partially"),
])
def test_planner_rejects_a_bad_record(lib, row, what):
    good = (A + (1 << 24), A + (1 << 24), 100, 0, 0)
    rc = plan(lib, descs([good, row]))[0]
    assert rc == ERR_ARG and what in err(lib) and "ccm_batch: record 1: " in err(lib), err(lib)


def test_planner_checks_the_length_field(lib):
    """nbytes < 2^(8 L): under a 13-byte nonce 65535 bytes pass and 65536 do not."""
    assert plan(lib, descs([(A, A, 65535, 0, 0)]), nonce_len=13)[0] == 0
    assert plan(lib, descs([(A, A, 100, 0, 0), (A + 4096, A + 4096, 65536, 0, 0)]), nonce_len=13)[0] == ERR_ARG
    assert "record 1" in err(lib) and "length field" in err(lib)
    assert plan(lib, descs([(A, A, 65536, 0, 0)]), nonce_len=12)[0] == 0
    for nl in range(7, 13):
        assert plan(lib, descs([(A, A, MAX_BYTES, A + (4 << 20) + 1, MAX_AAD)]), nonce_len=nl)[0] == 0  # the caps
    for nl in (6, 14, 0, -1):
        assert plan(lib, descs([(A, A, 16, 0, 0)]), nonce_len=nl)[0] == ERR_ARG and "7 to 13" in err(lib)


def test_planner_rejects_records_that_overlap(lib):
    B = A + (1 << 24)
    assert plan(lib, descs([(A, B, 100, 0, 0), (A + 4096, B + 96, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "output overlaps another record" in err(lib)
    assert plan(lib, descs([(A, B, 100, 0, 0), (B + 64, B + 4096, 100, 0, 0)]))[0] == ERR_ARG
    assert "record 1" in err(lib) and "input overlaps another record's output" in err(lib)
    assert plan(lib, descs([(A, B, 100, B + 50, 13)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, A, 100, A + 99, 1)]))[0] == ERR_ARG and "AAD overlaps" in err(lib)
    assert plan(lib, descs([(A, B, 100, B + 100, 13), (A + 4096, B + 4096, 100, B - 4, 4),
                            (A + 8192, B + 8192, 64, A + 8192, 64), (A, B, 0, 0, 0)]))[0] == 0


# ---- what the kernel reports about itself ------------------------------------------
def test_ws_bytes(lib):
    """The AAD is chained in the records' kernel: no workspace."""
    assert lib.otc_ccm_batch_ws_bytes(0) == 0 and lib.otc_ccm_batch_ws_bytes(1000) == 0


def test_spans(lib):
    buf = (ctypes.c_uint64 * 16)()
    n = lib.otc_ccm_batch_spans(buf, 16)
    spans = [int(v) for v in buf[:n]]
    # bytes: a block, a burst; records: a wave, a workgroup, the grid's first step
    assert n == 5 and spans[:4] == [16, 128, 64, 1024]
    assert spans[4] % 1024 == 0 and spans[4] >= 1024
    assert lib.otc_ccm_batch_spans(None, 0) == n
    one = (ctypes.c_uint64 * 2)(0, 0xDEAD)
    assert lib.otc_ccm_batch_spans(one, 1) == n and one[0] == spans[0] and one[1] == 0xDEAD  # max is honoured
    assert CB.CcmBatch.spans() == spans == CB.ccm_batch_spans()


# ---- the run entry point --------------------------------------------------------
def aead_batch(lib, k, **kw):
    a = dict(msgs=A, order=A + 0x2000, nmsg=4, key=ctypes.byref(k), dir=ENC, nonces=A + 0x5000, nonce_len=12,
             tags=A + 0x6000, tag_len=16, expect=None, ok=None, ws=None)
    a.update(kw)
    return lib.otc_aes_ccm_batch(a["msgs"], a["order"], a["nmsg"], a["key"], a["dir"], a["nonces"], a["nonce_len"],
                                 a["tags"], a["tag_len"], a["expect"], a["ok"], a["ws"], None)


@pytest.mark.parametrize("kw,what", [
    (dict(msgs=None), "null"),
    (dict(order=None), "null"),
    (dict(key=None), "null key"),
    (dict(nonces=None), "null nonces"),
    (dict(tags=None), "null"),
    (dict(msgs=A + 4), "misaligned"),
    (dict(order=A + 0x2002), "misaligned"),
    (dict(dir=2), "direction"),
    (dict(dir=-1), "direction"),
    (dict(nonce_len=6), "7 to 13"),
    (dict(nonce_len=14), "7 to 13"),
    (dict(tag_len=2), "4, 6, 8"),
    (dict(tag_len=5), "4, 6, 8"),
    (dict(tag_len=18), "4, 6, 8"),
    (dict(dir=DEC), "decryption needs"),
    (dict(dir=DEC, expect=A + 0x8000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000), "decryption needs"),
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000), "expected tags overlap"),        # the tag array itself
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 + 63), "expected tags overlap"),   # its last byte
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x6000 - 63), "expected tags overlap"),   # its first
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 - 63), "expected tags overlap"),   # the verdicts
    (dict(dir=DEC, ok=A + 0x9000, expect=A + 0x9000 + 3), "expected tags overlap"),
    (dict(dir=DEC, tag_len=4, ok=A + 0x9000, expect=A + 0x6000 + 15), "expected tags overlap"),  # 4 x 4 bytes of tags
])
def test_aead_batch_rejects_bad_arguments(lib, key, kw, what):
    assert aead_batch(lib, key, **kw) == ERR_ARG and what in err(lib), err(lib)


def test_aead_batch_wants_the_encryption_schedule(lib):
    assert aead_batch(lib, ops.expand_key(bytes(range(16)), decrypt=True)) == ERR_ARG
    assert aead_batch(lib, _native.OtcAesKey()) == ERR_ARG  # never initialised


def test_aead_batch_accepts_expected_tags_next_to_its_own(lib, key):
    """Adjacent is not overlapping: the checks above do not fire, and the next one in line does."""
    for exp in (A + 0x6000 + 64, A + 0x6000 - 64, A + 0x9000 + 4):
        assert aead_batch(lib, key, dir=DEC, ok=A + 0x9000, expect=exp, nonces=None) == ERR_ARG
        assert "null nonces" in err(lib)
    assert aead_batch(lib, key, dir=DEC, tag_len=4, ok=A + 0x9000, expect=A + 0x6000 + 16, nonces=None) == ERR_ARG
    assert "null nonces" in err(lib)


def test_an_empty_batch_launches_nothing(lib, key):
    assert aead_batch(lib, key, nmsg=0, msgs=None, order=None, nonces=None, tags=None) == 0
    assert aead_batch(lib, key, nmsg=0, dir=DEC) == 0
    assert aead_batch(lib, key, nmsg=0, dir=7) == ERR_ARG  # the direction is checked even then
    assert aead_batch(lib, key, nmsg=0, key=None) == ERR_ARG  # and the key
    assert aead_batch(lib, key, nmsg=0, tag_len=7) == ERR_ARG  # and the lengths


# ---- the Python layer -----------------------------------------------------------
def test_the_module_is_reachable_but_not_exported():
    for name in ("CcmBatch", "ccm_encrypt_batch", "ccm_decrypt_batch", "ccm_batch_spans", "ccm_encrypt", "ccm_decrypt"):
        assert hasattr(CB, name) and name not in ops.__all__
    assert hasattr(AES, "ccm_encrypt_batch") and hasattr(AES, "ccm_decrypt_batch")
    assert hasattr(CB.CcmBatch, "packed") and hasattr(CB.CcmBatch, "spans")
    assert CB.CcmTagError is cpu_ref.CcmTagError
    for f in (CB.ccm_encrypt, CB.ccm_decrypt):
        assert "one serial" in f.__doc__ and "1 MiB" in f.__doc__
    assert "uniqueness" in CB.CcmBatch.__doc__


@pytest.mark.parametrize("k", [bytes(15), bytes(17), bytes(33), b""])
def test_a_key_has_16_24_or_32_bytes(k):
    with pytest.raises(ValueError, match="16, 24 or 32"):
        CB.CcmBatch([], k)


def test_the_batchs_lengths_are_checked():
    for nb in (6, 14, "12", None):
        with pytest.raises(ValueError, match="7 to 13"):
            CB.CcmBatch([], bytes(16), nonce_bytes=nb)
    for tb in (2, 3, 5, 18, 16.0):
        with pytest.raises(ValueError, match="4, 6, 8"):
            CB.CcmBatch([], bytes(16), tag_bytes=tb)


def test_an_empty_batch_needs_no_device(lib):
    b = CB.CcmBatch([], bytes(24), nonce_bytes=13, tag_bytes=8)
    n0, t0 = torch.zeros((0, 13), dtype=torch.uint8), torch.zeros((0, 8), dtype=torch.uint8)
    outs, tags = b.encrypt(n0)
    assert outs == [] and tuple(tags.shape) == (0, 8) and tags.dtype == torch.uint8
    outs, ok = b.decrypt(n0, t0)
    assert outs == [] and tuple(ok.shape) == (0,) and ok.dtype == torch.bool
    assert CB.ccm_encrypt_batch([], bytes(16), n0)[0] == []
    assert AES(bytes(32)).ccm_decrypt_batch([], n0, t0)[0] == []
    for bad in (torch.zeros((0, 12), dtype=torch.uint8), torch.zeros((0, 13), dtype=torch.int32),
                torch.zeros((1, 13), dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8), b"", None):
        with pytest.raises(ValueError, match="nonces"):
            b.encrypt(bad)
    for bad in (torch.zeros((0, 16), dtype=torch.uint8), torch.zeros((0, 8), dtype=torch.int8),
                torch.zeros((2, 8), dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="tags"):
            b.decrypt(n0, bad)


def planned(n=2, nonce_bytes=12, tag_bytes=16):
    """A batch of n records as the constructor leaves it, without a device: what the run methods check first."""
    b = CB.CcmBatch.__new__(CB.CcmBatch)
    b._init_common(bytes(16), nonce_bytes, tag_bytes, True)
    b.n, b.device, b.outs = n, torch.device("cuda:0"), []
    b.tags, b.ok = torch.zeros((n, tag_bytes), dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
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
    for tb in (4, 16):
        b = planned(tag_bytes=tb)
        for own in (b.tags, b.tags[1:], b.ok.view(1, 2)):
            with pytest.raises(ValueError, match="own tags"):
                b.decrypt(torch.zeros((2, 12), dtype=torch.uint8), own)


def test_the_new_functions_are_declared():
    src = open(os.path.join(ROOT, "our_tree_amd", "_native.py")).read()
    declared = set(re.findall(r'"(otc_\w+|aes_\w+)": \(', src))
    assert {"otc_ccm_batch_plan", "otc_ccm_batch_ws_bytes", "otc_ccm_batch_spans", "otc_aes_ccm_batch",
            "aes_crypt_ccm", "aes_ccm_auth_decrypt"} <= declared
    hdr = open(os.path.join(ROOT, "csrc", "include", "otc.h")).read()
    for name in ("otc_ccm_msg", "OTC_CCM_BATCH_MAX_BYTES", "OTC_CCM_BATCH_MAX_AAD", "otc_ccm_batch_plan",
                 "otc_ccm_batch_ws_bytes", "otc_ccm_batch_spans", "otc_aes_ccm_batch"):
        assert name in hdr
