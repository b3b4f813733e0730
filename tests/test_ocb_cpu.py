"""AES-OCB3 (RFC 7253) in the C oracle (csrc/cpu/aes.c): the golden vectors
(RFC inputs, libcrypto outputs), a cross-check against libcrypto where it is
installed, the RFC's iterated self-check, the closed-form offsets against the
RFC's recurrence, pieces chained through the block primitive, the tamper
handling of the authenticated decryption, and the argument errors of the C
functions and of the Python wrappers.  No device is needed."""
import ctypes
import importlib.util
import json
import os
import random

import pytest

from our_tree_amd import _native
from our_tree_amd.models import AES, cpu_ref
from our_tree_amd.models.cpu_ref import OcbTagError

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ocb_vectors.json")) as f:
    VEC = json.load(f)
H = bytes.fromhex

_spec = importlib.util.spec_from_file_location("gen_ocb_vectors", os.path.join(os.path.dirname(HERE), "tools",
                                                                             "gen_ocb_vectors.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
LIBCRYPTO = gen.load_libcrypto()
needs_libcrypto = pytest.mark.skipif(LIBCRYPTO is None, reason="libcrypto with the OCB ciphers is not installed")

KEYS = {128: bytes(range(0x10, 0x20)), 192: bytes(range(0x30, 0x48)), 256: bytes(range(0x60, 0x80))}
NONCE = bytes(range(0x40, 0x4C))


def _rand(n, seed):
    return random.Random(seed).randbytes(n)


# ---- the golden vectors ---------------------------------------------------------
def test_golden_names_its_source():
    assert "libcrypto" in VEC["source"] and "RFC 7253" in VEC["source"]
    assert len(VEC["ocb"]) == 3 * (16 + 9)


def test_golden_anchors():
    """The two sample results of RFC 7253 Appendix A that the issue quotes."""
    by_name = {v["name"]: v for v in VEC["ocb"]}
    a, b = by_name["aes128-rfc7253-a-00"], by_name["aes128-rfc7253-a-01"]
    assert (a["nonce"], a["aad"], a["pt"], a["ct"]) == ("bbaa99887766554433221100", "", "", "")
    assert a["tag"].upper() == "785407BFFFC8AD9EDCC5520AC9111EE6"
    assert (b["nonce"], b["aad"], b["pt"]) == ("bbaa99887766554433221101", "0001020304050607", "0001020304050607")
    assert b["ct"].upper() == "6820B3657B6F615A" and b["tag"].upper() == "5725BDA0D3B4EB3A257C9AF1F8F03009"


def test_golden_covers_what_it_should():
    assert {len(H(v["key"])) for v in VEC["ocb"]} == {16, 24, 32}
    assert {len(H(v["nonce"])) for v in VEC["ocb"]} == {1, 8, 12, 15}
    assert {v["tag_bytes"] for v in VEC["ocb"]} == {8, 12, 16}
    assert {(len(H(v["aad"])), len(H(v["pt"]))) for v in VEC["ocb"] if "rfc7253" in v["name"]} == set(gen.RFC_LENGTHS)


@pytest.mark.parametrize("v", VEC["ocb"], ids=[v["name"] for v in VEC["ocb"]])
def test_oracle_matches_golden(v):
    key, nonce, aad, pt = H(v["key"]), H(v["nonce"]), H(v["aad"]), H(v["pt"])
    ct, tag = cpu_ref.ocb(key, nonce, pt, aad, tag_bytes=v["tag_bytes"])
    assert (ct.hex(), tag.hex()) == (v["ct"], v["tag"])
    back, tag2 = cpu_ref.ocb(key, nonce, ct, aad, decrypt=True, tag_bytes=v["tag_bytes"])
    assert (back, tag2) == (pt, tag)
    assert cpu_ref.ocb_auth_decrypt(key, nonce, ct, tag, aad) == pt
    assert AES(key).ocb_encrypt(pt, nonce, aad, tag_bytes=v["tag_bytes"]) == (ct, tag)
    assert AES(key).ocb_decrypt(ct, nonce, tag, aad) == pt


@needs_libcrypto
def test_golden_is_what_libcrypto_gives_today():
    assert gen.generate(LIBCRYPTO)["ocb"] == VEC["ocb"]


# ---- live libcrypto ---------------------------------------------------------------
@needs_libcrypto
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_matches_libcrypto(bits):
    """Random lengths 0..4100, nonce lengths 1..15, tag lengths 1..16 and the
    AAD lengths around a block and past 4096."""
    rng = random.Random(bits)
    lengths = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 4100] + [rng.randrange(0, 4101) for _ in range(40)]
    aads = [0, 1, 15, 16, 17, 4097]
    for i, n in enumerate(lengths):
        nl, tl, al = 1 + i % 15, 1 + (i * 7) % 16, aads[i % len(aads)]
        nonce, pt, aad = _rand(nl, 3 * i), _rand(n, 3 * i + 1), _rand(al, 3 * i + 2)
        assert cpu_ref.ocb(KEYS[bits], nonce, pt, aad, tag_bytes=tl) == \
            gen.libcrypto_ocb(LIBCRYPTO, KEYS[bits], nonce, pt, aad, tl), (n, nl, tl, al)


@needs_libcrypto
def test_every_nonce_and_tag_length_matches_libcrypto():
    pt, aad = _rand(77, 1), _rand(13, 2)
    for nl in range(1, 16):
        for tl in range(1, 17):
            nonce = _rand(nl, 100 + nl)
            assert cpu_ref.ocb(KEYS[128], nonce, pt, aad, tag_bytes=tl) == \
                gen.libcrypto_ocb(LIBCRYPTO, KEYS[128], nonce, pt, aad, tl), (nl, tl)


# ---- the RFC's iterated check -----------------------------------------------------
ITERATED = {  # RFC 7253 Appendix A, "Test vectors for ... other parameter sets"
    (128, 128): "67E944D23256C5E0B6C61FA22FDF1EA2", (128, 96): "77A3D8E73589158D25D01209", (128, 64): "192C9B7BD90BA06A",
    (192, 128): "F673F2C3E7174AAE7BAE986CA9F29E17", (192, 96): "05D56EAD2752C86BE6932C5E", (192, 64): "0066BC6E0EF34E24",
    (256, 128): "D90EB8E9C977C88B79DD793D7FFA161C", (256, 96): "5458359AC23B0CBA9E6330DD", (256, 64): "7D4EA5D445501CBE",
}


@pytest.mark.parametrize("bits,taglen", sorted(ITERATED))
def test_rfc_iterated_check(bits, taglen):
    key = bytes(bits // 8 - 1) + bytes([taglen])
    enc = lambda n, a, p: b"".join(cpu_ref.ocb(key, n.to_bytes(12, "big"), p, a, tag_bytes=taglen // 8))
    c = b""
    for i in range(128):
        s = bytes(i)
        c += enc(3 * i + 1, s, s) + enc(3 * i + 2, b"", s) + enc(3 * i + 3, s, b"")
    assert enc(385, c, b"").hex().upper() == ITERATED[bits, taglen]


# ---- offsets: the closed form against the recurrence ------------------------------
def _ntz(i):
    return (i & -i).bit_length() - 1


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def test_l_table_is_the_doubling_chain():
    """L_* = E(0), then doubling in GF(2^128), written here on Python integers."""
    dbl = lambda v: ((v << 1) ^ (0x87 if v >> 127 else 0)) & ((1 << 128) - 1)
    for key in KEYS.values():
        t = cpu_ref.ocb_l(key)
        assert t["star"] == cpu_ref.ecb(key, bytes(16))
        v, chain = int.from_bytes(t["star"], "big"), []
        for _ in range(34):
            v = dbl(v)
            chain.append(v.to_bytes(16, "big"))
        assert [t["dollar"]] + t["l"] == chain and len(t["l"]) == 33


def test_offsets_follow_the_recurrence():
    """Offset(i) ^ Offset(i - 1) == L_ntz(i): every i to 2^16, then around 2^20, 2^31 and 2^32."""
    key = KEYS[256]
    lib, ctx = _native.cpu_lib(), cpu_ref._ocb_ctx(key)
    off0 = cpu_ref.ocb_offset0(key, NONCE)
    ls = cpu_ref.ocb_l(key)["l"]
    o0 = (ctypes.c_uint8 * 16).from_buffer_copy(off0)

    def offset(i):
        out = (ctypes.c_uint8 * 16)()
        lib.aes_ocb_offset(ctypes.byref(ctx), o0, i, out)
        return bytes(out)

    assert offset(0) == off0
    prev = off0
    for i in range(1, (1 << 16) + 1):
        cur = offset(i)
        assert _xor(cur, prev) == ls[_ntz(i)], i
        prev = cur
    rng = random.Random(5)
    sampled = [c + d for c in (1 << 20, 1 << 31, 1 << 32) for d in range(-300, 1)] + \
              [c + d for c in (1 << 20, 1 << 31) for d in range(1, 300)] + \
              [rng.randrange(1, (1 << 32) + 1) for _ in range(2000)]
    for i in sampled:
        assert _xor(offset(i), offset(i - 1)) == ls[_ntz(i)], i
    assert cpu_ref.ocb_offset(key, off0, 1 << 32) == offset(1 << 32)


def test_offset0_is_the_rfc_stretch():
    """Nonce block, Ktop, Stretch and the shift by `bottom`, on Python integers."""
    for bits, key in KEYS.items():
        for nl, tl in ((12, 16), (1, 8), (15, 12), (8, 1), (12, 7)):
            for last in (0x00, 0x01, 0x3F, 0x40, 0xFF):  # every shift class of `bottom`
                nonce = _rand(nl - 1, bits + nl) + bytes([last])
                nb = ((tl * 8 % 128) << 121) | (1 << (8 * nl)) | int.from_bytes(nonce, "big")
                bottom = nb & 63
                ktop = cpu_ref.ecb(key, ((nb >> 6) << 6).to_bytes(16, "big"))
                stretch = int.from_bytes(ktop + _xor(ktop[:8], ktop[1:9]), "big")
                want = (stretch >> (64 - bottom)) & ((1 << 128) - 1)
                assert cpu_ref.ocb_offset0(key, nonce, tl) == want.to_bytes(16, "big"), (bits, nl, tl, last)


# ---- the block primitive ----------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
def test_pieces_chain_to_the_whole(bits):
    key, n = KEYS[bits], 16 * 1000
    pt, off0 = _rand(n, 9), cpu_ref.ocb_offset0(KEYS[bits], NONCE)
    whole, cs = cpu_ref.ocb_blocks(key, off0, pt)
    assert whole == cpu_ref.ocb(key, NONCE, pt)[0]
    x = 0
    for i in range(0, n, 16):
        x ^= int.from_bytes(pt[i:i + 16], "big")
    assert cs == x.to_bytes(16, "big")
    for first in (0, 254, (1 << 16) - 5, (1 << 31) - 100, (1 << 32) - 1000):
        whole, cs = cpu_ref.ocb_blocks(key, off0, pt, first)
        out, acc, at = b"", bytes(16), 0
        for cut in (1, 255, 256, 257, 231):
            o, acc = cpu_ref.ocb_blocks(key, off0, pt[16 * at:16 * (at + cut)], first + at, acc)
            out, at = out + o, at + cut
        assert at == 1000 and (out, acc) == (whole, cs), first
        back, cs2 = cpu_ref.ocb_blocks(key, off0, whole, first, decrypt=True)
        assert (back, cs2) == (pt, cs)


def test_large_calls_split_over_threads_agree():
    """From 2^16 blocks the oracle runs pieces on threads: the same bytes as the serial chain."""
    key, off0, n = KEYS[128], cpu_ref.ocb_offset0(KEYS[128], NONCE), 16 * ((1 << 16) + 77)
    pt = _rand(n, 11)
    big, cs = cpu_ref.ocb_blocks(key, off0, pt, 12345)
    half = 16 * 40000
    a, acc = cpu_ref.ocb_blocks(key, off0, pt[:half], 12345)
    b, acc = cpu_ref.ocb_blocks(key, off0, pt[half:], 12345 + 40000, acc)
    assert (a + b, acc) == (big, cs)


# ---- authenticated decryption -----------------------------------------------------
@pytest.mark.parametrize("n", [0, 5, 16, 4111])
def test_auth_decrypt_zeroes_on_tampering(n):
    key, aad = KEYS[192], _rand(13, 3)
    pt = _rand(n, 4)
    ct, tag = cpu_ref.ocb(key, NONCE, pt, aad)
    assert cpu_ref.ocb_auth_decrypt(key, NONCE, ct, tag, aad) == pt
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x20]) + b[i + 1:]
    bad = [(NONCE, ct, flip(tag, 7), aad), (NONCE, ct, tag, flip(aad, 12)), (flip(NONCE, 11), ct, tag, aad),
           (NONCE, ct, tag[:12], aad)]  # a shorter tag is another TAGLEN: another nonce block
    if n:
        bad.append((NONCE, flip(ct, n // 2), tag, aad))
    for nonce, c, t, a in bad:
        with pytest.raises(OcbTagError) as e:
            cpu_ref.ocb_auth_decrypt(key, nonce, c, t, a)
        assert e.value.output == bytes(n)
    assert issubclass(OcbTagError, ValueError)


def test_tag_length_changes_the_ciphertext():
    pt = _rand(100, 6)
    assert cpu_ref.ocb(KEYS[128], NONCE, pt, tag_bytes=16)[0] != cpu_ref.ocb(KEYS[128], NONCE, pt, tag_bytes=12)[0]


def test_oracle_is_right_with_both_library_copies_loaded():
    """The GPU library carries its own copy of aes.c and is loaded globally, so
    the oracle's calls between exported functions land in that copy while its
    static block functions use this copy's tables: every entry point has to
    build them itself.  A fresh process, since the order of loading matters."""
    import subprocess
    import sys

    if not _native.gpu_lib_available():
        pytest.skip("libotc.so is not built (make cpu)")
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "from our_tree_amd import _native\n"
            "_native.require_gpu_lib()\n"
            "from our_tree_amd.models import cpu_ref\n"
            "k, n, d = bytes(range(16)), bytes.fromhex('BBAA99887766554433221101'), bytes(range(8))\n"
            "c, t = cpu_ref.ocb(k, n, d, d)\n"
            "print(c.hex(), t.hex(), cpu_ref.ocb_auth_decrypt(k, n, c, t, d).hex(), cpu_ref.ocb_hash(k, d).hex(),\n"
            "      cpu_ref.ocb_blocks(k, cpu_ref.ocb_offset0(k, n), bytes(16))[0].hex())\n")
    r = subprocess.run([sys.executable, "-c", code, os.path.dirname(HERE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    k, n, d = bytes(range(16)), H("BBAA99887766554433221101"), bytes(range(8))
    assert r.stdout.split() == ["6820b3657b6f615a", "5725bda0d3b4eb3a257c9af1f8f03009", d.hex(), cpu_ref.ocb_hash(k, d).hex(),
                                cpu_ref.ocb_blocks(k, cpu_ref.ocb_offset0(k, n), bytes(16))[0].hex()]


# ---- argument errors --------------------------------------------------------------
def test_c_argument_errors():
    lib, ctx = _native.cpu_lib(), cpu_ref._ocb_ctx(KEYS[128])
    bad_len = -0x22
    buf, out, tag = (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 16)()
    n16 = (ctypes.c_uint8 * 16)()
    assert lib.aes_ocb_setkey(ctypes.byref(_native.AesOcbContext()), buf, 100) != 0
    for nl, tl in ((0, 16), (16, 16), (12, 0), (12, 17)):
        assert lib.aes_ocb_offset0(ctypes.byref(ctx), n16, nl, tl, out) == bad_len
        assert lib.aes_crypt_ocb(ctypes.byref(ctx), 1, 32, n16, nl, None, 0, buf, out, tag, tl) == bad_len
        assert lib.aes_ocb_auth_decrypt(ctypes.byref(ctx), 32, n16, nl, None, 0, tag, tl, buf, out) == bad_len
    assert lib.aes_ocb_offset0(ctypes.byref(ctx), None, 12, 16, out) == bad_len
    assert lib.aes_crypt_ocb(ctypes.byref(ctx), 1, (1 << 36) + 1, n16, 12, None, 0, buf, out, tag, 16) == bad_len
    cs = (ctypes.c_uint8 * 16)()
    assert lib.aes_crypt_ocb_blocks(ctypes.byref(ctx), 1, n16, (1 << 32) - 1, 2, buf, out, cs) == bad_len
    assert lib.aes_crypt_ocb_blocks(ctypes.byref(ctx), 1, n16, (1 << 32) + 1, 0, buf, out, cs) == bad_len
    assert lib.aes_crypt_ocb_blocks(ctypes.byref(ctx), 1, n16, (1 << 32) - 2, 2, buf, out, cs) == 0
    assert bytes(cs) == bytes(16)  # two zero blocks


def test_python_wrappers_raise_value_errors():
    k = KEYS[128]
    for bad in (lambda: cpu_ref.ocb(b"short", NONCE, b""), lambda: cpu_ref.ocb(k, b"", b""),
                lambda: cpu_ref.ocb(k, bytes(16), b""), lambda: cpu_ref.ocb(k, NONCE, b"", tag_bytes=0),
                lambda: cpu_ref.ocb(k, NONCE, b"", tag_bytes=17), lambda: cpu_ref.ocb_auth_decrypt(k, NONCE, b"", b""),
                lambda: cpu_ref.ocb_auth_decrypt(k, NONCE, b"", bytes(17)), lambda: cpu_ref.ocb_offset0(k, b""),
                lambda: cpu_ref.ocb_offset(k, bytes(15), 1), lambda: cpu_ref.ocb_offset(k, bytes(16), (1 << 32) + 1),
                lambda: cpu_ref.ocb_blocks(k, bytes(16), bytes(17)),
                lambda: cpu_ref.ocb_blocks(k, bytes(16), bytes(32), (1 << 32) - 1),
                lambda: cpu_ref.ocb_blocks(k, bytes(16), bytes(16), checksum=bytes(3)),
                lambda: cpu_ref.ocb_check(NONCE, 16, (1 << 36) + 1)):
        with pytest.raises(ValueError):
            bad()


def test_ops_wrappers_reject_before_any_device_call():
    """The device ops' own checks come before the native library is touched:
    a CPU tensor, a bad nonce, a bad tag length raise without a GPU."""
    import torch

    from our_tree_amd import ops

    assert not hasattr(ops, "ocb_encrypt") and "ocb_encrypt" not in ops.__all__  # reached as ops.ocb_ops.*
    x = torch.zeros(32, dtype=torch.uint8)
    for bad in (lambda: ops.ocb_ops.ocb_encrypt(x, KEYS[128], NONCE), lambda: ops.ocb_ops.ocb_decrypt(x, KEYS[128], NONCE, bytes(16)),
                lambda: ops.ocb_ops.ocb_blocks(x, KEYS[128], bytes(16))):
        with pytest.raises(ValueError, match="GPU tensor"):
            bad()
    with pytest.raises(TypeError):
        ops.ocb_ops.ocb_encrypt(b"bytes", KEYS[128], NONCE)
