"""ChaCha20, Poly1305 and ChaCha20-Poly1305 (RFC 8439) in the C oracle
(csrc/cpu/chacha.c): the golden vectors (RFC inputs, libcrypto outputs), a
second oracle written here from the RFC in Python integers, a cross-check
against libcrypto where it is installed, Poly1305's reduction edge cases, the
refused counter wrap, and the AEAD's tamper handling."""
import ctypes
import ctypes.util
import json
import os
import random

import pytest

from our_tree_amd import _native
from our_tree_amd.models import ChaCha20Poly1305, cpu_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chacha_vectors.json")
with open(GOLDEN) as f:
    VEC = json.load(f)
H = bytes.fromhex
P1305 = (1 << 130) - 5


# ---- the second oracle: straight from RFC 8439, on Python integers -------------
def py_chacha20_block(key, nonce, counter):
    rotl = lambda v, n: ((v << n) | (v >> (32 - n))) & 0xFFFFFFFF
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574]
    s += [int.from_bytes(key[i:i + 4], "little") for i in range(0, 32, 4)]
    s += [counter] + [int.from_bytes(nonce[i:i + 4], "little") for i in range(0, 12, 4)]
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return b"".join(((a + b) & 0xFFFFFFFF).to_bytes(4, "little") for a, b in zip(x, s))


def py_chacha20(key, nonce, data, counter=0):
    ks = b"".join(py_chacha20_block(key, nonce, counter + i) for i in range((len(data) + 63) // 64))
    return bytes(a ^ b for a, b in zip(data, ks))


def py_poly1305(key, msg):
    r = int.from_bytes(key[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(key[16:], "little")
    acc = 0
    for i in range(0, len(msg), 16):
        block = int.from_bytes(msg[i:i + 16] + b"\x01", "little")
        acc = ((acc + block) * r) % P1305
    return ((acc + s) % (1 << 128)).to_bytes(16, "little")


def py_aead(key, nonce, pt, aad):
    otk = py_chacha20_block(key, nonce, 0)[:32]
    ct = py_chacha20(key, nonce, pt, 1)
    pad = lambda b: b + bytes(-len(b) % 16)
    mac = pad(aad) + pad(ct) + len(aad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")
    return ct, py_poly1305(otk, mac)


def _rand(n, seed):
    return random.Random(seed).randbytes(n)


LENGTHS = list(range(0, 301)) + list(range(4093, 4100))


# ---- the golden vectors ---------------------------------------------------------
def test_golden_names_its_source():
    assert "libcrypto" in VEC["source"] and "RFC 8439" in VEC["source"]


def test_golden_anchors():
    """The three values the vectors must contain (RFC 8439 2.3.2 and 2.8.2)."""
    blk = next(v for v in VEC["chacha20"] if v["name"] == "rfc8439-2.3.2-block")
    assert blk["ct"].startswith("10f1e7e4d13b5915500fdd1fa32071c4")
    aead = next(v for v in VEC["aead"] if v["name"] == "rfc8439-2.8.2")
    assert aead["ct"].startswith("d31a8d34648e60db7b86afbc53ef7ec2")
    assert aead["tag"] == "1ae10b594f09e26a7e902ecbd0600691"


@pytest.mark.parametrize("v", VEC["chacha20"], ids=lambda v: v["name"])
def test_golden_chacha20(v):
    got = cpu_ref.chacha20(H(v["key"]), H(v["nonce"]), H(v["pt"]), v["counter"])
    assert got.hex() == v["ct"]
    assert cpu_ref.chacha20(H(v["key"]), H(v["nonce"]), got, v["counter"]) == H(v["pt"])
    assert py_chacha20(H(v["key"]), H(v["nonce"]), H(v["pt"]), v["counter"]).hex() == v["ct"]


@pytest.mark.parametrize("v", VEC["poly1305"], ids=lambda v: v["name"])
def test_golden_poly1305(v):
    assert cpu_ref.poly1305(H(v["key"]), H(v["msg"])).hex() == v["tag"]
    assert py_poly1305(H(v["key"]), H(v["msg"])).hex() == v["tag"]


@pytest.mark.parametrize("v", VEC["aead"], ids=lambda v: v["name"])
def test_golden_aead(v):
    key, nonce, aad, pt = H(v["key"]), H(v["nonce"]), H(v["aad"]), H(v["pt"])
    ct, tag = cpu_ref.chacha20_poly1305(key, nonce, pt, aad)
    assert (ct.hex(), tag.hex()) == (v["ct"], v["tag"])
    back, tag2 = cpu_ref.chacha20_poly1305(key, nonce, ct, aad, decrypt=True)
    assert (back, tag2) == (pt, tag)  # the computed tag in both directions
    assert cpu_ref.chacha20_poly1305_auth_decrypt(key, nonce, ct, tag, aad) == pt


def test_golden_key_generation():
    """RFC 8439 2.6.2: the one-time key is bytes 0..31 of block 0."""
    v = VEC["poly1305_keygen"][0]
    assert cpu_ref.chacha20(H(v["key"]), H(v["nonce"]), bytes(32), 0).hex() == v["otk"]


# ---- the C oracle against the Python-integer oracle ----------------------------
def test_chacha20_matches_python_oracle():
    for n in LENGTHS:
        key, nonce, data = _rand(32, n), _rand(12, n + 1), _rand(n, n + 2)
        counter = random.Random(n).choice([0, 1, 7, 0xFFFF, 0x7FFFFFF0])
        assert cpu_ref.chacha20(key, nonce, data, counter) == py_chacha20(key, nonce, data, counter), n


def test_poly1305_matches_python_oracle():
    for n in LENGTHS:
        key, data = _rand(32, 5000 + n), _rand(n, 6000 + n)
        assert cpu_ref.poly1305(key, data) == py_poly1305(key, data), n


def test_aead_matches_python_oracle():
    for n in list(range(0, 70)) + [255, 256, 257, 4093, 4099]:
        key, nonce, data = _rand(32, n), _rand(12, n + 1), _rand(n, n + 2)
        aad = _rand(n % 37, n + 3)
        assert cpu_ref.chacha20_poly1305(key, nonce, data, aad) == py_aead(key, nonce, data, aad), n


# ---- Poly1305's reduction: expected values from the Python-integer oracle ------
FF16 = b"\xff" * 16
R2 = (2).to_bytes(16, "little")
POLY_EDGES = {
    "r-all-bits-before-clamp": (FF16 + _rand(16, 1), _rand(100, 2)),
    "s-all-ones-carries-out": (_rand(16, 3) + FF16, _rand(64, 4)),
    "all-ff-blocks": (_rand(32, 5), FF16 * 8),
    "r-max-s-max-all-ff": (FF16 + FF16, FF16 * 16),
    "acc-passes-p": (R2 + bytes(16), FF16),                      # tag 03 00..00
    "s-ff-final-add-wraps": (R2 + FF16, (2).to_bytes(16, "little")),  # tag 03 00..00
    # r = 1: the accumulator is the plain sum of the blocks.  Three blocks carry 3 * 2^128;
    # with 2^128 - 5 (+ 3) in the first the unreduced sum is p (p + 3), inside [p, 2^130)
    "sum-equals-p": ((1).to_bytes(16, "little") + bytes(16), ((1 << 128) - 5).to_bytes(16, "little") + bytes(32)),
    "sum-p-plus-3": ((1).to_bytes(16, "little") + bytes(16), ((1 << 128) - 5).to_bytes(16, "little") + b"\x03" + bytes(31)),
    "partial-1": (_rand(32, 6), _rand(16 + 1, 7)),
    "partial-15": (_rand(32, 8), _rand(32 + 15, 9)),
    "partial-17": (_rand(32, 10), _rand(17, 11)),
    "only-partial-1": (_rand(32, 12), b"\x80"),
    "empty": (_rand(32, 13), b""),
}


@pytest.mark.parametrize("name", POLY_EDGES)
def test_poly1305_edges(name):
    key, msg = POLY_EDGES[name]
    assert cpu_ref.poly1305(key, msg) == py_poly1305(key, msg)


def test_poly1305_edge_values():
    three = b"\x03" + bytes(15)
    assert cpu_ref.poly1305(*POLY_EDGES["acc-passes-p"]) == three
    assert cpu_ref.poly1305(*POLY_EDGES["s-ff-final-add-wraps"]) == three
    assert cpu_ref.poly1305(*POLY_EDGES["sum-equals-p"]) == bytes(16)
    assert cpu_ref.poly1305(*POLY_EDGES["sum-p-plus-3"]) == three


# ---- libcrypto ------------------------------------------------------------------
EVP_CTRL_AEAD_SET_IVLEN, EVP_CTRL_AEAD_GET_TAG = 0x9, 0x10


def _libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
        for f in ("EVP_CIPHER_CTX_new", "EVP_chacha20", "EVP_chacha20_poly1305", "EVP_MAC_fetch", "EVP_MAC_CTX_new",
                  "EVP_MAC_CTX_free", "EVP_MAC_free"):
            getattr(lib, f).restype = ctypes.c_void_p
        vp, cp, ip = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)
        lib.EVP_CIPHER_CTX_free.argtypes = [vp]
        lib.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        lib.EVP_EncryptInit_ex.argtypes = [vp] * 3 + [cp, cp]
        lib.EVP_EncryptUpdate.argtypes = [vp, cp, ip, cp, ctypes.c_int]
        lib.EVP_EncryptFinal_ex.argtypes = [vp, cp, ip]
        lib.EVP_MAC_fetch.argtypes = [vp, cp, cp]
        lib.EVP_MAC_CTX_new.argtypes = [vp]
        lib.EVP_MAC_CTX_free.argtypes = [vp]
        lib.EVP_MAC_free.argtypes = [vp]
        lib.EVP_MAC_init.argtypes = [vp, cp, ctypes.c_size_t, vp]
        lib.EVP_MAC_update.argtypes = [vp, cp, ctypes.c_size_t]
        lib.EVP_MAC_final.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t]
        return lib
    except (OSError, AttributeError):
        return None


LIBCRYPTO = _libcrypto()
needs_libcrypto = pytest.mark.skipif(LIBCRYPTO is None, reason="libcrypto (3.x) is not installed")


def _evp_cipher(cipher, key, iv, pt, aad=None, ivlen=None):
    lib = LIBCRYPTO
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        assert lib.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
        if ivlen is not None:
            assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_SET_IVLEN, ivlen, None) == 1
        assert lib.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
        n = ctypes.c_int(0)
        if aad:
            assert lib.EVP_EncryptUpdate(ctx, None, ctypes.byref(n), aad, len(aad)) == 1
        out = ctypes.create_string_buffer(max(len(pt), 1))
        if pt:
            assert lib.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
            assert n.value == len(pt)
        fin = ctypes.create_string_buffer(16)
        assert lib.EVP_EncryptFinal_ex(ctx, fin, ctypes.byref(n)) == 1
        tag = None
        if aad is not None:
            t = ctypes.create_string_buffer(16)
            assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_GET_TAG, 16, t) == 1
            tag = t.raw
        return out.raw[: len(pt)], tag
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def libcrypto_chacha20(key, nonce, pt, counter):
    """EVP_chacha20: the 16-byte IV is LE32(counter) || nonce."""
    return _evp_cipher(LIBCRYPTO.EVP_chacha20(), key, counter.to_bytes(4, "little") + nonce, pt)[0]


def libcrypto_aead(key, nonce, pt, aad):
    return _evp_cipher(LIBCRYPTO.EVP_chacha20_poly1305(), key, nonce, pt, aad=aad, ivlen=12)


def libcrypto_poly1305(key, msg):
    lib = LIBCRYPTO
    mac = lib.EVP_MAC_fetch(None, b"POLY1305", None)
    assert mac
    ctx = lib.EVP_MAC_CTX_new(mac)
    try:
        assert lib.EVP_MAC_init(ctx, key, len(key), None) == 1
        if msg:
            assert lib.EVP_MAC_update(ctx, msg, len(msg)) == 1
        out, n = ctypes.create_string_buffer(16), ctypes.c_size_t(0)
        assert lib.EVP_MAC_final(ctx, out, ctypes.byref(n), 16) == 1 and n.value == 16
        return out.raw
    finally:
        lib.EVP_MAC_CTX_free(ctx)
        lib.EVP_MAC_free(mac)


@needs_libcrypto
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 4097, 65541])
def test_matches_libcrypto(n):
    """Counters far below the 32-bit wrap, where libcrypto (which carries into
    the nonce) and this engine (which refuses) differ by design."""
    key, nonce, data, aad = _rand(32, n), _rand(12, n + 1), _rand(n, n + 2), _rand(n % 29, n + 3)
    for counter in (0, 1, 0x0000FFFF, 0x7FFFFFF0):
        assert cpu_ref.chacha20(key, nonce, data, counter) == libcrypto_chacha20(key, nonce, data, counter)
    assert cpu_ref.poly1305(key, data) == libcrypto_poly1305(key, data)
    assert cpu_ref.chacha20_poly1305(key, nonce, data, aad) == libcrypto_aead(key, nonce, data, aad)


@needs_libcrypto
@pytest.mark.parametrize("name", POLY_EDGES)
def test_poly1305_edges_match_libcrypto(name):
    key, msg = POLY_EDGES[name]
    assert cpu_ref.poly1305(key, msg) == libcrypto_poly1305(key, msg)


# ---- the counter wrap is refused -------------------------------------------------
def _raw_crypt(counter, n):
    """chacha20_crypt itself (cpu_ref checks the counter before it calls): (rc, out)."""
    key, nonce, data = _rand(32, 1), _rand(12, 2), _rand(n, 3)
    out = (ctypes.c_uint8 * (n + 1)).from_buffer_copy(b"\xa5" * (n + 1))
    rc = _native.cpu_lib().chacha20_crypt(_native.as_u8p(key), _native.as_u8p(nonce), counter, _native.as_u8p(data), out, n)
    return rc, bytes(out), py_chacha20(key, nonce, data, counter)


@pytest.mark.parametrize("counter,n", [(0xFFFFFFFF, 64), (0xFFFFFFFF, 1), ((1 << 32) - 16, 1024), ((1 << 32) - 16, 961)])
def test_last_block_may_be_the_last_counter(counter, n):
    rc, out, want = _raw_crypt(counter, n)
    assert rc == 0 and out[:n] == want and out[n] == 0xA5
    assert cpu_ref.chacha20(_rand(32, 1), _rand(12, 2), _rand(n, 3), counter) == want


@pytest.mark.parametrize("counter,n", [(0xFFFFFFFF, 65), ((1 << 32) - 16, 1025), (1, 64 << 32)])
def test_wrap_is_refused_and_touches_nothing(counter, n):
    with pytest.raises(ValueError, match="2\\*\\*32 - 1"):
        cpu_ref.chacha_check_counter(counter, n)
    if n < 1 << 20:
        rc, out, _ = _raw_crypt(counter, n)
        assert rc != 0 and out == b"\xa5" * (n + 1)
        with pytest.raises(ValueError):
            cpu_ref.chacha20(_rand(32, 1), _rand(12, 2), bytes(n), counter)


def test_argument_errors():
    with pytest.raises(ValueError):
        cpu_ref.chacha20(bytes(31), bytes(12), b"x")
    with pytest.raises(ValueError):
        cpu_ref.chacha20(bytes(32), bytes(8), b"x")  # the original 8-byte-nonce layout is out of scope
    with pytest.raises(ValueError):
        cpu_ref.chacha20(bytes(32), bytes(12), b"x", counter=1 << 32)
    with pytest.raises(ValueError):
        cpu_ref.chacha20(bytes(32), bytes(12), b"x", counter=-1)
    with pytest.raises(ValueError):
        cpu_ref.poly1305(bytes(16), b"x")
    with pytest.raises(ValueError):
        cpu_ref.chacha20_poly1305_auth_decrypt(bytes(32), bytes(12), b"x", bytes(12))
    with pytest.raises(ValueError):
        ChaCha20Poly1305(bytes(16))


# ---- the AEAD ---------------------------------------------------------------------
@pytest.mark.parametrize("n,aadlen", [(0, 0), (0, 13), (1, 0), (64, 16), (117, 12), (4111, 4097)])
def test_aead_round_trip_and_tampering(n, aadlen):
    key, nonce, pt, aad = _rand(32, n), _rand(12, n + 1), _rand(n, n + 2), _rand(aadlen, n + 3)
    m = ChaCha20Poly1305(key)
    ct, tag = m.encrypt(pt, nonce, aad)
    assert len(ct) == n and len(tag) == 16
    assert m.decrypt(ct, nonce, tag, aad) == pt

    def refused(ct=ct, nonce=nonce, tag=tag, aad=aad):
        with pytest.raises(cpu_ref.ChaChaTagError) as e:
            m.decrypt(ct, nonce, tag, aad)
        assert isinstance(e.value, ValueError)
        assert e.value.output == bytes(n)  # zeroed, not the 0xA5 it held before

    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    refused(tag=flip(tag, 0))
    refused(tag=flip(tag, 15))
    refused(nonce=flip(nonce, 11))
    if n:
        refused(ct=flip(ct, 0))
        refused(ct=flip(ct, n - 1))
    if aadlen:
        refused(aad=flip(aad, aadlen - 1))
    refused(aad=aad + b"\x00")
