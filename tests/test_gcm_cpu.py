"""The CPU oracle's AES-GCM (csrc/cpu/aes.c aes_crypt_gcm, aes_ghash,
aes_crypt_ctr32 through cpu_ref.gcm / ghash / ctr32): known answers, a
cross-check against libcrypto where it is installed, CTR32's wrap, GHASH's
continuation, the tag check and the argument errors.  The device kernels are
tested against this oracle (tests/test_gpu_gcm.py)."""
import ctypes
import ctypes.util
import json
import os
import random

import pytest

from our_tree_amd.models import AESGCM, cpu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "gcm_vectors.json")))["vectors"]


def _fields(v):
    return tuple(bytes.fromhex(v[k]) for k in ("key", "iv", "aad", "pt", "ct", "tag"))


@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_known_answers(v):
    key, iv, aad, pt, ct, tag = _fields(v)
    assert cpu_ref.gcm(key, iv, pt, aad) == (ct, tag)
    assert cpu_ref.gcm(key, iv, ct, aad, decrypt=True) == (pt, tag)  # the computed tag, both ways
    assert cpu_ref.gcm_auth_decrypt(key, iv, ct, tag, aad) == pt
    assert AESGCM(key).encrypt(pt, iv, aad) == (ct, tag)
    assert AESGCM(key).decrypt(ct, iv, tag, aad) == pt


def test_vectors_cover_the_issue_set():
    by_name = {v["name"]: v for v in VECTORS}
    assert by_name["zero-key-128-empty"]["tag"] == "58e2fccefa7e3061367f1d57a4e7455a"
    assert (by_name["zero-key-128-one-block"]["ct"], by_name["zero-key-128-one-block"]["tag"]) == (
        "0388dace60b6a392f328c2b971b2fe78", "ab6e47d42cec13bdf53a67b21257bddf")
    assert (by_name["zero-key-256-one-block"]["ct"], by_name["zero-key-256-one-block"]["tag"]) == (
        "cea7403d4d606b6e074ec5d3baf39d18", "d0d1c8a799996bf0265b98b5d48ab919")
    f = [_fields(v) for v in VECTORS]
    assert any(len(k) == 24 for k, *_ in f)                      # AES-192
    assert any(len(aad) == 20 for _, _, aad, *_ in f)
    assert {1, 60} <= {len(iv) for _, iv, *_ in f}
    assert any(len(pt) == 33 for _, _, _, pt, *_ in f)


# ---- libcrypto ---------------------------------------------------------------
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10


def _libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
        for f in ("EVP_CIPHER_CTX_new", "EVP_aes_128_gcm", "EVP_aes_192_gcm", "EVP_aes_256_gcm"):
            getattr(lib, f).restype = ctypes.c_void_p
        lib.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        lib.EVP_CIPHER_CTX_ctrl.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_char_p, ctypes.c_char_p]
        lib.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p,
                                          ctypes.c_int]
        lib.EVP_EncryptFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
        return lib
    except (OSError, AttributeError):
        return None


LIBCRYPTO = _libcrypto()
needs_libcrypto = pytest.mark.skipif(LIBCRYPTO is None, reason="libcrypto is not installed")


def evp_gcm_encrypt(key: bytes, iv: bytes, pt: bytes, aad: bytes):
    """(ciphertext, tag) from EVP_aes_*_gcm."""
    lib = LIBCRYPTO
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        cipher = {16: lib.EVP_aes_128_gcm, 24: lib.EVP_aes_192_gcm, 32: lib.EVP_aes_256_gcm}[len(key)]()
        assert lib.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, len(iv), None) == 1
        assert lib.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
        n = ctypes.c_int(0)
        if aad:
            assert lib.EVP_EncryptUpdate(ctx, None, ctypes.byref(n), aad, len(aad)) == 1
        out = ctypes.create_string_buffer(len(pt) + 32)
        got = 0
        if pt:
            assert lib.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
            got = n.value
        fin = ctypes.create_string_buffer(32)
        assert lib.EVP_EncryptFinal_ex(ctx, fin, ctypes.byref(n)) == 1
        tag = ctypes.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag) == 1
        return out.raw[:got], tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


@needs_libcrypto
@pytest.mark.parametrize("ivlen", [1, 12, 16, 60])
@pytest.mark.parametrize("aadlen", [0, 20], ids=["noaad", "aad"])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33, 4111, 65541])
def test_matches_libcrypto(n, aadlen, ivlen):
    rng = random.Random(n * 977 + aadlen * 31 + ivlen)
    for keybytes in (16, 24, 32):
        key, iv, pt, aad = rng.randbytes(keybytes), rng.randbytes(ivlen), rng.randbytes(n), rng.randbytes(aadlen)
        ct, tag = cpu_ref.gcm(key, iv, pt, aad)
        assert (ct, tag) == evp_gcm_encrypt(key, iv, pt, aad)
        assert cpu_ref.gcm(key, iv, ct, aad, decrypt=True) == (pt, tag)


@needs_libcrypto
def test_threaded_ghash_matches_libcrypto():
    """From 4 MiB aes_ghash hashes pieces on threads and joins them with powers of H."""
    rng = random.Random(38)
    key, iv, pt, aad = rng.randbytes(16), rng.randbytes(12), rng.randbytes((5 << 20) + 7), rng.randbytes(13)
    assert cpu_ref.gcm(key, iv, pt, aad) == evp_gcm_encrypt(key, iv, pt, aad)


# ---- without libcrypto -------------------------------------------------------
def test_threaded_ghash_equals_block_by_block():
    rng = random.Random(39)
    h, y0, data = rng.randbytes(16), rng.randbytes(16), rng.randbytes((4 << 20) + 16 * 5 + 3)
    y = y0
    for off in range(0, len(data), 1 << 20):  # pieces below the threshold, chained
        y = cpu_ref.ghash(h, data[off: off + (1 << 20)], y)
    assert cpu_ref.ghash(h, data, y0) == y


def test_ghash_is_the_definition():
    """Y_i = (Y_{i-1} ^ X_i) . H with the bit-loop product, H with its top and bottom bits set."""
    rng = random.Random(40)
    h = bytes([0x80] + [0] * 14 + [0x01])
    data = rng.randbytes(16 * 5 + 9)
    y = bytes(16)
    for off in range(0, len(data), 16):
        x = data[off: off + 16].ljust(16, b"\0")
        y = cpu_ref.gf128_mul(bytes(a ^ b for a, b in zip(y, x)), h)
    assert cpu_ref.ghash(h, data) == y
    one = bytes([0x80] + [0] * 15)  # the field's 1: the leftmost bit is x^0
    assert cpu_ref.gf128_mul(h, one) == h == cpu_ref.gf128_mul(one, h)
    # x^127 . x = the reduction polynomial's low part, 0xE1 || 0^120
    assert cpu_ref.gf128_mul(bytes(15) + b"\x01", bytes([0x40] + [0] * 15)) == bytes([0xE1] + [0] * 15)


@pytest.mark.parametrize("n", [16, 48, 16 * 9 + 5])
def test_ghash_continues_through_y0(n):
    rng = random.Random(n)
    h, y0, data = rng.randbytes(16), rng.randbytes(16), rng.randbytes(n)
    whole = cpu_ref.ghash(h, data, y0)
    for cut in range(0, n + 1, 16):
        assert cpu_ref.ghash(h, data[cut:], cpu_ref.ghash(h, data[:cut], y0)) == whole


def test_ctr32_increments_only_the_low_word():
    rng = random.Random(41)
    key, data = rng.randbytes(16), rng.randbytes(5 * 16)
    top = rng.randbytes(11) + b"\xff"  # a carry out of the low word would show in byte 11
    ctr = top + bytes.fromhex("fffffffe")
    lows = [0xFFFFFFFE, 0xFFFFFFFF, 0, 1, 2]
    want = b"".join(
        bytes(a ^ b for a, b in zip(cpu_ref.ecb(key, top + lo.to_bytes(4, "big")), data[16 * i: 16 * i + 16]))
        for i, lo in enumerate(lows))
    got = cpu_ref.ctr32(key, ctr, data)
    assert got == want
    # the 128-bit counter carries into byte 11 at block 2: equal before, different from there on
    full = cpu_ref.ctr(key, ctr, data)
    assert full[:32] == got[:32]
    assert all(full[16 * i: 16 * i + 16] != got[16 * i: 16 * i + 16] for i in (2, 3, 4))


def test_ctr32_partial_tail():
    rng = random.Random(42)
    key, ctr, data = rng.randbytes(32), rng.randbytes(16), rng.randbytes(16 * 3 + 5)
    assert cpu_ref.ctr32(key, ctr, data) == cpu_ref.ctr32(key, ctr, data + bytes(11))[: len(data)]
    assert cpu_ref.ctr32(key, ctr, cpu_ref.ctr32(key, ctr, data)) == data


def test_tag_mismatch_zeroes_the_output():
    rng = random.Random(43)
    key, iv, pt, aad = rng.randbytes(16), rng.randbytes(12), rng.randbytes(100), rng.randbytes(20)
    ct, tag = cpu_ref.gcm(key, iv, pt, aad)
    assert cpu_ref.gcm_auth_decrypt(key, iv, ct, tag, aad) == pt
    assert cpu_ref.gcm_auth_decrypt(key, iv, ct, tag[:12], aad) == pt  # a truncated tag
    bad_ct = bytes([ct[0] ^ 1]) + ct[1:]
    bad_tag = tag[:15] + bytes([tag[15] ^ 0x80])
    for args in ((bad_ct, tag, aad), (ct, bad_tag, aad), (ct, tag, aad + b"x"), (ct, bad_tag[8:], aad)):
        with pytest.raises(cpu_ref.GcmTagError) as e:
            cpu_ref.gcm_auth_decrypt(key, iv, *args)
        assert e.value.output == bytes(len(ct))
    assert issubclass(cpu_ref.GcmTagError, ValueError)


def test_argument_errors():
    with pytest.raises(ValueError):
        cpu_ref.gcm(bytes(15), bytes(12), b"")                 # no such key size
    with pytest.raises(ValueError):
        cpu_ref.gcm(bytes(16), b"", b"data")                   # an empty IV
    with pytest.raises(ValueError):
        cpu_ref.gcm_auth_decrypt(bytes(16), bytes(12), b"", bytes(3))    # a 3-byte tag
    with pytest.raises(ValueError):
        cpu_ref.gcm_auth_decrypt(bytes(16), bytes(12), b"", bytes(17))
    with pytest.raises(ValueError):
        cpu_ref.ghash(bytes(15), b"")
    with pytest.raises(ValueError):
        cpu_ref.ghash(bytes(16), b"", y0=bytes(8))
    with pytest.raises(ValueError):
        cpu_ref.ctr32(bytes(16), bytes(12), b"")
    with pytest.raises(ValueError):
        AESGCM(bytes(20))
