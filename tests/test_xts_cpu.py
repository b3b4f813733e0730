"""The CPU oracle's XTS-AES (csrc/cpu/aes.c aes_crypt_xts / _units through
cpu_ref.xts): IEEE 1619 known answers, a cross-check against libcrypto where
it is installed, and the argument errors.  The device kernels are tested
against this oracle (tests/test_gpu_xts.py)."""
import ctypes
import ctypes.util
import json
import os
import random

import pytest

from our_tree_amd.models import cpu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "xts_vectors.json")))["vectors"]


@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_known_answers(v):
    key, pt, ct = (bytes.fromhex(v[k]) for k in ("key", "pt", "ct"))
    t0 = int(v["tweak0"], 16)
    assert cpu_ref.xts(key, t0, pt, v["unit_bytes"]) == ct
    assert cpu_ref.xts(key, t0, ct, v["unit_bytes"], decrypt=True) == pt
    # the tweak as its 16 little-endian bytes
    assert cpu_ref.xts(key, t0.to_bytes(16, "little"), pt, v["unit_bytes"]) == ct


def test_vectors_are_the_issue_set():
    assert [v["name"] for v in VECTORS] == ["ieee1619-1", "ieee1619-2", "aes128-cts-17", "aes256-cts-47",
                                            "two-units-tweak-carry"]
    assert len(bytes.fromhex(VECTORS[2]["pt"])) == 17 and len(bytes.fromhex(VECTORS[3]["pt"])) == 47


# ---- libcrypto ---------------------------------------------------------------
def _libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
        for f in ("EVP_CIPHER_CTX_new", "EVP_aes_128_xts", "EVP_aes_256_xts"):
            getattr(lib, f).restype = ctypes.c_void_p
        lib.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        lib.EVP_CipherInit_ex.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
        lib.EVP_CipherUpdate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p,
                                         ctypes.c_int]
        lib.EVP_CipherFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
        return lib
    except (OSError, AttributeError):
        return None


LIBCRYPTO = _libcrypto()
needs_libcrypto = pytest.mark.skipif(LIBCRYPTO is None, reason="libcrypto is not installed")


def evp_xts(key: bytes, tweak: int, data: bytes, encrypt: bool) -> bytes:
    """One data unit through EVP_aes_*_xts (the IV is the little-endian tweak number)."""
    lib = LIBCRYPTO
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        cipher = lib.EVP_aes_128_xts() if len(key) == 32 else lib.EVP_aes_256_xts()
        iv = (tweak % (1 << 128)).to_bytes(16, "little")
        assert lib.EVP_CipherInit_ex(ctx, cipher, None, key, iv, 1 if encrypt else 0) == 1
        out = ctypes.create_string_buffer(len(data) + 32)
        n = ctypes.c_int(0)
        assert lib.EVP_CipherUpdate(ctx, out, ctypes.byref(n), data, len(data)) == 1
        fin = ctypes.c_int(0)
        assert lib.EVP_CipherFinal_ex(ctx, ctypes.cast(ctypes.byref(out, n.value), ctypes.c_char_p), ctypes.byref(fin)) == 1
        return out.raw[: n.value + fin.value]
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def _key(rng, nbytes):
    while True:  # distinct halves: OpenSSL 3 refuses equal ones when encrypting
        k = rng.randbytes(nbytes)
        if k[: nbytes // 2] != k[nbytes // 2:]:
            return k


@needs_libcrypto
@pytest.mark.parametrize("keybytes", [32, 64])
@pytest.mark.parametrize("n", [16, 17, 31, 32, 33, 511, 4096, 4111, 65536 + 5])
def test_single_unit_matches_libcrypto(n, keybytes):
    rng = random.Random(n * 131 + keybytes)
    key, data, tweak = _key(rng, keybytes), rng.randbytes(n), rng.getrandbits(128)
    ct = cpu_ref.xts(key, tweak, data)
    assert ct == evp_xts(key, tweak, data, True)
    assert cpu_ref.xts(key, tweak, ct, decrypt=True) == data == evp_xts(key, tweak, ct, False)


@needs_libcrypto
@pytest.mark.parametrize("keybytes", [32, 64])
@pytest.mark.parametrize("unit", [16, 48, 512, 528, 4096])
def test_units_match_libcrypto(unit, keybytes):
    """Five units from 2**64 - 2: the tweak number's carry crosses into the high qword."""
    rng = random.Random(unit * 7 + keybytes)
    key, data, t0 = _key(rng, keybytes), rng.randbytes(5 * unit), 2**64 - 2
    ct = cpu_ref.xts(key, t0, data, unit)
    assert ct == b"".join(evp_xts(key, t0 + s, data[s * unit: (s + 1) * unit], True) for s in range(5))
    assert cpu_ref.xts(key, t0, ct, unit, decrypt=True) == data


# ---- without libcrypto -------------------------------------------------------
@pytest.mark.parametrize("keybytes", [32, 64])
def test_units_are_single_units_with_consecutive_tweaks(keybytes):
    rng = random.Random(keybytes)
    key, data = rng.randbytes(keybytes), rng.randbytes(4 * 528)
    for t0 in (2**64 - 2, 2**128 - 2):  # carry into the high qword; wrap at 2**128
        whole = cpu_ref.xts(key, t0, data, 528)
        assert whole == b"".join(cpu_ref.xts(key, t0 + s, data[s * 528: (s + 1) * 528]) for s in range(4))
        assert cpu_ref.xts(key, t0, whole, 528, decrypt=True) == data


def test_threaded_bulk_equals_unit_by_unit():
    """aes_crypt_xts_units splits large calls over threads."""
    rng = random.Random(5)
    key, data = rng.randbytes(32), rng.randbytes(5 << 20)
    whole = cpu_ref.xts(key, 9, data, 4096)
    for s in (0, 1, 640, 1279):
        assert whole[s * 4096: (s + 1) * 4096] == cpu_ref.xts(key, 9 + s, data[s * 4096: (s + 1) * 4096])


def test_argument_errors():
    with pytest.raises(ValueError):
        cpu_ref.xts(bytes(48), 0, bytes(32))            # no AES-192 form
    with pytest.raises(ValueError):
        cpu_ref.xts(bytes(32), 0, bytes(15))            # below one block
    with pytest.raises(ValueError):
        cpu_ref.xts(bytes(32), 0, bytes(48), 24)        # two units, no multiple of 16
    with pytest.raises(ValueError):
        cpu_ref.xts(bytes(32), b"short", bytes(32))     # a tweak of other than 16 bytes
