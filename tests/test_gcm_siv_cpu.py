"""The AES-GCM-SIV oracle (csrc/cpu/aes.c, models/cpu_ref.py) without a GPU:
RFC 8452's POLYVAL example, derivation and sealed vectors, two vectors of an
independent model of the RFC, POLYVAL's identity with GHASH, the
little-endian counter across its wrap, round trips, tampering, the property
the mode exists for (a repeated nonce gives unrelated keystreams), and the
argument errors of the oracle and of the device ops' own checks."""
import ctypes
import random

import pytest

from our_tree_amd import _native
from our_tree_amd.models import cpu_ref
from our_tree_amd.models.cpu_ref import GcmSivTagError

H = bytes.fromhex
K128_1, K256_1 = H("01" + "00" * 15), H("01" + "00" * 31)
N3 = H("03" + "00" * 11)
NA = bytes(range(0xA0, 0xAC))
AAD_M, PT_M = bytes(range(100, 121)), bytes(range(1, 50))

# key, nonce, aad, plaintext, ciphertext || tag: RFC 8452 appendix C; the last two from an independent model
SEALED = [
    (K128_1, N3, b"", b"", "dc20e2d83f25705bb49e439eca56de25"),
    (K128_1, N3, b"", H("0100000000000000"), "b5d839330ac7b786578782fff6013b815b287c22493a364c"),
    (K128_1, N3, H("01"), H("0200000000000000"), "1e6daba35669f4273b0a1a2560969cdf790d99759abd1508"),
    (K256_1, N3, b"", b"", "07f5f4169bbf55a8400cd47ea6fd400f"),
    (K256_1, N3, b"", H("0100000000000000"), "c2ef328e5c71c83b843122130f7364b761e0b97427e3df28"),
    (bytes(range(16)), NA, AAD_M, PT_M,
     "65483eb7d1533466ead8e673d7270e99ea4ffe611498a5f768131b4cd04e371ea2cdcbb60c093766b35139add04a79ddf740928eb78fabbf"
     "8f4ee555ae38f2d815"),
    (bytes(range(32)), NA, AAD_M, PT_M,
     "c2f39d921b077cbba73072360062d524e91677592a794769b8106c9d4dfbf643dbda8d4cac178311cf1ca57ec80cad12c052296c35a730ac"
     "e425c50d199ebfd125"),
]
KEY, KEY256 = bytes(range(0x10, 0x20)), bytes(range(0x60, 0x80))
NONCE = bytes(range(0x40, 0x4C))


def _rand(n, seed):
    return random.Random(seed).randbytes(n)


def test_polyval_rfc_example():
    h = H("25629347589242761d31f826ba4b757b")
    x = H("4f4f95668c83dfb6401762bb2d01a262d1a24ddd2721d006bbe45f20d3c9f362")
    assert cpu_ref.polyval(h, x).hex() == "f7a3b47b846119fae5b7866cf5e5b77e"


def test_derivation_rfc_example():
    ak, ek = cpu_ref.gcm_siv_derive(H("ee8e1ed9ff2540ae8f2ba9f50bc2f27c"), H("752abad3e0afb5f434dc4310"))
    assert (ak.hex(), ek.hex()) == ("310728d9911f1f3837b24316c3fab9a0", "a4c5ae6249963279c100be4d7e2c6edd")
    ak, ek = cpu_ref.gcm_siv_derive(KEY256, NONCE)
    blocks = [cpu_ref.ecb(KEY256, i.to_bytes(4, "little") + NONCE)[:8] for i in range(6)]
    assert ak == b"".join(blocks[:2]) and ek == b"".join(blocks[2:]) and len(ek) == 32


@pytest.mark.parametrize("key,nonce,aad,pt,sealed", SEALED, ids=[f"v{i}" for i in range(len(SEALED))])
def test_sealed_vectors(key, nonce, aad, pt, sealed):
    ct, tag = cpu_ref.gcm_siv(key, nonce, pt, aad)
    assert (ct + tag).hex() == sealed
    assert cpu_ref.gcm_siv_auth_decrypt(key, nonce, ct, tag, aad) == pt
    assert cpu_ref.gcm_siv(key, nonce, ct, aad, decrypt=True, tag=tag) == (pt, tag)


def test_the_library_self_test_runs_the_vectors():
    assert _native.cpu_lib().aes_gcmsiv_self_test(0) == 0
    assert cpu_ref.self_tests(0)["aes"] == 0


def _ghash_mulx(v: bytes) -> bytes:
    """v . x in GHASH's convention: a right shift of the byte string, 0xE1 folded into byte 0."""
    n = int.from_bytes(v, "big")
    return ((n >> 1) ^ (0xE1 << 120 if n & 1 else 0)).to_bytes(16, "big")


@pytest.mark.parametrize("nblocks", [1, 2, 7, 300])
def test_polyval_is_ghash_in_the_other_byte_order(nblocks):
    """POLYVAL(H, X_1..X_n) = rev(GHASH(mulX_GHASH(rev(H)), rev(X_1)..rev(X_n)))  (RFC 8452 appendix A)"""
    h, data = _rand(16, nblocks), _rand(16 * nblocks, 100 + nblocks)
    rev_blocks = b"".join(data[i:i + 16][::-1] for i in range(0, len(data), 16))
    assert cpu_ref.polyval(h, data) == cpu_ref.ghash(_ghash_mulx(h[::-1]), rev_blocks)[::-1]


def test_polyval_continues_from_y0():
    h, data = _rand(16, 1), _rand(16 * 40 + 5, 2)
    whole = cpu_ref.polyval(h, data)
    for cut in (16, 160, 16 * 40):
        assert cpu_ref.polyval(h, data[cut:], cpu_ref.polyval(h, data[:cut])) == whole
    assert cpu_ref.polyval(h, b"", whole) == whole
    assert cpu_ref.polyval(h, data[:5]) == cpu_ref.polyval(h, data[:5] + bytes(11))  # zero padding


def test_polyval_dot_is_the_rfc_product():
    a, b, c = _rand(16, 3), _rand(16, 4), _rand(16, 5)
    dot = cpu_ref.polyval_dot
    x128 = H("01" + "00" * 14 + "c2")  # x^128 = x^127 + x^126 + x^121 + 1: dot's neutral element
    assert dot(a, x128) == a
    assert dot(a, b) == dot(b, a) and dot(dot(a, b), c) == dot(a, dot(b, c))
    assert cpu_ref.polyval(a, b) == dot(b, a)


def test_large_calls_split_over_threads_agree():
    """From 4 MiB the oracle hashes pieces on threads and joins them with powers of H."""
    h, data = _rand(16, 6), _rand((4 << 20) + 16 * 3 + 7, 7)
    y = bytes(16)
    for off in range(0, len(data), 1 << 20):  # the serial path, 1 MiB at a time (whole blocks)
        y = cpu_ref.polyval(h, data[off:off + (1 << 20)], y)
    assert cpu_ref.polyval(h, data) == y


@pytest.mark.parametrize("key", [KEY, KEY256], ids=["128", "256"])
@pytest.mark.parametrize("start", [0xFFFFFFFE, 0xFFFFFFFF])
def test_ctr_le32_across_the_wrap(key, start):
    rest = bytes(range(0x81, 0x8D))
    ctr = start.to_bytes(4, "little") + rest
    data = _rand(16 * 5 + 7, start & 0xFF)
    ks = b"".join(cpu_ref.ecb(key, ((start + i) % (1 << 32)).to_bytes(4, "little") + rest) for i in range(6))
    assert cpu_ref.ctr_le32(key, ctr, data) == bytes(a ^ b for a, b in zip(data, ks))
    # nothing carries into byte 4: the block after the wrap is counter 0 (or 1) over the same bytes 4..15
    assert cpu_ref.ctr_le32(key, ctr, bytes(48))[16 * (0x100000000 - start):][:16] == cpu_ref.ecb(key, bytes(4) + rest)


@pytest.mark.parametrize("key", [KEY, KEY256], ids=["128", "256"])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
def test_round_trip(key, n):
    pt, aad = _rand(n, n), _rand(13, n + 1)
    ct, tag = cpu_ref.gcm_siv(key, NONCE, pt, aad)
    assert len(ct) == n and len(tag) == 16
    assert cpu_ref.gcm_siv_auth_decrypt(key, NONCE, ct, tag, aad) == pt
    # the structure: the tag starts the counter mode under the derived encryption key
    ek = cpu_ref.gcm_siv_derive(key, NONCE)[1]
    assert cpu_ref.ctr_le32(ek, tag[:15] + bytes([tag[15] | 0x80]), pt) == ct


@pytest.mark.parametrize("n", [1, 16, 100])
def test_auth_decrypt_zeroes_on_tampering(n):
    pt, aad = _rand(n, 20 + n), _rand(13, 21)
    ct, tag = cpu_ref.gcm_siv(KEY, NONCE, pt, aad)
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    for c, t, a in ((ct, flip(tag, 0), aad), (ct, flip(tag, 15), aad), (flip(ct, 0), tag, aad),
                    (flip(ct, n - 1), tag, aad), (ct, tag, flip(aad, 3)), (ct, tag, aad + b"\0")):
        with pytest.raises(GcmSivTagError) as e:
            cpu_ref.gcm_siv_auth_decrypt(KEY, NONCE, c, t, a)
        assert e.value.output == bytes(n)


def test_a_repeated_nonce_gives_unrelated_keystreams():
    """The property the mode exists for: under one (key, nonce) two plaintexts
    that differ get different tags, hence different counter blocks, and the XOR
    of the ciphertexts is NOT the XOR of the plaintexts (as it is for GCM)."""
    p1 = _rand(64, 30)
    p2 = p1[:63] + bytes([p1[63] ^ 1])
    (c1, t1), (c2, t2) = cpu_ref.gcm_siv(KEY, NONCE, p1), cpu_ref.gcm_siv(KEY, NONCE, p2)
    assert t1 != t2
    xor = lambda a, b: bytes(x ^ y for x, y in zip(a, b))
    ks1, ks2 = xor(c1, p1), xor(c2, p2)
    assert all(ks1[i:i + 16] != ks2[i:i + 16] for i in range(0, 64, 16))
    assert xor(c1, c2) != xor(p1, p2)
    g1, g2 = cpu_ref.gcm(KEY, NONCE, p1)[0], cpu_ref.gcm(KEY, NONCE, p2)[0]
    assert xor(g1, g2) == xor(p1, p2)  # what GCM gives away
    assert cpu_ref.gcm_siv(KEY, NONCE, p1) == (c1, t1)  # equal messages are all a repeat shows


def test_c_argument_errors():
    lib = _native.cpu_lib()
    bad_len, bad_key = -0x22, -0x20
    buf, out, tag = (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 16)()
    n12 = (ctypes.c_uint8 * 12)()
    k128, k192 = cpu_ref._ctx(KEY), cpu_ref._ctx(bytes(24))
    assert lib.aes_gcmsiv_derive(ctypes.byref(k192), n12, out, out) == bad_key
    assert lib.aes_crypt_gcmsiv(ctypes.byref(k192), 1, 16, n12, None, 0, buf, out, None, tag) == bad_key
    assert lib.aes_crypt_gcmsiv(ctypes.byref(k128), 1, (1 << 36) + 1, n12, None, 0, buf, out, None, tag) == bad_len
    assert lib.aes_crypt_gcmsiv(ctypes.byref(k128), 1, 16, n12, None, (1 << 36) + 1, buf, out, None, tag) == bad_len
    assert lib.aes_crypt_gcmsiv(ctypes.byref(k128), 0, 16, n12, None, 0, buf, out, None, tag) == bad_len  # no received tag
    assert lib.aes_crypt_gcmsiv(ctypes.byref(k128), 1, 16, n12, None, 0, buf, out, None, tag) == 0


def test_python_wrappers_raise_value_errors():
    for bad in (lambda: cpu_ref.gcm_siv(bytes(24), NONCE, b""), lambda: cpu_ref.gcm_siv(b"short", NONCE, b""),
                lambda: cpu_ref.gcm_siv(KEY, NONCE[:11], b""), lambda: cpu_ref.gcm_siv(KEY, NONCE + b"\0", b""),
                lambda: cpu_ref.gcm_siv_auth_decrypt(KEY, NONCE, b"", bytes(15)),
                lambda: cpu_ref.gcm_siv_auth_decrypt(KEY, NONCE, b"", bytes(17)),
                lambda: cpu_ref.gcm_siv(KEY, NONCE, b"", decrypt=True, tag=bytes(12)),
                lambda: cpu_ref.gcm_siv_derive(bytes(24), NONCE), lambda: cpu_ref.gcm_siv_derive(KEY, bytes(13)),
                lambda: cpu_ref.polyval(bytes(15), b""), lambda: cpu_ref.polyval(bytes(16), b"", bytes(3)),
                lambda: cpu_ref.ctr_le32(KEY, bytes(15), b""), lambda: cpu_ref.ctr_le32(b"k", bytes(16), b""),
                lambda: cpu_ref.gcm_siv_check(KEY, NONCE, (1 << 36) + 1),
                lambda: cpu_ref.gcm_siv_check(KEY, NONCE, 0, (1 << 36) + 1)):
        with pytest.raises(ValueError):
            bad()
    assert issubclass(GcmSivTagError, ValueError) and cpu_ref.GCM_SIV_MAX_BYTES == 1 << 36


def test_ops_wrappers_reject_before_any_device_call():
    """The device ops' own checks come before the native library is touched: a
    CPU tensor raises without a GPU; the module's names stay outside ops.__all__."""
    import torch

    from our_tree_amd import ops

    siv = ops.gcm_siv_ops
    names = ("polyval", "polyval_spans", "ctr_le32", "gcm_siv_encrypt", "gcm_siv_decrypt", "GcmSivTagError")
    assert all(hasattr(siv, n) for n in names)
    assert not any(hasattr(ops, n) or n in ops.__all__ for n in names)  # reached as ops.gcm_siv_ops.*
    assert siv.GcmSivTagError is GcmSivTagError
    x = torch.zeros(32, dtype=torch.uint8)
    for bad in (lambda: siv.gcm_siv_encrypt(x, KEY, NONCE), lambda: siv.gcm_siv_decrypt(x, KEY, NONCE, bytes(16)),
                lambda: siv.polyval(x, bytes(16)), lambda: siv.ctr_le32(x, KEY, bytes(16))):
        with pytest.raises(ValueError, match="GPU tensor"):
            bad()
    with pytest.raises(ValueError, match="16 bytes"):
        siv.gcm_siv_decrypt(x, KEY, NONCE, bytes(12))  # a short tag: before anything else
    with pytest.raises(TypeError):
        siv.gcm_siv_encrypt(b"bytes", KEY, NONCE)
