"""Fault injection against the GCM-SIV entry points of the native device API
(csrc/hip/aead.cpp, C API csrc/include/otc.h) without a GPU, in the manner of
tests/test_api_validation_cpu.py: every bad argument of otc_polyval,
otc_aes_ctr_le32 and otc_aes_gcm_siv must be rejected with OTC_ERR_ARG and a
message *before* any HIP call, so the fake pointers below are never
dereferenced."""
import ctypes

import pytest

from our_tree_amd import _native

ERR_ARG = -1
ENC, DEC = 1, 0
A = 0x7F0000000000  # fake, 16-byte aligned device addresses (never touched)
T = A + (1 << 30)   # a tag, far from the data
BIG = (1 << 36) + 1


@pytest.fixture(scope="module")
def lib():
    if not _native.gpu_lib_available():
        pytest.skip("libotc.so not built")
    return _native.require_gpu_lib()


def err(lib) -> str:
    return lib.otc_last_error().decode()


def c16():
    return (ctypes.c_uint8 * 16)()


def aes_key(lib, bits=128, d=ENC):
    k = _native.OtcAesKey()
    assert lib.otc_aes_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(bits // 8))), bits, d) == 0
    return k


def siv_key(lib, bits=256):
    k = _native.OtcGcmSivKey()
    assert lib.otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(bits // 8))), bits) == 0
    return k


def test_key_init(lib):
    k = _native.OtcGcmSivKey()
    for bits in (128, 256):
        assert lib.otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(bytes(32)), bits) == 0
        assert (k.kgk.bits, k.kgk.dir) == (bits, ENC)
    for bits in (192, 0, 512):
        assert lib.otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(bytes(64)), bits) == ERR_ARG
        assert "128 or 256" in err(lib)
    assert lib.otc_gcm_siv_key_init(None, _native.as_u8p(bytes(32)), 128) == ERR_ARG
    assert lib.otc_gcm_siv_key_init(ctypes.byref(k), None, 128) == ERR_ARG


def test_polyval_validation(lib):
    h, y0 = c16(), c16()
    assert lib.otc_polyval(A, 64, None, y0, T, None) == ERR_ARG and "null" in err(lib)
    assert lib.otc_polyval(A, 64, h, None, T, None) == ERR_ARG
    assert lib.otc_polyval(A, 64, h, y0, None, None) == ERR_ARG
    assert lib.otc_polyval(A, 64, h, y0, T + 2, None) == ERR_ARG and "4-byte aligned" in err(lib)
    assert lib.otc_polyval(A, BIG, h, y0, T, None) == ERR_ARG and "2^36" in err(lib)
    assert lib.otc_polyval(None, 64, h, y0, T, None) == ERR_ARG and "null buffer" in err(lib)
    assert lib.otc_polyval(A + 8, 64, h, y0, T, None) == ERR_ARG and "16-byte aligned" in err(lib)


def test_polyval_spans_are_the_hash_decomposition(lib):
    buf, gh = (ctypes.c_uint64 * 16)(), (ctypes.c_uint64 * 16)()
    n = lib.otc_polyval_spans(buf, 16)
    assert n == lib.otc_ghash_spans(gh, 16) and list(buf[:n]) == list(gh[:n])
    assert list(buf[:3]) == [1024, 8192, 32768]
    assert lib.otc_polyval_spans(None, 16) == n


@pytest.mark.parametrize("inp,out,what", [
    (A + 1, A + 4096, "aligned"),
    (A, A + 4096 + 8, "aligned"),
    (None, A, "null"),
    (A, None, "null"),
    (A, A + 16, "overlap"),
    (A + 32, A, "overlap"),
])
def test_ctr_le32_rejects_bad_buffers(lib, inp, out, what):
    k = aes_key(lib)
    assert lib.otc_aes_ctr_le32(inp, out, 1024, ctypes.byref(k), T, None) == ERR_ARG and what in err(lib)


def test_ctr_le32_validation(lib):
    k = aes_key(lib, 192)
    assert lib.otc_aes_ctr_le32(A, A + 4096, 64, None, T, None) == ERR_ARG and "null key" in err(lib)
    kd = aes_key(lib, 128, DEC)
    assert lib.otc_aes_ctr_le32(A, A + 4096, 64, ctypes.byref(kd), T, None) == ERR_ARG and "encryption schedule" in err(lib)
    assert lib.otc_aes_ctr_le32(A, A + 4096, 64, ctypes.byref(k), None, None) == ERR_ARG and "counter block" in err(lib)
    assert lib.otc_aes_ctr_le32(A, A + 4096, 64, ctypes.byref(k), T + 1, None) == ERR_ARG and "4-byte aligned" in err(lib)
    assert lib.otc_aes_ctr_le32(A, A + (1 << 40), BIG, ctypes.byref(k), T, None) == ERR_ARG and "2^32 blocks" in err(lib)
    # the counter block inside the output: its first and its last bytes
    for c in (A + 4096, A + 4096 + 60, A + 4096 - 12):
        assert lib.otc_aes_ctr_le32(A, A + 4096, 64, ctypes.byref(k), c, None) == ERR_ARG and "lies in the output" in err(lib)
    assert lib.otc_aes_ctr_le32(None, None, 0, ctypes.byref(k), T, None) == 0  # nothing to do, nothing launched


def _siv(lib, k, inp=A, out=A + 4096, n=64, d=ENC, nonce=True, aad=None, aad_len=0, tag_in=None, tag=T):
    n12 = (ctypes.c_uint8 * 12)()
    return lib.otc_aes_gcm_siv(inp, out, n, ctypes.byref(k) if k is not None else None, d, n12 if nonce else None, aad,
                               aad_len, tag_in, tag, None)


def test_gcm_siv_validation(lib):
    k = siv_key(lib)
    assert _siv(lib, None) == ERR_ARG and "null key" in err(lib)
    k192 = _native.OtcGcmSivKey()
    k192.kgk = aes_key(lib, 192)
    assert _siv(lib, k192) == ERR_ARG and "128 or 256" in err(lib)
    kdec = _native.OtcGcmSivKey()
    kdec.kgk = aes_key(lib, 256, DEC)
    assert _siv(lib, kdec) == ERR_ARG and "encryption schedule" in err(lib)
    assert _siv(lib, k, d=2) == ERR_ARG and "direction" in err(lib)
    assert _siv(lib, k, nonce=False) == ERR_ARG and "null nonce" in err(lib)
    assert _siv(lib, k, aad=None, aad_len=5) == ERR_ARG and "null aad" in err(lib)
    assert _siv(lib, k, aad=_native.as_u8p(bytes(16)), aad_len=BIG) == ERR_ARG and "AAD" in err(lib)
    assert _siv(lib, k, tag=None) == ERR_ARG and "tag" in err(lib)
    assert _siv(lib, k, tag=T + 2) == ERR_ARG and "4-byte aligned" in err(lib)
    assert _siv(lib, k, d=DEC, tag_in=None) == ERR_ARG and "received tag" in err(lib)
    assert _siv(lib, k, d=DEC, tag_in=T + 64 + 1) == ERR_ARG and "received tag" in err(lib)
    assert _siv(lib, k, n=BIG, out=A + (1 << 40)) == ERR_ARG and "2^36" in err(lib)


@pytest.mark.parametrize("inp,out,what", [
    (A + 1, A + 4096, "aligned"),
    (A, A + 4096 + 8, "aligned"),
    (None, A, "null"),
    (A, None, "null"),
    (A, A + 16, "overlap"),
    (A + 32, A, "overlap"),
])
@pytest.mark.parametrize("d", [ENC, DEC])
def test_gcm_siv_rejects_bad_buffers(lib, inp, out, what, d):
    assert _siv(lib, siv_key(lib, 128), inp=inp, out=out, n=1024, d=d, tag_in=T + 64) == ERR_ARG and what in err(lib)


def test_gcm_siv_rejects_a_tag_in_the_data(lib):
    """The whole buffer range is checked before any launch: the counter kernel
    reads a tag while it writes out, and the hash reads the data before the tag is written."""
    k = siv_key(lib)
    for tag in (A, A + 60, A - 12, A + 4096, A + 4096 + 48):
        assert _siv(lib, k, tag=tag) == ERR_ARG and "lies in the data" in err(lib)
    for tag_in in (A + 4096, A + 4096 + 60):
        assert _siv(lib, k, d=DEC, tag_in=tag_in) == ERR_ARG and "lies in the data" in err(lib)
    assert _siv(lib, k, inp=A, out=A, tag=A + 64 - 4) == ERR_ARG  # in place: the last word of the data
