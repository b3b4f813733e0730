"""Fault injection against the native device API (csrc/hip/engine.cpp and
aead.cpp, C API csrc/include/otc.h) without a GPU: every bad argument -- misaligned or null
pointers, partial overlaps, bad lengths, wrong key schedules, size overflow --
must be rejected with OTC_ERR_ARG and a message *before* any HIP call, so the
fake pointers below are never dereferenced.  (The reference checks nothing:
AES.cu:217-254 ignores every CUDA return code; SURVEY.md section 5 "Failure
detection".)"""
import ctypes

import pytest

from our_tree_amd import _native

ERR_ARG = -1
ENC, DEC = 1, 0
A = 0x7F0000000000  # fake, 16-byte aligned device addresses (never touched)


@pytest.fixture(scope="module")
def lib():
    if not _native.gpu_lib_available():
        pytest.skip("libotc.so not built")
    return _native.require_gpu_lib()


def key(lib, bits=128, d=ENC):
    k = _native.OtcAesKey()
    assert lib.otc_aes_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(bits // 8))), bits, d) == 0
    return k


def err(lib) -> str:
    return lib.otc_last_error().decode()


def c16():
    return (ctypes.c_uint8 * 16)()


def test_key_init_rejects_bad_sizes(lib):
    k = _native.OtcAesKey()
    assert lib.otc_aes_key_init(ctypes.byref(k), _native.as_u8p(bytes(20)), 160, ENC) == ERR_ARG
    assert "128/192/256" in err(lib)


@pytest.mark.parametrize("inp,out,what", [
    (A + 1, A + 4096, "aligned"),
    (A, A + 4096 + 8, "aligned"),
    (None, A, "null"),
    (A, None, "null"),
    (A, A + 16, "overlap"),
    (A + 32, A, "overlap"),
])
def test_ctr_rejects_bad_buffers(lib, inp, out, what):
    k = key(lib)
    rc = lib.otc_aes_ctr(inp, out, 1024, ctypes.byref(k), c16(), 0, 0, None)
    assert rc == ERR_ARG and what in err(lib)


def test_zero_length_is_a_noop(lib):
    k = key(lib)
    assert lib.otc_aes_ctr(None, None, 0, ctypes.byref(k), c16(), 0, 0, None) == 0
    assert lib.otc_aes_ecb(A + 3, A + 5, 0, ctypes.byref(k), 0, None) == 0


def test_ecb_length_and_alignment(lib):
    k = key(lib)
    assert lib.otc_aes_ecb(A, A + 4096, 17, ctypes.byref(k), 0, None) == ERR_ARG
    assert "multiple of 16" in err(lib)
    assert lib.otc_aes_ecb(A + 8, A + 4096, 32, ctypes.byref(k), 0, None) == ERR_ARG


def test_wrong_schedule_direction(lib):
    kd = key(lib, 256, DEC)
    assert lib.otc_aes_ctr(A, A + 4096, 64, ctypes.byref(kd), c16(), 0, 0, None) == ERR_ARG
    assert "encryption schedule" in err(lib)
    ke = key(lib, 192, ENC)
    assert lib.otc_aes_cbc_decrypt(A, A + 4096, 64, ctypes.byref(ke), c16(), None) == ERR_ARG
    assert "decryption schedule" in err(lib)


def test_cbc_cfb_in_place_rules(lib):
    kd, ke = key(lib, 128, DEC), key(lib, 128, ENC)
    assert lib.otc_aes_cbc_decrypt(A, A, 64, ctypes.byref(kd), c16(), None) == ERR_ARG
    assert "in-place" in err(lib)
    assert lib.otc_aes_cfb128_decrypt(A, A, 64, ctypes.byref(ke), c16(), None) == ERR_ARG
    assert lib.otc_aes_cbc_decrypt_segments(A, A, 64, 4, ctypes.byref(kd), c16(), None) == ERR_ARG
    assert lib.otc_aes_cbc_decrypt(A, A + 4096, 64, ctypes.byref(kd), None, None) == ERR_ARG
    assert "null iv" in err(lib)


def test_segment_size_overflow(lib):
    k = key(lib)
    big = 1 << 62
    assert lib.otc_aes_cbc_encrypt_segments(A, A + 4096, big, 16, ctypes.byref(k), c16(), None) == ERR_ARG
    assert "overflow" in err(lib)
    assert lib.otc_aes_cbc_encrypt_segments(A, A + 4096, 20, 2, ctypes.byref(k), c16(), None) == ERR_ARG


def test_stream_ops_validation(lib):
    assert lib.otc_xor(A + 4, A + 4096, A + 8192, 64, None) == ERR_ARG
    assert lib.otc_xor(A, A + 4096, A + 4096 + 16, 64, None) == ERR_ARG  # b overlaps out
    assert lib.otc_checksum(A + 4, 64, A + 4096, None) == ERR_ARG
    assert lib.otc_checksum(A, 63, A + 4096, None) == ERR_ARG
    assert lib.otc_rc4_multi(A, 0, 4, 16, 0, None, A + 4096, None) == ERR_ARG
    assert lib.otc_rc4_multi(A, 257, 4, 16, 0, None, A + 4096, None) == ERR_ARG
    assert lib.otc_rc4_multi(A, 16, 4, 64, 0, A, A + 16, None) == ERR_ARG
    assert "overlap" in err(lib)
    assert lib.otc_fill_random(A + 2, 64, 1, None) == ERR_ARG


def test_engine_and_multi_reject_bad_arguments(lib):
    assert lib.otc_engine_run(None, 1, None, None, 16, None, None, 0, 0, None) == ERR_ARG
    st = _native.MultiStats() if hasattr(_native, "MultiStats") else None
    rc = lib.otc_multi_run(0, 0, 1, None, None, 16, None, None, 0, 0,
                           ctypes.byref(st) if st is not None else None)
    assert rc == ERR_ARG


@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("dec", [False, True])
def test_aesni_schedule_bytes_equal_kernel_schedule(lib, bits, dec):
    """otc_aesni.h passes AES-NI schedules straight to the kernels: the
    AES_*_Key_Expansion / AES_Key_Expansion_Dec bytes must equal the PolarSSL
    word schedule (otc_aes_key.rk) byte for byte."""
    from our_tree_amd.models import cpu_ref
    if not cpu_ref.aesni_supported():
        pytest.skip("no AES-NI on this CPU")
    kb = bytes((7 * i + 3) & 0xFF for i in range(bits // 8))
    sched, nr = cpu_ref.aesni_schedule(kb, decrypt=dec)
    k = _native.OtcAesKey()
    assert lib.otc_aes_key_init(ctypes.byref(k), _native.as_u8p(kb), bits, DEC if dec else ENC) == 0
    assert k.nr == nr
    assert bytes(k)[: 16 * (nr + 1)] == sched


def test_aesni_shaped_api_rejects_bad_rounds(lib):
    sched = (ctypes.c_uint8 * 240)()
    assert lib.otc_AES_ECB_encrypt(A, A + 4096, 64, sched, 11, None) == ERR_ARG
    assert "number_of_rounds" in err(lib)
    assert lib.otc_AES_CTR_encrypt(A + 1, A + 4096, c16(), c16(), 64, sched, 10, None) == ERR_ARG


class CtrMsg(ctypes.Structure):
    """Mirror of otc_ctr_msg (otc.h)."""
    _fields_ = [("inp", ctypes.c_uint64), ("out", ctypes.c_uint64), ("nbytes", ctypes.c_uint64),
                ("ctr_hi", ctypes.c_uint64), ("ctr_lo", ctypes.c_uint64), ("key", ctypes.c_uint32),
                ("align", ctypes.c_uint32)]


def test_ctr_batch_planner_and_python_plan_agree(lib):
    """The C host planner (otc_ctr_batch_plan) builds the tile map ops.CtrBatch
    builds with numpy: 4 KiB tiles, empty messages own none."""
    import numpy as np

    from our_tree_amd.ops import batch_ops

    sizes = [0, 1, 4096, 4097, 16, 0, 3 * 4096 + 15, 100000, 1504]
    msgs = (CtrMsg * len(sizes))(*[CtrMsg(0, 0, n, 0, 0, 0, 0) for n in sizes])
    fn = lib.otc_ctr_batch_plan
    fn.restype = ctypes.c_uint64
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    for tb in (64, 128, 256):
        nt = fn(msgs, len(sizes), tb, None, None)
        tmap = np.zeros(nt, np.uint32)
        first = np.zeros(len(sizes), np.uint64)
        assert fn(msgs, len(sizes), tb, tmap.ctypes.data, first.ctypes.data) == nt
        tiles = (np.array(sizes, np.uint64) + 16 * tb - 1) // (16 * tb)
        assert nt == tiles.sum()
        assert (tmap == np.repeat(np.arange(len(sizes), dtype=np.uint32), tiles.astype(np.int64))).all()
        assert first[0] == 0 and (first[1:] == np.cumsum(tiles)[:-1]).all()
    assert fn(msgs, len(sizes), 100, None, None) == 0
    # counter-aligned messages (OTC_BATCH_ALIGNED | shift) own ceil((bytes + 16 shift) / tile) tiles
    al = (CtrMsg * 2)(CtrMsg(0, 0, 4096 * 10, 0, 0, 0, 0x80000000 | 5), CtrMsg(0, 0, 4096 * 10, 0, 0, 0, 0x80000000))
    assert fn(al, 2, 256, None, None) == 11 + 10
    # tile choice: 4 KiB messages fill 256-block tiles exactly, 1 KiB ones 64-block tiles
    assert batch_ops._pick_tile(np.full(100, 4096, np.uint64)) == 256
    assert batch_ops._pick_tile(np.full(100, 1024, np.uint64)) == 64


def test_ctr_batch_rejects_bad_launch_args(lib):
    f = lib.otc_aes_ctr_batch
    assert f(A, A, A, A, 0, 256, 10, None) == 0  # nothing to do
    assert f(None, A, A, A, 4, 256, 10, None) == ERR_ARG and "null" in err(lib)
    assert f(A, A, A, A, 4, 256, 11, None) == ERR_ARG and "nr" in err(lib)
    assert f(A, A, A, A, 4, 100, 10, None) == ERR_ARG and "tile_blocks" in err(lib)
    assert f(A + 4, A, A, A, 4, 64, 10, None) == ERR_ARG and "misaligned" in err(lib)


def test_ctr_batch_python_validation_without_gpu():
    import torch

    from our_tree_amd import ops

    x = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one counter"):
        ops.CtrBatch([x], [bytes(16)], [])
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.CtrBatch([x], [bytes(16)], [bytes(16)])
    with pytest.raises(ValueError, match="key_index"):
        ops.CtrBatch([x], [bytes(16)], [bytes(16)], key_index=[3])


def test_packed_batch_validation_without_gpu():
    """Packed-buffer planning rejects bad layouts before touching a device."""
    import torch

    from our_tree_amd import ops

    buf = torch.zeros(4096, dtype=torch.uint8)
    k, c = [bytes(16)], [bytes(16)] * 2
    with pytest.raises(ValueError, match="inside the buffer"):
        ops.CtrBatch.packed(buf, [4000, 200], k, c, key_index=[0, 0])
    with pytest.raises(ValueError, match="multiples of 16"):
        ops.CtrBatch.packed(buf, [10, 10], k, c, offsets=[0, 24], key_index=[0, 0])
    with pytest.raises(ValueError, match="overlap"):
        ops.CtrBatch.packed(buf, [100, 100], k, c, offsets=[0, 64], key_index=[0, 0])
    with pytest.raises(ValueError, match="16-byte counter"):
        ops.CtrBatch.packed(buf, [100, 100], k, [bytes(16)], key_index=[0, 0])
    with pytest.raises(ValueError, match="key_index"):
        ops.CtrBatch.packed(buf, [100, 100], k, c, key_index=[0, 1])
    with pytest.raises(ValueError, match="GPU tensor"):  # layout valid: only the device is wrong
        ops.CtrBatch.packed(buf, [100, 100], k, c, key_index=[0, 0])


def test_rccl_strategy_warns_on_pageable_host_buffers():
    """otc_multi_run strategy 1 enqueues every host copy from one thread, so
    pageable buffers serialise it: the Python API warns before the call
    (VERDICT r2 weak #8); the native call warns once on stderr too."""
    import numpy as np

    from our_tree_amd.parallel import stream as pstream

    x = np.zeros(4096, np.uint8)
    y = np.zeros(4096, np.uint8)
    assert pstream.pageable_buffers(x, y) == [0, 1]
    with pytest.warns(RuntimeWarning, match="host_in and host_out are pageable"):
        with pytest.raises(RuntimeError):  # no GPU here: the native call then refuses
            pstream.multi_gpu_run("ctr", x, y, bytes(16), bytes(16), ngpus=1, strategy="rccl")


# ---- XTS, CTR32, GHASH, GCM, ChaCha20, Poly1305, the AEADs, batched GCM, RC4 states ----
# Every case below is refused by argument validation (or is a zero-length
# no-op) before any HIP call: these tests also run where a GPU is present, and
# a fake pointer that passed validation would be dereferenced by a kernel.
# The whole message is pinned, not a substring: the messages are API.
B = A + (1 << 40)  # a second fake buffer, far from A
NOT_ENC = "key schedule is not an encryption schedule"
GCM_MAX = (1 << 36) - 32          # AES_GCM_MAX_BYTES (aes.h)
CCP_MAX = ((1 << 32) - 1) * 64    # CHACHA20_POLY1305_MAX_BYTES (chacha.h)


def refused(lib, rc, msg):
    assert rc == ERR_ARG
    assert err(lib) == msg


def buffer_cases(what, misaligned=True):
    """(in, out, whole message) of what check_bufs refuses, over 1024 bytes"""
    al = [(A + 1, B, "device buffers must be 16-byte aligned"),
          (A, B + 8, "device buffers must be 16-byte aligned")] if misaligned else []
    return [(i, o, f"{what}: {m}") for i, o, m in al + [
        (None, B, "null buffer"), (A, None, "null buffer"),
        (A, A + 16, "input and output overlap partially"),
        (A + 1008, A, "input and output overlap partially")]]


def xts_key(lib, bits=256, d=ENC):
    k = _native.OtcXtsKey()
    assert lib.otc_xts_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(bits // 8))), bits, d) == 0
    return k


def gcm_key(lib, bits=128):
    k = _native.OtcGcmKey()
    assert lib.otc_gcm_key_init(ctypes.byref(k), _native.as_u8p(bytes(range(bits // 8))), bits) == 0
    return k


def test_xts_key_init_rejects_bad_arguments(lib):
    k = _native.OtcXtsKey()
    kb = _native.as_u8p(bytes(64))
    refused(lib, lib.otc_xts_key_init(None, kb, 256, ENC), "null argument")
    refused(lib, lib.otc_xts_key_init(ctypes.byref(k), kb, 384, ENC),
            "invalid XTS key size (K1 || K2 must be 256 or 512 bits)")
    refused(lib, lib.otc_xts_key_init(ctypes.byref(k), kb, 256, 2), "bad direction")


@pytest.mark.parametrize("inp,out,msg", buffer_cases("aes_xts"))
def test_xts_rejects_bad_buffers(lib, inp, out, msg):
    k = xts_key(lib)
    refused(lib, lib.otc_aes_xts(inp, out, 512, 2, ctypes.byref(k), c16(), None), msg)


def test_xts_rejects_bad_units_and_keys(lib):
    k = xts_key(lib)
    f = lib.otc_aes_xts
    refused(lib, f(A, B, 512, 2, None, c16(), None), "null key")
    refused(lib, f(A, B, 512, 2, ctypes.byref(k), None, None), "null tweak")
    refused(lib, f(A, B, 15, 1, ctypes.byref(k), c16(), None), "XTS data unit must be at least 16 bytes")
    refused(lib, f(A, B, (16 << 20) + 16, 1, ctypes.byref(k), c16(), None), "XTS data unit above 2^20 blocks")
    refused(lib, f(A, B, 520, 2, ctypes.byref(k), c16(), None),
            "XTS data units of several must be multiples of 16 bytes")
    refused(lib, f(A, B, 16 << 20, 1 << 62, ctypes.byref(k), c16(), None), "size overflow")
    assert f(A + 3, None, 512, 0, ctypes.byref(k), c16(), None) == 0  # no units: nothing to do
    # the tweak key is always an encryption schedule; the two halves have one size, 128 or 256
    bad = xts_key(lib)
    bad.tweak = key(lib, 128, DEC)
    refused(lib, f(A, B, 512, 2, ctypes.byref(bad), c16(), None), NOT_ENC)
    bad = xts_key(lib)
    bad.data = key(lib, 256, ENC)
    refused(lib, f(A, B, 512, 2, ctypes.byref(bad), c16(), None),
            "bad XTS key (two AES-128 or two AES-256 schedules)")
    bad.data = bad.tweak = key(lib, 192, ENC)
    refused(lib, f(A, B, 512, 2, ctypes.byref(bad), c16(), None),
            "bad XTS key (two AES-128 or two AES-256 schedules)")


@pytest.mark.parametrize("inp,out,msg", buffer_cases("aes_ctr32"))
def test_ctr32_rejects_bad_buffers(lib, inp, out, msg):
    k = key(lib)
    refused(lib, lib.otc_aes_ctr32(inp, out, 1024, ctypes.byref(k), c16(), 0, None), msg)


def test_ctr32_rejects_bad_arguments(lib):
    k, kd = key(lib), key(lib, 128, DEC)
    f = lib.otc_aes_ctr32
    refused(lib, f(A, B, 1024, ctypes.byref(k), None, 0, None), "null counter")
    refused(lib, f(A, B, (1 << 36) + 1, ctypes.byref(k), c16(), 0, None), "ctr32: more than 2^32 blocks")
    refused(lib, f(A, B, 1024, ctypes.byref(kd), c16(), 0, None), NOT_ENC)
    refused(lib, f(A, B, 1024, None, c16(), 0, None), "null key")
    # across the wrap of the low word the head is checked like any call, before anything runs
    wrap = (ctypes.c_uint8 * 16)(*([0] * 12 + [0xFF] * 4))
    refused(lib, f(A, B, 1024, ctypes.byref(kd), wrap, 0, None), NOT_ENC)
    assert f(None, None, 0, ctypes.byref(k), c16(), 0, None) == 0


def test_ghash_rejects_bad_arguments(lib):
    f = lib.otc_ghash
    h, y0 = c16(), c16()
    refused(lib, f(A, 1024, None, y0, B, None), "null argument")
    refused(lib, f(A, 1024, h, None, B, None), "null argument")
    refused(lib, f(A, 1024, h, y0, None, None), "null argument")
    refused(lib, f(A, 1024, h, y0, B + 2, None), "ghash: the result must be 4-byte aligned")
    refused(lib, f(A, (1 << 36) + 1, h, y0, B, None), "ghash: more than 2^36 bytes")
    refused(lib, f(None, 1024, h, y0, B, None), "ghash: null buffer")
    refused(lib, f(A + 8, 1024, h, y0, B, None), "ghash: device buffers must be 16-byte aligned")


def test_gcm_key_init_rejects_bad_arguments(lib):
    k = _native.OtcGcmKey()
    refused(lib, lib.otc_gcm_key_init(None, _native.as_u8p(bytes(16)), 128), "null argument")
    refused(lib, lib.otc_gcm_key_init(ctypes.byref(k), None, 128), "null argument")
    refused(lib, lib.otc_gcm_key_init(ctypes.byref(k), _native.as_u8p(bytes(20)), 160),
            "invalid AES key size (must be 128/192/256)")


def gcm_call(lib, inp=A, out=B, n=1024, k="ok", d=ENC, iv=b"\0" * 12, iv_len=12, aad=None, aad_len=0, tag=B + 4096,
             impl=0):
    if isinstance(k, str):
        k = ctypes.byref(gcm_key(lib))
    return lib.otc_aes_gcm(inp, out, n, k, d, _native.as_u8p(iv) if iv is not None else None, iv_len,
                           _native.as_u8p(aad) if aad is not None else None, aad_len, tag, impl, None)


@pytest.mark.parametrize("d", [ENC, DEC])
@pytest.mark.parametrize("inp,out,msg", buffer_cases("aes_gcm"))
def test_gcm_rejects_bad_buffers(lib, inp, out, msg, d):
    refused(lib, gcm_call(lib, inp, out, d=d), msg)


def test_gcm_rejects_bad_arguments(lib):
    refused(lib, gcm_call(lib, k=None), "null key")
    bad = gcm_key(lib)
    bad.enc = key(lib, 128, DEC)
    refused(lib, gcm_call(lib, k=ctypes.byref(bad)), NOT_ENC)
    refused(lib, gcm_call(lib, d=2), "bad direction")
    refused(lib, gcm_call(lib, iv=None), "gcm: the IV must have at least 1 byte")
    refused(lib, gcm_call(lib, iv_len=0), "gcm: the IV must have at least 1 byte")
    refused(lib, gcm_call(lib, aad_len=5), "gcm: null aad")
    refused(lib, gcm_call(lib, iv_len=1 << 61), "gcm: IV or AAD too long")
    refused(lib, gcm_call(lib, aad=b"x", aad_len=1 << 61), "gcm: IV or AAD too long")
    refused(lib, gcm_call(lib, tag=None), "gcm: the tag must be 4-byte aligned device memory")
    refused(lib, gcm_call(lib, tag=B + 4098), "gcm: the tag must be 4-byte aligned device memory")
    refused(lib, gcm_call(lib, n=GCM_MAX + 1), "gcm: a message has at most 2^36 - 32 bytes")
    refused(lib, gcm_call(lib, impl=99), "impl must be OTC_IMPL_AUTO, OTC_IMPL_TTABLE, OTC_IMPL_BITSLICE or OTC_IMPL_SPLIT")
    # which error wins: the direction before the IV, the tag before the length, the length before the buffers
    refused(lib, gcm_call(lib, d=7, iv=None, tag=None), "bad direction")
    refused(lib, gcm_call(lib, inp=None, n=GCM_MAX + 1, tag=B + 1), "gcm: the tag must be 4-byte aligned device memory")
    refused(lib, gcm_call(lib, inp=A + 1, n=GCM_MAX + 1), "gcm: a message has at most 2^36 - 32 bytes")


def test_chacha20_rejects_bad_arguments(lib):
    f = lib.otc_chacha20
    k32, n12 = _native.as_u8p(bytes(32)), _native.as_u8p(bytes(12))
    refused(lib, f(A, B, 1024, None, n12, 0, None), "chacha20: null key or nonce")
    refused(lib, f(A, B, 1024, k32, None, 0, None), "chacha20: null key or nonce")
    refused(lib, f(None, B, 1024, k32, n12, 0, None), "chacha20: null buffer")
    refused(lib, f(A, None, 1024, k32, n12, 0, None), "chacha20: null buffer")
    # any alignment is allowed; a partial overlap is not, in either direction
    refused(lib, f(A + 3, A + 4, 1024, k32, n12, 0, None), "chacha20: input and output overlap partially")
    refused(lib, f(A + 1023, A, 1024, k32, n12, 0, None), "chacha20: input and output overlap partially")
    # blocks counter .. counter + nblk - 1 must stay below 2^32
    wrap = "chacha20: the 32-bit block counter would pass 2^32 - 1"
    refused(lib, f(A, B, 65, k32, n12, 0xFFFFFFFF, None), wrap)
    refused(lib, f(A, B, 64 * 3 + 1, k32, n12, 0xFFFFFFFD, None), wrap)
    refused(lib, f(None, None, (1 << 38) + 1, k32, n12, 0, None), wrap)  # the counter before the buffers
    assert f(None, None, 0, k32, n12, 0xFFFFFFFF, None) == 0


def test_poly1305_rejects_bad_arguments(lib):
    f = lib.otc_poly1305
    k32 = _native.as_u8p(bytes(32))
    refused(lib, f(A, 1024, None, B, None), "poly1305: null argument")
    refused(lib, f(A, 1024, k32, None, None), "poly1305: null argument")
    refused(lib, f(A, 1024, k32, B + 2, None), "poly1305: the tag must be 4-byte aligned")
    refused(lib, f(None, 1024, k32, B, None), "poly1305: null buffer")
    refused(lib, f(A + 4, 1024, k32, B, None), "poly1305: device buffers must be 16-byte aligned")


def ccp_call(lib, inp=A, out=B, n=1024, k=b"\1" * 32, d=ENC, nonce=b"\0" * 12, aad=None, aad_len=0, tag=B + 4096):
    u8 = lambda v: _native.as_u8p(v) if v is not None else None  # noqa: E731
    return lib.otc_chacha20_poly1305(inp, out, n, u8(k), d, u8(nonce), u8(aad), aad_len, tag, None)


@pytest.mark.parametrize("d", [ENC, DEC])
@pytest.mark.parametrize("inp,out,msg", buffer_cases("chacha20_poly1305"))
def test_chacha20_poly1305_rejects_bad_buffers(lib, inp, out, msg, d):
    refused(lib, ccp_call(lib, inp, out, d=d), msg)


def test_chacha20_poly1305_rejects_bad_arguments(lib):
    refused(lib, ccp_call(lib, k=None), "chacha20_poly1305: null key or nonce")
    refused(lib, ccp_call(lib, nonce=None), "chacha20_poly1305: null key or nonce")
    refused(lib, ccp_call(lib, d=-1), "bad direction")
    refused(lib, ccp_call(lib, aad_len=3), "chacha20_poly1305: null aad")
    refused(lib, ccp_call(lib, tag=None), "chacha20_poly1305: the tag must be 4-byte aligned device memory")
    refused(lib, ccp_call(lib, tag=B + 4097), "chacha20_poly1305: the tag must be 4-byte aligned device memory")
    refused(lib, ccp_call(lib, n=CCP_MAX + 1), "chacha20_poly1305: a message has at most (2^32 - 1) * 64 bytes")
    # which error wins: the tag before the length, the length before the buffers
    refused(lib, ccp_call(lib, inp=None, n=CCP_MAX + 1, tag=B + 2),
            "chacha20_poly1305: the tag must be 4-byte aligned device memory")
    refused(lib, ccp_call(lib, inp=A + 1, n=CCP_MAX + 1),
            "chacha20_poly1305: a message has at most (2^32 - 1) * 64 bytes")


class GcmMsg(ctypes.Structure):
    """Mirror of otc_gcm_msg (otc.h)."""
    _fields_ = [("inp", ctypes.c_uint64), ("out", ctypes.c_uint64), ("nbytes", ctypes.c_uint64),
                ("aad", ctypes.c_uint64), ("aad_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


def test_gcm_batch_plan_rejects_bad_records(lib):
    f = lib.otc_gcm_batch_plan

    def plan(recs, tb=256):
        arr = (GcmMsg * len(recs))(*[GcmMsg(*r, 0) for r in recs])
        return f(arr, len(recs), tb, None, None, None)

    ok = (A, B, 4096, 0, 0)
    assert plan([ok, (A + 8192, A + 8192, 100, 0, 0), (0, 0, 0, 0, 0)]) == 2
    refused(lib, plan([ok], 100), "gcm_batch: tile_blocks must be 64, 128 or 256")
    refused(lib, f(None, 2, 64, None, None, None), "gcm_batch: null descriptors")
    assert f(None, 0, 64, None, None, None) == 0
    refused(lib, plan([ok, (A + 8192, A + 8192 + 16, 4096, 0, 0)]),
            "gcm_batch: record 1: input and output overlap partially")
    refused(lib, plan([ok, (A + 8192 + 32, A + 8192, 4096, 0, 0)]),
            "gcm_batch: record 1: input and output overlap partially")
    refused(lib, plan([(A + 4, B, 64, 0, 0)]), "gcm_batch: record 0: data buffers must be 16-byte aligned")
    refused(lib, plan([ok, (0, B + 8192, 64, 0, 0)]), "gcm_batch: record 1: null buffer")
    refused(lib, plan([(A, B, (1 << 20) + 1, 0, 0)]), "gcm_batch: record 0: more than 1 MiB of data (use otc_aes_gcm)")
    refused(lib, plan([(A, B, 64, A, (1 << 16) + 1)]), "gcm_batch: record 0: more than 64 KiB of AAD")
    refused(lib, plan([(A, B, 64, 0, 5)]), "gcm_batch: record 0: null aad")
    refused(lib, plan([ok, (A + 8192, B + 4000, 4096, 0, 0)]), "gcm_batch: record 1: its output overlaps another record's")
    refused(lib, plan([ok, (B + 4000, A + 8192, 4096, 0, 0)]),
            "gcm_batch: record 1: its input overlaps another record's output")
    refused(lib, plan([ok, (A + 8192, B + 8192, 64, B + 4090, 16)]), "gcm_batch: record 1: its AAD overlaps a record's output")


def test_gcm_batch_tables_and_hash_reject_bad_launch_args(lib):
    k = gcm_key(lib)
    t = lib.otc_gcm_batch_tables
    refused(lib, t(None, A, None), "null key")
    bad = gcm_key(lib)
    bad.enc = key(lib, 128, DEC)
    refused(lib, t(ctypes.byref(bad), A, None), NOT_ENC)
    refused(lib, t(ctypes.byref(k), None, None), "gcm_batch: the tables must be 16-byte aligned device memory")
    refused(lib, t(ctypes.byref(k), A + 8, None), "gcm_batch: the tables must be 16-byte aligned device memory")
    g = lib.otc_ghash_batch
    assert g(None, 0, None, None, 5, None) == 0  # nothing to do
    refused(lib, g(A, 4, A + 4096, B, 32, None), "gcm_batch: lanes must be 16 or 64 (0: 64)")
    refused(lib, g(None, 4, A + 4096, B, 16, None), "gcm_batch: null array")
    refused(lib, g(A, 4, None, B, 64, None), "gcm_batch: null array")
    refused(lib, g(A, 4, A + 4096, None, 0, None), "gcm_batch: null array")
    refused(lib, g(A + 4, 4, A + 4096, B, 0, None), "gcm_batch: misaligned descriptor array")
    refused(lib, g(A, 4, A + 4096 + 8, B, 0, None), "gcm_batch: the tables must be 16-byte aligned")
    refused(lib, g(A, 4, A + 4096, B + 8, 0, None), "gcm_batch: the hash array must be 16-byte aligned")


def gcm_batch_call(lib, **kw):
    """otc_aes_gcm_batch over 4 records with fake, well-formed arrays; kw replaces arguments by name"""
    a = dict(msgs=A, ctr_msgs=A + 0x1000, tile_msg=A + 0x2000, tile_first=A + 0x3000, ntiles=4, tile_blocks=256,
             nmsg=4, k="ok", key_dev=A + 0x4000, tab=A + 0x10000, d=ENC, ivs=A + 0x5000, tags=A + 0x6000,
             expect=A + 0x7000, tag_bytes=16, ok=A + 0x8000, ws=A + 0x9000, lanes=0)
    a.update(kw)
    if isinstance(a["k"], str):
        a["k"] = ctypes.byref(gcm_key(lib))
    return lib.otc_aes_gcm_batch(a["msgs"], a["ctr_msgs"], a["tile_msg"], a["tile_first"], a["ntiles"], a["tile_blocks"],
                                 a["nmsg"], a["k"], a["key_dev"], a["tab"], a["d"], a["ivs"], a["tags"], a["expect"],
                                 a["tag_bytes"], a["ok"], a["ws"], a["lanes"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(k=None), "null key"),
    (dict(d=2), "bad direction"),
    (dict(tile_blocks=100), "gcm_batch: tile_blocks must be 64, 128 or 256"),
    (dict(tile_blocks=0), "gcm_batch: tile_blocks must be 64, 128 or 256"),
    (dict(tag_bytes=3), "gcm_batch: a tag has 4 to 16 bytes"),
    (dict(tag_bytes=17), "gcm_batch: a tag has 4 to 16 bytes"),
    (dict(lanes=32), "gcm_batch: lanes must be 16 or 64 (0: 64)"),
    (dict(msgs=None), "gcm_batch: null array"),
    (dict(tab=None), "gcm_batch: null array"),
    (dict(tags=None), "gcm_batch: null array"),
    (dict(msgs=A + 4), "gcm_batch: misaligned descriptor array"),
    (dict(tab=A + 0x10008), "gcm_batch: the tables must be 16-byte aligned"),
    (dict(tags=A + 0x6008), "gcm_batch: the tag array must be 16-byte aligned"),
    (dict(ctr_msgs=None), "gcm_batch: null array"),
    (dict(key_dev=None), "gcm_batch: null array"),
    (dict(ws=None), "gcm_batch: null array"),
    (dict(tile_msg=None), "gcm_batch: null tile map"),
    (dict(tile_first=None), "gcm_batch: null tile map"),
    (dict(ctr_msgs=A + 0x1004), "gcm_batch: misaligned descriptor arrays"),
    (dict(key_dev=A + 0x4004), "gcm_batch: misaligned descriptor arrays"),
    (dict(tile_first=A + 0x3004), "gcm_batch: misaligned descriptor arrays"),
    (dict(tile_msg=A + 0x2002), "gcm_batch: misaligned descriptor arrays"),
    (dict(ws=A + 0x9008), "gcm_batch: the workspace must be 16-byte aligned"),
    (dict(d=DEC, expect=None), "gcm_batch: decryption needs the expected tags and the verdict array"),
    (dict(d=DEC, ok=None), "gcm_batch: decryption needs the expected tags and the verdict array"),
    (dict(d=DEC, expect=A + 0x6000 + 48), "gcm_batch: the expected tags overlap the computed tags or the verdicts"),
    (dict(d=DEC, expect=A + 0x6000 - 8, tag_bytes=4),
     "gcm_batch: the expected tags overlap the computed tags or the verdicts"),
    (dict(d=DEC, expect=A + 0x8000 - 60), "gcm_batch: the expected tags overlap the computed tags or the verdicts"),
    (dict(d=DEC, expect=A + 0x8003, tag_bytes=4),
     "gcm_batch: the expected tags overlap the computed tags or the verdicts"),
    (dict(ivs=None), "gcm_batch: null IVs"),
    (dict(d=DEC, ivs=None), "gcm_batch: null IVs"),
    # which error wins
    (dict(d=5, tile_blocks=1, tag_bytes=0), "bad direction"),
    (dict(tile_blocks=1, tag_bytes=0), "gcm_batch: tile_blocks must be 64, 128 or 256"),
    (dict(lanes=1, msgs=None), "gcm_batch: lanes must be 16 or 64 (0: 64)"),
])
def test_gcm_batch_rejects_bad_launch_args(lib, kw, msg):
    refused(lib, gcm_batch_call(lib, **kw), msg)


def test_gcm_batch_wrong_schedule_and_empty_batch(lib):
    bad = gcm_key(lib)
    bad.enc = key(lib, 128, DEC)
    refused(lib, gcm_batch_call(lib, k=ctypes.byref(bad)), NOT_ENC)
    assert gcm_batch_call(lib, nmsg=0, msgs=None, tab=None, tags=None, ivs=None) == 0  # nothing to do


def test_rc4_crypt_batch_rejects_bad_arguments(lib):
    f = lib.otc_rc4_crypt_batch
    S = A + (1 << 41)  # 4 states of 264 bytes
    assert f(None, 0, 64, None, None, None) == 0 and f(None, 4, 0, None, None, None) == 0
    refused(lib, f(None, 4, 64, A, B, None), "rc4_crypt_batch: null buffer")
    refused(lib, f(S, 4, 64, None, B, None), "rc4_crypt_batch: null buffer")
    refused(lib, f(S, 4, 64, A, None, None), "rc4_crypt_batch: null buffer")
    refused(lib, f(S + 2, 4, 64, A, B, None), "rc4_crypt_batch: states must be 4-byte aligned")
    refused(lib, f(S, 1 << 40, 1 << 40, A, B, None), "size overflow")
    refused(lib, f(S, 4, 64, A, A + 16, None), "rc4_crypt_batch: input and output overlap partially")
    refused(lib, f(S, 4, 64, A + 255, A, None), "rc4_crypt_batch: input and output overlap partially")
    refused(lib, f(A + 252, 4, 64, A, B, None), "rc4_crypt_batch: states overlap the input or output")
    refused(lib, f(B - 1052, 4, 64, A, B, None), "rc4_crypt_batch: states overlap the input or output")
    refused(lib, f(A, 4, 64, A, A, None), "rc4_crypt_batch: states overlap the input or output")


def test_rc4_multi_rejects_partial_overlap_both_ways(lib):
    f = lib.otc_rc4_multi
    refused(lib, f(A, 16, 4, 64, 0, A + 4096, A + 4096 + 16, None), "rc4_multi: input and output overlap partially")
    refused(lib, f(A, 16, 4, 64, 0, A + 4096 + 255, A + 4096, None), "rc4_multi: input and output overlap partially")
    refused(lib, f(None, 16, 4, 64, 0, None, B, None), "rc4_multi: null buffer")
    refused(lib, f(A, 16, 1 << 40, 1 << 40, 0, None, B, None), "size overflow")


def test_ctr_stream_rejects_partial_overlap_both_ways(lib):
    ctx, k = _native.OtcCtrCtx(), key(lib)
    assert lib.otc_aes_ctr_ctx_init(ctypes.byref(ctx), c16()) == 0
    f = lib.otc_aes_ctr_stream
    refused(lib, f(ctypes.byref(ctx), ctypes.byref(k), 100, A, A + 16, 0, None),
            "aes_ctr_stream: input and output overlap partially")
    refused(lib, f(ctypes.byref(ctx), ctypes.byref(k), 100, A + 99, A, 0, None),
            "aes_ctr_stream: input and output overlap partially")
    refused(lib, f(ctypes.byref(ctx), ctypes.byref(k), 100, None, A, 0, None), "aes_ctr_stream: null buffer")
    refused(lib, f(ctypes.byref(ctx), ctypes.byref(k), 100, A + 1, B, 0, None),
            "aes_ctr_stream: in and out must have the same alignment modulo 16")


def spans_of(fn):
    buf = (ctypes.c_uint64 * 8)()
    n = fn(buf, 8)
    return n, list(buf[:n])


def test_hash_span_lists(lib):
    """The boundaries the GPU tests walk (tests/test_gpu_gcm.py, test_gpu_chacha.py, test_gpu_gcm_batch.py):
    bytes for the two level hashes, hashed blocks for the batched one."""
    want = [
        (lib.otc_ghash_spans, [1024, 8192, 32768, 524288, 67108864, 137438953472]),
        (lib.otc_poly1305_spans, [1024, 4096, 32768, 131072, 67108864, 137438953472]),
        (lib.otc_gcm_batch_spans, [16, 64, 256]),
    ]
    for fn, spans in want:
        assert spans_of(fn) == (len(spans), spans)
        # a short array gets the first `max`, no array nothing: the count comes back all the same
        buf = (ctypes.c_uint64 * 8)(*([0xAA] * 8))
        assert fn(buf, 2) == len(spans)
        assert list(buf) == spans[:2] + [0xAA] * 6
        assert fn(buf, 0) == len(spans) and list(buf) == spans[:2] + [0xAA] * 6
        assert fn(None, 8) == len(spans)
        assert fn(None, 0) == len(spans)
