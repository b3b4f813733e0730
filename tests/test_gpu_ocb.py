"""AES-OCB3 on the device (csrc/hip/aes_ocb.hip through ops.ocb_ops) against
the C oracle, byte for byte: the lengths around a block and around every
boundary the bulk kernel reports, a second grid step, the golden vectors, tag,
nonce and AAD lengths, in place, misaligned views, the block primitive at block
indices up to 2^32, tampering, and the argument errors of the C API."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import AES, cpu_ref
from our_tree_amd.models.cpu_ref import OcbTagError

ocb = ops.ocb_ops
pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ocb_vectors.json")) as f:
    VEC = json.load(f)["ocb"]
H = bytes.fromhex
MIB = 1 << 20
KEYS = {128: bytes(range(0x10, 0x20)), 192: bytes(range(0x30, 0x48)), 256: bytes(range(0x60, 0x80))}
NONCE = bytes(range(0x40, 0x4C))
AAD13 = bytes(range(0x80, 0x8D))
POOL_BYTES = 130 * MIB  # one pool of random bytes: every test takes a prefix


def host(t):
    return t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def dev(b, gpu):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)


@pytest.fixture(scope="module")
def pool(gpu):
    """Seeded random bytes, on the host and on the device, made once."""
    b = np.random.default_rng(7253).integers(0, 256, POOL_BYTES, dtype=np.uint8)
    return {"host": b.tobytes(), "dev": torch.from_numpy(b).to(gpu)}


def _both_ways(pool, gpu, bits, n, nonce=NONCE, aad=b"", tl=16, decrypt_too=True):
    """Encryption of the pool's first n bytes equals the oracle's, tag included;
    the authenticated decryption of that ciphertext gives the plaintext back."""
    key, pt = KEYS[bits], pool["host"][:n]
    ct, tag = cpu_ref.ocb(key, nonce, pt, aad, tag_bytes=tl)
    out, t = ocb.ocb_encrypt(pool["dev"][:n], key, nonce, aad, tag_bytes=tl)
    assert t.shape == (tl,) and t.dtype == torch.uint8
    assert host(t) == tag, f"tag, n={n}"
    assert torch.equal(out, dev(ct, gpu)), f"ciphertext, n={n}"
    assert ops.last_impl() == "ttable"
    if decrypt_too:
        back = ocb.ocb_decrypt(out, key, nonce, tag, aad)
        assert torch.equal(back, pool["dev"][:n]), f"decryption, n={n}"


@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 65541])
def test_lengths(pool, gpu, bits, n):
    _both_ways(pool, gpu, bits, n, aad=AAD13)


def test_spans_are_the_kernels_boundaries(gpu):
    s = ocb.ocb_spans()
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert s == [16, 1024, 4096, 32768, 512 * 1024, cus * 512 * 1024] and s == sorted(s)


SPANS_TO_64M = [16, 1024, 4096, 32768, 512 * 1024]  # the parametrisation needs them before a device is there


def test_the_span_cases_are_every_span_to_64_mib(gpu):
    assert SPANS_TO_64M == [s for s in ocb.ocb_spans() if s <= 64 * MIB]


@pytest.mark.parametrize("decrypt", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("span", SPANS_TO_64M)
def test_around_every_span(pool, gpu, bits, span, decrypt):
    assert span in ocb.ocb_spans() and span <= 64 * MIB
    key = KEYS[bits]
    for n in (span - 16, span - 1, span, span + 1, span + 16):
        x = pool["host"][:n]  # taken as a ciphertext when decrypting
        want, tag = cpu_ref.ocb(key, NONCE, x, AAD13, decrypt=decrypt)
        if decrypt:
            got = ocb.ocb_decrypt(pool["dev"][:n], key, NONCE, tag, AAD13)
        else:
            got, t = ocb.ocb_encrypt(pool["dev"][:n], key, NONCE, AAD13)
            assert host(t) == tag, n
        assert torch.equal(got, dev(want, gpu)), n


def test_second_grid_step(pool, gpu):
    """Past the full grid's first step some workgroups take a second chunk, one
    of them a partial one, and the last run ends in the middle of a pass."""
    grid = ocb.ocb_spans()[-1]
    if grid > 192 * MIB:
        pytest.skip("the full grid's step is above 192 MiB on this device")
    n = grid + 512 * 1024 + 3 * 32768 + 4097
    assert n <= POOL_BYTES
    _both_ways(pool, gpu, 128, n, aad=AAD13)


@pytest.mark.parametrize("v", VEC, ids=[v["name"] for v in VEC])
def test_golden_vectors_on_the_device(gpu, v):
    key, nonce, aad, pt = H(v["key"]), H(v["nonce"]), H(v["aad"]), H(v["pt"])
    out, tag = ocb.ocb_encrypt(dev(pt, gpu), key, nonce, aad, tag_bytes=v["tag_bytes"])
    assert (host(out).hex(), host(tag).hex()) == (v["ct"], v["tag"])
    assert host(ocb.ocb_decrypt(out, key, nonce, H(v["tag"]), aad)) == pt


@pytest.mark.parametrize("nl", [1, 15])
@pytest.mark.parametrize("tl", [8, 12, 16])
@pytest.mark.parametrize("al", [0, 13, 4097])
def test_tag_nonce_and_aad_lengths(pool, gpu, tl, nl, al):
    _both_ways(pool, gpu, 256, 4096 + 77, nonce=bytes(range(0xE0, 0xE0 + nl)), aad=pool["host"][100:100 + al], tl=tl)


def test_tag_bytes_beyond_the_tag_are_zero(pool, gpu):
    """The C call fills all 16 bytes of tag_dev: the tag, then zeros."""
    lib, n, key = _native.require_gpu_lib(), 4096 + 5, KEYS[128]
    k = _native.OtcOcbKey()
    assert lib.otc_ocb_key_init(ctypes.byref(k), _native.as_u8p(key), 128) == 0
    x = pool["dev"][:n].clone()
    out = torch.empty_like(x)
    for direction in (1, 0):
        tag = torch.full((16,), 0xA5, dtype=torch.uint8, device=gpu)
        rc = lib.otc_aes_ocb(x.data_ptr(), out.data_ptr(), n, ctypes.byref(k), direction, _native.as_u8p(NONCE), 12, None, 0,
                             9, tag.data_ptr(), None)
        assert rc == 0
        assert host(tag) == cpu_ref.ocb(key, NONCE, host(x), decrypt=not direction, tag_bytes=9)[1] + bytes(7)


@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("n", [5, 4097, MIB + 7])
def test_in_place_round_trip(pool, gpu, bits, n):
    key, pt = KEYS[bits], pool["host"][:n]
    ct, tag = cpu_ref.ocb(key, NONCE, pt, AAD13)
    x = pool["dev"][:n].clone()
    out, t = ocb.ocb_encrypt(x, key, NONCE, AAD13, out=x)
    assert out.data_ptr() == x.data_ptr() and host(x) == ct and host(t) == tag
    back = ocb.ocb_decrypt(x, key, NONCE, t, AAD13, out=x)
    assert back.data_ptr() == x.data_ptr() and host(x) == pt
    assert host(AES(key).ocb_decrypt(AES(key).ocb_encrypt(x, NONCE, AAD13)[0], NONCE, tag, AAD13)) == pt


@pytest.mark.parametrize("shift", [16, 3])
def test_views_at_byte_offsets(pool, gpu, shift):
    n, key = 65536 + 21, KEYS[192]
    buf = pool["dev"][:n + 64].clone()
    obuf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    x, out = buf[shift:shift + n], obuf[shift:shift + n]
    ct, tag = cpu_ref.ocb(key, NONCE, host(x), AAD13)
    _, t = ocb.ocb_encrypt(x, key, NONCE, AAD13, out=out)
    assert host(out) == ct and host(t) == tag
    assert host(obuf[:shift]) == bytes([0xA5]) * shift and host(obuf[shift + n:]) == bytes([0xA5]) * (64 - shift)
    ocb.ocb_decrypt(out, key, NONCE, tag, AAD13, out=out)
    assert torch.equal(out, x)
    assert host(obuf[:shift]) == bytes([0xA5]) * shift and host(obuf[shift + n:]) == bytes([0xA5]) * (64 - shift)


# ---- the block primitive ----------------------------------------------------------
FIRSTS = [0, 254, (1 << 16) - 5, (1 << 31) - 100, (1 << 32) - 1000]
NBLOCKS = [1, 255, 256, 257, 1000]


@pytest.mark.parametrize("decrypt", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("first", FIRSTS)
def test_blocks_against_the_oracle(pool, gpu, first, decrypt):
    """Output and checksum at block indices near 2^16, 2^31 and 2^32; two chained calls equal one."""
    for bits in (128, 256):
        key = KEYS[bits]
        off0 = cpu_ref.ocb_offset0(key, NONCE)
        for nb in NBLOCKS:
            x = pool["dev"][1024:1024 + 16 * nb]
            want, cs = cpu_ref.ocb_blocks(key, off0, host(x), first, decrypt=decrypt)
            got, c = ocb.ocb_blocks(x, key, off0, first, decrypt=decrypt)
            assert (host(got), host(c)) == (want, cs), (bits, first, nb)
            if nb > 1:
                cut = nb // 3 + 1
                a, acc = ocb.ocb_blocks(x[:16 * cut], key, off0, first, decrypt=decrypt)
                b, acc2 = ocb.ocb_blocks(x[16 * cut:], key, off0, first + cut, checksum=acc, decrypt=decrypt)
                assert acc2.data_ptr() == acc.data_ptr()
                assert (host(a) + host(b), host(acc)) == (want, cs), (bits, first, nb, cut)


def test_blocks_end_exactly_at_the_cap(pool, gpu):
    key, nb = KEYS[128], 1000
    off0 = cpu_ref.ocb_offset0(key, NONCE)
    x = pool["dev"][:16 * nb]
    got, c = ocb.ocb_blocks(x, key, off0, (1 << 32) - nb)
    assert (host(got), host(c)) == cpu_ref.ocb_blocks(key, off0, host(x), (1 << 32) - nb)
    with pytest.raises(ValueError):
        ocb.ocb_blocks(x, key, off0, (1 << 32) - nb + 1)
    with pytest.raises(ValueError):
        ocb.ocb_blocks(pool["dev"][:17], key, off0)


def test_blocks_assemble_a_message(pool, gpu):
    """A message cut into three calls, finished on the host as aes_crypt_ocb does: the AEAD's ciphertext and tag."""
    key, n = KEYS[256], 16 * 5000
    pt = pool["host"][:n]
    ct, tag = cpu_ref.ocb(key, NONCE, pt)
    off0 = cpu_ref.ocb_offset0(key, NONCE)
    acc, outs, at = None, [], 0
    for nb in (300, 2048, 2652):
        o, acc = ocb.ocb_blocks(pool["dev"][16 * at:16 * (at + nb)], key, off0, at, checksum=acc)
        outs.append(host(o))
        at += nb
    assert b"".join(outs) == ct
    x = lambda a, b: bytes(p ^ q for p, q in zip(a, b))
    last = x(x(host(acc), cpu_ref.ocb_offset(key, off0, n // 16)), cpu_ref.ocb_l(key)["dollar"])
    assert cpu_ref.ecb(key, last) == tag  # empty AAD: HASH is zero


# ---- tampering --------------------------------------------------------------------
@pytest.mark.parametrize("n", [4111, MIB + 7])
def test_tampering_zeroes_the_output(pool, gpu, n):
    key = KEYS[128]
    ct, tag = cpu_ref.ocb(key, NONCE, pool["host"][:n], AAD13)
    c = dev(ct, gpu)
    assert torch.equal(ocb.ocb_decrypt(c, key, NONCE, tag, AAD13), pool["dev"][:n])
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x04]) + b[i + 1:]
    bad_c = c.clone()
    bad_c[n // 2] ^= 0x04
    for what, args in (("ciphertext", (bad_c, key, NONCE, tag, AAD13)), ("tag", (c, key, NONCE, flip(tag, 15), AAD13)),
                       ("tag tensor", (c, key, NONCE, dev(flip(tag, 0), gpu), AAD13)),
                       ("aad", (c, key, NONCE, tag, flip(AAD13, 6))),
                       ("nonce", (c, key, flip(NONCE, 11), tag, AAD13))):
        out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
        with pytest.raises(OcbTagError):
            ocb.ocb_decrypt(*args, out=out)
        assert not bool(out.any()), what
    assert issubclass(OcbTagError, ValueError)


# ---- arguments --------------------------------------------------------------------
def test_argument_errors_return_before_any_launch(pool, gpu):
    lib = _native.require_gpu_lib()
    k = _native.OtcOcbKey()
    assert lib.otc_ocb_key_init(ctypes.byref(k), _native.as_u8p(KEYS[128]), 128) == 0
    assert lib.otc_ocb_key_init(ctypes.byref(_native.OtcOcbKey()), _native.as_u8p(KEYS[128]), 100) == -1
    n = 4096
    x = pool["dev"][:n].clone()
    out = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=gpu)
    tag = torch.full((32,), 0xA5, dtype=torch.uint8, device=gpu)
    nonce, off0 = _native.as_u8p(NONCE), _native.as_u8p(bytes(16))
    X, O, T = x.data_ptr(), out.data_ptr(), tag.data_ptr()
    kb = ctypes.byref(k)
    broken = _native.OtcOcbKey.from_buffer_copy(bytes(k))
    broken.dec.dir = 1
    bad = [
        lib.otc_aes_ocb(X, O, n, kb, 1, nonce, 0, None, 0, 16, T, None),            # nonce length 0
        lib.otc_aes_ocb(X, O, n, kb, 1, nonce, 16, None, 0, 16, T, None),           # nonce length 16
        lib.otc_aes_ocb(X, O, n, kb, 1, None, 12, None, 0, 16, T, None),            # no nonce
        lib.otc_aes_ocb(X, O, n, kb, 1, nonce, 12, None, 0, 0, T, None),            # tag_bytes 0
        lib.otc_aes_ocb(X, O, n, kb, 1, nonce, 12, None, 0, 17, T, None),           # tag_bytes 17
        lib.otc_aes_ocb(X, O, (1 << 36) + 1, kb, 1, nonce, 12, None, 0, 16, T, None),  # above the cap
        lib.otc_aes_ocb(X, O + 3, n, kb, 1, nonce, 12, None, 0, 16, T, None),       # misaligned out
        lib.otc_aes_ocb(X + 8, O, n - 8, kb, 1, nonce, 12, None, 0, 16, T, None),   # misaligned in
        lib.otc_aes_ocb(X, O, n, kb, 1, nonce, 12, None, 0, 16, T + 1, None),       # misaligned tag
        lib.otc_aes_ocb(X, O, n, kb, 1, nonce, 12, None, 0, 16, None, None),        # no tag
        lib.otc_aes_ocb(X, X + 16, n - 16, kb, 1, nonce, 12, None, 0, 16, T, None),  # partial overlap
        lib.otc_aes_ocb(X, O, n, kb, 1, nonce, 12, None, 5, 16, T, None),           # AAD length without AAD
        lib.otc_aes_ocb(X, O, n, kb, 2, nonce, 12, None, 0, 16, T, None),           # direction
        lib.otc_aes_ocb(X, O, n, None, 1, nonce, 12, None, 0, 16, T, None),         # no key
        lib.otc_aes_ocb(X, O, n, ctypes.byref(broken), 1, nonce, 12, None, 0, 16, T, None),  # not a decryption schedule
        lib.otc_aes_ocb_blocks(X, O, 2, kb, 1, off0, (1 << 32) - 1, T, None),       # indices past 2^32
        lib.otc_aes_ocb_blocks(X, O, 1, kb, 1, off0, (1 << 32) + 1, T, None),
        lib.otc_aes_ocb_blocks(X, O, 16, kb, 1, off0, 0, T + 4, None),              # misaligned checksum
        lib.otc_aes_ocb_blocks(X, O, 16, kb, 1, off0, 0, None, None),
        lib.otc_aes_ocb_blocks(X, O, 16, kb, 1, None, 0, T, None),                  # no offset
        lib.otc_aes_ocb_blocks(X, O + 3, 16, kb, 1, off0, 0, T, None),
    ]
    assert bad == [-1] * len(bad)  # OTC_ERR_ARG
    assert lib.otc_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((tag == 0xA5).all()) and torch.equal(x, pool["dev"][:n])
    assert lib.otc_aes_ocb(None, None, 0, kb, 1, nonce, 12, None, 0, 16, T, None) == 0  # nothing to read: only the finisher
    assert lib.otc_aes_ocb_blocks(None, None, 0, kb, 1, off0, 7, T + 16, None) == 0  # nothing at all
    torch.cuda.synchronize()
    assert host(tag[:16]) == cpu_ref.ocb(KEYS[128], NONCE, b"")[1] and bool((tag[16:] == 0xA5).all())
    for f in (lambda: ocb.ocb_encrypt(x, KEYS[128], b""), lambda: ocb.ocb_encrypt(x, KEYS[128], bytes(16)),
              lambda: ocb.ocb_encrypt(x, KEYS[128], NONCE, tag_bytes=0), lambda: ocb.ocb_encrypt(x, b"key", NONCE),
              lambda: ocb.ocb_decrypt(x, KEYS[128], NONCE, b""), lambda: ocb.ocb_decrypt(x, KEYS[128], NONCE, bytes(17)),
              lambda: ocb.ocb_encrypt(x, KEYS[128], NONCE, out=out),
              lambda: ocb.ocb_blocks(x, KEYS[128], bytes(15)),
              lambda: ocb.ocb_blocks(x, KEYS[128], bytes(16), checksum=tag[1:17])):
        with pytest.raises(ValueError):
            f()


def test_the_call_allocates_nothing(pool, gpu):
    """With the allocation fault armed the call still succeeds and the fault is
    still pending: nothing was allocated, so there is no failure path to cover."""
    lib, n, key = _native.require_gpu_lib(), MIB + 7, KEYS[256]
    k = _native.OtcOcbKey()
    assert lib.otc_ocb_key_init(ctypes.byref(k), _native.as_u8p(key), 256) == 0
    x = pool["dev"][:n]
    out, tag = torch.empty(n, dtype=torch.uint8, device=gpu), torch.empty(16, dtype=torch.uint8, device=gpu)
    lib.otc_fault_inject_alloc(0)
    try:
        rc = lib.otc_aes_ocb(x.data_ptr(), out.data_ptr(), n, ctypes.byref(k), 1, _native.as_u8p(NONCE), 12,
                             _native.as_u8p(AAD13), 13, 16, tag.data_ptr(), None)
        pending = lib.otc_fault_inject_pending()
    finally:
        lib.otc_fault_inject_alloc(-1)
    assert rc == 0 and pending == 0
    assert (host(out), host(tag)) == cpu_ref.ocb(key, NONCE, pool["host"][:n], AAD13)


def test_captured_in_a_graph(pool, gpu):
    """No synchronisation and no allocation: an encryption and the decryption
    of its result capture into one graph and replay over changed input."""
    lib, n, key = _native.require_gpu_lib(), MIB + 7, KEYS[128]
    k = _native.OtcOcbKey()
    assert lib.otc_ocb_key_init(ctypes.byref(k), _native.as_u8p(key), 128) == 0
    x = pool["dev"][:n].clone()
    c, p = torch.empty_like(x), torch.empty_like(x)
    t1, t2 = torch.empty(16, dtype=torch.uint8, device=gpu), torch.empty(16, dtype=torch.uint8, device=gpu)
    nonce = _native.as_u8p(NONCE)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
        assert lib.otc_aes_ocb(x.data_ptr(), c.data_ptr(), n, ctypes.byref(k), 1, nonce, 12, None, 0, 16, t1.data_ptr(), st) == 0
        assert lib.otc_aes_ocb(c.data_ptr(), p.data_ptr(), n, ctypes.byref(k), 0, nonce, 12, None, 0, 16, t2.data_ptr(), st) == 0
    for off in (0, 4096):
        x.copy_(pool["dev"][off:off + n])
        g.replay()
        torch.cuda.synchronize()
        ct, tag = cpu_ref.ocb(key, NONCE, pool["host"][off:off + n])
        assert host(c) == ct and host(t1) == tag and host(t2) == tag and torch.equal(p, x)
