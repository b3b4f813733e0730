"""AES-GCM on the device: the parallel GHASH kernel (csrc/hip/aes_gcm.hip
through ops.ghash), GCM's counter mode (ops.ctr32) and the authenticated ops
(ops.gcm_encrypt / gcm_decrypt, models.AESGCM), each against the C oracle
(cpu_ref, itself pinned to known answers and libcrypto in tests/test_gcm_cpu.py).

The GHASH shapes come from the kernel's own decomposition (otc_ghash_spans:
a pass of 64 lanes, a batch of passes, a wave's span, a workgroup's spans, a
level-2 span ...): the lengths around every span up to 64 MiB, which include
the first length with a second and a third level and -- 2 x 64 MiB + 5 -- the
first where the grid-stride loop of a 256-CU chip wraps.  Everything is
compared exactly."""
import functools
import json
import os

import pytest
import torch

from our_tree_amd import _native, models, ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "gcm_vectors.json")))["vectors"]


def _fields(v):
    return tuple(bytes.fromhex(v[k]) for k in ("key", "iv", "aad", "pt", "ct", "tag"))


MIB = 1 << 20
CAP = 64 * MIB               # spans up to here are walked around
POOL = 2 * CAP + 64
GUARD = 64

H = bytes.fromhex("66e94bd4ef8a2c3b884cfa59ca342b2e")   # E_0(0), the zero key's hash key
H_ENDS = bytes([0x80] + [0] * 14 + [0x01])               # top and bottom bit: a reflected table shows here
Y0 = bytes(range(0xA0, 0xB0))
KEYS = {16: bytes(range(3, 19)), 24: bytes(range(40, 64)), 32: bytes(range(101, 133))}
IVS = {12: bytes(range(0xC0, 0xCC)), 60: bytes(range(7, 67))}
AADS = {0: b"", 13: bytes(range(13)), 4097: bytes(i * 5 & 0xFF for i in range(4097))}

_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host."""
    if not _pool:
        g = torch.Generator(device=gpu).manual_seed(38)
        dev = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes())
    return _pool


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


# ---- GHASH ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ghash_ref(n, h, y0):
    return cpu_ref.ghash(h, _pool["host"][:n], y0)


def check_ghash(pool, n, h=H, y0=bytes(16)):
    got = host(ops.ghash(pool["dev"][:n], h, y0))
    want = _ghash_ref(n, h, y0)
    print(f"ghash n={n}: {got.hex()} want {want.hex()}")
    assert got == want, n


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 32, 33, 255, 4096, 65541, MIB + 7, 32 * MIB + 5])
def test_ghash_lengths(pool, n):
    check_ghash(pool, n)


def test_ghash_spans_are_reported():
    """At least the two smallest pieces are under the cap, so the lengths
    around them are walked below; they grow, and each is whole blocks."""
    spans = ops.ghash_spans()
    assert len(spans) >= 2 and spans[0] <= CAP and spans[1] <= CAP
    assert spans == sorted(set(spans)) and all(s % 16 == 0 and s > 0 for s in spans)


AROUND = {"S-16": lambda s: s - 16, "S-1": lambda s: s - 1, "S": lambda s: s, "S+1": lambda s: s + 1,
          "S+16": lambda s: s + 16, "2S+5": lambda s: 2 * s + 5}


@pytest.mark.parametrize("where", list(AROUND))
def test_ghash_around_every_span(pool, where):
    spans = [s for s in ops.ghash_spans() if s <= CAP]
    assert len(spans) >= 2
    for s in spans:
        check_ghash(pool, AROUND[where](s))


@pytest.mark.parametrize("n", [1, 16, 33, 4096, 65541, MIB + 7])
def test_ghash_continues_from_y0(pool, n):
    check_ghash(pool, n, H, Y0)


@pytest.mark.parametrize("n", [16, 17, 4096, 65541, MIB + 7])
def test_ghash_key_with_both_end_bits(pool, n):
    check_ghash(pool, n, H_ENDS, Y0)


def test_ghash_empty_returns_y0(pool):
    assert host(ops.ghash(pool["dev"][:0], H, Y0)) == Y0


def test_ghash_split_equals_whole(pool):
    """Two device calls chained through y0 (the second on a view that starts
    mid-buffer, and one that is not 16-byte aligned) equal one call."""
    n, cut = 3 * MIB + 11, MIB + 16 * 3
    mid = host(ops.ghash(pool["dev"][:cut], H, Y0))
    assert host(ops.ghash(pool["dev"][cut:n], H, mid)) == _ghash_ref(n, H, Y0)
    assert host(ops.ghash(pool["dev"][3: 3 + 4099], H)) == cpu_ref.ghash(H, pool["host"][3: 3 + 4099])


def test_ghash_does_not_read_past_the_end(pool, gpu):
    """The bytes after nbytes differ between two buffers; the hashes do not."""
    for n in (1, 17, 4099):
        a = torch.full((n + GUARD,), 0x00, dtype=torch.uint8, device=gpu)
        b = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=gpu)
        a[:n] = pool["dev"][:n]
        b[:n] = pool["dev"][:n]
        assert host(ops.ghash(a[:n], H)) == host(ops.ghash(b[:n], H)) == _ghash_ref(n, H, bytes(16))


# ---- CTR32 ----------------------------------------------------------------------
def _ctr(low: int) -> bytes:
    return bytes(range(0x10, 0x1B)) + b"\xff" + low.to_bytes(4, "big")  # byte 11 = ff: a carry would show


@functools.lru_cache(maxsize=None)
def _ctr32_ref(n, low):
    return cpu_ref.ctr32(KEYS[16], _ctr(low), _pool["host"][:n])


@pytest.mark.parametrize("impl", ["ttable", "bitslice"])
@pytest.mark.parametrize("low,n", [(0xFFFFFFF0, 4096 + 3), (2**32 - 1000, 8 * MIB + 3), (0, 4096 + 3)],
                         ids=["wrap-after-16", "wrap-after-1000", "from-zero"])
def test_ctr32(pool, low, n, impl):
    y = ops.ctr32(pool["dev"][:n], KEYS[16], _ctr(low), impl=impl)
    assert ops.last_impl() == impl
    assert host(y) == _ctr32_ref(n, low)


def test_ctr32_in_place_round_trip(pool):
    n = MIB + 5
    x = pool["dev"][:n].clone()
    assert ops.ctr32(x, KEYS[32], _ctr(0xFFFFFF00), out=x) is x
    ops.ctr32(x, KEYS[32], _ctr(0xFFFFFF00), out=x)
    assert torch.equal(x, pool["dev"][:n])


# ---- GCM ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gcm_ref(n, keylen, ivlen, aadlen):
    return cpu_ref.gcm(KEYS[keylen], IVS[ivlen], _pool["host"][:n], AADS[aadlen])


def check_gcm(pool, gpu, n, keylen, ivlen, aadlen):
    """Encrypt out of place and in place, decrypt out of place and in place;
    nothing is written past the output."""
    key, iv, aad = KEYS[keylen], IVS[ivlen], AADS[aadlen]
    ct, tag = _gcm_ref(n, keylen, ivlen, aadlen)
    x = pool["dev"][:n]
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    c, t = ops.gcm_encrypt(x, key, iv, aad, out=buf[:n])
    what = (n, keylen, ivlen, aadlen)
    assert host(t) == tag and host(buf[:n]) == ct, what
    assert bool((buf[n:] == 0xA5).all()), what
    p = ops.gcm_decrypt(c, key, iv, tag, aad)
    assert torch.equal(p, x), what
    # in place, both ways
    y = x.clone()
    c2, t2 = ops.gcm_encrypt(y, key, iv, aad, out=y)
    assert c2 is y and host(t2) == tag and host(y) == ct, what
    assert ops.gcm_decrypt(y, key, iv, t2, aad, out=y) is y
    assert torch.equal(y, x), what


@pytest.mark.parametrize("ivlen", [12, 60])
@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_gcm_small(pool, gpu, keylen, ivlen):
    for aadlen in AADS:
        for n in (0, 1, 16, 4111):
            check_gcm(pool, gpu, n, keylen, ivlen, aadlen)


@pytest.mark.parametrize("keylen,ivlen,aadlen", [(16, 12, 0), (24, 60, 13), (32, 12, 4097)])
@pytest.mark.parametrize("n", [MIB + 7, 32 * MIB + 5])
def test_gcm_large(pool, gpu, n, keylen, ivlen, aadlen):
    check_gcm(pool, gpu, n, keylen, ivlen, aadlen)


@pytest.mark.parametrize("impl", ["ttable", "bitslice"])
def test_gcm_reports_the_ctr_half(pool, impl):
    n = MIB + 7
    c, t = ops.gcm_encrypt(pool["dev"][:n], KEYS[16], IVS[12], impl=impl)
    assert ops.last_impl() == impl
    assert (host(c), host(t)) == _gcm_ref(n, 16, 12, 0)
    ops.gcm_decrypt(c, KEYS[16], IVS[12], t, impl=impl)
    assert ops.last_impl() == impl


@pytest.mark.parametrize("shift", [16, 3], ids=["offset-16", "offset-3"])
def test_gcm_on_views(pool, shift):
    """A view that starts 16 bytes into its allocation (aligned, but not where
    the allocator put it) and one that is not 16-byte aligned at all."""
    n = 4111
    x = pool["dev"][shift: shift + n]
    want = cpu_ref.gcm(KEYS[16], IVS[12], pool["host"][shift: shift + n], AADS[13])
    out = torch.zeros(shift + n, dtype=torch.uint8, device=x.device)
    c, t = ops.gcm_encrypt(x, KEYS[16], IVS[12], AADS[13], out=out[shift:])
    assert (host(c), host(t)) == want
    assert torch.equal(ops.gcm_decrypt(c, KEYS[16], IVS[12], t, AADS[13]), x)


@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_golden_vectors_on_the_device(gpu, v):
    key, iv, aad, pt, ct, tag = _fields(v)
    x = torch.frombuffer(bytearray(pt), dtype=torch.uint8).to(gpu) if pt else torch.empty(0, dtype=torch.uint8, device=gpu)
    c, t = models.AESGCM(key).encrypt(x, iv, aad)
    assert (host(c), host(t)) == (ct, tag)
    assert host(models.AESGCM(key).decrypt(c, iv, tag, aad)) == pt


@pytest.mark.parametrize("n", [4111, MIB + 7])
def test_tampering_is_refused(pool, gpu, n):
    """A flipped ciphertext bit, a flipped tag bit and a changed AAD each raise
    GcmTagError and leave the output all zero."""
    key, iv, aad = KEYS[16], IVS[12], AADS[13]
    ct, tag = _gcm_ref(n, 16, 12, 13)
    c = torch.frombuffer(bytearray(ct), dtype=torch.uint8).to(gpu)
    bad_c = c.clone()
    bad_c[n // 2] ^= 0x10
    bad_tag = tag[:7] + bytes([tag[7] ^ 1]) + tag[8:]
    assert issubclass(ops.GcmTagError, ValueError)
    for cc, tt, aa in ((bad_c, tag, aad), (c, bad_tag, aad), (c, tag, aad[:-1] + b"\xff"), (c, bad_tag[:8], aad)):
        out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
        with pytest.raises(ops.GcmTagError):
            ops.gcm_decrypt(cc, key, iv, tt, aa, out=out)
        assert bool((out == 0).all())
    # in place: the ciphertext is gone, zeroed as well
    with pytest.raises(ops.GcmTagError):
        ops.gcm_decrypt(bad_c, key, iv, tag, aad, out=bad_c)
    assert bool((bad_c == 0).all())


def test_truncated_tag_is_accepted(pool, gpu):
    n = 4111
    ct, tag = _gcm_ref(n, 32, 60, 13)
    c = torch.frombuffer(bytearray(ct), dtype=torch.uint8).to(gpu)
    for tl in (12, 4):
        assert torch.equal(ops.gcm_decrypt(c, KEYS[32], IVS[60], tag[:tl], AADS[13]), pool["dev"][:n])
    # the tag as a device tensor
    assert torch.equal(ops.gcm_decrypt(c, KEYS[32], IVS[60], torch.frombuffer(bytearray(tag), dtype=torch.uint8).to(gpu),
                                       AADS[13]), pool["dev"][:n])


def test_argument_errors(pool, gpu):
    x = pool["dev"][:64]
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        ops.gcm_encrypt(x, bytes(15), IVS[12], out=out)          # no such key size
    with pytest.raises(ValueError):
        ops.gcm_encrypt(x, KEYS[16], b"", out=out)               # an empty IV
    with pytest.raises(ValueError):
        ops.gcm_decrypt(x, KEYS[16], IVS[12], bytes(3), out=out)  # a 3-byte tag
    with pytest.raises(ValueError):
        ops.gcm_decrypt(x, KEYS[16], IVS[12], bytes(17), out=out)
    with pytest.raises(ValueError):
        ops.ghash(x, bytes(15))
    with pytest.raises(ValueError):
        ops.ctr32(x, KEYS[16], bytes(12), out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_injected_allocation_failure(pool, gpu):
    """The hash's tables and partials are a per-call allocation made before
    anything is launched: when it fails (injected, not a GPU fault) the call
    returns an error with out and the tag untouched, and the next identical
    call is right."""
    lib = _native.require_gpu_lib()
    n = MIB + 7
    x = pool["dev"][:n]
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
    lib.otc_fault_inject_alloc(0)
    try:
        with pytest.raises(RuntimeError):
            ops.gcm_encrypt(x, KEYS[16], IVS[12], out=out, impl="ttable")
        assert lib.otc_fault_inject_pending() == -1
    finally:
        lib.otc_fault_inject_alloc(-1)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    c, t = ops.gcm_encrypt(x, KEYS[16], IVS[12], out=out, impl="ttable")
    assert (host(c), host(t)) == _gcm_ref(n, 16, 12, 0)
    # the same for the hash by itself
    lib.otc_fault_inject_alloc(0)
    try:
        with pytest.raises(RuntimeError):
            ops.ghash(x, H)
        assert lib.otc_fault_inject_pending() == -1
    finally:
        lib.otc_fault_inject_alloc(-1)
    assert host(ops.ghash(x, H)) == _ghash_ref(n, H, bytes(16))
