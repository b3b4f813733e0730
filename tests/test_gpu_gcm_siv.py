"""AES-GCM-SIV on the device (csrc/hip/aes_gcm_siv.hip through ops.gcm_siv_ops):
POLYVAL over the whole chip, the counter mode that reads its starting block
from device memory, and the authenticated ops, each byte for byte against the C
oracle (cpu_ref, itself pinned to RFC 8452's vectors in tests/test_gcm_siv_cpu.py).

POLYVAL's shapes come from the kernel's own decomposition (polyval_spans: a
pass of 64 lanes, a batch of passes, a wave's span, a workgroup's spans, a
level-2 span): the lengths around every span up to 64 MiB, which include the
first lengths with a second and a third level.  The counter mode's come from
k_aes_ctr_le32's geometry (ctr_le32_spans: a pass of 256 blocks, a wave's run
of 2048, a workgroup's chunk of 32768)."""
import ctypes
import functools

import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref
from test_gcm_siv_cpu import SEALED

siv = ops.gcm_siv_ops
pytestmark = pytest.mark.gpu

MIB = 1 << 20
CAP = 64 * MIB               # spans up to here are walked around
POOL = CAP + 64
GUARD = 64

H = bytes.fromhex("25629347589242761d31f826ba4b757b")    # RFC 8452 appendix A
H_ENDS = bytes([0x01] + [0] * 14 + [0x80])               # x^0 and x^127: a reflected table shows here
Y0 = bytes(range(0xA0, 0xB0))
KEYS = {16: bytes(range(3, 19)), 32: bytes(range(101, 133))}
NONCE = bytes(range(0xC0, 0xCC))
AADS = {0: b"", 13: bytes(range(13)), 4096: bytes(i * 5 & 0xFF for i in range(4096))}

PASS, RUN, CHUNK = 256 * 16, 2048 * 16, 32768 * 16       # k_aes_ctr_le32: bytes of a wave's pass and run, a workgroup's chunk
WAVE_SPAN = 2048 * 16                                    # the hash's wave span

_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host."""
    if not _pool:
        g = torch.Generator(device=gpu).manual_seed(52)
        dev = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes())
    return _pool


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def dev(b: bytes, gpu) -> torch.Tensor:
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)


# ---- POLYVAL --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _polyval_ref(n, h, y0):
    return cpu_ref.polyval(h, _pool["host"][:n], y0)


def check_polyval(pool, n, h=H, y0=bytes(16)):
    got = host(siv.polyval(pool["dev"][:n], h, y0))
    want = _polyval_ref(n, h, y0)
    print(f"polyval n={n}: {got.hex()} want {want.hex()}")
    assert got == want, n


def test_polyval_rfc_example(gpu):
    x = bytes.fromhex("4f4f95668c83dfb6401762bb2d01a262d1a24ddd2721d006bbe45f20d3c9f362")
    assert host(siv.polyval(dev(x, gpu), H)).hex() == "f7a3b47b846119fae5b7866cf5e5b77e"


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 1024, 1025])
def test_polyval_lengths(pool, n):
    check_polyval(pool, n)


def test_polyval_spans_are_reported():
    spans = siv.polyval_spans()
    assert spans == ops.ghash_spans()  # one level kernel, one decomposition
    assert len([s for s in spans if s <= CAP]) >= 5 and spans[0] == 1024
    assert spans == sorted(set(spans)) and all(s % 16 == 0 and s > 0 for s in spans)


AROUND = {"S-16": lambda s: s - 16, "S-1": lambda s: s - 1, "S": lambda s: s, "S+1": lambda s: s + 1,
          "S+16": lambda s: s + 16}


@pytest.mark.parametrize("where", list(AROUND))
def test_polyval_around_every_span(pool, where):
    """Up to 64 MiB: past the wave span (32 KiB) a second level begins, past the level-2 span (64 MiB) a third."""
    spans = [s for s in siv.polyval_spans() if s <= CAP]
    assert WAVE_SPAN in spans and CAP in spans
    for s in spans:
        check_polyval(pool, AROUND[where](s))


@pytest.mark.parametrize("n", [1, 16, 33, 4096, 65541, MIB + 7])
def test_polyval_continues_from_y0(pool, n):
    check_polyval(pool, n, H, Y0)


@pytest.mark.parametrize("n", [16, 17, 4096, 65541, MIB + 7])
def test_polyval_key_with_both_end_bits(pool, n):
    check_polyval(pool, n, H_ENDS, Y0)


def test_polyval_empty_returns_y0(pool):
    assert host(siv.polyval(pool["dev"][:0], H, Y0)) == Y0


def test_polyval_split_equals_whole(pool):
    """Two device calls chained through y0 equal one call; a view that is not 16-byte aligned is staged."""
    n, cut = MIB + 11, 65536 + 16 * 3
    mid = host(siv.polyval(pool["dev"][:cut], H, Y0))
    assert host(siv.polyval(pool["dev"][cut:n], H, mid)) == cpu_ref.polyval(H, pool["host"][:n], Y0)
    assert host(siv.polyval(pool["dev"][3: 3 + 4099], H)) == cpu_ref.polyval(H, pool["host"][3: 3 + 4099])


# ---- the counter mode ---------------------------------------------------------------
def _ctr(start: int) -> bytes:
    """Byte 4 = ff (a carry out of the counter would show) and byte 15 below 0x80 (the kernel forces the bit on)."""
    return (start % (1 << 32)).to_bytes(4, "little") + b"\xff" + bytes(range(0x21, 0x2C))


def _ctr_forced(start: int) -> bytes:
    c = _ctr(start)
    return c[:15] + bytes([c[15] | 0x80])


@functools.lru_cache(maxsize=None)
def _ctr_ref(n, keylen, start):
    return cpu_ref.ctr_le32(KEYS[keylen], _ctr_forced(start), _pool["host"][:n])


STARTS = {"3-before": -3, "70-before": -70,
          "in-a-chunk": -(CHUNK // 16 + 1000)}  # the wrap falls into the second workgroup's chunk, in the middle of a pass
LENGTHS = [1, 17, PASS + 5, CHUNK + RUN + 17]


@pytest.mark.parametrize("keylen", [16, 32])
@pytest.mark.parametrize("start", list(STARTS))
@pytest.mark.parametrize("n", LENGTHS)
def test_ctr_le32(pool, gpu, n, start, keylen):
    s = STARTS[start]
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    y = siv.ctr_le32(pool["dev"][:n], KEYS[keylen], dev(_ctr(s), gpu), out=buf[:n])
    assert ops.last_impl() == "ttable"
    assert host(y) == _ctr_ref(n, keylen, s), (n, start, keylen)
    assert bool((buf[n:] == 0xA5).all())


def test_ctr_le32_counter_as_bytes_and_in_place(pool, gpu):
    n, s = CHUNK + RUN + 17, STARTS["in-a-chunk"]
    x = pool["dev"][:n].clone()
    assert siv.ctr_le32(x, KEYS[32], _ctr(s), out=x) is x
    assert host(x) == _ctr_ref(n, 32, s)
    siv.ctr_le32(x, KEYS[32], dev(_ctr(s), gpu), out=x)
    assert torch.equal(x, pool["dev"][:n])


def test_ctr_le32_reads_its_counter_in_stream_order(pool, gpu):
    """The counter block is the result of the op in front on the same stream: no host value exists when the call is made."""
    n = PASS + 5
    c = torch.zeros(16, dtype=torch.uint8, device=gpu)
    c.copy_(dev(_ctr(-3), gpu))  # queued in front of the kernel
    assert host(siv.ctr_le32(pool["dev"][:n], KEYS[16], c)) == _ctr_ref(n, 16, -3)


# ---- GCM-SIV ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _siv_ref(n, keylen, aadlen):
    return cpu_ref.gcm_siv(KEYS[keylen], NONCE, _pool["host"][:n], AADS[aadlen])


def check_siv(pool, gpu, n, keylen, aadlen):
    """Encrypt out of place and in place, decrypt out of place (the tag as
    bytes) and in place (the tag as a device tensor); nothing is written past the output."""
    key, aad = KEYS[keylen], AADS[aadlen]
    ct, tag = _siv_ref(n, keylen, aadlen)
    x = pool["dev"][:n]
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    c, t = siv.gcm_siv_encrypt(x, key, NONCE, aad, out=buf[:n])
    what = (n, keylen, aadlen)
    assert host(t) == tag, what
    assert host(buf[:n]) == ct, what
    assert bool((buf[n:] == 0xA5).all()), what
    assert torch.equal(siv.gcm_siv_decrypt(c, key, NONCE, tag, aad), x), what
    y = x.clone()
    c2, t2 = siv.gcm_siv_encrypt(y, key, NONCE, aad, out=y)
    assert c2 is y and host(t2) == tag and host(y) == ct, what
    assert siv.gcm_siv_decrypt(y, key, NONCE, t2, aad, out=y) is y
    assert torch.equal(y, x), what


@pytest.mark.parametrize("key,nonce,aad,pt,sealed", SEALED, ids=[f"v{i}" for i in range(len(SEALED))])
def test_known_answers_on_the_device(gpu, key, nonce, aad, pt, sealed):
    c, t = siv.gcm_siv_encrypt(dev(pt, gpu), key, nonce, aad)
    assert (host(c) + host(t)).hex() == sealed
    assert host(siv.gcm_siv_decrypt(c, key, nonce, t, aad)) == pt
    assert host(siv.gcm_siv_decrypt(c, key, nonce, bytes.fromhex(sealed)[len(pt):], aad)) == pt


@pytest.mark.parametrize("keylen", [16, 32])
@pytest.mark.parametrize("aadlen", list(AADS))
def test_gcm_siv_small(pool, gpu, keylen, aadlen):
    for n in (0, 1, 16, 4097):
        check_siv(pool, gpu, n, keylen, aadlen)


@pytest.mark.parametrize("keylen,aadlen", [(16, 0), (32, 13)])
@pytest.mark.parametrize("n", [WAVE_SPAN + 5, 512 * 1024 + 16 * 37 + 5, 64 * MIB + 5],
                         ids=["wave-span+5", "512K+597", "64M+5"])
def test_gcm_siv_large(pool, gpu, n, keylen, aadlen):
    check_siv(pool, gpu, n, keylen, aadlen)


@pytest.mark.parametrize("shift", [0, 3])
def test_gcm_siv_on_views(pool, shift):
    """A view at the allocation's start and one that is not 16-byte aligned at all, in and out."""
    n = 4097
    x = pool["dev"][shift: shift + n]
    want = cpu_ref.gcm_siv(KEYS[16], NONCE, pool["host"][shift: shift + n], AADS[13])
    out = torch.zeros(shift + n, dtype=torch.uint8, device=x.device)
    c, t = siv.gcm_siv_encrypt(x, KEYS[16], NONCE, AADS[13], out=out[shift:])
    assert (host(c), host(t)) == want
    assert torch.equal(siv.gcm_siv_decrypt(c, KEYS[16], NONCE, t, AADS[13]), x)
    y = x.clone()[shift:]  # in place on a misaligned view
    want = cpu_ref.gcm_siv(KEYS[32], NONCE, host(y), AADS[0])
    c, t = siv.gcm_siv_encrypt(y, KEYS[32], NONCE, out=y)
    assert c is y and (host(y), host(t)) == want


@pytest.mark.parametrize("n", [4097, 512 * 1024 + 16 * 37 + 5])
def test_tampering_is_refused(pool, gpu, n):
    """A flipped tag bit, a flipped ciphertext byte at the start, in the middle
    and at the end, and a changed AAD each raise GcmSivTagError and leave the output all zero."""
    key, aad = KEYS[16], AADS[13]
    ct, tag = _siv_ref(n, 16, 13)
    c = dev(ct, gpu)
    bad_tag = tag[:7] + bytes([tag[7] ^ 1]) + tag[8:]
    assert issubclass(siv.GcmSivTagError, ValueError)
    cases = [(c, bad_tag, aad), (c, dev(bad_tag, gpu), aad), (c, tag, aad[:-1] + b"\xff")]
    for at in (0, n // 2, n - 1):
        bad_c = c.clone()
        bad_c[at] ^= 0x10
        cases.append((bad_c, tag, aad))
    for cc, tt, aa in cases:
        out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
        with pytest.raises(siv.GcmSivTagError):
            siv.gcm_siv_decrypt(cc, key, NONCE, tt, aa, out=out)
        assert bool((out == 0).all())
    # in place: the ciphertext is gone, zeroed as well
    bad_c = cases[-1][0]
    with pytest.raises(siv.GcmSivTagError):
        siv.gcm_siv_decrypt(bad_c, key, NONCE, tag, aad, out=bad_c)
    assert bool((bad_c == 0).all())


def test_a_repeated_nonce_gives_another_tag_and_keystream(pool, gpu):
    n = 4097
    x = pool["dev"][:n]
    x2 = x.clone()
    x2[n - 1] ^= 1
    (c1, t1), (c2, t2) = siv.gcm_siv_encrypt(x, KEYS[32], NONCE), siv.gcm_siv_encrypt(x2, KEYS[32], NONCE)
    assert host(t1) != host(t2)
    assert host(c1 ^ c2)[:16] != bytes(16)  # GCM would give the plaintexts' XOR here: zero
    assert (host(c2), host(t2)) == cpu_ref.gcm_siv(KEYS[32], NONCE, host(x2))


def test_argument_errors(pool, gpu):
    x = pool["dev"][:64]
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=gpu)
    for bad in (lambda: siv.gcm_siv_encrypt(x, bytes(24), NONCE, out=out),        # no 192-bit keys
                lambda: siv.gcm_siv_encrypt(x, KEYS[16], NONCE[:11], out=out),
                lambda: siv.gcm_siv_encrypt(x, KEYS[16], NONCE + b"\0", out=out),
                lambda: siv.gcm_siv_decrypt(x, KEYS[16], NONCE, bytes(15), out=out),
                lambda: siv.gcm_siv_decrypt(x, KEYS[16], NONCE, torch.zeros(12, dtype=torch.uint8, device=gpu), out=out),
                lambda: siv.gcm_siv_encrypt(x, KEYS[16], NONCE, out=out[:32]),
                lambda: siv.polyval(x, bytes(15)),
                lambda: siv.ctr_le32(x, KEYS[16], bytes(12), out=out),
                lambda: siv.ctr_le32(x, bytes(5), bytes(16), out=out)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_injected_allocation_failure(pool, gpu):
    """The hash's tables and partials are a per-call allocation made before
    anything is launched: when it fails (injected, not a GPU fault) the call
    returns an error with out and the tag untouched, in both directions, and
    the next identical call is right."""
    lib = _native.require_gpu_lib()
    n = MIB + 7
    x = pool["dev"][:n]
    ct, tag = _siv_ref(n, 16, 0)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
    tag_dev = torch.full((16,), 0xA5, dtype=torch.uint8, device=gpu)
    k = _native.OtcGcmSivKey()
    assert lib.otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(KEYS[16]), 128) == 0
    received = dev(tag, gpu)

    def call(direction):
        with torch.cuda.device(gpu):
            return lib.otc_aes_gcm_siv(x.data_ptr(), out.data_ptr(), n, ctypes.byref(k), direction, _native.as_u8p(NONCE),
                                       None, 0, received.data_ptr(), tag_dev.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))

    for direction in (1, 0):
        lib.otc_fault_inject_alloc(0)
        try:
            assert call(direction) != 0 and b"no memory" in lib.otc_last_error()
            assert lib.otc_fault_inject_pending() == -1
        finally:
            lib.otc_fault_inject_alloc(-1)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and bool((tag_dev == 0xA5).all()), direction
    assert call(1) == 0
    assert (host(out), host(tag_dev)) == (ct, tag)
    # the ops raise, and the next call is right; the same for the hash by itself
    for f, want in ((lambda: host(siv.gcm_siv_encrypt(x, KEYS[16], NONCE)[0]), ct),
                    (lambda: host(siv.polyval(x, H)), _polyval_ref(n, H, bytes(16)))):
        lib.otc_fault_inject_alloc(0)
        try:
            with pytest.raises(RuntimeError):
                f()
            assert lib.otc_fault_inject_pending() == -1
        finally:
            lib.otc_fault_inject_alloc(-1)
        assert f() == want
