"""ChaCha20, Poly1305 and ChaCha20-Poly1305 on the device (csrc/hip/chacha.hip
through ops.chacha20 / poly1305 / chacha20_poly1305_*, models.ChaCha20Poly1305),
byte-exact against the C oracle (cpu_ref, itself pinned to RFC 8439, a Python
integer oracle and libcrypto in tests/test_chacha_cpu.py).

The ChaCha20 lengths cross a lane's block (64 B), a pass of 64 lanes (4 KiB),
a wave's run of passes (16 KiB), a workgroup (64 KiB) and the bulk / edge split
(the last whole pass); the Poly1305 lengths come from the kernel's own
decomposition (otc_poly1305_spans)."""
import functools
import json
import os

import pytest
import torch

from our_tree_amd import _native, models, ops
from our_tree_amd.models import cpu_ref
from our_tree_amd.ops import chacha_ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "chacha_vectors.json")))
H = bytes.fromhex

MIB = 1 << 20
CAP = 128 * MIB              # Poly1305 spans below this are walked around
POOL = 64 * MIB + 64
GUARD = 64

KEY = bytes(range(101, 133))
NONCE = bytes(range(0xC0, 0xCC))
PKEY = bytes((i * 37 + 11) & 0xFF for i in range(32))
AADS = {0: b"", 13: bytes(range(13)), 4097: bytes(i * 5 & 0xFF for i in range(4097))}

# chacha.hip: CC_PASS = 4 KiB per wave pass, CC_RUN = 4 passes per wave, CC_WAVES = 4 waves per workgroup
PASS, WAVE_RUN, WORKGROUP = 4096, 4 * 4096, 4 * 4 * 4096
LENGTHS = [0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 4096, 4097, 65541, MIB + 7, 32 * MIB + 5]
GRID_EDGES = [PASS - 1, PASS + 1, WAVE_RUN - 1, WAVE_RUN, WAVE_RUN + 1, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1,
              WORKGROUP + PASS - 1, 2 * WORKGROUP + 63]

_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host."""
    if not _pool:
        g = torch.Generator(device=gpu).manual_seed(8439)
        dev = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes())
    return _pool


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def dev_bytes(b: bytes, gpu):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)


def first_diff(a: bytes, b: bytes):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)


# ---- ChaCha20 -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cc_ref(n, counter, off=0):
    return cpu_ref.chacha20(KEY, NONCE, _pool["host"][off: off + n], counter)


def check_chacha(pool, gpu, n, counter=0):
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    y = ops.chacha20(pool["dev"][:n], KEY, NONCE, counter, out=buf[:n])
    got, want = host(y), _cc_ref(n, counter)
    assert got == want, (n, counter, first_diff(got, want))
    assert bool((buf[n:] == 0xA5).all()), (n, counter)


@pytest.mark.parametrize("n", LENGTHS + GRID_EDGES)
def test_chacha20_lengths(pool, gpu, n):
    check_chacha(pool, gpu, n)


@pytest.mark.parametrize("counter,n", [(0, 65541), (1, 65541), (0x0000FFFF, 65541), (0x7FFFFFF0, 65541),
                                       (0x00FFFFFE, 4097), (0xFFFFF000, 0x1000 * 64)],
                         ids=["0", "1", "0000FFFF", "7FFFFFF0", "00FFFFFE", "ends-at-the-last-counter"])
def test_chacha20_start_counters(pool, gpu, counter, n):
    """The per-lane counter addition carries across byte boundaries; the last
    case ends exactly at block 2**32 - 1."""
    check_chacha(pool, gpu, n, counter)


@pytest.mark.parametrize("counter,n", [(0xFFFFFFFF, 64), ((1 << 32) - 16, 1024)])
def test_chacha20_last_counter_is_accepted(pool, gpu, counter, n):
    check_chacha(pool, gpu, n, counter)


@pytest.mark.parametrize("counter,n", [(0xFFFFFFFF, 65), ((1 << 32) - 16, 1025)])
def test_chacha20_wrap_is_refused(pool, gpu, counter, n):
    """ValueError in Python, OTC_ERR_ARG from the C call itself before any HIP
    call; out is untouched."""
    lib = _native.require_gpu_lib()
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        ops.chacha20(pool["dev"][:n], KEY, NONCE, counter, out=out)
    rc = lib.otc_chacha20(pool["dev"].data_ptr(), out.data_ptr(), n, _native.as_u8p(KEY), _native.as_u8p(NONCE), counter,
                          None)
    assert rc == -1 and b"2^32" in lib.otc_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


@pytest.mark.parametrize("n", [1, 65, 4097, WORKGROUP + 5, MIB + 7])
def test_chacha20_in_place(pool, n):
    x = pool["dev"][:n].clone()
    assert ops.chacha20(x, KEY, NONCE, 5, out=x) is x
    assert host(x) == _cc_ref(n, 5)
    ops.chacha20(x, KEY, NONCE, 5, out=x)
    assert torch.equal(x, pool["dev"][:n])


@pytest.mark.parametrize("n", [63, 4111, WORKGROUP + 77])
@pytest.mark.parametrize("out_shift", [0, 16, 3])
@pytest.mark.parametrize("in_shift", [0, 16, 3])
def test_chacha20_on_views(pool, gpu, n, in_shift, out_shift):
    """Views 16 bytes into their allocation (aligned, but not where the
    allocator put them) and views that are not 16-byte aligned, for the input
    and the output independently; nothing is written before or after."""
    x = pool["dev"][in_shift: in_shift + n]
    buf = torch.full((GUARD + out_shift + n + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    a = GUARD + out_shift
    ops.chacha20(x, KEY, NONCE, 3, out=buf[a: a + n])
    assert host(buf[a: a + n]) == _cc_ref(n, 3, in_shift)
    assert bool((buf[:a] == 0xA5).all()) and bool((buf[a + n:] == 0xA5).all())
    if in_shift == out_shift:  # in place on the view
        y = pool["dev"][: in_shift + n].clone()
        ops.chacha20(y[in_shift:], KEY, NONCE, 3, out=y[in_shift:])
        assert host(y[in_shift:]) == _cc_ref(n, 3, in_shift)
        assert torch.equal(y[:in_shift], pool["dev"][:in_shift])


@pytest.mark.parametrize("cut,n", [(64, 200), (PASS, 3 * PASS + 9), (WORKGROUP + 64, MIB + 7)])
def test_chacha20_split_equals_whole(pool, cut, n):
    """chacha20(a) from counter c and chacha20(b) from c + len(a) / 64 equal chacha20(a + b)."""
    c = 0x00FFFF80
    x = pool["dev"][:n]
    out = torch.empty_like(x)
    ops.chacha20(x[:cut], KEY, NONCE, c, out=out[:cut])
    ops.chacha20(x[cut:], KEY, NONCE, c + cut // 64, out=out[cut:])
    assert host(out) == _cc_ref(n, c)


def test_chacha20_golden_vectors(gpu):
    for v in VEC["chacha20"]:
        y = ops.chacha20(dev_bytes(H(v["pt"]), gpu), H(v["key"]), H(v["nonce"]), v["counter"])
        assert host(y).hex() == v["ct"], v["name"]


# ---- Poly1305 -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _poly_ref(n, key=PKEY):
    return cpu_ref.poly1305(key, _pool["host"][:n])


def check_poly(pool, n, key=PKEY):
    got, want = host(ops.poly1305(pool["dev"][:n], key)), _poly_ref(n, key)
    print(f"poly1305 n={n}: {got.hex()} want {want.hex()}")
    assert got == want, n


@pytest.mark.parametrize("n", LENGTHS)
def test_poly1305_lengths(pool, n):
    check_poly(pool, n)


def test_poly1305_spans_are_reported():
    spans = ops.poly1305_spans()
    assert len(spans) >= 2 and spans[0] <= CAP and spans[1] <= CAP
    assert spans == sorted(set(spans)) and all(s % 16 == 0 and s > 0 for s in spans)


AROUND = {"S-16": -16, "S-1": -1, "S": 0, "S+1": 1, "S+16": 16}


@pytest.mark.parametrize("where", list(AROUND))
def test_poly1305_around_every_span(pool, where):
    spans = [s for s in ops.poly1305_spans() if s < CAP]
    assert len(spans) >= 2 and max(spans) + 16 <= POOL
    for s in spans:
        check_poly(pool, s + AROUND[where])


def _edge_cases():
    """The CPU test's edge keys and messages (r with every bit set, s = ff..ff,
    all-ff blocks, the accumulator at and past p, short last blocks)."""
    ff16, r2, r1 = b"\xff" * 16, (2).to_bytes(16, "little"), (1).to_bytes(16, "little")
    first = ((1 << 128) - 5).to_bytes(16, "little")
    return {
        "r-all-bits": (ff16 + bytes(range(16)), bytes(range(100))),
        "s-all-ones": (bytes(range(7, 23)) + ff16, bytes(range(64))),
        "all-ff-blocks": (bytes(range(40, 72)), ff16 * 8),
        "r-max-s-max-all-ff": (ff16 + ff16, ff16 * 16),
        "acc-passes-p": (r2 + bytes(16), ff16),
        "s-ff-final-add-wraps": (r2 + ff16, r2),
        "sum-equals-p": (r1 + bytes(16), first + bytes(32)),
        "sum-p-plus-3": (r1 + bytes(16), first + b"\x03" + bytes(31)),
        "partial-1": (PKEY, bytes(range(17))),
        "partial-15": (PKEY, bytes(range(47))),
    }


EDGES = _edge_cases()


@pytest.mark.parametrize("name", list(EDGES))
def test_poly1305_edge_cases(gpu, name):
    """As they are, and repeated to 4096 and 65541 bytes (more than one wave span)."""
    key, msg = EDGES[name]
    for n in (len(msg), 4096, 65541):
        m = (msg * (n // len(msg) + 1))[:n]
        got = host(ops.poly1305(dev_bytes(m, gpu), key))
        assert got == cpu_ref.poly1305(key, m), (name, n)
    if name in ("acc-passes-p", "s-ff-final-add-wraps", "sum-p-plus-3"):
        assert host(ops.poly1305(dev_bytes(msg, gpu), key)) == b"\x03" + bytes(15)


def test_poly1305_golden_vectors(gpu):
    for v in VEC["poly1305"]:
        assert host(ops.poly1305(dev_bytes(H(v["msg"]), gpu), H(v["key"]))).hex() == v["tag"], v["name"]


def test_poly1305_does_not_read_past_the_end(pool, gpu):
    """The bytes after nbytes differ between two buffers; the tags do not."""
    for n in (1, 17, 4099, 65541):
        a = torch.full((n + GUARD,), 0x00, dtype=torch.uint8, device=gpu)
        b = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=gpu)
        a[:n] = pool["dev"][:n]
        b[:n] = pool["dev"][:n]
        assert host(ops.poly1305(a[:n], PKEY)) == host(ops.poly1305(b[:n], PKEY)) == _poly_ref(n)


def test_poly1305_on_an_unaligned_view(pool):
    assert host(ops.poly1305(pool["dev"][3: 3 + 4099], PKEY)) == cpu_ref.poly1305(PKEY, pool["host"][3: 3 + 4099])


# ---- the AEAD -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _aead_ref(n, aadlen):
    return cpu_ref.chacha20_poly1305(KEY, NONCE, _pool["host"][:n], AADS[aadlen])


def check_aead(pool, gpu, n, aadlen):
    """Encrypt out of place and in place, decrypt out of place and in place;
    nothing is written past the output."""
    aad = AADS[aadlen]
    ct, tag = _aead_ref(n, aadlen)
    x = pool["dev"][:n]
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    c, t = ops.chacha20_poly1305_encrypt(x, KEY, NONCE, aad, out=buf[:n])
    what = (n, aadlen)
    assert host(t) == tag and host(buf[:n]) == ct, what
    assert bool((buf[n:] == 0xA5).all()), what
    p = ops.chacha20_poly1305_decrypt(c, KEY, NONCE, tag, aad)
    assert torch.equal(p, x), what
    # in place, both ways
    y = x.clone()
    c2, t2 = ops.chacha20_poly1305_encrypt(y, KEY, NONCE, aad, out=y)
    assert c2 is y and host(t2) == tag and host(y) == ct, what
    assert ops.chacha20_poly1305_decrypt(y, KEY, NONCE, t2, aad, out=y) is y
    assert torch.equal(y, x), what


@pytest.mark.parametrize("aadlen", list(AADS))
def test_aead_small(pool, gpu, aadlen):
    for n in (0, 1, 63, 64, 65, 4111):
        check_aead(pool, gpu, n, aadlen)


@pytest.mark.parametrize("n,aadlen", [(MIB + 7, 0), (MIB + 7, 4097), (32 * MIB + 5, 13)])
def test_aead_large(pool, gpu, n, aadlen):
    check_aead(pool, gpu, n, aadlen)


@pytest.mark.parametrize("v", VEC["aead"], ids=[v["name"] for v in VEC["aead"]])
def test_golden_vectors_on_the_device(gpu, v):
    key, nonce, aad, pt, ct, tag = (H(v[k]) for k in ("key", "nonce", "aad", "pt", "ct", "tag"))
    m = models.ChaCha20Poly1305(key)
    c, t = m.encrypt(dev_bytes(pt, gpu), nonce, aad)
    assert (host(c), host(t)) == (ct, tag)
    assert host(m.decrypt(c, nonce, tag, aad)) == pt
    assert m.encrypt(pt, nonce, aad) == (ct, tag)  # bytes go to the oracle


@pytest.mark.parametrize("shift", [16, 3], ids=["offset-16", "offset-3"])
def test_aead_on_views(pool, shift):
    n = 4111
    x = pool["dev"][shift: shift + n]
    want = cpu_ref.chacha20_poly1305(KEY, NONCE, pool["host"][shift: shift + n], AADS[13])
    out = torch.zeros(shift + n, dtype=torch.uint8, device=x.device)
    c, t = ops.chacha20_poly1305_encrypt(x, KEY, NONCE, AADS[13], out=out[shift:])
    assert (host(c), host(t)) == want
    assert torch.equal(ops.chacha20_poly1305_decrypt(c, KEY, NONCE, t, AADS[13]), x)


@pytest.mark.parametrize("n", [4111, MIB + 7])
def test_tampering_is_refused(pool, gpu, n):
    """A flipped ciphertext bit, a flipped tag bit, a changed AAD and a changed
    nonce each raise ChaChaTagError and leave the output all zero."""
    aad = AADS[13]
    ct, tag = _aead_ref(n, 13)
    c = dev_bytes(ct, gpu)
    bad_c = c.clone()
    bad_c[n // 2] ^= 0x10
    bad_tag = tag[:7] + bytes([tag[7] ^ 1]) + tag[8:]
    bad_nonce = NONCE[:11] + bytes([NONCE[11] ^ 1])
    assert issubclass(ops.ChaChaTagError, ValueError)
    for cc, nn, tt, aa in ((bad_c, NONCE, tag, aad), (c, NONCE, bad_tag, aad), (c, NONCE, tag, aad[:-1] + b"\xff"),
                           (c, bad_nonce, tag, aad)):
        out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
        with pytest.raises(ops.ChaChaTagError):
            ops.chacha20_poly1305_decrypt(cc, KEY, nn, tt, aa, out=out)
        assert bool((out == 0).all())
    # in place: the ciphertext is gone, zeroed as well
    with pytest.raises(ops.ChaChaTagError):
        ops.chacha20_poly1305_decrypt(bad_c, KEY, NONCE, tag, aad, out=bad_c)
    assert bool((bad_c == 0).all())
    # the tag as a device tensor
    assert torch.equal(ops.chacha20_poly1305_decrypt(c, KEY, NONCE, dev_bytes(tag, gpu), aad), pool["dev"][:n])


def test_argument_errors(pool, gpu):
    x = pool["dev"][:64]
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        ops.chacha20(x, bytes(16), NONCE, out=out)                 # a 16-byte key
    with pytest.raises(ValueError):
        ops.chacha20(x, KEY, bytes(8), out=out)                    # the original 8-byte nonce
    with pytest.raises(ValueError):
        ops.chacha20(x, KEY, bytes(24), out=out)                   # XChaCha20's nonce
    with pytest.raises(ValueError):
        ops.chacha20(x, KEY, NONCE, 1 << 32, out=out)
    with pytest.raises(ValueError):
        ops.chacha20(x, KEY, NONCE, -1, out=out)
    with pytest.raises(ValueError):
        ops.poly1305(x, bytes(16))
    with pytest.raises(ValueError):
        ops.chacha20_poly1305_encrypt(x, bytes(31), NONCE, out=out)
    with pytest.raises(ValueError):
        ops.chacha20_poly1305_encrypt(x, KEY, bytes(13), out=out)
    for taglen in (0, 12, 15, 17):
        with pytest.raises(ValueError):
            ops.chacha20_poly1305_decrypt(x, KEY, NONCE, bytes(taglen), out=out)
    with pytest.raises(ValueError):
        models.ChaCha20Poly1305(bytes(16))
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_injected_allocation_failure(pool, gpu):
    """The hash's partials are a per-call allocation made before anything is
    launched: when it fails (injected, not a GPU fault) the call returns an
    error with out and the tag untouched, and the next identical call is right."""
    lib = _native.require_gpu_lib()
    n = MIB + 7
    x = pool["dev"][:n]
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=gpu)
    tag = torch.full((16,), 0xA5, dtype=torch.uint8, device=gpu)
    for direction in (1, 0):  # otc.h OTC_DIR_ENCRYPT, OTC_DIR_DECRYPT
        lib.otc_fault_inject_alloc(0)
        try:
            rc = lib.otc_chacha20_poly1305(x.data_ptr(), out.data_ptr(), n, _native.as_u8p(KEY), direction,
                                           _native.as_u8p(NONCE), None, 0, tag.data_ptr(), None)
            assert rc == -5 and lib.otc_fault_inject_pending() == -1  # OTC_ERR_NOMEM
        finally:
            lib.otc_fault_inject_alloc(-1)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and bool((tag == 0xA5).all())
    lib.otc_fault_inject_alloc(0)
    try:
        with pytest.raises(RuntimeError):
            ops.chacha20_poly1305_encrypt(x, KEY, NONCE, out=out)
    finally:
        lib.otc_fault_inject_alloc(-1)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    c, t = ops.chacha20_poly1305_encrypt(x, KEY, NONCE, out=out)
    assert (host(c), host(t)) == _aead_ref(n, 0)
    # the same for the hash by itself
    lib.otc_fault_inject_alloc(0)
    try:
        with pytest.raises(RuntimeError):
            ops.poly1305(x, PKEY)
        assert lib.otc_fault_inject_pending() == -1
    finally:
        lib.otc_fault_inject_alloc(-1)
    assert host(ops.poly1305(x, PKEY)) == _poly_ref(n)


def test_captured_in_a_graph(pool, gpu):
    """One capture of an encryption and the decryption of its result
    (torch.cuda.CUDAGraph: the hash's stream-ordered workspace, the powers of r
    by value, no synchronisation), replayed twice over changed input."""
    n = MIB + 7
    x = pool["dev"][:n].clone()
    ct, back = torch.empty_like(x), torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up outside the capture
        ops.chacha20_poly1305_encrypt(x, KEY, NONCE, AADS[13], out=ct)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, t_enc = ops.chacha20_poly1305_encrypt(x, KEY, NONCE, AADS[13], out=ct)
        _, t_dec = chacha_ops._aead(ct, KEY, NONCE, AADS[13], back, True)  # without the readback
    for replay, off in ((1, 0), (2, 4096)):
        x.copy_(pool["dev"][off: off + n])
        ct.zero_(), back.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = cpu_ref.chacha20_poly1305(KEY, NONCE, pool["host"][off: off + n], AADS[13])
        assert (host(ct), host(t_enc)) == want, replay
        assert host(t_dec) == want[1] and torch.equal(back, x), replay
