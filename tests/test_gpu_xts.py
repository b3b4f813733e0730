"""XTS-AES on the device (csrc/hip/aes_xts.hip through ops.xts_encrypt /
xts_decrypt and models.AESXTS) against the C oracle (cpu_ref.xts, itself
pinned to IEEE 1619 vectors and libcrypto in tests/test_xts_cpu.py).

Shapes come from the kernel's launch constants (aes_xts.hip):
  * a wave's run is XTS_RUN = 2048 blocks = 32 KiB (8 passes of 256 blocks);
  * a workgroup's chunk is XTS_CHUNK = 16 runs = 32768 blocks = 512 KiB;
  * the grid is min(chunks, CUs) workgroups, so the grid-stride loop wraps
    from CUs x 512 KiB (128 MiB on a 256-CU MI355X);
  * units of 1..4 blocks take the per-block tweak form (SMALL), 5 blocks and
    more the cached one; a position in a unit from 64 blocks on is reached by
    x^64 steps (4096-byte units: up to 255).
Every case is compared with torch.equal."""
import functools

import pytest
import torch

from our_tree_amd import models, ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

RUN = 2048 * 16          # bytes of a wave's run
CHUNK = 16 * RUN         # bytes of a workgroup's chunk: 512 KiB
GUARD = 64

KEYS = {128: bytes(range(7, 39)), 256: bytes(range(101, 165))}  # K1 || K2, distinct halves


_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host.  Large enough for
    the totals that wrap the grid (CUs x chunk, plus a little)."""
    if not _pool:
        cus = torch.cuda.get_device_properties(gpu).multi_processor_count
        g = torch.Generator(device=gpu).manual_seed(1619)
        dev = torch.randint(0, 256, (cus * CHUNK + 4 * CHUNK,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes(), cus=cus)
    return _pool


@functools.lru_cache(maxsize=4)
def _oracle(n, bits, tweak0, unit, dec):
    return cpu_ref.xts(KEYS[bits], tweak0, _pool["host"][:n], unit, decrypt=dec)


def ref(pool, n, bits, tweak0, unit, dec):
    """The oracle's output for the first n pool bytes, computed once for the cases that share it."""
    return torch.frombuffer(bytearray(_oracle(n, bits, tweak0, unit, dec)), dtype=torch.uint8)


def run(x, bits, tweak0, unit, dec, out=None):
    fn = ops.xts_decrypt if dec else ops.xts_encrypt
    y = fn(x, KEYS[bits], tweak0, unit, out=out)
    torch.cuda.synchronize()
    return y


def check(pool, n, bits, tweak0, unit, dec):
    y = run(pool["dev"][:n], bits, tweak0, unit, dec)
    assert torch.equal(y.cpu(), ref(pool, n, bits, tweak0, unit, dec))


# 16 B: every block a new unit; 32 / 48: the per-block tweak form; 512 / 528: the
# cached form, 528 (33 blocks) never aligned to a pass; 4096: positions to 255
UNITS = [16, 32, 48, 512, 528, 4096]


@pytest.mark.parametrize("dec", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("unit", UNITS)
def test_unit_sizes(pool, unit, bits, dec):
    """One chunk plus one unit: two workgroups, the second with one partial pass."""
    check(pool, (CHUNK // unit + 1) * unit, bits, 0x0123456789ABCDEF, unit, dec)


def _totals(cus):
    wrap = cus * CHUNK
    return {
        "one-unit": lambda unit: unit,
        "one-chunk": lambda unit: CHUNK // unit * unit,            # exactly one chunk where the unit divides it
        "wrap": lambda unit: (wrap // unit + 3) * unit + (2 * CHUNK // unit) * unit,  # past grid x chunk
    }


@pytest.mark.parametrize("dec", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("kind", ["one-unit", "one-chunk", "wrap"])
@pytest.mark.parametrize("unit", [528, 4096])
def test_totals(pool, unit, kind, dec):
    """One unit; one workgroup chunk; more than grid x chunk, so that the
    grid-stride loop wraps (with 528-byte units that total is no multiple of
    the chunk either).  One chunk plus one unit: test_unit_sizes."""
    n = _totals(pool["cus"])[kind](unit)
    if kind == "wrap":
        assert n > pool["cus"] * CHUNK and (unit == 4096 or n % CHUNK)
    check(pool, n, 128, 5, unit, dec)


@pytest.mark.parametrize("dec", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 16])
def test_runs_start_mid_unit(pool, n, dec):
    """One unit larger than a run: every wave but the first starts deep in the unit."""
    check(pool, n, 256 if dec else 128, 2**70 + 9, None, dec)


def test_largest_unit(pool):
    """2^20 blocks, the IEEE limit, as one unit."""
    check(pool, 16 << 20, 128, 77, None, False)


@pytest.mark.parametrize("dec", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("inplace", [False, True], ids=["outofplace", "inplace"])
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("n", [16, 17, 31, 33, 4096 + 15, (1 << 20) + 5])
def test_ciphertext_stealing(pool, gpu, n, bits, inplace, dec):
    """A single unit of any length; nothing is written past the output."""
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    if inplace:
        buf[:n] = pool["dev"][:n]
    y = run(buf[:n] if inplace else pool["dev"][:n], bits, 0x1F2E3D4C5B6A7988, None, dec, out=buf[:n])
    assert y.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:n].cpu(), ref(pool, n, bits, 0x1F2E3D4C5B6A7988, None, dec))
    assert bool((buf[n:] == 0xA5).all())


@pytest.mark.parametrize("dec", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("tweak0", [2**64 - 2, 2**128 - 2], ids=["into-high-qword", "wraps"])
def test_tweak_carry(pool, tweak0, dec):
    check(pool, 4 * 512, 128, tweak0, 512, dec)


def test_tweak_as_bytes(pool):
    t = 0x0F0E0D0C0B0A09080706050403020100
    y = run(pool["dev"][:2048], 128, t.to_bytes(16, "little"), 512, False)
    assert torch.equal(y.cpu(), ref(pool, 2048, 128, t, 512, False))


def test_round_trip_in_place(pool):
    """models.AESXTS over 1024 units of 4096 bytes in place; any dtype is a byte buffer."""
    n = 4096 * 1024
    x = pool["dev"][:n].clone().view(torch.int32)
    want = x.clone()
    c = models.AESXTS(KEYS[256])
    assert c.encrypt(x, 42, 4096, out=x) is x
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.uint8).cpu(), ref(pool, n, 256, 42, 4096, False))
    c.decrypt(x, 42, 4096, out=x)
    torch.cuda.synchronize()
    assert torch.equal(x, want)


def test_halves_equal_the_whole(pool):
    """Two calls over the halves, the second from tweak0 + n / 2, equal one call."""
    unit, nu, t0 = 512, 2 * (CHUNK // 512) + 6, 2**64 - 5
    x = pool["dev"][: unit * nu]
    whole = run(x, 128, t0, unit, False)
    half = unit * nu // 2
    a = run(x[:half], 128, t0, unit, False)
    b = run(x[half:], 128, t0 + nu // 2, unit, False)
    assert torch.equal(torch.cat([a, b]), whole)


@pytest.mark.parametrize("fn", [ops.xts_encrypt, ops.xts_decrypt], ids=["enc", "dec"])
def test_argument_errors(pool, gpu, fn):
    """Refused before any launch; the output stays as it was."""
    out = torch.full((48,), 0xA5, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        fn(pool["dev"][:48], KEYS[128], 0, 24, out=out)          # two units of 24 bytes
    with pytest.raises(ValueError):
        fn(pool["dev"][:15], KEYS[128], 0, out=out[:15])         # below one block
    with pytest.raises(ValueError):
        fn(pool["dev"][:48], bytes(48), 0, 16, out=out)          # no AES-192 form
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_runs_the_ttable_kernels(pool):
    run(pool["dev"][:4096], 128, 0, 512, False)
    assert ops.last_impl() == "ttable"
