"""The Python op layer on the GPU: which error a call with several bad
arguments reports first, the staging of misaligned views for the op families
``test_gpu_kernels.py::test_misaligned_tensors_are_staged`` does not reach,
and the checks every caller's ``out`` goes through."""
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

K128, K256, XTS_KEY = bytes(range(16)), bytes(range(32)), bytes(range(64))
IV, CTR32_WRAP = bytes(range(0x40, 0x50)), bytes(range(12)) + b"\xff\xff\xff\xfe"
NONCE4, IVEC8, NONCE12, AAD = bytes(range(4)), bytes(range(8, 16)), bytes(range(12)), b"header bytes"
SEG, N_SEG, N_ODD = 1024, 4 * 1024, 4099
FILL, PAD = 0xA5, 64


def host(t):
    return t.cpu().numpy().tobytes()


def rnd(n, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).to(dev)


# ---- which error comes first, with valid device tensors ----
def test_first_error_with_device_tensors(gpu):
    x = rnd(64, gpu, 1)
    with pytest.raises(ValueError, match="AES key must be 16/24/32 bytes"):
        ops.ctr(x, bytes(15), bytes(3))
    with pytest.raises(ValueError, match="counter must be 16 bytes"):
        ops.ctr(x, bytes(16), bytes(3))


def test_segment_size_errors(gpu):
    x48 = rnd(48, gpu, 2)
    # cbc_decrypt_segments alone leaves the multiple-of-16 rule to the native check
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.cbc_decrypt_segments(x48, K128, IV, 24)
    with pytest.raises(ValueError, match="positive multiple of 16"):
        ops.cfb128_decrypt_segments(x48, K128, IV, 24)
    with pytest.raises(ValueError, match="positive multiple of 16"):
        ops.cbc_encrypt_segments(x48, K128, IV, 24)
    with pytest.raises(ValueError, match="positive multiple of 16"):
        ops.cfb128_encrypt_segments(x48, K128, IV, 24)
    with pytest.raises(ValueError, match="byte size must be a multiple of segment_bytes"):
        ops.cbc_decrypt_segments(x48, K128, IV, 32)


# ---- staging: (bytes, op(x, out) -> outputs, reference(data) -> the same outputs as bytes) ----
def _pair(res):
    return [host(t) for t in res]


STAGED = {
    "cbc_encrypt_segments": (N_SEG, lambda x, o: [ops.cbc_encrypt_segments(x, K128, IV, SEG, out=o)],
                             lambda d: [cpu_ref.cbc_segments(K128, IV, d, SEG)]),
    "cbc_decrypt_segments": (N_SEG, lambda x, o: [ops.cbc_decrypt_segments(x, K128, IV, SEG, out=o)],
                             lambda d: [cpu_ref.cbc_segments(K128, IV, d, SEG, decrypt=True)]),
    "cfb128_encrypt_segments": (N_SEG, lambda x, o: [ops.cfb128_encrypt_segments(x, K256, IV, SEG, out=o)],
                                lambda d: [cpu_ref.cfb128_segments(K256, IV, d, SEG)]),
    "cfb128_decrypt_segments": (N_SEG, lambda x, o: [ops.cfb128_decrypt_segments(x, K256, IV, SEG, out=o)],
                                lambda d: [cpu_ref.cfb128_segments(K256, IV, d, SEG, decrypt=True)]),
    "xts_encrypt": (N_ODD, lambda x, o: [ops.xts_encrypt(x, XTS_KEY, 7, out=o)],  # one unit of 4099 bytes steals
                    lambda d: [cpu_ref.xts(XTS_KEY, 7, d)]),
    "gcm_encrypt": (N_ODD, lambda x, o: ops.gcm_encrypt(x, K128, NONCE12, AAD, out=o),
                    lambda d: cpu_ref.gcm(K128, NONCE12, d, AAD)),
    "chacha20_poly1305_encrypt": (N_ODD, lambda x, o: ops.chacha20_poly1305_encrypt(x, K256, NONCE12, AAD, out=o),
                                  lambda d: cpu_ref.chacha20_poly1305(K256, NONCE12, d, AAD)),
    "ctr32": (N_ODD, lambda x, o: [ops.ctr32(x, K256, CTR32_WRAP, out=o)], lambda d: [cpu_ref.ctr32(K256, CTR32_WRAP, d)]),
    "ctr_rfc3686": (N_ODD, lambda x, o: [ops.ctr_rfc3686(x, K128, NONCE4, IVEC8, out=o)],  # no 64-bit wrap: the 128-bit oracle
                    lambda d: [cpu_ref.ctr(K128, NONCE4 + IVEC8 + b"\x00\x00\x00\x01", d)]),
}


@pytest.mark.parametrize("name", list(STAGED))
def test_misaligned_views_are_staged(gpu, name):
    """Input at byte 3 of a larger buffer, ``out`` at byte 5 of another, then
    in place at byte 3: the reference's result, and nothing around the views
    changes."""
    n, op, ref = STAGED[name]
    data = rnd(n, gpu, 31)
    want = [bytes(w) for w in ref(host(data))]

    def framed(off):
        base = torch.full((n + PAD,), FILL, dtype=torch.uint8, device=gpu)
        assert base.data_ptr() % 16 == 0
        return base, base[off:off + n]

    def frame_intact(base, off):
        raw = host(base)
        return raw[:off] == bytes([FILL]) * off and raw[off + n:] == bytes([FILL]) * (PAD - off)

    (bi, x), (bo, out) = framed(3), framed(5)
    x.copy_(data)
    res = op(x, out)
    assert res[0].data_ptr() == out.data_ptr()
    assert _pair(res) == want
    assert host(x) == host(data)  # the input is only read
    assert frame_intact(bi, 3) and frame_intact(bo, 5)

    res = op(x, x)  # in place on the misaligned view
    assert res[0].data_ptr() == x.data_ptr()
    assert _pair(res) == want
    assert frame_intact(bi, 3)


# ---- a caller's ``out`` is checked before any launch ----
def test_xor_checks_out(gpu):
    a, b = rnd(64, gpu, 41), rnd(64, gpu, 42)
    small = torch.full((32,), FILL, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="out must have the same byte size"):
        ops.xor(a, b, out=small)
    assert host(small) == bytes([FILL]) * 32
    on_cpu = torch.full((64,), FILL, dtype=torch.uint8)
    with pytest.raises(ValueError, match="out must be a GPU tensor"):
        ops.xor(a, b, out=on_cpu)
    assert on_cpu.numpy().tobytes() == bytes([FILL]) * 64
    strided = torch.full((64, 2), FILL, dtype=torch.uint8, device=gpu)[:, 0]
    with pytest.raises(ValueError, match="out must be contiguous"):
        ops.xor(a, b, out=strided)
    assert host(strided.contiguous()) == bytes([FILL]) * 64
    with pytest.raises(ValueError, match="b must be a GPU tensor"):
        ops.xor(a, b.cpu())
    assert torch.equal(ops.xor(a, b, out=torch.empty_like(a)), a ^ b)


def test_rc4_multi_checks_out(gpu):
    keys = rnd(4 * 16, gpu, 43).view(4, 16)
    too_small = torch.full((4, 63), FILL, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="out must hold nstreams"):
        ops.rc4_multi(keys, 64, out=too_small)
    assert host(too_small) == bytes([FILL]) * (4 * 63)
    with pytest.raises(ValueError, match="out must be a GPU tensor"):
        ops.rc4_multi(keys, 64, out=torch.zeros((4, 64), dtype=torch.uint8))
    out = torch.empty((4, 64), dtype=torch.uint8, device=gpu)
    assert ops.rc4_multi(keys, 64, out=out) is out
    assert torch.equal(out, ops.rc4_multi(keys, 64))


def test_out_on_another_device_is_refused(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    x = rnd(64, gpu, 44)
    y = torch.full((64,), FILL, dtype=torch.uint8, device="cuda:1")
    with pytest.raises(ValueError, match="cuda:1.*cuda:0"):
        ops.ctr(x, K128, IV, out=y)
    assert host(y) == bytes([FILL]) * 64
    with pytest.raises(ValueError, match="cuda:1"):
        ops.xor(x, y)
