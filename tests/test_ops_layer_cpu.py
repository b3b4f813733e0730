"""The Python op layer (``our_tree_amd/ops``) without a GPU: its public
surface, the pointer logic of ``_run`` on CPU tensors, the argument helpers and
which error a call with several bad arguments reports first."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.ops import _common, aes_ops, batch_ops

T, TN = "'torch.Tensor'", "'torch.Tensor | None'"
SEG = f"(x: {T}, key: 'bytes', iv0: 'bytes', segment_bytes: 'int', out=None, impl='auto') -> {T}"
CHAIN = f"(x: {T}, key: 'bytes', iv: 'bytes', out=None, impl='auto') -> {T}"
ECB = f"(x: {T}, key: 'bytes', out=None, impl='auto') -> {T}"
XTS = f"(x: {T}, key: 'bytes', tweak0, unit_bytes: 'int | None' = None, out=None) -> {T}"
SPANS = "() -> 'list[int]'"

SIGNATURES = {
    "CtrBatch": "(xs, keys, counters, outs=None, key_index=None, tile_blocks=None)",
    "CtrBatch.packed": f"(buf: {T}, lengths, keys, counters, out: {TN} = None, offsets=None, key_index=None, "
                       "tile_blocks=None) -> \"'CtrBatch'\"",
    "CtrBatch.run": "(self, stream=None)",
    "CtrStream": "(key: 'bytes', nonce_counter: 'bytes', impl='auto')",
    "CtrStream.from_state": "(key: 'bytes', state: 'dict', impl='auto') -> \"'CtrStream'\"",
    "CtrStream.nc_off": "property",
    "CtrStream.nonce_counter": "property",
    "CtrStream.state": "(self) -> 'dict'",
    "CtrStream.stream_block": "property",
    "CtrStream.update": f"(self, x: {T}, out: {TN} = None) -> {T}",
    "GcmBatch": "(xs, key: 'bytes', outs=None, aads=None, tag_bytes: 'int' = 16, tile_blocks=None, lanes=None)",
    "GcmBatch.decrypt": f"(self, ivs: {T}, tags: {T}, stream=None)",
    "GcmBatch.encrypt": f"(self, ivs: {T}, stream=None)",
    "GcmBatch.ghash": f"(self, stream=None) -> {T}",
    "GcmBatch.packed": f"(buf: {T}, lengths, key: 'bytes', out: {TN} = None, offsets=None, aad=None, "
                       "tag_bytes: 'int' = 16, tile_blocks=None, lanes=None) -> \"'GcmBatch'\"",
    "cbc_decrypt": CHAIN,
    "cbc_decrypt_segments": SEG,
    "cbc_encrypt_segments": SEG,
    "cfb128_decrypt": CHAIN,
    "cfb128_decrypt_segments": SEG,
    "cfb128_encrypt_segments": SEG,
    "chacha20": f"(x: {T}, key: 'bytes', nonce: 'bytes', counter: 'int' = 0, out: {TN} = None) -> {T}",
    "chacha20_poly1305_decrypt": f"(c: {T}, key: 'bytes', nonce: 'bytes', tag, aad: 'bytes' = b'', out=None) -> {T}",
    "chacha20_poly1305_encrypt": f"(x: {T}, key: 'bytes', nonce: 'bytes', aad: 'bytes' = b'', out=None)",
    "checksum": f"(t: {T}) -> 'int'",
    "clock_ghz": f"(probe: {T}) -> 'float'",
    "clock_probe": f"(delay_s: 'float', window_s: 'float', device=None, stream=None) -> {T}",
    "ctr": f"(x: {T}, key: 'bytes', counter: 'bytes', out: {TN} = None, block_offset: 'int' = 0, impl='auto') -> {T}",
    "ctr32": f"(x: {T}, key: 'bytes', counter: 'bytes', out: {TN} = None, impl='auto') -> {T}",
    "ctr_batch": "(xs, keys, counters, outs=None, key_index=None, tile_blocks=None)",
    "ctr_rfc3686": f"(x: {T}, key: 'bytes', nonce: 'bytes', ivec: 'bytes', out=None, block_offset: 'int' = 0, "
                   f"impl='auto') -> {T}",
    "ecb_decrypt": ECB,
    "ecb_encrypt": ECB,
    "expand_key": "(key: 'bytes', decrypt: 'bool' = False) -> '_native.OtcAesKey'",
    "fill_random_": f"(t: {T}, seed: 'int' = 0) -> {T}",
    "gcm_batch_spans": SPANS,
    "gcm_decrypt": f"(x: {T}, key: 'bytes', iv: 'bytes', tag, aad: 'bytes' = b'', out=None, impl='auto') -> {T}",
    "gcm_decrypt_batch": f"(xs, key: 'bytes', ivs: {T}, tags: {T}, aads=None, outs=None)",
    "gcm_encrypt": f"(x: {T}, key: 'bytes', iv: 'bytes', aad: 'bytes' = b'', out=None, impl='auto')",
    "gcm_encrypt_batch": f"(xs, key: 'bytes', ivs: {T}, aads=None, outs=None)",
    "ghash": f"(x: {T}, h: 'bytes', y0: 'bytes' = {bytes(16)!r}) -> {T}",
    "ghash_batch": f"(xs, key: 'bytes', aads=None, lanes=None) -> {T}",
    "ghash_spans": SPANS,
    "last_impl": "() -> 'str'",
    "pick_impl": "(impl='auto', bits: 'int' = 128, mode: 'str' = 'ctr', nbytes: 'int' = 0) -> 'str'",
    "poly1305": f"(x: {T}, key: 'bytes') -> {T}",
    "poly1305_spans": SPANS,
    "rc4_crypt_batch": f"(states: {T}, x: {T}, out: {TN} = None) -> {T}",
    "rc4_multi": f"(keys: {T}, length: 'int', x: {TN} = None, drop: 'int' = 0, out: {TN} = None) -> {T}",
    "rc4_states": f"(keys) -> {T}",
    "split_fallback_reason": "() -> 'str'",
    "xor": f"(a: {T}, b: {T}, out: {TN} = None) -> {T}",
    "xts_decrypt": XTS,
    "xts_encrypt": XTS,
}
NOT_CALLABLE = {"IMPLS", "GcmTagError", "ChaChaTagError"}  # a dict and two ValueError subclasses


def _surface():
    got = {}
    for name in ops.__all__:
        obj = getattr(ops, name)
        if name in NOT_CALLABLE:
            continue
        got[name] = str(inspect.signature(obj))
        if inspect.isclass(obj):
            for m, v in vars(obj).items():
                if not m.startswith("_"):
                    got[f"{name}.{m}"] = "property" if isinstance(v, property) else str(inspect.signature(getattr(obj, m)))
    return got


def test_public_surface_is_pinned():
    assert set(ops.__all__) == {n for n in SIGNATURES if "." not in n} | NOT_CALLABLE
    assert len(ops.__all__) == len(set(ops.__all__))
    got = _surface()
    assert set(got) == set(SIGNATURES)
    for name, sig in SIGNATURES.items():
        assert got[name] == sig, name
    assert ops.IMPLS == {"auto": 0, "ttable": 1, "bitslice": 2, "split": 3}
    assert issubclass(ops.GcmTagError, ValueError) and issubclass(ops.ChaChaTagError, ValueError)
    assert ops.stream_ops.RC4_STATE_BYTES == 264
    assert callable(ops.chacha_ops._aead)


def test_empty_ctr_batch_needs_no_device():
    b = ops.CtrBatch([], [], [])
    assert b.outs == [] and b.ntiles == 0 and b.tile_blocks == 256 and b.device is None
    assert b.run() == []


# ---- _run: pointer logic only, so CPU tensors and a Python ``call`` do ----
PAD, FILL = 48, 0xC3


def _base(n):
    """(base buffer, index of its first 16-byte aligned byte)"""
    base = torch.full((n + 2 * PAD,), FILL, dtype=torch.uint8)
    return base, (-base.data_ptr()) % 16


def _view(base, a0, off, n):
    return base[a0 + off:a0 + off + n]


def _pattern(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def _xor5a(data: bytes) -> bytes:
    return bytes(b ^ 0x5A for b in data)


def _recorder(n, log, rc=0):
    def call(ip, op):
        log.append((ip, op))
        if n:
            ctypes.memmove(op, _xor5a(ctypes.string_at(ip, n)), n)
        return rc
    return call


def _outside_untouched(base, a0, off, n):
    raw = base.numpy().tobytes()
    return raw[:a0 + off] == bytes([FILL]) * (a0 + off) and raw[a0 + off + n:] == bytes([FILL]) * (len(raw) - a0 - off - n)


@pytest.mark.parametrize("n", [48, 4099])
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (3, 0), (0, 5), (3, 5)])
def test_run_stages_misaligned_views(n, off_in, off_out):
    (bi, ai), (bo, ao) = _base(n), _base(n)
    x, out = _view(bi, ai, off_in, n), _view(bo, ao, off_out, n)
    x.copy_(_pattern(n, n + off_in))
    src, log = x.numpy().tobytes(), []
    assert _common._run(x, out, _recorder(n, log)) == 0
    assert len(log) == 1 and all(p % 16 == 0 for p in log[0])
    if not (off_in or off_out):
        assert log[0] == (x.data_ptr(), out.data_ptr())  # aligned tensors are passed as they are
    assert out.numpy().tobytes() == _xor5a(src)
    assert x.numpy().tobytes() == src
    assert _outside_untouched(bi, ai, off_in, n) and _outside_untouched(bo, ao, off_out, n)


@pytest.mark.parametrize("n", [48, 4099])
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("inplace_ok", [True, False])
def test_run_in_place(n, off, inplace_ok):
    base, a0 = _base(n)
    x = _view(base, a0, off, n)
    x.copy_(_pattern(n, n + off))
    src, log = x.numpy().tobytes(), []
    assert _common._run(x, x, _recorder(n, log), inplace_ok=inplace_ok) == 0
    (ip, op), = log
    assert ip % 16 == 0 and op % 16 == 0
    if inplace_ok:
        assert ip == op  # in place stays in place, staged or not
        if off == 0:
            assert ip == x.data_ptr()
    else:
        assert ip != op  # CBC / CFB decryption reads a copy of the input
    assert x.numpy().tobytes() == _xor5a(src)
    assert _outside_untouched(base, a0, off, n)


def test_run_zero_bytes_calls_once_with_the_original_pointers():
    (bi, ai), (bo, ao) = _base(0), _base(0)
    x, out = _view(bi, ai, 3, 0), _view(bo, ao, 5, 0)
    log = []
    assert _common._run(x, out, _recorder(0, log)) == 0
    assert log == [(x.data_ptr(), out.data_ptr())]
    log.clear()
    assert _common._run(x, x, _recorder(0, log), inplace_ok=False) == 0
    assert log == [(x.data_ptr(), x.data_ptr())]


@pytest.mark.parametrize("n", [48, 4099])
def test_run_failed_call_leaves_a_staged_out_untouched(n):
    (bi, ai), (bo, ao) = _base(n), _base(n)
    x, out = _view(bi, ai, 0, n), _view(bo, ao, 5, n)
    x.copy_(_pattern(n, 7))
    log = []
    assert _common._run(x, out, _recorder(n, log, rc=-1)) == -1
    assert len(log) == 1 and log[0][1] != out.data_ptr()
    assert bo.numpy().tobytes() == bytes([FILL]) * (n + 2 * PAD)


# ---- argument helpers ----
def test_argument_helpers():
    with pytest.raises(ValueError, match=r"impl must be one of \['auto', 'ttable', 'bitslice', 'split'\]"):
        _common._impl("bogus")
    assert [_common._impl(v) for v in ("auto", "ttable", "bitslice", "split", 2)] == [0, 1, 2, 3, 2]
    with pytest.raises(ValueError, match="iv must be 16 bytes"):
        _common._b16(bytes(15), "iv")
    assert bytes(_common._b16(bytes(range(16)), "iv")) == bytes(range(16))
    assert bytes(aes_ops._xts_tweak(-1)) == b"\xff" * 16
    assert bytes(aes_ops._xts_tweak(2**128 + 5)) == (5).to_bytes(16, "little")
    assert bytes(aes_ops._xts_tweak(bytes(range(16)))) == bytes(range(16))


def test_pick_tile():
    assert batch_ops._pick_tile(np.full(100, 4096, np.uint64)) == 256
    assert batch_ops._pick_tile(np.full(100, 1024, np.uint64)) == 64
    # 2 KiB messages fill 128-block tiles exactly; the 4 KiB ones take two each at 1.5 % more per slot
    assert batch_ops._pick_tile(np.array([2048] * 10 + [4096] * 10, np.uint64)) == 128
    assert batch_ops._pick_tile(np.array([4096] * 10 + [1024] * 10 + [100] * 5, np.uint64)) == 64


# ---- which error comes first, on CPU tensors ----
def test_first_error_on_cpu_tensors():
    cpu = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="x must be a GPU tensor"):
        ops.ctr(cpu, bytes(15), bytes(3))  # not the key, not the counter
    buf, k, c = torch.zeros(4096, dtype=torch.uint8), [bytes(16)], [bytes(16)] * 2
    with pytest.raises(ValueError, match="messages must lie inside the buffer"):
        ops.CtrBatch.packed(buf, [4000, 200], k, c, key_index=[0, 0])
    with pytest.raises(ValueError, match="message offsets must be multiples of 16"):
        ops.CtrBatch.packed(buf, [10, 10], k, c, offsets=[0, 24], key_index=[0, 0])
    with pytest.raises(ValueError, match="one offset per message"):
        ops.CtrBatch.packed(buf, [10, 10], k, c, offsets=[0], key_index=[0, 0])
    with pytest.raises(ValueError, match="buf must be a GPU tensor"):
        ops.GcmBatch.packed(buf, [4000, 200], bytes(16))
    with pytest.raises(ValueError, match="buf must be a GPU tensor"):
        ops.GcmBatch.packed(buf, [10, 10], bytes(16), offsets=[0, 24])


def test_gcm_batch_argument_messages():
    with pytest.raises(ValueError, match="a GCM tag has 4 to 16 bytes"):
        ops.GcmBatch([], bytes(16), tag_bytes=3)
    with pytest.raises(ValueError, match=r"lanes must be 16 or 64 \(default: picked from the record sizes\)"):
        ops.GcmBatch([], bytes(16), lanes=32)
    with pytest.raises(ValueError, match="a GCM tag has 4 to 16 bytes"):  # before the device
        ops.GcmBatch.packed(torch.zeros(64, dtype=torch.uint8), [16], bytes(16), tag_bytes=17)
