"""GHASH and AES-GCM (SP 800-38D) of one message on torch tensors, backed by
the gfx950 kernels of ``csrc/hip/aes_gcm.hip`` and the CTR kernels of
``aes_ops.ctr32``.  The batched records are ``batch_ops.GcmBatch``."""
from __future__ import annotations

import ctypes
import functools

import torch

from .. import _native
from ..models.cpu_ref import GCM_MAX_BYTES, GcmTagError  # SP 800-38D: 2**36 - 32 plaintext bytes in one message
from ._common import _aligned, _b16, _call, _check_dev, _impl, _lib, _nbytes, _open_with_tag, _out_like, _spans, _stream
from .keys import DECRYPT, ENCRYPT


@functools.lru_cache(maxsize=64)
def _gcm_key(key: bytes) -> _native.OtcGcmKey:
    k = _native.OtcGcmKey()
    if _lib().otc_gcm_key_init(ctypes.byref(k), _native.as_u8p(key), len(key) * 8):
        raise ValueError(f"AES key must be 16, 24 or 32 bytes, got {len(key)}")
    return k


def ghash(x: torch.Tensor, h: bytes, y0: bytes = bytes(16)) -> torch.Tensor:
    """GHASH (SP 800-38D) under the hash subkey ``h``, continued from ``y0``,
    over the bytes of ``x`` with the last partial block zero-padded: a 16-byte
    uint8 tensor on ``x``'s device.  Parallel over the whole chip
    (``csrc/hip/aes_gcm.hip``); asynchronous on the current stream."""
    _check_dev(x, "x")
    hb, yb = _b16(h, "h"), _b16(y0, "y0")
    y = torch.empty(16, dtype=torch.uint8, device=x.device)
    xb = _aligned(x)  # the kernel loads 16 bytes per lane
    with torch.cuda.device(x.device):
        rc = _lib().otc_ghash(xb.data_ptr(), _nbytes(x), hb, yb, y.data_ptr(), _stream(x))
    _native.check(rc, "otc_ghash")
    return y


def ghash_spans() -> list[int]:
    """Byte sizes of the pieces the GHASH kernel cuts its data into, smallest
    first (otc.h otc_ghash_spans): lengths around them take different paths."""
    return _spans("otc_ghash_spans")


def _gcm(x: torch.Tensor, key: bytes, iv: bytes, aad: bytes, out, impl, decrypt: bool):
    _check_dev(x, "x")
    key, iv, aad = bytes(key), bytes(iv), bytes(aad)
    if not iv:
        raise ValueError("the GCM IV must have at least 1 byte")
    n = _nbytes(x)
    if n > GCM_MAX_BYTES:
        raise ValueError("a GCM message has at most 2**36 - 32 bytes")
    k = _gcm_key(key)
    out = _out_like(x, out)
    tag = torch.empty(16, dtype=torch.uint8, device=x.device)
    _call("otc_aes_gcm", x, out, lambda ip, op: (
        ip, op, n, ctypes.byref(k), DECRYPT if decrypt else ENCRYPT, _native.as_u8p(iv), len(iv),
        _native.as_u8p(aad), len(aad), tag.data_ptr(), _impl(impl), _stream(x)))
    return out, tag


def gcm_encrypt(x: torch.Tensor, key: bytes, iv: bytes, aad: bytes = b"", out=None, impl="auto"):
    """AES-GCM (SP 800-38D) encryption of one message: ``(out, tag)``, the tag
    a 16-byte uint8 device tensor.  ``key`` is 16, 24 or 32 bytes, ``iv`` any
    length from 1 byte (12 is the fast path), ``aad`` host bytes (headers;
    hash large device data with ``ghash``).  Any byte length up to
    2**36 - 32; may run in place; asynchronous -- nothing is read back.
    ``impl`` chooses the CTR half's kernel (``last_impl()`` reports it)."""
    return _gcm(x, key, iv, aad, out, impl, False)


def gcm_decrypt(x: torch.Tensor, key: bytes, iv: bytes, tag, aad: bytes = b"", out=None, impl="auto") -> torch.Tensor:
    """Authenticated AES-GCM decryption.  ``tag`` is the received tag, 4 to 16
    bytes (bytes, or a uint8 tensor); the computed tag is read back -- 16
    bytes, the call's only synchronisation -- and compared in constant time.
    On a mismatch ``out`` is zeroed and ``GcmTagError`` (a ``ValueError``)
    raised.  May run in place."""
    return _open_with_tag(tag, range(4, 17), "a GCM tag has 4 to 16 bytes",
                          lambda: _gcm(x, key, iv, aad, out, impl, True),
                          GcmTagError, "GCM tag mismatch: the output was zeroed")
