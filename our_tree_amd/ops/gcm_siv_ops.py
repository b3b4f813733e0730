"""POLYVAL and AES-GCM-SIV (RFC 8452) of one message on torch tensors, backed
by the gfx950 kernels of ``csrc/hip/aes_gcm_siv.hip``: the AEAD that stays safe
when a nonce repeats under a key.  Its names are reached as
``ops.gcm_siv_ops.*``; they are not in ``ops.__all__`` yet (docs/API.md)."""
from __future__ import annotations

import ctypes
import functools

import torch

from .. import _native
from ..models.cpu_ref import GcmSivTagError, gcm_siv_check
from ._common import _aligned, _b16, _bytes, _call, _check_dev, _lib, _nbytes, _open_with_tag, _out_like, _spans, _stream
from .keys import DECRYPT, ENCRYPT, expand_key


@functools.lru_cache(maxsize=64)
def _siv_key(key: bytes) -> _native.OtcGcmSivKey:
    k = _native.OtcGcmSivKey()
    if _lib().otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(key), len(key) * 8):
        raise ValueError(f"an AES-GCM-SIV key has 16 or 32 bytes, got {len(key)}")
    return k


def polyval(x: torch.Tensor, h: bytes, y0: bytes = bytes(16)) -> torch.Tensor:
    """POLYVAL (RFC 8452 section 3) under the key ``h``, continued from ``y0``,
    over the bytes of ``x`` with the last partial block zero-padded: a 16-byte
    uint8 tensor on ``x``'s device.  Parallel over the whole chip (GHASH's
    level kernel over tables in POLYVAL's convention); asynchronous on the
    current stream."""
    _check_dev(x, "x")
    hb, yb = _b16(h, "h"), _b16(y0, "y0")
    y = torch.empty(16, dtype=torch.uint8, device=x.device)
    xb = _aligned(x)  # the kernel loads 16 bytes per lane
    with torch.cuda.device(x.device):
        rc = _lib().otc_polyval(xb.data_ptr(), _nbytes(x), hb, yb, y.data_ptr(), _stream(x))
    _native.check(rc, "otc_polyval")
    return y


def polyval_spans() -> list[int]:
    """Byte sizes of the pieces the POLYVAL kernel cuts its data into, smallest
    first (otc.h otc_polyval_spans; they are GHASH's): lengths around them take
    different paths."""
    return _spans("otc_polyval_spans")


def ctr_le32_spans() -> list[int]:
    """Byte sizes at which the counter kernel takes another path, smallest
    first (otc.h otc_ctr_le32_spans); the last is the full grid's first step."""
    return _spans("otc_ctr_le32_spans")


def _dev16(v, device, name: str) -> torch.Tensor:
    """16 bytes for a kernel to read: the caller's uint8 tensor where it is (a
    copy on the stream if it is elsewhere or misaligned), or bytes copied over."""
    if isinstance(v, torch.Tensor):
        if _nbytes(v) != 16:
            raise ValueError(f"{name} must be 16 bytes")
        t = _bytes(v.contiguous())
        return t if t.device == device and t.data_ptr() % 4 == 0 else t.to(device, copy=True)
    # a pinned copy on the stream: the host does not wait for the work in front of it
    return torch.frombuffer(bytearray(_b16(v, name)), dtype=torch.uint8).pin_memory().to(device, non_blocking=True)


def ctr_le32(x: torch.Tensor, key: bytes, ctr0, out=None) -> torch.Tensor:
    """GCM-SIV's counter mode over ``x``: bytes 0..3 of the counter block
    increment little-endian and wrap at 2**32 without carry, bytes 4..15 never
    change, bit 7 of byte 15 is forced on.  ``ctr0`` is the initial counter
    block, 16 bytes or a 16-byte uint8 tensor; a tensor on ``x``'s device is
    read by the kernel where it lies, in stream order, so it may be the result
    of an earlier op.  ``key`` is 16, 24 or 32 bytes.  Any byte length up to
    2**36; may run in place; asynchronous."""
    _check_dev(x, "x")
    c = _dev16(ctr0, x.device, "ctr0")
    k = expand_key(key)
    out = _out_like(x, out)
    return _call("otc_aes_ctr_le32", x, out, lambda ip, op: (ip, op, _nbytes(x), ctypes.byref(k), c.data_ptr(), _stream(x)))


def _gcm_siv(x: torch.Tensor, key: bytes, nonce: bytes, aad: bytes, out, tag_in):
    _check_dev(x, "x")
    key, nonce, aad = bytes(key), bytes(nonce), bytes(aad)
    n = _nbytes(x)
    gcm_siv_check(key, nonce, n, len(aad))
    k = _siv_key(key)
    out = _out_like(x, out)
    tag = torch.empty(16, dtype=torch.uint8, device=x.device)
    _call("otc_aes_gcm_siv", x, out, lambda ip, op: (
        ip, op, n, ctypes.byref(k), ENCRYPT if tag_in is None else DECRYPT, _native.as_u8p(nonce), _native.as_u8p(aad),
        len(aad), None if tag_in is None else tag_in.data_ptr(), tag.data_ptr(), _stream(x)))
    return out, tag


def gcm_siv_encrypt(x: torch.Tensor, key: bytes, nonce: bytes, aad: bytes = b"", out=None):
    """AES-GCM-SIV encryption of one message: ``(out, tag)``, the tag a 16-byte
    uint8 device tensor.  ``key`` is 16 or 32 bytes (a key-generating key:
    every nonce derives its own hash and encryption keys), ``nonce`` exactly
    12 bytes, ``aad`` host bytes.  A repeated nonce shows only whether two
    messages were equal.  Any byte length up to 2**36; may run in place;
    asynchronous -- the tag is also the counter mode's starting block, and the
    kernels hand it on in device memory: nothing is read back."""
    return _gcm_siv(x, key, nonce, aad, out, None)


def gcm_siv_decrypt(x: torch.Tensor, key: bytes, nonce: bytes, tag, aad: bytes = b"", out=None) -> torch.Tensor:
    """Authenticated AES-GCM-SIV decryption.  ``tag`` is the received 16-byte
    tag: bytes, which are copied to the device, or a uint8 tensor, which the
    counter kernel reads where it lies -- nothing is read back in front of the
    launches.  The computed tag is read back -- 16 bytes, the call's only
    synchronisation -- and compared in constant time.  On a mismatch ``out``
    is zeroed and ``GcmSivTagError`` (a ``ValueError``) raised.  May run in
    place."""
    def run():
        _check_dev(x, "x")
        return _gcm_siv(x, key, nonce, aad, out, _dev16(tag, x.device, "tag"))

    return _open_with_tag(tag, (16,), "an AES-GCM-SIV tag has 16 bytes", run,
                          GcmSivTagError, "GCM-SIV tag mismatch: the output was zeroed")
