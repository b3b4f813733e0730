"""ChaCha20, Poly1305 and the ChaCha20-Poly1305 AEAD (RFC 8439) on torch
tensors, backed by the gfx950 kernels of ``csrc/hip/chacha.hip``.

The IETF layout: a 32-byte key, a 12-byte nonce, a 32-bit block counter.
Every op runs asynchronously on torch's current HIP stream.  RFC 8439 leaves
an overflow of the counter undefined; here a call whose last block would pass
2**32 - 1 raises ``ValueError`` before any native call.  There is one kernel
family: ``last_impl`` / ``pick_impl`` do not know these ops.
"""
from __future__ import annotations

import torch

from .. import _native
from ..models.cpu_ref import CHACHA_MAX_BYTES, ChaChaTagError, _chacha_args, chacha_check_counter
from ._common import _aligned, _call, _check_dev, _lib, _nbytes, _open_with_tag, _out_like, _spans, _stream
from .keys import DECRYPT, ENCRYPT


def chacha20(x: torch.Tensor, key: bytes, nonce: bytes, counter: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """``x`` XOR the ChaCha20 keystream from block ``counter``.  Any byte
    length and any alignment (buffers that are not 16-byte aligned run on the
    slower byte-wise kernel); may run in place."""
    # written out, not through _call: the native op takes any alignment, so nothing is staged
    _check_dev(x, "x")
    key, nonce = _chacha_args(key, nonce)
    n = _nbytes(x)
    counter = chacha_check_counter(counter, n)
    out = _out_like(x, out)
    with torch.cuda.device(x.device):
        rc = _lib().otc_chacha20(x.data_ptr(), out.data_ptr(), n, _native.as_u8p(key), _native.as_u8p(nonce), counter,
                                 _stream(x))
    _native.check(rc, "otc_chacha20")
    return out


def poly1305(x: torch.Tensor, key: bytes) -> torch.Tensor:
    """The Poly1305 tag of the bytes of ``x`` under the 32-byte one-time key
    r || s: a 16-byte uint8 tensor on ``x``'s device.  Parallel over the whole
    chip; asynchronous on the current stream."""
    _check_dev(x, "x")
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("a Poly1305 key has 32 bytes")
    tag = torch.empty(16, dtype=torch.uint8, device=x.device)
    xb = _aligned(x)  # the kernel loads 16 bytes per lane
    with torch.cuda.device(x.device):
        rc = _lib().otc_poly1305(xb.data_ptr(), _nbytes(x), _native.as_u8p(key), tag.data_ptr(), _stream(x))
    _native.check(rc, "otc_poly1305")
    return tag


def poly1305_spans() -> list[int]:
    """Byte sizes of the pieces the Poly1305 kernel cuts its data into,
    smallest first (otc.h otc_poly1305_spans): lengths around them take
    different paths."""
    return _spans("otc_poly1305_spans")


def _aead(x: torch.Tensor, key: bytes, nonce: bytes, aad: bytes, out, decrypt: bool):
    _check_dev(x, "x")
    key, nonce = _chacha_args(key, nonce)
    aad = bytes(aad)
    n = _nbytes(x)
    if n > CHACHA_MAX_BYTES:
        raise ValueError("a ChaCha20-Poly1305 message has at most (2**32 - 1) * 64 bytes")
    out = _out_like(x, out)
    tag = torch.empty(16, dtype=torch.uint8, device=x.device)
    _call("otc_chacha20_poly1305", x, out, lambda ip, op: (
        ip, op, n, _native.as_u8p(key), DECRYPT if decrypt else ENCRYPT, _native.as_u8p(nonce),
        _native.as_u8p(aad), len(aad), tag.data_ptr(), _stream(x)))
    return out, tag


def chacha20_poly1305_encrypt(x: torch.Tensor, key: bytes, nonce: bytes, aad: bytes = b"", out=None):
    """ChaCha20-Poly1305 encryption of one message: ``(ct, tag)``, the tag a
    16-byte uint8 device tensor.  ``aad`` is host bytes.  Any byte length up
    to (2**32 - 1) * 64; may run in place; asynchronous -- nothing is read
    back."""
    return _aead(x, key, nonce, aad, out, False)


def chacha20_poly1305_decrypt(c: torch.Tensor, key: bytes, nonce: bytes, tag, aad: bytes = b"", out=None) -> torch.Tensor:
    """Authenticated decryption.  ``tag`` is the received 16-byte tag (bytes,
    or a uint8 tensor); the computed tag is read back -- 16 bytes, the call's
    only synchronisation -- and compared in constant time.  On a mismatch
    ``out`` is zeroed and ``ChaChaTagError`` (a ``ValueError``) raised.  May
    run in place."""
    return _open_with_tag(tag, (16,), "a ChaCha20-Poly1305 tag has 16 bytes",
                          lambda: _aead(c, key, nonce, aad, out, True),
                          ChaChaTagError, "ChaCha20-Poly1305 tag mismatch: the output was zeroed")
