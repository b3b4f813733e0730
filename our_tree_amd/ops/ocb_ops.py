"""AES-OCB3 (RFC 7253) of one message on torch tensors, backed by the gfx950
kernels of ``csrc/hip/aes_ocb.hip``: an AEAD in one pass over the data.  Its
names are reached as ``ops.ocb_ops.*``; they are not in ``ops.__all__`` yet
(docs/API.md)."""
from __future__ import annotations

import ctypes
import functools

import torch

from .. import _native
from ..models.cpu_ref import OcbTagError, ocb_check, ocb_check_blocks
from ._common import _b16, _call, _check_dev, _check_out, _lib, _nbytes, _open_with_tag, _out_like, _spans, _stream
from .keys import DECRYPT, ENCRYPT


@functools.lru_cache(maxsize=64)
def _ocb_key(key: bytes) -> _native.OtcOcbKey:
    k = _native.OtcOcbKey()
    if _lib().otc_ocb_key_init(ctypes.byref(k), _native.as_u8p(key), len(key) * 8):
        raise ValueError(f"AES key must be 16, 24 or 32 bytes, got {len(key)}")
    return k


def ocb_spans() -> list[int]:
    """Byte sizes at which the bulk kernel takes another path, smallest first
    (otc.h otc_ocb_spans); the last is the full grid's first step, past which
    workgroups take a second grid step."""
    return _spans("otc_ocb_spans")


def _ocb(x: torch.Tensor, key: bytes, nonce: bytes, aad: bytes, out, tag_bytes: int, decrypt: bool):
    _check_dev(x, "x")
    key, nonce, aad = bytes(key), bytes(nonce), bytes(aad)
    n = _nbytes(x)
    ocb_check(nonce, tag_bytes, n)
    k = _ocb_key(key)
    out = _out_like(x, out)
    tag = torch.empty(16, dtype=torch.uint8, device=x.device)
    _call("otc_aes_ocb", x, out, lambda ip, op: (
        ip, op, n, ctypes.byref(k), DECRYPT if decrypt else ENCRYPT, _native.as_u8p(nonce), len(nonce),
        _native.as_u8p(aad), len(aad), tag_bytes, tag.data_ptr(), _stream(x)))
    return out, tag


def ocb_encrypt(x: torch.Tensor, key: bytes, nonce: bytes, aad: bytes = b"", out=None, tag_bytes: int = 16):
    """AES-OCB3 encryption of one message: ``(out, tag)``, the tag a
    ``tag_bytes``-long uint8 device tensor.  ``key`` is 16, 24 or 32 bytes,
    ``nonce`` 1 to 15 bytes (never reuse one under a key), ``aad`` host bytes,
    ``tag_bytes`` 1 to 16 -- the tag length enters the nonce block, so another
    length gives another ciphertext.  Any byte length up to 2**36; may run in
    place; asynchronous -- nothing is read back and nothing is allocated
    beyond the results."""
    out, tag = _ocb(x, key, nonce, aad, out, tag_bytes, False)
    return out, tag[:tag_bytes]


def ocb_decrypt(x: torch.Tensor, key: bytes, nonce: bytes, tag, aad: bytes = b"", out=None) -> torch.Tensor:
    """Authenticated AES-OCB3 decryption.  ``tag`` is the received tag (bytes,
    or a uint8 tensor) and its length the message's TAGLEN, 1 to 16 bytes; the
    computed tag is read back -- 16 bytes, the call's only synchronisation --
    and compared in constant time.  On a mismatch ``out`` is zeroed and
    ``OcbTagError`` (a ``ValueError``) raised.  May run in place."""
    tag_bytes = int(tag.numel()) if isinstance(tag, torch.Tensor) else len(bytes(tag))  # a bad length: raised below
    return _open_with_tag(tag, range(1, 17), "an OCB tag has 1 to 16 bytes",
                          lambda: _ocb(x, key, nonce, aad, out, tag_bytes, True),
                          OcbTagError, "OCB tag mismatch: the output was zeroed")


def ocb_blocks(x: torch.Tensor, key: bytes, offset0: bytes, first_block: int = 0, checksum: torch.Tensor | None = None,
               out=None, decrypt: bool = False):
    """The primitive under the AEAD: the whole blocks ``first_block + 1 ..`` of
    a message whose ``Offset_0`` (``cpu_ref.ocb_offset0``) is given, ``x``
    holding them (a multiple of 16 bytes; ``first_block + blocks <= 2**32``).
    Returns ``(out, checksum)``: the XOR of the blocks' plaintexts is XORed
    into ``checksum``, 16 uint8 on ``x``'s device (a fresh zeroed one if none
    is given), so a message can be cut across calls, streams or devices; its
    trailing bytes and its tag are the caller's.  Needs 16-byte aligned
    buffers; may run in place; asynchronous."""
    _check_dev(x, "x")
    n = _nbytes(x)
    if n % 16:
        raise ValueError("OCB blocks are 16 bytes: the byte length must be a multiple of 16")
    ocb_check_blocks(first_block, n // 16)
    o0 = _b16(offset0, "offset0")
    k = _ocb_key(bytes(key))
    if checksum is None:
        checksum = torch.zeros(16, dtype=torch.uint8, device=x.device)
    else:
        _check_out(checksum, 16, x.device, "checksum must have 16 bytes")
        if checksum.data_ptr() % 16:
            raise ValueError("checksum must be 16-byte aligned")
    out = _out_like(x, out)
    _call("otc_aes_ocb_blocks", x, out, lambda ip, op: (
        ip, op, n // 16, ctypes.byref(k), DECRYPT if decrypt else ENCRYPT, o0, first_block, checksum.data_ptr(),
        _stream(x)))
    return out, checksum
