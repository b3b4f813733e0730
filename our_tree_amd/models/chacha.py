"""The ChaCha20-Poly1305 "model": the AEAD of RFC 8439 over the gfx950 kernels."""
from __future__ import annotations

import torch

from .. import ops
from . import cpu_ref


class ChaCha20Poly1305:
    """ChaCha20-Poly1305 (RFC 8439) with a 32-byte ``key``: one message per
    call, a 12-byte nonce never reused under the key, ``aad`` as host bytes.
    GPU tensors go to the HIP kernels (ChaCha20 + the parallel Poly1305; in
    place allowed), ``bytes`` to the C oracle.  ``encrypt`` returns
    ``(ciphertext, tag)``; ``decrypt`` takes the received 16-byte tag and
    raises ``ops.ChaChaTagError`` -- with the output zeroed -- when it does
    not match.  ``encrypt_batch`` / ``decrypt_batch`` take many GPU records at
    once, all under this key (``ops.chacha_batch_ops.ChaChaBatch``)."""

    def __init__(self, key: bytes):
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("a ChaCha20-Poly1305 key has 32 bytes")
        self._key = key

    def encrypt(self, data, nonce: bytes, aad: bytes = b"", out=None):
        if isinstance(data, torch.Tensor):
            return ops.chacha20_poly1305_encrypt(data, self._key, nonce, aad, out=out)
        return cpu_ref.chacha20_poly1305(self._key, nonce, data, aad)

    def decrypt(self, data, nonce: bytes, tag, aad: bytes = b"", out=None):
        if isinstance(data, torch.Tensor):
            return ops.chacha20_poly1305_decrypt(data, self._key, nonce, tag, aad, out=out)
        return cpu_ref.chacha20_poly1305_auth_decrypt(self._key, nonce, data, tag, aad)

    def encrypt_batch(self, xs, nonces: torch.Tensor, aads=None, outs=None):
        """Many GPU records under this key, record m with ``nonces[m]`` (a
        device uint8 [n, 12] tensor) and ``aads[m]``: ``(outs, tags)`` with the
        tags a device uint8 [n, 16] tensor."""
        return ops.chacha_batch_ops.chacha20_poly1305_encrypt_batch(xs, self._key, nonces, aads=aads, outs=outs)

    def decrypt_batch(self, xs, nonces: torch.Tensor, tags: torch.Tensor, aads=None, outs=None):
        """``(outs, ok)``: ``ok`` is a device bool [n] tensor; the output of
        every record whose tag does not match is zeroed.  Nothing is read
        back and nothing is raised: check ``ok``."""
        return ops.chacha_batch_ops.chacha20_poly1305_decrypt_batch(xs, self._key, nonces, tags, aads=aads, outs=outs)
