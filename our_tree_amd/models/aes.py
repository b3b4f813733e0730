"""The AES "model family": a BlockCipher-style object over the gfx950 kernels.

Parity: the reference's ``BlockCipher`` interface and ``AES`` host class
(/root/reference/aes-gpu/Source/BlockCipher.h:48-107, AES.h:84-147):
block/key size queries, ``make_key(key, bits, direction)``, ``encrypt`` /
``decrypt`` of n blocks -- extended with every mode the CPU API offers
(CBC, CFB128, CTR) plus sharding-friendly counter offsets.  GPU tensors go to
the HIP kernels; ``bytes`` go to the C oracle.
"""
from __future__ import annotations

import torch

from .. import ops
from . import cpu_ref

DIR_NONE, DIR_ENCRYPT, DIR_DECRYPT = 0, 1, 2
DIR_BOTH = DIR_ENCRYPT | DIR_DECRYPT


class AES:
    block_bits = 128
    block_size = 16

    def __init__(self, key: bytes | None = None, impl: str = "auto"):
        self._key = None
        self.impl = impl
        if key is not None:
            self.make_key(key)

    # ---- BlockCipher interface -------------------------------------------
    def make_key(self, key: bytes, key_bits: int | None = None, direction: int = DIR_BOTH):
        key = bytes(key)
        if key_bits is not None and key_bits != len(key) * 8:
            raise ValueError("key_bits does not match the key length")
        if len(key) not in (16, 24, 32):
            raise ValueError("Invalid AES key size.")
        self._key = key
        if direction & DIR_ENCRYPT:
            ops.expand_key(key)
        if direction & DIR_DECRYPT:
            ops.expand_key(key, decrypt=True)
        return self

    @property
    def key_bits(self) -> int:
        return len(self._key) * 8

    @property
    def key_size(self) -> int:
        return len(self._key)

    @property
    def rounds(self) -> int:
        return {16: 10, 24: 12, 32: 14}[len(self._key)]

    def encrypt(self, data, out=None):
        """ECB encryption of whole blocks."""
        if isinstance(data, torch.Tensor):
            return ops.ecb_encrypt(data, self._key, out=out, impl=self.impl)
        return cpu_ref.ecb(self._key, data)

    def decrypt(self, data, out=None):
        if isinstance(data, torch.Tensor):
            return ops.ecb_decrypt(data, self._key, out=out, impl=self.impl)
        return cpu_ref.ecb(self._key, data, decrypt=True)

    # ---- modes -------------------------------------------------------------
    def ctr(self, data, counter: bytes, block_offset: int = 0, out=None):
        if isinstance(data, torch.Tensor):
            return ops.ctr(data, self._key, counter, out=out, block_offset=block_offset, impl=self.impl)
        return cpu_ref.ctr(self._key, counter, data, block_offset)

    # exact single-stream CBC / CFB encryption is one serial chain: on a GPU it
    # would run on ONE lane (~67M dependent block encryptions per GiB), far
    # slower than one AES-NI core, so GPU tensors take the host chain unless
    # the caller opts in with device_serial=True (small buffers, no host trip)
    def _serial_on_host(self, mode: str, data: torch.Tensor, iv: bytes, out):
        res = cpu_ref.serial_encrypt(mode, self._key, iv, data.reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
        t = torch.frombuffer(bytearray(res), dtype=torch.uint8).to(data.device)
        if out is None:
            return t.view(data.dtype).view(data.shape)
        out.reshape(-1).view(torch.uint8).copy_(t)
        return out

    def cbc_encrypt(self, data, iv: bytes, segment_bytes: int | None = None, out=None, device_serial: bool = False):
        """CBC encryption.  ``segment_bytes``: independent segments with
        IV_s = iv + s (parallel, one lane per segment); None = one exact
        serial stream (host AES-NI chain for GPU tensors, see above)."""
        if isinstance(data, torch.Tensor):
            if segment_bytes:
                return ops.cbc_encrypt_segments(data, self._key, iv, segment_bytes, out=out)
            if device_serial:
                return ops.cbc_encrypt_segments(data, self._key, iv, data.numel() * data.element_size(), out=out)
            return self._serial_on_host("cbc", data, iv, out)
        if segment_bytes:
            return cpu_ref.cbc_segments(self._key, iv, data, segment_bytes)
        return cpu_ref.serial_encrypt("cbc", self._key, iv, data)

    def cbc_decrypt(self, data, iv: bytes, segment_bytes: int | None = None, out=None):
        if isinstance(data, torch.Tensor):
            if segment_bytes:
                return ops.cbc_decrypt_segments(data, self._key, iv, segment_bytes, out=out)
            return ops.cbc_decrypt(data, self._key, iv, out=out, impl=self.impl)
        if segment_bytes:
            return cpu_ref.cbc_segments(self._key, iv, data, segment_bytes, decrypt=True)
        return cpu_ref.cbc(self._key, iv, data, decrypt=True)

    def cfb128_decrypt(self, data, iv: bytes, segment_bytes: int | None = None, out=None):
        if isinstance(data, torch.Tensor):
            if segment_bytes:
                return ops.cfb128_decrypt_segments(data, self._key, iv, segment_bytes, out=out)
            return ops.cfb128_decrypt(data, self._key, iv, out=out, impl=self.impl)
        if segment_bytes:
            return cpu_ref.cfb128_segments(self._key, iv, data, segment_bytes, decrypt=True)
        return cpu_ref.cfb128(self._key, iv, data, decrypt=True)

    def cfb128_encrypt(self, data, iv: bytes, segment_bytes: int | None = None, out=None,
                       device_serial: bool = False):
        """CFB128 encryption (reference aes-modes/aes.c:822-862): a serial
        chain.  ``segment_bytes``: independent segments with IV_s = iv + s on
        the GPU sector kernel; None = exact single stream (host AES-NI chain
        for GPU tensors unless ``device_serial``)."""
        if isinstance(data, torch.Tensor):
            if segment_bytes:
                return ops.cfb128_encrypt_segments(data, self._key, iv, segment_bytes, out=out)
            if device_serial:
                return ops.cfb128_encrypt_segments(data, self._key, iv, data.numel() * data.element_size(), out=out)
            return self._serial_on_host("cfb128", data, iv, out)
        if segment_bytes:
            return cpu_ref.cfb128_segments(self._key, iv, data, segment_bytes)
        return cpu_ref.serial_encrypt("cfb128", self._key, iv, data)

    # ---- authenticated: AES-OCB3 (RFC 7253), one pass over the data ---------
    def ocb_encrypt(self, data, nonce: bytes, aad: bytes = b"", out=None, tag_bytes: int = 16):
        """``(ciphertext, tag)``: the nonce is 1 to 15 bytes and never reused
        under this key, the tag ``tag_bytes`` (1 to 16) long."""
        if isinstance(data, torch.Tensor):
            return ops.ocb_ops.ocb_encrypt(data, self._key, nonce, aad, out=out, tag_bytes=tag_bytes)
        return cpu_ref.ocb(self._key, nonce, data, aad, tag_bytes=tag_bytes)

    def ocb_decrypt(self, data, nonce: bytes, tag, aad: bytes = b"", out=None):
        """The plaintext; ``cpu_ref.OcbTagError`` -- with the output zeroed --
        when the received ``tag`` (its length is the message's TAGLEN) does not match."""
        if isinstance(data, torch.Tensor):
            return ops.ocb_ops.ocb_decrypt(data, self._key, nonce, tag, aad, out=out)
        return cpu_ref.ocb_auth_decrypt(self._key, nonce, data, tag, aad)

    def ocb_encrypt_batch(self, xs, nonces, aads=None, outs=None):
        """Many GPU records at once, all under this key, each with its own
        12-byte nonce (a device uint8 [n, 12] tensor) and AAD: ``(outs, tags)``
        with 16-byte tags (``ops.ocb_batch_ops.OcbBatch``)."""
        return ops.ocb_batch_ops.ocb_encrypt_batch(xs, self._key, nonces, aads=aads, outs=outs)

    def ocb_decrypt_batch(self, xs, nonces, tags, aads=None, outs=None):
        """``(outs, ok)``: ``ok`` is a device bool [n] tensor, and the output
        of every record whose tag does not match is zeroed."""
        return ops.ocb_batch_ops.ocb_decrypt_batch(xs, self._key, nonces, tags, aads=aads, outs=outs)

    # ---- authenticated: batched AES-CCM (SP 800-38C, RFC 3610), one record per lane ----
    def ccm_encrypt_batch(self, xs, nonces, aads=None, outs=None, tag_bytes: int = 16):
        """Many GPU records at once, all under this key, each with its own
        nonce (a device uint8 [n, 7 .. 13] tensor: its width is the batch's
        nonce length) and AAD: ``(outs, tags)`` with ``tag_bytes``-long tags
        (``ops.ccm_batch_ops.CcmBatch``)."""
        return ops.ccm_batch_ops.ccm_encrypt_batch(xs, self._key, nonces, aads=aads, outs=outs, tag_bytes=tag_bytes)

    def ccm_decrypt_batch(self, xs, nonces, tags, aads=None, outs=None):
        """``(outs, ok)``: ``ok`` is a device bool [n] tensor, and the output
        of every record whose tag (a device uint8 [n, tag length] tensor) does
        not match is zeroed."""
        return ops.ccm_batch_ops.ccm_decrypt_batch(xs, self._key, nonces, tags, aads=aads, outs=outs)

    # ---- authenticated: batched AES-GCM-SIV (RFC 8452), nonce-misuse resistant ----
    def gcm_siv_encrypt_batch(self, xs, nonces, aads=None, outs=None):
        """Many GPU records at once, this key (16 or 32 bytes) as the
        key-generating key, each record with its own 12-byte nonce (a device
        uint8 [n, 12] tensor) and AAD: ``(outs, tags)`` with 16-byte tags
        (``ops.gcm_siv_batch_ops.GcmSivBatch``)."""
        return ops.gcm_siv_batch_ops.gcm_siv_encrypt_batch(xs, self._key, nonces, aads=aads, outs=outs)

    def gcm_siv_decrypt_batch(self, xs, nonces, tags, aads=None, outs=None):
        """``(outs, ok)``: ``ok`` is a device bool [n] tensor, and the output
        of every record whose tag does not match is zeroed."""
        return ops.gcm_siv_batch_ops.gcm_siv_decrypt_batch(xs, self._key, nonces, tags, aads=aads, outs=outs)


class AESXTS:
    """XTS-AES (IEEE 1619) sector cipher: ``key`` is K1 || K2, 32 bytes
    (AES-128) or 64 (AES-256).  Data units of ``unit_bytes`` use tweak numbers
    ``tweak0``, ``tweak0 + 1``, ... (ints, or 16 bytes as a 128-bit
    little-endian number); ``unit_bytes=None`` takes the data as one unit of
    any length from 16 bytes (ciphertext stealing).  GPU tensors go to the HIP
    kernels (in place allowed), ``bytes`` to the C oracle."""

    def __init__(self, key: bytes):
        key = bytes(key)
        if len(key) not in (32, 64):
            raise ValueError("Invalid XTS key size (K1 || K2: 32 or 64 bytes).")
        self._key = key

    @property
    def key_bits(self) -> int:
        """Bits of each AES key half."""
        return len(self._key) * 4

    def encrypt(self, data, tweak0, unit_bytes: int | None = None, out=None):
        if isinstance(data, torch.Tensor):
            return ops.xts_encrypt(data, self._key, tweak0, unit_bytes, out=out)
        return cpu_ref.xts(self._key, tweak0, data, unit_bytes)

    def decrypt(self, data, tweak0, unit_bytes: int | None = None, out=None):
        if isinstance(data, torch.Tensor):
            return ops.xts_decrypt(data, self._key, tweak0, unit_bytes, out=out)
        return cpu_ref.xts(self._key, tweak0, data, unit_bytes, decrypt=True)


class AESGCM:
    """AES-GCM (NIST SP 800-38D) with a 16, 24 or 32-byte ``key``: one message
    per call, any IV length from 1 byte, ``aad`` as host bytes.  GPU tensors go
    to the HIP kernels (CTR32 + the parallel GHASH; in place allowed), ``bytes``
    to the C oracle.  ``encrypt`` returns ``(ciphertext, tag)``; ``decrypt``
    takes the received tag (4 to 16 bytes) and raises ``ops.GcmTagError`` --
    with the output zeroed -- when it does not match."""

    def __init__(self, key: bytes):
        key = bytes(key)
        if len(key) not in (16, 24, 32):
            raise ValueError("Invalid AES key size (16, 24 or 32 bytes).")
        self._key = key

    @property
    def key_bits(self) -> int:
        return len(self._key) * 8

    def encrypt(self, data, iv: bytes, aad: bytes = b"", out=None, impl="auto"):
        if isinstance(data, torch.Tensor):
            return ops.gcm_encrypt(data, self._key, iv, aad, out=out, impl=impl)
        return cpu_ref.gcm(self._key, iv, data, aad)

    def decrypt(self, data, iv: bytes, tag, aad: bytes = b"", out=None, impl="auto"):
        if isinstance(data, torch.Tensor):
            return ops.gcm_decrypt(data, self._key, iv, tag, aad, out=out, impl=impl)
        return cpu_ref.gcm_auth_decrypt(self._key, iv, data, tag, aad)

    def encrypt_batch(self, xs, ivs, aads=None, outs=None):
        """Many records in one run (``ops.GcmBatch``): GPU tensors ``xs``, a
        device uint8 [n, 12] tensor of IVs, never reused under this key;
        ``(outs, tags)`` with the tags a device uint8 [n, 16] tensor."""
        return ops.gcm_encrypt_batch(xs, self._key, ivs, aads=aads, outs=outs)

    def decrypt_batch(self, xs, ivs, tags, aads=None, outs=None):
        """``(outs, ok)``: ``ok`` a device bool [n] tensor; the output of every
        record whose tag (device uint8 [n, 4..16]) does not match is zeroed.
        Nothing is read back and nothing raised."""
        return ops.gcm_decrypt_batch(xs, self._key, ivs, tags, aads=aads, outs=outs)
