"""Device AES modes on torch tensors (ROCm ``cuda`` tensors), backed by the
hand-written gfx950 kernels in ``csrc/hip/aes_tt.hip`` (LDS T-table),
``csrc/hip/aes_bs.hip`` (bitsliced VALU) and ``csrc/hip/aes_xts.hip``: CTR,
ECB, CBC, CFB128, their segment forms and XTS.  GCM is ``gcm_ops``, the
batches of small messages ``batch_ops``.

Every op runs asynchronously on torch's current HIP stream and raises on any
native error.  Tensors may have any dtype; they are treated as contiguous byte
buffers.  Reference kernels: /root/reference/aes-gpu/Source/AES.cu:284-502
(ECB only, broken launch); everything else here is new capability.
"""
from __future__ import annotations

import ctypes
import functools

import torch

from .. import _native
from ._common import IMPLS, _b16, _bytes, _call, _check_dev, _impl, _lib, _nbytes, _out_like, _stream
from .keys import DECRYPT, ENCRYPT, expand_key

_IMPL_NAMES = {v: k for k, v in IMPLS.items()}
_PICK_MODES = {"ctr": 1, "ecb": 0, "dec": 2, "ecb-dec": 2, "cbc-dec": 2, "cfb-dec": 3, "seg-dec": 4, "seg-enc": 5}


def pick_impl(impl="auto", bits: int = 128, mode: str = "ctr", nbytes: int = 0) -> str:
    """The kernel family ``impl`` resolves to for a ``mode`` call ("ctr",
    "ecb" = ECB encryption, "dec" = ECB / CBC decryption, "cfb-dec") of ``nbytes`` with
    a ``bits``-bit key (the native routing rule)."""
    if mode not in _PICK_MODES:
        raise ValueError(f"mode must be one of {list(_PICK_MODES)}")
    r = _lib().otc_pick_impl(_impl(impl), int(bits), _PICK_MODES[mode], int(nbytes))
    if r < 0:
        raise ValueError(f"bad impl {impl!r}")
    return _IMPL_NAMES[r]


def last_impl() -> str:
    """What the calling thread's last ``ctr`` / ``ecb_*`` call actually ran."""
    return _IMPL_NAMES[_lib().otc_last_impl()]


def split_fallback_reason() -> str:
    """Why the calling thread's last split / bitsliced-claim request ran the
    T-table alone ("" if it did not fall back; otc.h otc_split_fallback_reason)."""
    return (_lib().otc_split_fallback_reason() or b"").decode()


def _aes_op(name: str, x: torch.Tensor, key: bytes, out, args, decrypt_key: bool = False, inplace_ok: bool = True,
            what: str | None = None) -> torch.Tensor:
    """The single-buffer AES op: ``x`` is checked, then ``out``, then the key
    is expanded, then ``_call`` runs the native ``name`` with the tuple
    ``args(key, in_ptr, out_ptr)`` -- whose own conversions (counter, IV,
    ``impl``) therefore report after those three."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = ctypes.byref(expand_key(key, decrypt=decrypt_key))
    return _call(name, x, out, functools.partial(args, k), inplace_ok, what)


def ctr(x: torch.Tensor, key: bytes, counter: bytes, out: torch.Tensor | None = None, block_offset: int = 0,
        impl="auto") -> torch.Tensor:
    """AES-CTR (128-bit big-endian counter starting at ``counter`` + ``block_offset``)."""
    return _aes_op("otc_aes_ctr", x, key, out, lambda k, ip, op: (
        ip, op, _nbytes(x), k, _b16(counter, "counter"), int(block_offset), _impl(impl), _stream(x)))


def ctr_rfc3686(x: torch.Tensor, key: bytes, nonce: bytes, ivec: bytes, out=None, block_offset: int = 0,
                impl="auto") -> torch.Tensor:
    """AES-CTR with the AES-NI/RFC 3686 counter block nonce||ivec||BE32(1) and
    64-bit increment (reference aesni.c:120-152)."""
    return _aes_op("otc_aes_ctr_rfc3686", x, key, out, lambda k, ip, op: (
        ip, op, _nbytes(x), k, (ctypes.c_uint8 * 4).from_buffer_copy(bytes(nonce)),
        (ctypes.c_uint8 * 8).from_buffer_copy(bytes(ivec)), int(block_offset), _impl(impl), _stream(x)))


def ctr32(x: torch.Tensor, key: bytes, counter: bytes, out: torch.Tensor | None = None, impl="auto") -> torch.Tensor:
    """GCM's counter mode: only bytes 12..15 of ``counter`` increment
    (big-endian), wrapping at 2**32 with bytes 0..11 unchanged.  The CTR
    kernels of ``ctr`` with every ``impl``; a call that crosses the wrap is
    two launches.  Any byte length up to 2**32 blocks; may run in place."""
    return _aes_op("otc_aes_ctr32", x, key, out, lambda k, ip, op: (
        ip, op, _nbytes(x), k, _b16(counter, "counter"), _impl(impl), _stream(x)))


class CtrStream:
    """Resumable AES-CTR over device tensors with the PolarSSL context
    semantics (reference aes-modes/aes.c:869-900): the stream may be split at
    ANY byte across ``update`` calls and the result equals one-shot ``ctr``.
    The context (``nonce_counter``, ``stream_block``, ``nc_off``) is host
    state; ``state()`` / ``CtrStream.from_state`` checkpoint and resume it.

    Tensors may start at any byte (slices): the native call handles a head
    from ``stream_block``, a misaligned body with the funnel-shift kernel and a
    tail whose keystream block is kept for the next call."""

    def __init__(self, key: bytes, nonce_counter: bytes, impl="auto"):
        self._key = bytes(key)
        self._k = expand_key(self._key)
        self._impl = _impl(impl)
        self.ctx = _native.OtcCtrCtx()
        _native.check(_lib().otc_aes_ctr_ctx_init(ctypes.byref(self.ctx), _b16(nonce_counter, "nonce_counter")),
                      "otc_aes_ctr_ctx_init")

    @property
    def nonce_counter(self) -> bytes:
        return bytes(self.ctx.nonce_counter)

    @property
    def stream_block(self) -> bytes:
        return bytes(self.ctx.stream_block)

    @property
    def nc_off(self) -> int:
        return int(self.ctx.nc_off)

    def state(self) -> dict:
        return {"nonce_counter": self.nonce_counter, "stream_block": self.stream_block, "nc_off": self.nc_off}

    @classmethod
    def from_state(cls, key: bytes, state: dict, impl="auto") -> "CtrStream":
        s = cls(key, state["nonce_counter"], impl)
        ctypes.memmove(s.ctx.stream_block, bytes(state["stream_block"]), 16)
        s.ctx.nc_off = int(state["nc_off"])
        return s

    def update(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        # written out, not through _call: the native call takes any common alignment, so only the output is staged
        _check_dev(x, "x")
        out = _out_like(x, out)
        n = _nbytes(x)
        if n == 0:
            return out
        xp, op = x.data_ptr(), out.data_ptr()
        target = out
        if xp % 16 != op % 16:  # the native call needs a common alignment: stage the output
            tmp = torch.empty(n + 16, dtype=torch.uint8, device=x.device)
            off = (xp - tmp.data_ptr()) % 16
            target = tmp[off:off + n]
        with torch.cuda.device(x.device):
            rc = _lib().otc_aes_ctr_stream(ctypes.byref(self.ctx), ctypes.byref(self._k), n, xp, target.data_ptr(),
                                           self._impl, _stream(x))
        _native.check(rc, "otc_aes_ctr_stream")
        if target is not out:
            _bytes(out).copy_(target)
        return out


def _ecb(x: torch.Tensor, key: bytes, out, impl, decrypt: bool) -> torch.Tensor:
    return _aes_op("otc_aes_ecb", x, key, out, lambda k, ip, op: (ip, op, _nbytes(x), k, _impl(impl), _stream(x)),
                   decrypt_key=decrypt, what=f"otc_aes_ecb({'decrypt' if decrypt else 'encrypt'})")


def ecb_encrypt(x: torch.Tensor, key: bytes, out=None, impl="auto") -> torch.Tensor:
    return _ecb(x, key, out, impl, False)


def ecb_decrypt(x: torch.Tensor, key: bytes, out=None, impl="auto") -> torch.Tensor:
    """ECB decryption: the T-table inverse cipher, the bitsliced one (the
    forward S-box as S^-1 = L S L), or both concurrently ("split").  "auto":
    the split from 2 GiB, the persistent T-table claim kernel alone from 512
    MiB, the grid T-table below (engine.cpp pick_ecb_impl / split_form)."""
    return _ecb(x, key, out, impl, True)


def _chain_decrypt(mode: str, x: torch.Tensor, key: bytes, iv: bytes, out, impl, decrypt_key: bool) -> torch.Tensor:
    return _aes_op(f"otc_aes_{mode}_decrypt_impl", x, key, out, lambda k, ip, op: (
        ip, op, _nbytes(x), k, _b16(iv, "iv"), _impl(impl), _stream(x)),
        decrypt_key=decrypt_key, inplace_ok=False, what=f"otc_aes_{mode}_decrypt")


def cbc_decrypt(x: torch.Tensor, key: bytes, iv: bytes, out=None, impl="auto") -> torch.Tensor:
    """Parallel CBC decryption (kernel choice as ecb_decrypt).  In place
    (out=x) runs through a copy of the input: block i needs ciphertext block
    i-1, which its own output overwrites."""
    return _chain_decrypt("cbc", x, key, iv, out, impl, True)


def cfb128_decrypt(x: torch.Tensor, key: bytes, iv: bytes, out=None, impl="auto") -> torch.Tensor:
    """Parallel CFB128 decryption, P_i = C_i ^ E(C_{i-1}) (encryption key).
    ``impl``: "ttable", "bitslice" (the forward bitsliced cipher on the input
    shifted one block), "split" (both at once, as ECB encryption) or "auto"
    (as ecb_decrypt).  In place runs through a copy of the input."""
    return _chain_decrypt("cfb128", x, key, iv, out, impl, False)


def _seg_call(mode: str, x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out, impl, decrypt: bool,
              decrypt_key: bool = False, py_mod16: bool = True) -> torch.Tensor:
    """The four segment ops (``mode``: "cbc" / "cfb128").  Decryption is
    parallel and so never in place on the device; CFB decrypts with the
    encryption key."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    n = _nbytes(x)
    if py_mod16:
        if segment_bytes <= 0 or segment_bytes % 16 or n % segment_bytes:
            raise ValueError("segment_bytes must be a positive multiple of 16 dividing the byte size")
    elif segment_bytes <= 0 or n % segment_bytes:
        # cbc_decrypt_segments alone leaves segment_bytes % 16 to the native check (a RuntimeError), under its own message
        raise ValueError("byte size must be a multiple of segment_bytes")
    k = expand_key(key, decrypt=decrypt_key)
    name = f"otc_aes_{mode}_{'decrypt' if decrypt else 'encrypt'}_segments"
    return _call(name + "_impl", x, out, lambda ip, op: (
        ip, op, segment_bytes, n // segment_bytes, ctypes.byref(k), _b16(iv0, "iv0"), _impl(impl), _stream(x)),
        inplace_ok=not decrypt, what=name if decrypt else name + "_impl")  # the names errors have carried so far


def cbc_encrypt_segments(x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out=None,
                         impl="auto") -> torch.Tensor:
    """CBC encryption of independent contiguous segments; segment s uses
    IV = iv0 + s (128-bit BE), one serial chain per segment, one chain per
    lane on the T-table kernels for every ``impl`` (the persistent claim
    kernel from 1 GiB, the grid kernel
    below; a VALU kernel for this mode lost at every size and was removed).  A
    single segment is exact serial CBC on ONE lane -- use
    ``models.AES.cbc_encrypt`` (routes exact single-stream encryption to the
    host AES-NI chain) unless the buffer is small.  May run in place."""
    return _seg_call("cbc", x, key, iv0, segment_bytes, out, impl, decrypt=False)


def cbc_decrypt_segments(x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out=None,
                         impl="auto") -> torch.Tensor:
    """Inverse of ``cbc_encrypt_segments``: fully parallel.  ``impl``:
    "ttable", "bitslice" (the bitsliced claim kernel alone), "split" (both at
    once), "auto" = split from 2 GiB of power-of-two segments, the persistent
    T-table claim kernel from 512 MiB (other segment sizes: the T-table)."""
    return _seg_call("cbc", x, key, iv0, segment_bytes, out, impl, decrypt=True, decrypt_key=True, py_mod16=False)


def cfb128_encrypt_segments(x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out=None,
                            impl="auto") -> torch.Tensor:
    """CFB128 encryption of independent segments (IV_s = iv0 + s), one
    serial chain per segment (``impl`` as ``cbc_encrypt_segments``)."""
    return _seg_call("cfb128", x, key, iv0, segment_bytes, out, impl, decrypt=False)


def cfb128_decrypt_segments(x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out=None,
                            impl="auto") -> torch.Tensor:
    """Inverse of ``cfb128_encrypt_segments``: fully parallel (``impl`` as
    ``cbc_decrypt_segments``)."""
    return _seg_call("cfb128", x, key, iv0, segment_bytes, out, impl, decrypt=True)


XTS_MAX_UNIT = 1 << 24  # bytes: 2**20 blocks, the IEEE 1619 limit


@functools.lru_cache(maxsize=64)
def _xts_key(key: bytes, direction: int) -> _native.OtcXtsKey:
    k = _native.OtcXtsKey()
    _native.check(_lib().otc_xts_key_init(ctypes.byref(k), _native.as_u8p(key), len(key) * 8, direction),
                  "otc_xts_key_init")
    return k


def _xts_tweak(tweak0) -> ctypes.Array:
    """A tweak number as 16 little-endian bytes (an int modulo 2**128, or 16 bytes as they are)."""
    if isinstance(tweak0, int):
        tweak0 = (tweak0 % (1 << 128)).to_bytes(16, "little")
    return _b16(tweak0, "tweak0")


def _xts(x: torch.Tensor, key: bytes, tweak0, unit_bytes, out, decrypt: bool) -> torch.Tensor:
    # not through _aes_op: the units and the tweak are checked before ``out``, and the key is K1 || K2
    _check_dev(x, "x")
    key = bytes(key)
    if len(key) not in (32, 64):
        raise ValueError(f"XTS key must be 32 or 64 bytes (K1 || K2), got {len(key)}")
    n = _nbytes(x)
    unit = n if unit_bytes is None else int(unit_bytes)
    if unit < 16 or unit > XTS_MAX_UNIT or n % unit:
        raise ValueError("an XTS data unit is 16 bytes to 16 MiB and divides the byte size")
    if n // unit > 1 and unit % 16:
        raise ValueError("XTS data units of several must be multiples of 16 bytes")
    tw = _xts_tweak(tweak0)
    out = _out_like(x, out)
    k = _xts_key(key, DECRYPT if decrypt else ENCRYPT)
    return _call("otc_aes_xts", x, out, lambda ip, op: (ip, op, unit, n // unit, ctypes.byref(k), tw, _stream(x)))


def xts_encrypt(x: torch.Tensor, key: bytes, tweak0, unit_bytes: int | None = None, out=None) -> torch.Tensor:
    """XTS-AES (IEEE 1619) encryption of data units (sectors) of ``unit_bytes``
    each; ``None`` takes the whole tensor as one unit, which may then have any
    length from 16 bytes (ciphertext stealing).  ``key`` is K1 || K2 (32 or 64
    bytes); unit s uses tweak number ``tweak0 + s`` -- an int, or 16 bytes read
    as a 128-bit little-endian number (dm-crypt plain64: the sector number).
    Fully parallel; may run in place; the grid T-table kernels of
    ``csrc/hip/aes_xts.hip`` (``last_impl() == "ttable"``)."""
    return _xts(x, key, tweak0, unit_bytes, out, False)


def xts_decrypt(x: torch.Tensor, key: bytes, tweak0, unit_bytes: int | None = None, out=None) -> torch.Tensor:
    """Inverse of ``xts_encrypt`` (as parallel, and also allowed in place)."""
    return _xts(x, key, tweak0, unit_bytes, out, True)
