"""CPU oracle wrappers (bytes in, bytes out) over the C reference-compatible
API in ``csrc/cpu`` (aes.h / arc4.h / rc4.h / aesni.h).  Used by the tests, by
the CPU fallback of the distributed planner tests, and as the verification
oracle for every device kernel.  API parity: /root/reference/aes-modes/aes.h,
/root/reference/arc4.h, /root/reference/rc4.h, /root/reference/aes-modes/aesni.h.
"""
from __future__ import annotations

import ctypes

from .. import _native

AES_ENCRYPT = 1
AES_DECRYPT = 0


def _ctx(key: bytes, decrypt: bool = False) -> _native.AesContext:
    lib = _native.cpu_lib()
    ctx = _native.AesContext()
    fn = lib.aes_setkey_dec if decrypt else lib.aes_setkey_enc
    rc = fn(ctypes.byref(ctx), _native.as_u8p(bytes(key)), len(key) * 8)
    if rc:
        raise ValueError("invalid AES key length")
    return ctx


def _buf(n: int):
    return (ctypes.c_uint8 * max(n, 1))()


def ecb(key: bytes, data: bytes, decrypt: bool = False, threads: int = 1) -> bytes:
    if len(data) % 16:
        raise ValueError("ECB needs a multiple of 16 bytes")
    ctx = _ctx(key, decrypt)
    out = _buf(len(data))
    _native.cpu_lib().aes_ecb_bulk(ctypes.byref(ctx), AES_DECRYPT if decrypt else AES_ENCRYPT,
                                   _native.as_u8p(bytes(data)), out, len(data), threads)
    return bytes(out)[: len(data)]


def ctr(key: bytes, counter: bytes, data: bytes, block_offset: int = 0, threads: int = 1) -> bytes:
    ctx = _ctx(key)
    nc = (ctypes.c_uint8 * 16).from_buffer_copy(bytes(counter))
    if block_offset:
        _native.cpu_lib().aes_ctr128_add(nc, block_offset)
    out = _buf(len(data))
    _native.cpu_lib().aes_ctr_bulk(ctypes.byref(ctx), nc, _native.as_u8p(bytes(data)), out, len(data), threads)
    return bytes(out)[: len(data)]


def ctr_stream(key: bytes, nonce_counter: bytearray, stream_block: bytearray, nc_off: list, data: bytes) -> bytes:
    """Byte-granular resumable CTR exactly as aes_crypt_ctr (updates the
    counter, stream block and offset in place)."""
    ctx = _ctx(key)
    nc = (ctypes.c_uint8 * 16).from_buffer(nonce_counter)
    sb = (ctypes.c_uint8 * 16).from_buffer(stream_block)
    off = ctypes.c_int(nc_off[0])
    out = _buf(len(data))
    _native.cpu_lib().aes_crypt_ctr(ctypes.byref(ctx), len(data), ctypes.byref(off), nc, sb,
                                    _native.as_u8p(bytes(data)), out)
    nc_off[0] = off.value
    return bytes(out)[: len(data)]


def cbc(key: bytes, iv: bytes, data: bytes, decrypt: bool = False) -> bytes:
    ctx = _ctx(key, decrypt)
    ivb = (ctypes.c_uint8 * 16).from_buffer_copy(bytes(iv))
    out = _buf(len(data))
    rc = _native.cpu_lib().aes_crypt_cbc(ctypes.byref(ctx), AES_DECRYPT if decrypt else AES_ENCRYPT, len(data), ivb,
                                         _native.as_u8p(bytes(data)), out)
    if rc:
        raise ValueError("CBC needs a multiple of 16 bytes")
    return bytes(out)[: len(data)]


def cfb128(key: bytes, iv: bytes, data: bytes, decrypt: bool = False) -> bytes:
    ctx = _ctx(key)
    ivb = (ctypes.c_uint8 * 16).from_buffer_copy(bytes(iv))
    off = ctypes.c_int(0)
    out = _buf(len(data))
    _native.cpu_lib().aes_crypt_cfb128(ctypes.byref(ctx), AES_DECRYPT if decrypt else AES_ENCRYPT, len(data),
                                       ctypes.byref(off), ivb, _native.as_u8p(bytes(data)), out)
    return bytes(out)[: len(data)]


def ctr128_add(counter: bytes, blocks: int) -> bytes:
    v = (int.from_bytes(bytes(counter), "big") + blocks) % (1 << 128)
    return v.to_bytes(16, "big")


def cbc_segments(key: bytes, iv0: bytes, data: bytes, segment_bytes: int, decrypt: bool = False) -> bytes:
    """Per-segment CBC with IV_s = iv0 + s (the device segment semantics)."""
    out = bytearray()
    for s, off in enumerate(range(0, len(data), segment_bytes)):
        out += cbc(key, ctr128_add(iv0, s), data[off: off + segment_bytes], decrypt)
    return bytes(out)


def cfb128_segments(key: bytes, iv0: bytes, data: bytes, segment_bytes: int, decrypt: bool = False) -> bytes:
    """Per-segment CFB128 with IV_s = iv0 + s (the device segment semantics)."""
    out = bytearray()
    for s, off in enumerate(range(0, len(data), segment_bytes)):
        out += cfb128(key, ctr128_add(iv0, s), data[off: off + segment_bytes], decrypt)
    return bytes(out)


def xts_tweak(tweak0) -> bytes:
    """A tweak number as its 16 little-endian bytes (an int modulo 2**128, or
    16 bytes taken as they are)."""
    if isinstance(tweak0, int):
        return (tweak0 % (1 << 128)).to_bytes(16, "little")
    tweak0 = bytes(tweak0)
    if len(tweak0) != 16:
        raise ValueError("tweak0 must be an int or 16 bytes")
    return tweak0


def xts(key: bytes, tweak0, data: bytes, unit_bytes: int | None = None, decrypt: bool = False) -> bytes:
    """XTS-AES (IEEE 1619) over data units of ``unit_bytes`` (None: the data
    is one unit); unit s uses tweak number ``tweak0 + s`` (128-bit
    little-endian).  ``key`` is K1 || K2, 32 or 64 bytes.  A single unit may
    have any length from 16 bytes (ciphertext stealing)."""
    key, data = bytes(key), bytes(data)
    if len(key) not in (32, 64):
        raise ValueError("XTS key must be 32 or 64 bytes (K1 || K2)")
    unit = len(data) if unit_bytes is None else int(unit_bytes)
    if unit < 16 or len(data) % unit:
        raise ValueError("unit_bytes must be at least 16 and divide the data")
    nunits = len(data) // unit
    if unit > 1 << 24 or (nunits > 1 and unit % 16):
        raise ValueError("units of several must be multiples of 16 bytes, at most 2**20 blocks each")
    lib = _native.cpu_lib()
    ctx = _native.AesXtsContext()
    rc = (lib.aes_xts_setkey_dec if decrypt else lib.aes_xts_setkey_enc)(ctypes.byref(ctx), _native.as_u8p(key),
                                                                       len(key) * 8)
    if rc:
        raise ValueError("invalid XTS key length")
    out = _buf(len(data))
    rc = lib.aes_crypt_xts_units(ctypes.byref(ctx), AES_DECRYPT if decrypt else AES_ENCRYPT, unit, nunits,
                                 _native.as_u8p(xts_tweak(tweak0)), _native.as_u8p(data), out)
    if rc:
        raise ValueError("invalid XTS length")
    return bytes(out)[: len(data)]


GCM_MAX_BYTES = (1 << 36) - 32


class GcmTagError(ValueError):
    """The tag of an AES-GCM message did not match; the plaintext was zeroed."""


def _gcm_ctx(key: bytes) -> _native.AesGcmContext:
    ctx = _native.AesGcmContext()
    key = bytes(key)
    if _native.cpu_lib().aes_gcm_setkey(ctypes.byref(ctx), _native.as_u8p(key), len(key) * 8):
        raise ValueError("invalid AES key length")
    return ctx


def _b16(v, name: str) -> bytes:
    v = bytes(v)
    if len(v) != 16:
        raise ValueError(f"{name} must be 16 bytes")
    return v


def gf128_mul(x: bytes, y: bytes) -> bytes:
    """x . y in GF(2^128) in GCM's bit order (the leftmost bit is x^0)."""
    z = _buf(16)
    _native.cpu_lib().aes_gf128_mul(z, _native.as_u8p(_b16(x, "x")), _native.as_u8p(_b16(y, "y")))
    return bytes(z)


def ghash(h: bytes, data: bytes, y0: bytes = bytes(16)) -> bytes:
    """GHASH under ``h`` continued from ``y0`` over ``data``; the last partial
    block is zero-padded (SP 800-38D)."""
    ctx = _native.AesGcmContext()
    lib = _native.cpu_lib()
    lib.aes_gcm_set_h(ctypes.byref(ctx), _native.as_u8p(_b16(h, "h")))
    y = (ctypes.c_uint8 * 16).from_buffer_copy(_b16(y0, "y0"))
    data = bytes(data)
    lib.aes_ghash(ctypes.byref(ctx), y, _native.as_u8p(data), len(data))
    return bytes(y)


def gcm_h(key: bytes) -> bytes:
    """The hash subkey H = E_K(0^128)."""
    return bytes(_gcm_ctx(key).h)


def ctr32(key: bytes, ctr: bytes, data: bytes) -> bytes:
    """GCM's counter mode: only bytes 12..15 of ``ctr`` increment (big-endian),
    wrapping at 2**32 without carry into byte 11."""
    ctx = _gcm_ctx(key)
    c = (ctypes.c_uint8 * 16).from_buffer_copy(_b16(ctr, "ctr"))
    data = bytes(data)
    out = _buf(len(data))
    _native.cpu_lib().aes_crypt_ctr32(ctypes.byref(ctx), len(data), c, _native.as_u8p(data), out)
    return bytes(out)[: len(data)]


def gcm(key: bytes, iv: bytes, data: bytes, aad: bytes = b"", decrypt: bool = False):
    """AES-GCM (SP 800-38D) of one message: ``(out, tag)`` with the COMPUTED
    16-byte tag in both directions.  Any IV length from 1 byte."""
    ctx = _gcm_ctx(key)
    iv, data, aad = bytes(iv), bytes(data), bytes(aad)
    if not iv:
        raise ValueError("the GCM IV must have at least 1 byte")
    if len(data) > GCM_MAX_BYTES:
        raise ValueError("a GCM message has at most 2**36 - 32 bytes")
    out, tag = _buf(len(data)), _buf(16)
    rc = _native.cpu_lib().aes_crypt_gcm(ctypes.byref(ctx), AES_DECRYPT if decrypt else AES_ENCRYPT, len(data),
                                         _native.as_u8p(iv), len(iv), _native.as_u8p(aad), len(aad),
                                         _native.as_u8p(data), out, tag)
    if rc:
        raise ValueError("invalid GCM lengths")
    return bytes(out)[: len(data)], bytes(tag)


def gcm_mk_batch(keys, key_index, ivs, datas, aads=None, decrypt: bool = False):
    """The oracle of the batched AES-GCM with a key per record: a loop over
    ``gcm``.  Record ``m`` is SP 800-38D GCM under ``(keys[key_index[m]],
    ivs[m], aads[m])`` (``key_index`` None: key m for record m): a list of
    ``(out, tag)`` with the COMPUTED 16-byte tags in both directions."""
    keys, ivs, datas = [bytes(k) for k in keys], [bytes(v) for v in ivs], [bytes(d) for d in datas]
    aads = [b""] * len(datas) if aads is None else [bytes(a) for a in aads]
    kidx = list(range(len(datas))) if key_index is None else [int(k) for k in key_index]
    if len(ivs) != len(datas) or len(aads) != len(datas) or len(kidx) != len(datas):
        raise ValueError("one key index, one IV and one AAD per record")
    if any(k < 0 or k >= len(keys) for k in kidx):
        raise ValueError("key_index out of range")
    return [gcm(keys[k], v, d, a, decrypt=decrypt) for k, v, d, a in zip(kidx, ivs, datas, aads)]


def gcm_auth_decrypt(key: bytes, iv: bytes, data: bytes, tag: bytes, aad: bytes = b"") -> bytes:
    """Authenticated decryption: compares 4..16 tag bytes in constant time and
    raises GcmTagError (the C side zeroes its output) on a mismatch."""
    ctx = _gcm_ctx(key)
    iv, data, aad, tag = bytes(iv), bytes(data), bytes(aad), bytes(tag)
    if not iv or not 4 <= len(tag) <= 16:
        raise ValueError("GCM needs an IV of at least 1 byte and a tag of 4 to 16 bytes")
    # not zero to begin with: err.output shows what the C side left on a mismatch
    out = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(b"\xa5" * max(len(data), 1))
    rc = _native.cpu_lib().aes_gcm_auth_decrypt(ctypes.byref(ctx), len(data), _native.as_u8p(iv), len(iv),
                                                _native.as_u8p(aad), len(aad), _native.as_u8p(tag), len(tag),
                                                _native.as_u8p(data), out)
    if rc == -0x12:
        err = GcmTagError("GCM tag mismatch")
        err.output = bytes(out)[: len(data)]
        raise err
    if rc:
        raise ValueError("invalid GCM lengths")
    return bytes(out)[: len(data)]


GCM_SIV_MAX_BYTES = 1 << 36  # RFC 8452: plaintext and AAD each (aes.h AES_GCM_SIV_MAX_BYTES)


class GcmSivTagError(ValueError):
    """The tag of an AES-GCM-SIV message did not match; the plaintext was zeroed."""


def polyval_dot(x: bytes, y: bytes) -> bytes:
    """dot(x, y) = x . y . x^-128 in POLYVAL's field and little-endian bit order (RFC 8452 section 3)."""
    z = _buf(16)
    _native.cpu_lib().aes_polyval_dot(z, _native.as_u8p(_b16(x, "x")), _native.as_u8p(_b16(y, "y")))
    return bytes(z)


def polyval(h: bytes, data: bytes, y0: bytes = bytes(16)) -> bytes:
    """POLYVAL under ``h`` continued from ``y0`` over ``data``; the last partial
    block is zero-padded."""
    y = (ctypes.c_uint8 * 16).from_buffer_copy(_b16(y0, "y0"))
    data = bytes(data)
    _native.cpu_lib().aes_polyval(_native.as_u8p(_b16(h, "h")), y, _native.as_u8p(data), len(data))
    return bytes(y)


def gcm_siv_check(key: bytes, nonce: bytes, nbytes: int = 0, aad_bytes: int = 0):
    """What every GCM-SIV call checks of its key (16 or 32 bytes), its nonce
    (exactly 12 bytes) and its lengths: ValueError, as the device ops raise."""
    if len(key) not in (16, 32):
        raise ValueError(f"an AES-GCM-SIV key has 16 or 32 bytes, got {len(key)}")
    if len(nonce) != 12:
        raise ValueError("an AES-GCM-SIV nonce has exactly 12 bytes")
    if nbytes > GCM_SIV_MAX_BYTES or aad_bytes > GCM_SIV_MAX_BYTES:
        raise ValueError("an AES-GCM-SIV message and its AAD have at most 2**36 bytes each")


def gcm_siv_derive(key: bytes, nonce: bytes):
    """RFC 8452 section 4: ``(authentication key, encryption key)`` of ``nonce`` under the key-generating ``key``."""
    key, nonce = bytes(key), bytes(nonce)
    gcm_siv_check(key, nonce)
    ak, ek = _buf(16), _buf(32)
    n = _native.cpu_lib().aes_gcmsiv_derive(ctypes.byref(_ctx(key)), _native.as_u8p(nonce), ak, ek)
    return bytes(ak), bytes(ek)[:n]


def ctr_le32(key: bytes, ctr: bytes, data: bytes) -> bytes:
    """GCM-SIV's counter mode: only bytes 0..3 of ``ctr`` increment
    (little-endian), wrapping at 2**32 without carry into byte 4.  ``ctr`` is
    used as given: GCM-SIV passes the tag with bit 7 of byte 15 set."""
    ctx = _ctx(key)
    c = (ctypes.c_uint8 * 16).from_buffer_copy(_b16(ctr, "ctr"))
    data = bytes(data)
    out = _buf(len(data))
    _native.cpu_lib().aes_crypt_ctr_le32(ctypes.byref(ctx), len(data), c, _native.as_u8p(data), out)
    return bytes(out)[: len(data)]


def gcm_siv(key: bytes, nonce: bytes, data: bytes, aad: bytes = b"", decrypt: bool = False, tag: bytes | None = None):
    """AES-GCM-SIV (RFC 8452) of one message: ``(out, tag)`` with the COMPUTED
    16-byte tag in both directions.  A decryption runs its counter mode from
    ``tag``, the received one."""
    key, nonce, data, aad = bytes(key), bytes(nonce), bytes(data), bytes(aad)
    gcm_siv_check(key, nonce, len(data), len(aad))
    tag_in = _b16(tag, "tag") if decrypt else bytes(16)
    out, t = _buf(len(data)), _buf(16)
    rc = _native.cpu_lib().aes_crypt_gcmsiv(ctypes.byref(_ctx(key)), AES_DECRYPT if decrypt else AES_ENCRYPT, len(data),
                                            _native.as_u8p(nonce), _native.as_u8p(aad), len(aad), _native.as_u8p(data),
                                            out, _native.as_u8p(tag_in), t)
    if rc:
        raise ValueError("invalid GCM-SIV lengths")
    return bytes(out)[: len(data)], bytes(t)


def gcm_siv_batch(key: bytes, nonces, datas, aads=None, decrypt: bool = False, tags=None):
    """The batched AES-GCM-SIV oracle: a loop over ``gcm_siv``.  Record ``m`` is
    RFC 8452 under ``(key, nonces[m], aads[m])``: a list of ``(out, tag)`` with
    the COMPUTED tags in both directions (a decryption starts its counter mode
    from ``tags[m]``, the received one)."""
    nonces, datas = [bytes(n) for n in nonces], [bytes(d) for d in datas]
    aads = [b""] * len(datas) if aads is None else [bytes(a) for a in aads]
    tags = [None] * len(datas) if tags is None else list(tags)
    if len(nonces) != len(datas) or len(aads) != len(datas) or len(tags) != len(datas):
        raise ValueError("one nonce, one AAD and one tag per record")
    return [gcm_siv(key, n, d, a, decrypt=decrypt, tag=t) for n, d, a, t in zip(nonces, datas, aads, tags)]


def gcm_siv_auth_decrypt(key: bytes, nonce: bytes, data: bytes, tag: bytes, aad: bytes = b"") -> bytes:
    """Authenticated decryption: compares the 16-byte tag in constant time and
    raises GcmSivTagError (the C side zeroes its output) on a mismatch."""
    key, nonce, data, aad, tag = bytes(key), bytes(nonce), bytes(data), bytes(aad), bytes(tag)
    gcm_siv_check(key, nonce, len(data), len(aad))
    if len(tag) != 16:
        raise ValueError("an AES-GCM-SIV tag has 16 bytes")
    # not zero to begin with: err.output shows what the C side left on a mismatch
    out = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(b"\xa5" * max(len(data), 1))
    rc = _native.cpu_lib().aes_gcmsiv_auth_decrypt(ctypes.byref(_ctx(key)), len(data), _native.as_u8p(nonce),
                                                   _native.as_u8p(aad), len(aad), _native.as_u8p(tag),
                                                   _native.as_u8p(data), out)
    if rc == -0x12:
        err = GcmSivTagError("GCM-SIV tag mismatch")
        err.output = bytes(out)[: len(data)]
        raise err
    if rc:
        raise ValueError("invalid GCM-SIV lengths")
    return bytes(out)[: len(data)]


OCB_MAX_BYTES = 1 << 36  # RFC 7253 as this engine cuts it: block indices reach 2**32 (aes.h AES_OCB_MAX_BYTES)
OCB_MAX_BLOCKS = 1 << 32


class OcbTagError(ValueError):
    """The tag of an AES-OCB3 message did not match; the plaintext was zeroed."""


def _ocb_ctx(key: bytes) -> _native.AesOcbContext:
    ctx = _native.AesOcbContext()
    key = bytes(key)
    if _native.cpu_lib().aes_ocb_setkey(ctypes.byref(ctx), _native.as_u8p(key), len(key) * 8):
        raise ValueError("invalid AES key length")
    return ctx


def ocb_check(nonce: bytes, tag_bytes: int, nbytes: int = 0):
    """What every OCB3 call checks of its nonce (1..15 bytes), its tag length
    (1..16 bytes) and its message length: ValueError, as the device ops raise."""
    if not 1 <= len(nonce) <= 15:
        raise ValueError("an OCB nonce has 1 to 15 bytes")
    if not isinstance(tag_bytes, int) or not 1 <= tag_bytes <= 16:
        raise ValueError("an OCB tag has 1 to 16 bytes")
    if nbytes > OCB_MAX_BYTES:
        raise ValueError("an OCB message has at most 2**36 bytes")


def ocb_check_blocks(first_block: int, nblocks: int):
    if first_block < 0 or nblocks < 0 or first_block + nblocks > OCB_MAX_BLOCKS:
        raise ValueError("OCB block indices reach at most 2**32")


def ocb_l(key: bytes) -> dict:
    """The key's constants: ``{"star": L_*, "dollar": L_$, "l": [L_0 .. L_32]}``."""
    ctx = _ocb_ctx(key)
    return {"star": bytes(ctx.l_star), "dollar": bytes(ctx.l_dollar), "l": [bytes(v) for v in ctx.l]}


def ocb_offset0(key: bytes, nonce: bytes, tag_bytes: int = 16) -> bytes:
    """Offset_0 of (nonce, tag length): RFC 7253's nonce block, Ktop, Stretch."""
    nonce = bytes(nonce)
    ocb_check(nonce, tag_bytes)
    out = _buf(16)
    _native.cpu_lib().aes_ocb_offset0(ctypes.byref(_ocb_ctx(key)), _native.as_u8p(nonce), len(nonce), tag_bytes, out)
    return bytes(out)


def ocb_offset(key: bytes, offset0: bytes, i: int) -> bytes:
    """Offset_i by the closed form Offset_0 ^ XOR{L_j : bit j of i ^ (i >> 1)}, 0 <= i <= 2**32."""
    ocb_check_blocks(i, 0)
    out = _buf(16)
    _native.cpu_lib().aes_ocb_offset(ctypes.byref(_ocb_ctx(key)), _native.as_u8p(_b16(offset0, "offset0")), i, out)
    return bytes(out)


def ocb_hash(key: bytes, aad: bytes) -> bytes:
    """HASH(K, A) of RFC 7253; an empty A hashes to zero."""
    aad, out = bytes(aad), _buf(16)
    _native.cpu_lib().aes_ocb_hash(ctypes.byref(_ocb_ctx(key)), _native.as_u8p(aad), len(aad), out)
    return bytes(out)


def ocb_blocks(key: bytes, offset0: bytes, data: bytes, first_block: int = 0, checksum: bytes = bytes(16),
               decrypt: bool = False):
    """The whole blocks ``first_block + 1 ..`` of a message: ``(out, checksum)``,
    the checksum continued from the one given."""
    data = bytes(data)
    if len(data) % 16:
        raise ValueError("OCB blocks are 16 bytes")
    ocb_check_blocks(first_block, len(data) // 16)
    out = _buf(len(data))
    cs = (ctypes.c_uint8 * 16).from_buffer_copy(_b16(checksum, "checksum"))
    rc = _native.cpu_lib().aes_crypt_ocb_blocks(ctypes.byref(_ocb_ctx(key)), AES_DECRYPT if decrypt else AES_ENCRYPT,
                                                _native.as_u8p(_b16(offset0, "offset0")), first_block, len(data) // 16,
                                                _native.as_u8p(data), out, cs)
    if rc:
        raise ValueError("invalid OCB block range")
    return bytes(out)[: len(data)], bytes(cs)


def ocb(key: bytes, nonce: bytes, data: bytes, aad: bytes = b"", decrypt: bool = False, tag_bytes: int = 16):
    """AES-OCB3 (RFC 7253) of one message: ``(out, tag)`` with the COMPUTED
    ``tag_bytes``-long tag in both directions."""
    ctx = _ocb_ctx(key)
    nonce, data, aad = bytes(nonce), bytes(data), bytes(aad)
    ocb_check(nonce, tag_bytes, len(data))
    out, tag = _buf(len(data)), _buf(16)
    rc = _native.cpu_lib().aes_crypt_ocb(ctypes.byref(ctx), AES_DECRYPT if decrypt else AES_ENCRYPT, len(data),
                                         _native.as_u8p(nonce), len(nonce), _native.as_u8p(aad), len(aad),
                                         _native.as_u8p(data), out, tag, tag_bytes)
    if rc:
        raise ValueError("invalid OCB lengths")
    return bytes(out)[: len(data)], bytes(tag)[:tag_bytes]


def ocb_auth_decrypt(key: bytes, nonce: bytes, data: bytes, tag: bytes, aad: bytes = b"") -> bytes:
    """Authenticated decryption: TAGLEN is ``len(tag)``; compares in constant
    time and raises OcbTagError (the C side zeroes its output) on a mismatch."""
    ctx = _ocb_ctx(key)
    nonce, data, aad, tag = bytes(nonce), bytes(data), bytes(aad), bytes(tag)
    ocb_check(nonce, len(tag), len(data))
    # not zero to begin with: err.output shows what the C side left on a mismatch
    out = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(b"\xa5" * max(len(data), 1))
    rc = _native.cpu_lib().aes_ocb_auth_decrypt(ctypes.byref(ctx), len(data), _native.as_u8p(nonce), len(nonce),
                                                _native.as_u8p(aad), len(aad), _native.as_u8p(tag), len(tag),
                                                _native.as_u8p(data), out)
    if rc == -0x14:
        err = OcbTagError("OCB tag mismatch")
        err.output = bytes(out)[: len(data)]
        raise err
    if rc:
        raise ValueError("invalid OCB lengths")
    return bytes(out)[: len(data)]


def ocb_batch(key: bytes, nonces, datas, aads=None, decrypt: bool = False):
    """The batched AES-OCB3 oracle: a loop over ``ocb``.  Record ``m`` is OCB3
    under ``(key, nonces[m], aads[m])`` with a 12-byte nonce and a 16-byte
    tag: a list of ``(out, tag)`` with the COMPUTED tags in both directions."""
    nonces, datas = [bytes(n) for n in nonces], [bytes(d) for d in datas]
    aads = [b""] * len(datas) if aads is None else [bytes(a) for a in aads]
    if len(nonces) != len(datas) or len(aads) != len(datas):
        raise ValueError("one nonce and one AAD per record")
    if any(len(n) != 12 for n in nonces):
        raise ValueError("a batched OCB nonce has 12 bytes")
    return [ocb(key, n, d, a, decrypt=decrypt) for n, d, a in zip(nonces, datas, aads)]


CCM_NONCE_BYTES = tuple(range(7, 14))  # L = 15 - len(nonce): 8 .. 2 bytes of length field
CCM_TAG_BYTES = (4, 6, 8, 10, 12, 14, 16)


class CcmTagError(ValueError):
    """The tag of an AES-CCM message did not match; the plaintext was zeroed."""


def ccm_check(nonce_bytes: int, tag_bytes: int, nbytes: int = 0):
    """What every CCM call checks of its nonce length (7..13 bytes), its tag
    length (4, 6, .., 16 bytes) and its message length (below 2**(8 L) with
    L = 15 - nonce length): ValueError, as the device ops raise."""
    if not isinstance(nonce_bytes, int) or nonce_bytes not in CCM_NONCE_BYTES:
        raise ValueError("a CCM nonce has 7 to 13 bytes")
    if not isinstance(tag_bytes, int) or tag_bytes not in CCM_TAG_BYTES:
        raise ValueError("a CCM tag has 4, 6, 8, 10, 12, 14 or 16 bytes")
    if nbytes >> (8 * (15 - nonce_bytes)):
        raise ValueError(f"a CCM message under a {nonce_bytes}-byte nonce has fewer than "
                         f"2**{8 * (15 - nonce_bytes)} bytes")


def ccm(key: bytes, nonce: bytes, data: bytes, aad: bytes = b"", decrypt: bool = False, tag_bytes: int = 16):
    """AES-CCM (SP 800-38C, RFC 3610) of one message: ``(out, tag)`` with the
    COMPUTED ``tag_bytes``-long tag in both directions."""
    ctx = _ctx(key)
    nonce, data, aad = bytes(nonce), bytes(data), bytes(aad)
    ccm_check(len(nonce), tag_bytes, len(data))
    out, tag = _buf(len(data)), _buf(16)
    rc = _native.cpu_lib().aes_crypt_ccm(ctypes.byref(ctx), AES_DECRYPT if decrypt else AES_ENCRYPT, len(data),
                                         _native.as_u8p(nonce), len(nonce), _native.as_u8p(aad), len(aad),
                                         _native.as_u8p(data), out, tag, tag_bytes)
    if rc:
        raise ValueError("invalid CCM lengths")
    return bytes(out)[: len(data)], bytes(tag)[:tag_bytes]


def ccm_auth_decrypt(key: bytes, nonce: bytes, data: bytes, tag: bytes, aad: bytes = b"") -> bytes:
    """Authenticated decryption: the tag length is ``len(tag)``; compares in
    constant time and raises CcmTagError (the C side zeroes its output) on a
    mismatch."""
    ctx = _ctx(key)
    nonce, data, aad, tag = bytes(nonce), bytes(data), bytes(aad), bytes(tag)
    ccm_check(len(nonce), len(tag), len(data))
    # not zero to begin with: err.output shows what the C side left on a mismatch
    out = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(b"\xa5" * max(len(data), 1))
    rc = _native.cpu_lib().aes_ccm_auth_decrypt(ctypes.byref(ctx), len(data), _native.as_u8p(nonce), len(nonce),
                                                _native.as_u8p(aad), len(aad), _native.as_u8p(tag), len(tag),
                                                _native.as_u8p(data), out)
    if rc == -0x16:
        err = CcmTagError("CCM tag mismatch")
        err.output = bytes(out)[: len(data)]
        raise err
    if rc:
        raise ValueError("invalid CCM lengths")
    return bytes(out)[: len(data)]


def ccm_batch(key: bytes, nonces, datas, aads=None, decrypt: bool = False, tag_bytes: int = 16):
    """The batched AES-CCM oracle: a loop over ``ccm``.  Record ``m`` is CCM
    under ``(key, nonces[m], aads[m])``; one nonce length and one tag length
    for the batch: a list of ``(out, tag)`` with the COMPUTED tags in both
    directions."""
    nonces, datas = [bytes(n) for n in nonces], [bytes(d) for d in datas]
    aads = [b""] * len(datas) if aads is None else [bytes(a) for a in aads]
    if len(nonces) != len(datas) or len(aads) != len(datas):
        raise ValueError("one nonce and one AAD per record")
    if len({len(n) for n in nonces}) > 1:
        raise ValueError("a CCM batch has one nonce length")
    return [ccm(key, n, d, a, decrypt=decrypt, tag_bytes=tag_bytes) for n, d, a in zip(nonces, datas, aads)]


CHACHA_MAX_BYTES = ((1 << 32) - 1) * 64  # chacha.h CHACHA20_POLY1305_MAX_BYTES


class ChaChaTagError(ValueError):
    """The tag of a ChaCha20-Poly1305 message did not match; the plaintext was zeroed."""


def _chacha_args(key, nonce):
    key, nonce = bytes(key), bytes(nonce)
    if len(key) != 32:
        raise ValueError("a ChaCha20 key has 32 bytes")
    if len(nonce) != 12:
        raise ValueError("a ChaCha20 nonce has 12 bytes (RFC 8439)")
    return key, nonce


def chacha_check_counter(counter: int, nbytes: int) -> int:
    """The 32-bit block counter of a call over ``nbytes``: RFC 8439 leaves its
    overflow undefined, and this engine refuses a call whose last block would
    pass 2**32 - 1 (the last block may be exactly that)."""
    counter = int(counter)
    if not 0 <= counter < 1 << 32:
        raise ValueError("the ChaCha20 block counter is 0 .. 2**32 - 1")
    if counter + (nbytes + 63) // 64 > 1 << 32:
        raise ValueError("the ChaCha20 block counter would pass 2**32 - 1 (the 32-bit counter never wraps here)")
    return counter


def chacha20(key: bytes, nonce: bytes, data: bytes, counter: int = 0) -> bytes:
    """ChaCha20 (RFC 8439: 32-byte key, 12-byte nonce, 32-bit block counter)
    over any byte count, from block ``counter``."""
    key, nonce = _chacha_args(key, nonce)
    data = bytes(data)
    counter = chacha_check_counter(counter, len(data))
    out = _buf(len(data))
    if _native.cpu_lib().chacha20_crypt(_native.as_u8p(key), _native.as_u8p(nonce), counter, _native.as_u8p(data), out,
                                        len(data)):
        raise ValueError("the ChaCha20 block counter would pass 2**32 - 1")
    return bytes(out)[: len(data)]


def poly1305(key: bytes, data: bytes) -> bytes:
    """The 16-byte Poly1305 tag of ``data`` under the 32-byte one-time key r || s."""
    key, data = bytes(key), bytes(data)
    if len(key) != 32:
        raise ValueError("a Poly1305 key has 32 bytes")
    tag = _buf(16)
    _native.cpu_lib().poly1305_mac(_native.as_u8p(key), _native.as_u8p(data), len(data), tag)
    return bytes(tag)


def chacha20_poly1305(key: bytes, nonce: bytes, data: bytes, aad: bytes = b"", decrypt: bool = False):
    """ChaCha20-Poly1305 (RFC 8439 section 2.8) of one message: ``(out, tag)``
    with the COMPUTED 16-byte tag in both directions."""
    key, nonce = _chacha_args(key, nonce)
    data, aad = bytes(data), bytes(aad)
    if len(data) > CHACHA_MAX_BYTES:
        raise ValueError("a ChaCha20-Poly1305 message has at most (2**32 - 1) * 64 bytes")
    lib = _native.cpu_lib()
    out, tag = _buf(len(data)), _buf(16)
    k, n, a, d = _native.as_u8p(key), _native.as_u8p(nonce), _native.as_u8p(aad), _native.as_u8p(data)
    if decrypt:
        rc = lib.chacha20_poly1305_tag(k, n, a, len(aad), d, len(data), tag) or lib.chacha20_crypt(k, n, 1, d, out, len(data))
    else:
        rc = lib.chacha20_poly1305_encrypt(k, n, a, len(aad), d, out, len(data), tag)
    if rc:
        raise ValueError("invalid ChaCha20-Poly1305 lengths")
    return bytes(out)[: len(data)], bytes(tag)


def chacha20_poly1305_auth_decrypt(key: bytes, nonce: bytes, data: bytes, tag: bytes, aad: bytes = b"") -> bytes:
    """Authenticated decryption: compares the 16-byte tag in constant time and
    raises ChaChaTagError (the C side zeroes its output) on a mismatch."""
    key, nonce = _chacha_args(key, nonce)
    data, aad, tag = bytes(data), bytes(aad), bytes(tag)
    if len(tag) != 16:
        raise ValueError("a ChaCha20-Poly1305 tag has 16 bytes")
    # not zero to begin with: err.output shows what the C side left on a mismatch
    out = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(b"\xa5" * max(len(data), 1))
    rc = _native.cpu_lib().chacha20_poly1305_auth_decrypt(_native.as_u8p(key), _native.as_u8p(nonce), _native.as_u8p(aad),
                                                         len(aad), _native.as_u8p(tag), _native.as_u8p(data), out,
                                                         len(data))
    if rc == -0x12:
        err = ChaChaTagError("ChaCha20-Poly1305 tag mismatch")
        err.output = bytes(out)[: len(data)]
        raise err
    if rc:
        raise ValueError("invalid ChaCha20-Poly1305 lengths")
    return bytes(out)[: len(data)]


def serial_encrypt(mode: str, key: bytes, iv: bytes, data: bytes) -> bytes:
    """Exact single-stream CBC / CFB128 encryption on one core with AES-NI
    (the C oracle where AES-NI is absent).  This is the host path for the
    serial chain: a GPU runs it on one lane, far slower than one x86 core."""
    if mode not in ("cbc", "cfb128"):
        raise ValueError("mode must be 'cbc' or 'cfb128'")
    if mode == "cbc" and len(data) % 16:
        raise ValueError("CBC needs a multiple of 16 bytes")
    if not aesni_supported():
        return cbc(key, iv, data) if mode == "cbc" else cfb128(key, iv, data)
    sched, nr = aesni_schedule(key)
    ivb = (ctypes.c_uint8 * 16).from_buffer_copy(bytes(iv))
    out = _buf(len(data))
    fn = _native.cpu_lib().AES_CBC_encrypt if mode == "cbc" else _native.cpu_lib().AES_CFB128_encrypt
    fn(_native.as_u8p(bytes(data)), out, ivb, len(data), _native.as_u8p(sched), nr)
    return bytes(out)[: len(data)]


def arc4_keystream(key: bytes, n: int, drop: int = 0) -> bytes:
    lib = _native.cpu_lib()
    ctx = _native.Arc4Context()
    lib.arc4_setup(ctypes.byref(ctx), _native.as_u8p(bytes(key)), len(key))
    if drop:
        lib.arc4_prep(ctypes.byref(ctx), drop, _buf(drop))
    ks = _buf(n)
    lib.arc4_prep(ctypes.byref(ctx), n, ks)
    return bytes(ks)[:n]


def arc4_crypt(data: bytes, keystream: bytes, threads: int = 1) -> bytes:
    out = _buf(len(data))
    _native.cpu_lib().arc4_crypt_mt(len(data), _native.as_u8p(bytes(data)), _native.as_u8p(bytes(keystream)), out,
                                    threads)
    return bytes(out)[: len(data)]


def rc4_oneshot(key: bytes, data: bytes) -> bytes:
    """rc4.h API (rc4_init + rc4_crypt)."""
    lib = _native.cpu_lib()
    st = _native.Rc4State()
    lib.rc4_init(ctypes.byref(st), bytes(key), len(key))
    out = ctypes.create_string_buffer(max(len(data), 1))
    lib.rc4_crypt(ctypes.byref(st), bytes(data), out, len(data))
    return out.raw[: len(data)]


def aesni_supported() -> bool:
    return bool(_native.cpu_lib().CheckAESSupport())


def aesni_ctr(key: bytes, nonce: bytes, ivec: bytes, data: bytes, block_offset: int = 0) -> bytes:
    lib = _native.cpu_lib()
    nr = {16: 10, 24: 12, 32: 14}[len(key)]
    sched = (ctypes.c_uint8 * 240)()
    {10: lib.AES_128_Key_Expansion, 12: lib.AES_192_Key_Expansion, 14: lib.AES_256_Key_Expansion}[nr](
        _native.as_u8p(bytes(key)), sched)
    out = _buf(len(data))
    lib.AES_CTR_encrypt_at(_native.as_u8p(bytes(data)), out, _native.as_u8p(bytes(ivec)), _native.as_u8p(bytes(nonce)),
                           len(data), sched, nr, block_offset)
    return bytes(out)[: len(data)]


def aesni_schedule(key: bytes, decrypt: bool = False):
    """(schedule bytes, Nr) as AES_*_Key_Expansion / AES_Key_Expansion_Dec
    produce them (16*(Nr+1) bytes)."""
    lib = _native.cpu_lib()
    nr = {16: 10, 24: 12, 32: 14}[len(key)]
    sched = (ctypes.c_uint8 * 240)()
    {10: lib.AES_128_Key_Expansion, 12: lib.AES_192_Key_Expansion, 14: lib.AES_256_Key_Expansion}[nr](
        _native.as_u8p(bytes(key)), sched)
    if decrypt:
        dsched = (ctypes.c_uint8 * 240)()
        lib.AES_Key_Expansion_Dec(sched, dsched, nr)
        sched = dsched
    return bytes(sched)[: 16 * (nr + 1)], nr


def aesni_ecb(key: bytes, data: bytes, decrypt: bool = False) -> bytes:
    lib = _native.cpu_lib()
    nr = {16: 10, 24: 12, 32: 14}[len(key)]
    sched = (ctypes.c_uint8 * 240)()
    {10: lib.AES_128_Key_Expansion, 12: lib.AES_192_Key_Expansion, 14: lib.AES_256_Key_Expansion}[nr](
        _native.as_u8p(bytes(key)), sched)
    out = _buf(len(data))
    if decrypt:
        dsched = (ctypes.c_uint8 * 240)()
        lib.AES_Key_Expansion_Dec(sched, dsched, nr)
        lib.AES_ECB_decrypt(_native.as_u8p(bytes(data)), out, len(data), dsched, nr)
    else:
        lib.AES_ECB_encrypt(_native.as_u8p(bytes(data)), out, len(data), sched, nr)
    return bytes(out)[: len(data)]


def self_tests(verbose: int = 0) -> dict:
    lib = _native.cpu_lib()
    return {
        "aes": lib.aes_self_test(verbose),
        "arc4": lib.arc4_self_test(verbose),
        "bitslice": lib.otc_bitslice_selftest(verbose),
    }
