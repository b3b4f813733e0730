"""Device AES ops on torch tensors (ROCm ``cuda`` tensors), backed by the
hand-written gfx950 kernels in ``csrc/hip/aes_tt.hip`` (LDS T-table) and
``csrc/hip/aes_bs.hip`` (bitsliced VALU).

Every op runs asynchronously on torch's current HIP stream and raises on any
native error.  Tensors may have any dtype; they are treated as contiguous byte
buffers.  Reference kernels: /root/reference/aes-gpu/Source/AES.cu:284-502
(ECB only, broken launch); everything else here is new capability.
"""
from __future__ import annotations

import ctypes
import functools
import hmac

import torch

from .. import _native
from ..models.cpu_ref import GcmTagError
from .keys import DECRYPT, ENCRYPT, expand_key

IMPLS = {"auto": 0, "ttable": 1, "bitslice": 2, "split": 3}  # otc.h OTC_IMPL_*


def _impl(impl) -> int:
    if isinstance(impl, int):
        return impl
    try:
        return IMPLS[impl]
    except KeyError:
        raise ValueError(f"impl must be one of {list(IMPLS)}") from None


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


def _check_dev(t: torch.Tensor, name: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a GPU tensor (got {t.device})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _out_like(x: torch.Tensor, out):
    if out is None:
        return torch.empty_like(x)
    _check_dev(out, "out")
    if _nbytes(out) != _nbytes(x):
        raise ValueError("out must have the same byte size as the input")
    return out


def _bytes(t: torch.Tensor) -> torch.Tensor:
    """Flat uint8 view of a contiguous tensor."""
    return t.reshape(-1).view(torch.uint8)


def _run(x: torch.Tensor, out: torch.Tensor, call, inplace_ok: bool = True):
    """call(in_ptr, out_ptr) -> rc.  The kernels move 16 bytes per lane, so the
    native API requires 16-byte aligned buffers; a misaligned tensor (e.g. a
    byte slice ``t[3:]``) is staged through an aligned temporary (torch's
    allocator aligns every fresh allocation) and copied back.  Modes whose
    parallel kernel reads ciphertext block i-1 while block i-1's output is
    written (CBC / CFB decryption, ``inplace_ok=False``) run in place through
    a copy of the input."""
    xp, op = x.data_ptr(), out.data_ptr()
    if not inplace_ok and xp == op and _nbytes(x) > 16:
        x = _bytes(x).clone()
        xp = x.data_ptr()
    if not (xp % 16 or op % 16) or _nbytes(x) == 0:
        return call(xp, op)
    xi = _bytes(x).clone() if xp % 16 else _bytes(x)
    if op == xp:
        xo = xi  # in place stays in place (the native API rejects modes that forbid it)
    elif op % 16:
        xo = torch.empty_like(xi)
    else:
        xo = _bytes(out)
    rc = call(xi.data_ptr(), xo.data_ptr())
    if rc == 0 and xo.data_ptr() != op:
        _bytes(out).copy_(xo)
    return rc


def _b16(v, name) -> ctypes.Array:
    v = bytes(v)
    if len(v) != 16:
        raise ValueError(f"{name} must be 16 bytes")
    return (ctypes.c_uint8 * 16).from_buffer_copy(v)


def _lib():
    return _native.require_gpu_lib()


def ctr(x: torch.Tensor, key: bytes, counter: bytes, out: torch.Tensor | None = None, block_offset: int = 0,
        impl="auto") -> torch.Tensor:
    """AES-CTR (128-bit big-endian counter starting at ``counter`` + ``block_offset``)."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = expand_key(key)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_ctr(ip, op, _nbytes(x), ctypes.byref(k), _b16(counter, "counter"),
            int(block_offset), _impl(impl), _stream(x)))
    _native.check(rc, "otc_aes_ctr")
    return out


BATCH_TILES = (256, 128, 64)  # tile sizes in blocks the batch kernel supports (otc.h)
BATCH_ALIGNED = 0x80000000  # otc.h OTC_BATCH_ALIGNED
BATCH_ALIGN_MIN_TILES = 6  # counter-aligned tiling pays once (n+1) x 133 < n x 160 lookups
# relative cost per tile block slot, measured on MI355X with 16384 x 4 KiB
# messages (960 / 946 / 910 GB/s at 256 / 128 / 64 blocks per tile,
# profiles/r1/batch_ctr_tiles.jsonl): fewer blocks per lane hide less LDS latency
BATCH_TILE_COST = {256: 1.0, 128: 1.015, 64: 1.055}


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


def _pick_tile(nbytes) -> int:
    """Tile size minimising (tile slots issued) x (cost per slot)."""
    best, best_cost = 256, None
    for t in BATCH_TILES:
        slots = int(((nbytes + 16 * t - 1) // (16 * t)).sum()) * t
        cost = slots * BATCH_TILE_COST[t]
        if best_cost is None or cost < best_cost:
            best, best_cost = t, cost
    return best


class CtrBatch:
    """A planned batch of independent AES-CTR messages -- own buffers, key and
    counter each -- executed by ONE kernel launch per key size
    (``otc_aes_ctr_batch``).

    The serving shape: thousands of packets / sectors / objects of a few KiB.
    One ``ctr()`` launch per message is launch-bound (microseconds of host and
    dispatch work per message) and puts a few workgroups on a 256-CU chip; the
    batch kernel instead deals 4 KiB tiles of all messages to persistent
    workgroups, one per CU.  Planning (validation, descriptors, tile map, key
    schedules; one pinned H2D copy) happens once here; ``run()`` only launches,
    so it can be replayed with new data in the same buffers, and captured in a
    HIP graph.

    xs / outs: GPU tensors (contiguous, 16-byte aligned; ``outs[i] is xs[i]``
    for in place); keys: AES keys (16/24/32 bytes) selected per message by
    ``key_index`` (default: keys[i] for message i); counters: the 16-byte
    initial counter block of every message (128-bit big-endian increment);
    tile_blocks: 64 / 128 / 256 blocks per tile (default: picked from the
    message sizes).  Distinct messages must not overlap.
    """

    def __init__(self, xs, keys, counters, outs=None, key_index=None, tile_blocks=None):
        import numpy as np

        n = len(xs)
        if len(counters) != n:
            raise ValueError("one counter per message")
        if outs is None:
            outs = [torch.empty_like(x) for x in xs]
        if len(outs) != n:
            raise ValueError("one output per message")
        if key_index is None:
            if len(keys) != n:
                raise ValueError("one key per message, or pass key_index")
            key_index = range(n)
        kidx = np.fromiter((int(k) for k in key_index), dtype=np.int64, count=n)
        if n and (kidx.min() < 0 or kidx.max() >= len(keys)):
            raise ValueError("key_index out of range")
        self.outs = list(outs)
        self._keep = list(xs)  # descriptors hold raw addresses: keep the tensors alive
        self._launches = []
        self.device = xs[0].device if n else None
        self.ntiles, self.tile_blocks = 0, tile_blocks or 256
        if n == 0:
            return
        desc = np.zeros((n, 6), dtype=np.uint64)  # in, out, nbytes, ctr_hi, ctr_lo, key
        for i, (x, o) in enumerate(zip(xs, outs)):
            _check_dev(x, f"xs[{i}]")
            _check_dev(o, f"outs[{i}]")
            if x.device != self.device or o.device != self.device:
                raise ValueError("all messages must be on one device")
            nb = _nbytes(x)
            if _nbytes(o) != nb:
                raise ValueError(f"outs[{i}] must have the byte size of xs[{i}]")
            pi, po = x.data_ptr(), o.data_ptr()
            if nb and (pi % 16 or po % 16):
                raise ValueError(f"message {i}: batch buffers must be 16-byte aligned (clone a sliced tensor)")
            if pi != po and pi < po + nb and po < pi + nb:
                raise ValueError(f"message {i}: input and output overlap partially")
            c = bytes(counters[i])
            if len(c) != 16:
                raise ValueError(f"counters[{i}] must be 16 bytes")
            desc[i, :5] = (pi, po, nb, int.from_bytes(c[:8], "big"), int.from_bytes(c[8:], "big"))
        desc[:, 5] = kidx.astype(np.uint64)

        self._build(desc, keys, kidx, tile_blocks)

    @classmethod
    def packed(cls, buf: torch.Tensor, lengths, keys, counters, out: torch.Tensor | None = None, offsets=None,
               key_index=None, tile_blocks=None) -> "CtrBatch":
        """Messages packed in ONE device buffer (the usual serving layout):
        message i is ``buf[offsets[i] : offsets[i] + lengths[i]]`` (offsets
        default to back-to-back 16-byte aligned slots) and lands at the same
        offset of ``out`` (default: a new buffer; ``out is buf`` for in
        place).  counters: (n, 16) uint8 array / tensor or a list of 16-byte
        blocks.  Planning is vectorised (no per-message Python work); the
        outputs are ``self.out``."""
        import numpy as np

        nb = _nbytes(buf)
        lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
        n = lens.size
        if offsets is None:
            offs = np.zeros(n, dtype=np.int64)
            if n > 1:
                offs[1:] = np.cumsum((lens[:-1] + 15) // 16 * 16)
        else:
            offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
        if offs.size != n:
            raise ValueError("one offset per message")
        if n and ((lens < 0).any() or (offs < 0).any() or (offs + lens > nb).any()):
            raise ValueError("messages must lie inside the buffer")
        if n and (offs % 16).any():
            raise ValueError("message offsets must be multiples of 16")
        nz = np.nonzero(lens)[0]  # disjoint messages (empty ones occupy nothing)
        if nz.size > 1:
            so, sl = offs[nz], lens[nz]
            o = np.argsort(so, kind="stable")
            if ((so[o][:-1] + sl[o][:-1]) > so[o][1:]).any():
                raise ValueError("messages overlap")
        ctr = counters.cpu().numpy() if isinstance(counters, torch.Tensor) else counters
        if isinstance(ctr, np.ndarray):
            c = np.ascontiguousarray(ctr, dtype=np.uint8).reshape(-1, 16)
        else:
            if len(ctr) != n or any(len(bytes(x)) != 16 for x in ctr):
                raise ValueError("one 16-byte counter per message")
            c = np.frombuffer(b"".join(bytes(x) for x in ctr), dtype=np.uint8).reshape(-1, 16)
        if c.shape[0] != n:
            raise ValueError("one 16-byte counter per message")
        if key_index is None:
            if len(keys) != n:
                raise ValueError("one key per message, or pass key_index")
            kidx = np.arange(n, dtype=np.int64)
        else:
            kidx = np.asarray(key_index, dtype=np.int64).reshape(-1)
            if kidx.size != n:
                raise ValueError("one key index per message")
        if n and (kidx.min() < 0 or kidx.max() >= len(keys)):
            raise ValueError("key_index out of range")
        _check_dev(buf, "buf")
        out = _out_like(buf, out)
        pi, po = buf.data_ptr(), out.data_ptr()
        if (pi | po) % 16:
            raise ValueError("buf / out must be 16-byte aligned")
        if pi != po and pi < po + nb and po < pi + nb:
            raise ValueError("buf and out overlap partially")
        self = cls.__new__(cls)
        self.out = out
        self.outs = [out]
        self._keep = [buf]
        self._launches = []
        self.device = buf.device
        if n == 0:
            self.ntiles, self.tile_blocks = 0, tile_blocks or 256
            return self
        desc = np.zeros((n, 6), dtype=np.uint64)
        desc[:, 0] = np.uint64(pi) + offs.astype(np.uint64)
        desc[:, 1] = np.uint64(po) + offs.astype(np.uint64)
        desc[:, 2] = lens.astype(np.uint64)
        desc[:, 3] = c[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
        desc[:, 4] = c[:, 8:].copy().view(">u8").reshape(-1).astype(np.uint64)
        desc[:, 5] = kidx.astype(np.uint64)
        self._build(desc, keys, kidx, tile_blocks)
        return self

    def _build(self, desc, keys, kidx, tile_blocks):
        """Tile map + key schedules + descriptors -> one pinned upload."""
        import numpy as np

        if tile_blocks is None:
            tile_blocks = _pick_tile(desc[:, 2])
        if tile_blocks not in BATCH_TILES:
            raise ValueError(f"tile_blocks must be one of {BATCH_TILES}")
        self.tile_blocks = tile_blocks
        tile_bytes = 16 * tile_blocks
        # messages of many tiles use counter-aligned tiles (otc.h
        # OTC_BATCH_ALIGNED): one partial tile more, but rounds 1-2 are mostly
        # computed once per tile (133 instead of 160 lookups per block)
        tb = np.uint64(tile_blocks)
        aligned = (desc[:, 2] + np.uint64(15)) // np.uint64(16) >= np.uint64(BATCH_ALIGN_MIN_TILES) * tb
        shift = np.where(aligned, desc[:, 4] % tb, np.uint64(0)).astype(np.uint64)
        align = np.where(aligned, np.uint64(BATCH_ALIGNED) | shift, np.uint64(0)).astype(np.uint64)
        desc[:, 5] = (desc[:, 5] & np.uint64(0xFFFFFFFF)) | (align << np.uint64(32))
        self.aligned_msgs = int(aligned.sum())
        ek = [expand_key(k) for k in keys]
        key_blob = b"".join(bytes(k) for k in ek)  # otc_aes_key[] (256 B each)
        nr_msg = np.array([k.nr for k in ek], dtype=np.int64)[kidx]
        parts, launches, off = [key_blob], [], len(key_blob)

        def add(b: bytes) -> int:
            nonlocal off
            pad = (-off) % 16
            if pad:
                parts.append(bytes(pad))
                off += pad
            at = off
            parts.append(b)
            off += len(b)
            return at

        for nr in (10, 12, 14):
            sel = np.nonzero(nr_msg == nr)[0]
            if not len(sel):
                continue
            d = desc[sel]
            sh = (d[:, 5] >> np.uint64(32)) & np.uint64(0xFFFF)
            tiles = np.where(d[:, 2] > 0, (d[:, 2] + np.uint64(16) * sh + np.uint64(tile_bytes - 1)) // np.uint64(tile_bytes),
                             np.uint64(0))
            ntiles = int(tiles.sum())
            if ntiles == 0:
                continue
            first = np.zeros(len(sel), dtype=np.uint64)
            first[1:] = np.cumsum(tiles)[:-1]
            tmap = np.repeat(np.arange(len(sel), dtype=np.uint32), tiles.astype(np.int64))
            assert tmap.size == ntiles and int(tmap.max()) < len(sel)
            launches.append((add(d.tobytes()), add(first.tobytes()), add(tmap.tobytes()), ntiles, nr))
        host = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).pin_memory()
        self._plan = host.to(self.device, non_blocking=True)
        self._ready = torch.cuda.Event()
        self._ready.record(torch.cuda.current_stream(self.device))
        self._launches = launches
        self.ntiles = sum(t for *_, t, _ in launches)

    def run(self, stream=None):
        """Launch the batch on ``stream`` (default: the current stream);
        returns the list of outputs."""
        if not self._launches:
            return self.outs
        st = stream or torch.cuda.current_stream(self.device)
        st.wait_event(self._ready)
        base = self._plan.data_ptr()
        lib = _lib()
        with torch.cuda.device(self.device):
            for o_desc, o_first, o_map, ntiles, nr in self._launches:
                rc = lib.otc_aes_ctr_batch(base + o_desc, base, base + o_map, base + o_first, ntiles,
                                           self.tile_blocks, nr, ctypes.c_void_p(st.cuda_stream))
                _native.check(rc, "otc_aes_ctr_batch")
        return self.outs


def ctr_batch(xs, keys, counters, outs=None, key_index=None, tile_blocks=None):
    """Plan and run a ``CtrBatch`` once."""
    return CtrBatch(xs, keys, counters, outs=outs, key_index=key_index, tile_blocks=tile_blocks).run()


def ctr_rfc3686(x: torch.Tensor, key: bytes, nonce: bytes, ivec: bytes, out=None, block_offset: int = 0,
                impl="auto") -> torch.Tensor:
    """AES-CTR with the AES-NI/RFC 3686 counter block nonce||ivec||BE32(1) and
    64-bit increment (reference aesni.c:120-152)."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = expand_key(key)
    n = (ctypes.c_uint8 * 4).from_buffer_copy(bytes(nonce))
    iv = (ctypes.c_uint8 * 8).from_buffer_copy(bytes(ivec))
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_ctr_rfc3686(ip, op, _nbytes(x), ctypes.byref(k), n, iv,
            int(block_offset), _impl(impl), _stream(x)))
    _native.check(rc, "otc_aes_ctr_rfc3686")
    return out


def ecb_encrypt(x: torch.Tensor, key: bytes, out=None, impl="auto") -> torch.Tensor:
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = expand_key(key)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_ecb(ip, op, _nbytes(x), ctypes.byref(k), _impl(impl), _stream(x)))
    _native.check(rc, "otc_aes_ecb(encrypt)")
    return out


def ecb_decrypt(x: torch.Tensor, key: bytes, out=None, impl="auto") -> torch.Tensor:
    """ECB decryption: the T-table inverse cipher, the bitsliced one (the
    forward S-box as S^-1 = L S L), or both concurrently ("split").  "auto":
    the split from 2 GiB, the persistent T-table claim kernel alone from 512
    MiB, the grid T-table below (engine.cpp pick_ecb_impl / split_form)."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = expand_key(key, decrypt=True)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_ecb(ip, op, _nbytes(x), ctypes.byref(k), _impl(impl),
                                                           _stream(x)))
    _native.check(rc, "otc_aes_ecb(decrypt)")
    return out


def cbc_decrypt(x: torch.Tensor, key: bytes, iv: bytes, out=None, impl="auto") -> torch.Tensor:
    """Parallel CBC decryption (kernel choice as ecb_decrypt).  In place
    (out=x) runs through a copy of the input: block i needs ciphertext block
    i-1, which its own output overwrites."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = expand_key(key, decrypt=True)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_cbc_decrypt_impl(ip, op, _nbytes(x), ctypes.byref(k),
            _b16(iv, "iv"), _impl(impl), _stream(x)), inplace_ok=False)
    _native.check(rc, "otc_aes_cbc_decrypt")
    return out


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
    return _seg_call("otc_aes_cbc_encrypt_segments_impl", x, key, iv0, segment_bytes, out, True, impl)


def cbc_decrypt_segments(x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out=None,
                         impl="auto") -> torch.Tensor:
    """Inverse of ``cbc_encrypt_segments``: fully parallel.  ``impl``:
    "ttable", "bitslice" (the bitsliced claim kernel alone), "split" (both at
    once), "auto" = split from 2 GiB of power-of-two segments, the persistent
    T-table claim kernel from 512 MiB (other segment sizes: the T-table)."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    n = _nbytes(x)
    if segment_bytes <= 0 or n % segment_bytes:
        raise ValueError("byte size must be a multiple of segment_bytes")
    k = expand_key(key, decrypt=True)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_cbc_decrypt_segments_impl(ip, op, segment_bytes,
            n // segment_bytes, ctypes.byref(k), _b16(iv0, "iv0"), _impl(impl), _stream(x)), inplace_ok=False)
    _native.check(rc, "otc_aes_cbc_decrypt_segments")
    return out


def cfb128_decrypt(x: torch.Tensor, key: bytes, iv: bytes, out=None, impl="auto") -> torch.Tensor:
    """Parallel CFB128 decryption, P_i = C_i ^ E(C_{i-1}) (encryption key).
    ``impl``: "ttable", "bitslice" (the forward bitsliced cipher on the input
    shifted one block), "split" (both at once, as ECB encryption) or "auto"
    (as ecb_decrypt).  In place runs through a copy of the input."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = expand_key(key)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_cfb128_decrypt_impl(ip, op, _nbytes(x), ctypes.byref(k),
            _b16(iv, "iv"), _impl(impl), _stream(x)), inplace_ok=False)
    _native.check(rc, "otc_aes_cfb128_decrypt")
    return out


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
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_xts(ip, op, unit, n // unit, ctypes.byref(k), tw, _stream(x)))
    _native.check(rc, "otc_aes_xts")
    return out


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


GCM_MAX_BYTES = (1 << 36) - 32  # SP 800-38D: plaintext bytes of one message


@functools.lru_cache(maxsize=64)
def _gcm_key(key: bytes) -> _native.OtcGcmKey:
    k = _native.OtcGcmKey()
    if _lib().otc_gcm_key_init(ctypes.byref(k), _native.as_u8p(key), len(key) * 8):
        raise ValueError(f"AES key must be 16, 24 or 32 bytes, got {len(key)}")
    return k


def ctr32(x: torch.Tensor, key: bytes, counter: bytes, out: torch.Tensor | None = None, impl="auto") -> torch.Tensor:
    """GCM's counter mode: only bytes 12..15 of ``counter`` increment
    (big-endian), wrapping at 2**32 with bytes 0..11 unchanged.  The CTR
    kernels of ``ctr`` with every ``impl``; a call that crosses the wrap is
    two launches.  Any byte length up to 2**32 blocks; may run in place."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    k = expand_key(key)
    c = _b16(counter, "counter")
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_ctr32(ip, op, _nbytes(x), ctypes.byref(k), c, _impl(impl),
                                                             _stream(x)))
    _native.check(rc, "otc_aes_ctr32")
    return out


def ghash(x: torch.Tensor, h: bytes, y0: bytes = bytes(16)) -> torch.Tensor:
    """GHASH (SP 800-38D) under the hash subkey ``h``, continued from ``y0``,
    over the bytes of ``x`` with the last partial block zero-padded: a 16-byte
    uint8 tensor on ``x``'s device.  Parallel over the whole chip
    (``csrc/hip/aes_gcm.hip``); asynchronous on the current stream."""
    _check_dev(x, "x")
    hb, yb = _b16(h, "h"), _b16(y0, "y0")
    y = torch.empty(16, dtype=torch.uint8, device=x.device)
    xb = _bytes(x)
    if xb.data_ptr() % 16 and xb.numel():
        xb = xb.clone()  # the kernel loads 16 bytes per lane
    with torch.cuda.device(x.device):
        rc = _lib().otc_ghash(xb.data_ptr(), xb.numel(), hb, yb, y.data_ptr(), _stream(x))
    _native.check(rc, "otc_ghash")
    return y


def ghash_spans() -> list[int]:
    """Byte sizes of the pieces the GHASH kernel cuts its data into, smallest
    first (otc.h otc_ghash_spans): lengths around them take different paths."""
    buf = (ctypes.c_uint64 * 16)()
    n = _lib().otc_ghash_spans(buf, 16)
    return [int(v) for v in buf[:n]]


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
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_gcm(
            ip, op, n, ctypes.byref(k), DECRYPT if decrypt else ENCRYPT, _native.as_u8p(iv), len(iv),
            _native.as_u8p(aad), len(aad), tag.data_ptr(), _impl(impl), _stream(x)))
    _native.check(rc, "otc_aes_gcm")
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
    tag = bytes(tag.cpu().numpy().tobytes()) if isinstance(tag, torch.Tensor) else bytes(tag)
    if not 4 <= len(tag) <= 16:
        raise ValueError("a GCM tag has 4 to 16 bytes")
    out, t = _gcm(x, key, iv, aad, out, impl, True)
    if not hmac.compare_digest(t.cpu().numpy().tobytes()[: len(tag)], tag):
        out.zero_()
        raise GcmTagError("GCM tag mismatch: the output was zeroed")
    return out


GCM_BATCH_MAX_BYTES = 1 << 20  # otc.h OTC_GCM_BATCH_MAX_BYTES
GCM_BATCH_MAX_AAD = 1 << 16  # otc.h OTC_GCM_BATCH_MAX_AAD


class GcmBatch:
    """A planned batch of AES-GCM records under ONE key -- own buffers, own
    12-byte IV, own AAD and own 16-byte tag each (``otc_aes_gcm_batch``).
    Record ``m`` is SP 800-38D GCM under ``(key, ivs[m], aads[m])``.

    The serving shape: TLS records, ESP / QUIC packets, sealed sectors.  One
    ``gcm_encrypt`` per record pays an allocation, 384 KiB of hash tables and
    a launch per level each time; here planning -- validation, descriptors,
    the CTR half's tile map, the key schedule, the per-key hash tables, the
    workspace, one pinned upload -- happens once in the constructor, and
    ``encrypt`` / ``decrypt`` only launch one linear chain of kernels on one
    stream: no allocation, no host synchronisation, capturable in a
    ``torch.cuda.CUDAGraph``.  They can be replayed with new data in the same
    buffers.

    **IV uniqueness under a key is the caller's duty, and a replay must bring
    new IVs**: that is why the IVs are no part of the plan but a device
    ``uint8 [n, 12]`` tensor handed to every run (a captured graph reads the
    tensor's contents at replay: change them in place).  Only 12-byte IVs.

    xs / outs: GPU tensors (contiguous, 16-byte aligned; ``outs[i] is xs[i]``
    for in place), 0 .. 1 MiB each, any byte count -- larger messages belong
    to ``gcm_encrypt``.  Distinct records must not overlap.  aads: ``None``, a
    device ``uint8 [n, A]`` tensor (row m is record m's AAD), or a list with
    one entry per record: a device tensor or host bytes (uploaded once with
    the plan), 0 .. 64 KiB each, any alignment; no AAD may overlap any
    record's output (an encryption writes the outputs before it hashes).  A
    record of 0 bytes is valid, with AAD (GMAC) or without.  One key per batch: the hash tables are 64 KiB
    per constant and cannot be held per record.  tag_bytes: how many bytes of a
    tag ``decrypt`` compares (4 .. 16).  lanes: 16 or 64 lanes of the hash
    kernel per record (default: 16 for records up to 12 KiB on average and no
    record above 64 KiB, else 64; the result is the same, only the speed
    differs).

    ``tags`` and ``ok`` are the batch's own tensors, overwritten by the next
    run; ``decrypt`` therefore refuses ``self.tags`` as the expected tags."""

    def __init__(self, xs, key: bytes, outs=None, aads=None, tag_bytes: int = 16, tile_blocks=None, lanes=None):
        import numpy as np

        self._init_common(key, tag_bytes, lanes)
        xs = list(xs)
        n = len(xs)
        if outs is None:
            outs = [torch.empty_like(x) for x in xs]
        outs = list(outs)
        if len(outs) != n:
            raise ValueError("one output per record")
        self.outs = outs
        self._keep = [xs]
        self.device = xs[0].device if n else None
        desc = np.zeros((n, 6), dtype=np.uint64)  # in, out, nbytes, aad, aad_bytes, reserved
        for i, (x, o) in enumerate(zip(xs, outs)):
            _check_dev(x, f"xs[{i}]")
            _check_dev(o, f"outs[{i}]")
            if x.device != self.device or o.device != self.device:
                raise ValueError("all records must be on one device")
            nb = _nbytes(x)
            if _nbytes(o) != nb:
                raise ValueError(f"outs[{i}] must have the byte size of xs[{i}]")
            if nb > GCM_BATCH_MAX_BYTES:
                raise ValueError(f"record {i}: more than 1 MiB of data (use gcm_encrypt for large messages)")
            desc[i, :3] = (x.data_ptr() if nb else 0, o.data_ptr() if nb else 0, nb)
        self._set_aads(desc, aads)
        self._build(desc, tile_blocks)

    @classmethod
    def packed(cls, buf: torch.Tensor, lengths, key: bytes, out: torch.Tensor | None = None, offsets=None, aad=None,
               tag_bytes: int = 16, tile_blocks=None, lanes=None) -> "GcmBatch":
        """Records packed in ONE device buffer, ``CtrBatch.packed``'s layout:
        record i is ``buf[offsets[i] : offsets[i] + lengths[i]]`` (offsets
        default to back-to-back 16-byte aligned slots) and lands at the same
        offset of ``out`` (default: a new buffer; ``out is buf`` for in
        place).  aad: ``None`` or a device ``uint8 [n, A]`` tensor.  Bytes of
        ``out`` outside the records are not written.  The output is
        ``self.out``."""
        import numpy as np

        self = cls.__new__(cls)
        self._init_common(key, tag_bytes, lanes)
        _check_dev(buf, "buf")
        nb = _nbytes(buf)
        lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
        n = lens.size
        if offsets is None:
            offs = np.zeros(n, dtype=np.int64)
            if n > 1:
                offs[1:] = np.cumsum((lens[:-1] + 15) // 16 * 16)
        else:
            offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
        if offs.size != n:
            raise ValueError("one offset per record")
        if n and ((lens < 0).any() or (offs < 0).any() or (offs + lens > nb).any()):
            raise ValueError("records must lie inside the buffer")
        if n and (offs % 16).any():
            raise ValueError("record offsets must be multiples of 16")
        if n and (lens > GCM_BATCH_MAX_BYTES).any():
            raise ValueError("a record has at most 1 MiB of data (use gcm_encrypt for large messages)")
        out = _out_like(buf, out)
        pi, po = buf.data_ptr(), out.data_ptr()
        if (pi | po) % 16:
            raise ValueError("buf / out must be 16-byte aligned")
        if pi != po and pi < po + nb and po < pi + nb:
            raise ValueError("buf and out overlap partially")
        if out.device != buf.device:
            raise ValueError("buf and out must be on one device")
        self.out = out
        self.outs = [out]
        self._keep = [buf]
        self.device = buf.device
        desc = np.zeros((n, 6), dtype=np.uint64)
        desc[:, 0] = np.uint64(pi) + offs.astype(np.uint64)
        desc[:, 1] = np.uint64(po) + offs.astype(np.uint64)
        desc[:, 2] = lens.astype(np.uint64)
        if aad is not None and not isinstance(aad, torch.Tensor):
            raise ValueError("aad must be a device uint8 [n, A] tensor")
        self._set_aads(desc, aad)
        self._build(desc, tile_blocks)
        return self

    def _init_common(self, key, tag_bytes, lanes):
        if not isinstance(tag_bytes, int) or not 4 <= tag_bytes <= 16:
            raise ValueError("a GCM tag has 4 to 16 bytes")
        if lanes not in (None, 16, 64):
            raise ValueError("lanes must be 16 or 64 (default: picked from the record sizes)")
        self.tag_bytes = tag_bytes
        self.lanes = lanes
        self._k = _gcm_key(bytes(key))
        self.n = 0
        self.ntiles = 0
        self.tags = self.ok = None

    def _set_aads(self, desc, aads):
        """Columns 3 and 4 of the descriptors; host AADs go to one device buffer."""
        import numpy as np

        n = desc.shape[0]
        if aads is None or n == 0:
            if isinstance(aads, (list, tuple)) and len(aads) != n:
                raise ValueError("one AAD per record")
            return
        if isinstance(aads, torch.Tensor):
            _check_dev(aads, "aads")
            if aads.dtype != torch.uint8 or aads.dim() != 2 or aads.shape[0] != n:
                raise ValueError(f"aads must be a uint8 [{n}, A] tensor")
            if aads.device != self.device:
                raise ValueError("aads must be on the records' device")
            a = int(aads.shape[1])
            if a > GCM_BATCH_MAX_AAD:
                raise ValueError("a record has at most 64 KiB of AAD")
            self._keep.append(aads)
            if a:
                desc[:, 3] = np.uint64(aads.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(a)
                desc[:, 4] = a
            return
        aads = list(aads)
        if len(aads) != n:
            raise ValueError("one AAD per record")
        host, at = [], 0
        for i, a in enumerate(aads):
            if isinstance(a, torch.Tensor):
                _check_dev(a, f"aads[{i}]")
                if a.device != self.device:
                    raise ValueError("aads must be on the records' device")
                na = _nbytes(a)
                addr = a.data_ptr()
            else:
                a = b"" if a is None else bytes(a)
                na, addr = len(a), None
            if na > GCM_BATCH_MAX_AAD:
                raise ValueError(f"record {i}: more than 64 KiB of AAD")
            if na and addr is None:
                host.append((i, at, a))
                at += na
            elif na:
                desc[i, 3] = addr
            desc[i, 4] = na
        self._keep.append(aads)
        if host:
            blob = torch.frombuffer(bytearray(b"".join(a for _, _, a in host)), dtype=torch.uint8).pin_memory()
            dev = blob.to(self.device, non_blocking=True)
            self._keep.append((blob, dev))
            for i, off, _ in host:
                desc[i, 3] = dev.data_ptr() + off

    def _build(self, desc, tile_blocks):
        """Planner (validation + the CTR half's tile map) -> one pinned upload;
        the key's hash tables; workspace, tags, verdicts."""
        import numpy as np

        n = desc.shape[0]
        self.n = n
        if tile_blocks is None:
            tile_blocks = _pick_tile(desc[:, 2]) if n else 256
        if tile_blocks not in BATCH_TILES:
            raise ValueError(f"tile_blocks must be one of {BATCH_TILES}")
        self.tile_blocks = tile_blocks
        if n == 0:
            return
        lib = _lib()
        desc = np.ascontiguousarray(desc)
        ntiles = lib.otc_gcm_batch_plan(desc.ctypes.data, n, tile_blocks, None, None, None)
        if ntiles < 0:
            raise ValueError((lib.otc_last_error() or b"").decode())
        ctr = np.zeros((n, 6), dtype=np.uint64)
        first = np.zeros(n, dtype=np.uint64)
        tmap = np.zeros(max(ntiles, 1), dtype=np.uint32)
        if lib.otc_gcm_batch_plan(desc.ctypes.data, n, tile_blocks, ctr.ctypes.data, tmap.ctypes.data,
                                  first.ctypes.data) != ntiles:
            raise RuntimeError("otc_gcm_batch_plan: the two passes disagree")
        parts, off = [], 0

        def add(b: bytes) -> int:
            nonlocal off
            pad = (-off) % 16
            if pad:
                parts.append(bytes(pad))
                off += pad
            at = off
            parts.append(b)
            off += len(b)
            return at

        if self.lanes is None:
            self.lanes = lib.otc_gcm_batch_lanes(desc.ctypes.data, n)
        self._o_key = add(bytes(self._k.enc))  # otc_aes_key[1]: the CTR half reads round keys from memory
        self._o_desc = add(desc.tobytes())
        self._o_ctr = add(ctr.tobytes())
        self._o_first = add(first.tobytes())
        self._o_map = add(tmap.tobytes())
        self.ntiles = int(ntiles)
        dev = self.device
        with torch.cuda.device(dev):
            host = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).pin_memory()
            self._plan = host.to(dev, non_blocking=True)
            self._tab = torch.empty(lib.otc_gcm_batch_table_bytes(), dtype=torch.uint8, device=dev)
            self._ws = torch.empty(lib.otc_gcm_batch_ws_bytes(n), dtype=torch.uint8, device=dev)
            self.tags = torch.empty((n, 16), dtype=torch.uint8, device=dev)
            self.ok = torch.zeros(n, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev)
            _native.check(lib.otc_gcm_batch_tables(ctypes.byref(self._k), self._tab.data_ptr(),
                                                   ctypes.c_void_p(st.cuda_stream)), "otc_gcm_batch_tables")
            # planning may wait; the runs never do, on whatever stream (or capture) they go
            st.synchronize()

    def _check_ivs(self, ivs):
        if not isinstance(ivs, torch.Tensor) or ivs.device.type != "cuda":
            raise ValueError("ivs must be a GPU tensor, uint8 [n, 12]")
        if ivs.dtype != torch.uint8 or ivs.dim() != 2 or not ivs.is_contiguous():
            raise ValueError("ivs must be a contiguous uint8 [n, 12] tensor")
        if ivs.shape[1] != 12:
            raise ValueError(f"only 12-byte IVs are accepted (got {ivs.shape[1]} bytes): other lengths need a hash "
                             "to form J0 -- use gcm_encrypt")
        if ivs.shape[0] != self.n:
            raise ValueError(f"one IV per record: ivs must be [{self.n}, 12]")
        if self.n and ivs.device != self.device:
            raise ValueError("ivs must be on the records' device")

    def _launch(self, decrypt, ivs, expect, stream):
        if self.n == 0:
            return
        st = stream or torch.cuda.current_stream(self.device)
        base = self._plan.data_ptr()
        with torch.cuda.device(self.device):
            rc = _lib().otc_aes_gcm_batch(
                base + self._o_desc, base + self._o_ctr, base + self._o_map, base + self._o_first, self.ntiles,
                self.tile_blocks, self.n, ctypes.byref(self._k), base + self._o_key, self._tab.data_ptr(),
                DECRYPT if decrypt else ENCRYPT, ivs.data_ptr(), self.tags.data_ptr(),
                expect.data_ptr() if decrypt else None, self.tag_bytes, self.ok.data_ptr() if decrypt else None,
                self._ws.data_ptr(), self.lanes, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_aes_gcm_batch")

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device or "cpu")

    def encrypt(self, ivs: torch.Tensor, stream=None):
        """Seal every record under ``ivs`` (device uint8 [n, 12]):
        ``(outs, tags)``, the tags a device uint8 [n, 16] tensor.  Only
        launches; every call must bring IVs never used under this key."""
        self._check_ivs(ivs)
        self._launch(False, ivs, None, stream)
        return self.outs, (self.tags if self.n else self._empty((0, 16), torch.uint8))

    def decrypt(self, ivs: torch.Tensor, tags: torch.Tensor, stream=None):
        """Open every record: ``(outs, ok)`` with ``ok`` a device bool [n]
        tensor.  tags: the received tags, device uint8 [n, tag_bytes].  The
        comparison runs on the device; the output of every record whose tag
        does not match is zeroed (in place: the ciphertext with it) and so is
        its row of ``self.tags`` -- the computed tag of a forged record is the
        valid tag of that forgery and is not handed out; the others are
        unaffected.  Nothing is read back.  ``tags`` must not be (or overlap)
        the batch's own ``self.tags``, which every run overwrites with what
        it computes: pass a copy (``ValueError`` otherwise)."""
        self._check_ivs(ivs)
        if not isinstance(tags, torch.Tensor) or tags.device.type != "cuda":
            raise ValueError(f"tags must be a GPU tensor, uint8 [n, {self.tag_bytes}]")
        if tags.dtype != torch.uint8 or tags.dim() != 2 or not tags.is_contiguous() or \
                tuple(tags.shape) != (self.n, self.tag_bytes):
            raise ValueError(f"tags must be a contiguous uint8 [{self.n}, {self.tag_bytes}] tensor")
        if self.n and tags.device != self.device:
            raise ValueError("tags must be on the records' device")
        if self.n:
            e0, e1 = tags.data_ptr(), tags.data_ptr() + self.n * self.tag_bytes
            for own in (self.tags, self.ok):
                if e0 < own.data_ptr() + _nbytes(own) and own.data_ptr() < e1:
                    raise ValueError("tags overlaps the batch's own tags / verdicts, which this run overwrites: "
                                     "pass a copy (tags.clone())")
        self._launch(True, ivs, tags, stream)
        return self.outs, (self.ok.view(torch.bool) if self.n else self._empty((0,), torch.bool))

    def ghash(self, stream=None) -> torch.Tensor:
        """The hash half by itself (``otc_ghash_batch``): a device uint8
        [n, 16] tensor, row m the GHASH under the key's H of record m's
        ``pad16(AAD) || pad16(input) || lengths``."""
        if self.n == 0:
            return self._empty((0, 16), torch.uint8)
        st = stream or torch.cuda.current_stream(self.device)
        s = torch.empty((self.n, 16), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = _lib().otc_ghash_batch(self._plan.data_ptr() + self._o_desc, self.n, self._tab.data_ptr(),
                                        s.data_ptr(), self.lanes, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_ghash_batch")
        return s


def gcm_batch_spans() -> list[int]:
    """The batched GHASH kernel's own boundaries in hashed blocks (AAD, data
    and length block together), smallest first (otc.h otc_gcm_batch_spans)."""
    buf = (ctypes.c_uint64 * 16)()
    n = _lib().otc_gcm_batch_spans(buf, 16)
    return [int(v) for v in buf[:n]]


def ghash_batch(xs, key: bytes, aads=None, lanes=None) -> torch.Tensor:
    """GHASH of every record of a batch under ``key``'s hash subkey, length
    block included: device uint8 [n, 16] (the hash kernel of ``GcmBatch``
    alone)."""
    xs = list(xs)
    return GcmBatch(xs, key, outs=xs, aads=aads, lanes=lanes).ghash()


def gcm_encrypt_batch(xs, key: bytes, ivs: torch.Tensor, aads=None, outs=None):
    """Plan and run a ``GcmBatch`` once: ``(outs, tags)``."""
    return GcmBatch(xs, key, outs=outs, aads=aads).encrypt(ivs)


def gcm_decrypt_batch(xs, key: bytes, ivs: torch.Tensor, tags: torch.Tensor, aads=None, outs=None):
    """Plan and run a ``GcmBatch`` once: ``(outs, ok)``; the tag length is
    ``tags.shape[1]``."""
    tb = int(tags.shape[1]) if isinstance(tags, torch.Tensor) and tags.dim() == 2 else 16
    return GcmBatch(xs, key, outs=outs, aads=aads, tag_bytes=tb).decrypt(ivs, tags)


def _seg_call(fn_name: str, x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out, inplace_ok: bool,
              impl="auto"):
    _check_dev(x, "x")
    out = _out_like(x, out)
    n = _nbytes(x)
    if segment_bytes <= 0 or segment_bytes % 16 or n % segment_bytes:
        raise ValueError("segment_bytes must be a positive multiple of 16 dividing the byte size")
    k = expand_key(key)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: getattr(_lib(), fn_name)(ip, op, segment_bytes, n // segment_bytes,
                  ctypes.byref(k), _b16(iv0, "iv0"), _impl(impl), _stream(x)), inplace_ok=inplace_ok)
    _native.check(rc, fn_name)
    return out


def cfb128_encrypt_segments(x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out=None,
                            impl="auto") -> torch.Tensor:
    """CFB128 encryption of independent segments (IV_s = iv0 + s), one
    serial chain per segment (``impl`` as ``cbc_encrypt_segments``)."""
    return _seg_call("otc_aes_cfb128_encrypt_segments_impl", x, key, iv0, segment_bytes, out, True, impl)


def cfb128_decrypt_segments(x: torch.Tensor, key: bytes, iv0: bytes, segment_bytes: int, out=None,
                            impl="auto") -> torch.Tensor:
    """Inverse of ``cfb128_encrypt_segments``: fully parallel (``impl`` as
    ``cbc_decrypt_segments``)."""
    _check_dev(x, "x")
    out = _out_like(x, out)
    n = _nbytes(x)
    if segment_bytes <= 0 or segment_bytes % 16 or n % segment_bytes:
        raise ValueError("segment_bytes must be a positive multiple of 16 dividing the byte size")
    k = expand_key(key)
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: _lib().otc_aes_cfb128_decrypt_segments_impl(ip, op, segment_bytes,
            n // segment_bytes, ctypes.byref(k), _b16(iv0, "iv0"), _impl(impl), _stream(x)), inplace_ok=False)
    _native.check(rc, "otc_aes_cfb128_decrypt_segments")
    return out
