"""``ChaChaBatch``: a planned batch of ChaCha20-Poly1305 records (RFC 8439
section 2.8), each with its own key, nonce, AAD and tag, backed by the gfx950
kernels of ``csrc/hip/chacha_batch.hip`` (``otc_chacha20_poly1305_batch``), and
the plan-and-run-once functions around it.

The names of this module are not in ``ops.__all__`` yet (reach them as
``ops.chacha_batch_ops.ChaChaBatch`` or through ``models.ChaCha20Poly1305``);
the planning pieces -- packed layout, descriptors, key index, AAD columns, the
pinned upload -- are ``batch_ops``'s."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from ._common import _check_dev, _lib, _nbytes, _spans
from .batch_ops import _Blob, _key_index, _packed_buffers, _packed_layout, _set_aads, _tensor_descs
from .keys import DECRYPT, ENCRYPT

CHACHA_BATCH_MAX_BYTES = 1 << 20  # otc.h OTC_CHACHA_BATCH_MAX_BYTES


def _keys32(keys) -> list[bytes]:
    """One 32-byte key or a list of them, as a list."""
    if isinstance(keys, (bytes, bytearray, memoryview)):
        keys = [keys]
    keys = [bytes(k) for k in keys]
    if not keys:
        raise ValueError("at least one key")
    for i, k in enumerate(keys):
        if len(k) != 32:
            raise ValueError(f"keys[{i}]: a ChaCha20 key has 32 bytes")
    return keys


class ChaChaBatch:
    """A planned batch of ChaCha20-Poly1305 records -- own buffers, own key,
    own 12-byte nonce, own AAD and own 16-byte tag each
    (``otc_chacha20_poly1305_batch``).  Record ``m`` is RFC 8439 section 2.8
    under ``(keys[key_index[m]], nonces[m], aads[m])``.

    The serving shape: WireGuard and QUIC packets, TLS 1.3 records, SSH
    packets.  One ``chacha20_poly1305_encrypt`` per record pays a host-side
    ChaCha block, the host-side powers of ``r``, an allocation and three or four
    launches each time; here planning -- validation, descriptors, the cipher's
    tile map, the keys, the workspace, one pinned upload -- happens once in the
    constructor, the one-time keys and the powers of ``r`` are made on the
    device, and ``encrypt`` / ``decrypt`` only launch one linear chain of
    kernels on one stream: no allocation, no host synchronisation, capturable
    in a ``torch.cuda.CUDAGraph``.  They can be replayed with new data in the
    same buffers.  A key per record costs nothing extra: Poly1305 has no tables.

    **Nonce uniqueness under a key is the caller's duty, and a replay must
    bring new nonces**: that is why the nonces are no part of the plan but a
    device ``uint8 [n, 12]`` tensor handed to every run (a captured graph reads
    the tensor's contents at replay: change them in place).

    xs / outs: GPU tensors (contiguous, 16-byte aligned; ``outs[i] is xs[i]``
    for in place), 0 .. 1 MiB each, any byte count -- larger messages belong
    to ``chacha20_poly1305_encrypt``.  Distinct records must not overlap, and
    no input may overlap another record's output.  keys: one 32-byte key or a
    list; key_index: the key of every record (default: ``keys[i]`` for record
    ``i`` when there are ``n`` keys, ``keys[0]`` when there is one).  aads:
    ``None``, a device ``uint8 [n, A]`` tensor (row m is record m's AAD), or a
    list with one entry per record: a device tensor or host bytes (uploaded
    once with the plan), 0 .. 64 KiB each, any alignment; no AAD may overlap
    any record's output (an encryption writes the outputs before it hashes).
    A record of 0 bytes is valid, with AAD or without.  Tags are 16 bytes.
    lanes: 16 or 64 lanes of the hash kernel per record (default: 16 for
    records that hash up to 512 blocks, 8 KiB, on average, else 64; the result
    is the same, only the speed differs).

    ``tags`` and ``ok`` are the batch's own tensors, overwritten by the next
    run; ``decrypt`` therefore refuses ``self.tags`` as the expected tags."""

    def __init__(self, xs, keys, outs=None, aads=None, key_index=None, lanes=None):
        import numpy as np
        self._init_common(keys, lanes)
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
        desc = np.zeros((n, 6), dtype=np.uint64)  # in, out, nbytes, aad, aad_bytes, key
        for i, pi, po, nb in _tensor_descs(xs, outs, self.device, "record"):
            if nb > CHACHA_BATCH_MAX_BYTES:
                raise ValueError(f"record {i}: more than 1 MiB of data (use chacha20_poly1305_encrypt for large messages)")
            desc[i, :3] = (pi if nb else 0, po if nb else 0, nb)
        _set_aads(desc, aads, self.device, self._keep)
        self._build(desc, key_index)

    @classmethod
    def packed(cls, buf: torch.Tensor, lengths, keys, out: torch.Tensor | None = None, offsets=None, aad=None,
               key_index=None, lanes=None) -> "ChaChaBatch":
        """Records packed in ONE device buffer, ``CtrBatch.packed``'s layout:
        record i is ``buf[offsets[i] : offsets[i] + lengths[i]]`` (offsets
        default to back-to-back 16-byte aligned slots) and lands at the same
        offset of ``out`` (default: a new buffer; ``out is buf`` for in
        place).  aad: ``None`` or a device ``uint8 [n, A]`` tensor.  Bytes of
        ``out`` outside the records are not written.  The output is
        ``self.out``."""
        self = cls.__new__(cls)
        self._init_common(keys, lanes)
        _check_dev(buf, "buf")
        lens, offs = _packed_layout(buf, lengths, offsets, "record")
        if lens.size and (lens > CHACHA_BATCH_MAX_BYTES).any():
            raise ValueError("a record has at most 1 MiB of data (use chacha20_poly1305_encrypt for large messages)")
        out, desc = _packed_buffers(buf, out, lens, offs)
        self.out = out
        self.outs = [out]
        self._keep = [buf]
        self.device = buf.device
        if aad is not None and not isinstance(aad, torch.Tensor):
            raise ValueError("aad must be a device uint8 [n, A] tensor")
        _set_aads(desc, aad, self.device, self._keep)
        self._build(desc, key_index)
        return self

    def _init_common(self, keys, lanes):
        if lanes not in (None, 16, 64):
            raise ValueError("lanes must be 16 or 64 (default: picked from the record sizes)")
        self.lanes = lanes
        self._keys = _keys32(keys)
        self.n = 0
        self.ntiles = 0
        self.tags = self.ok = None

    def _build(self, desc, key_index):
        """Key index -> planner (validation + the cipher's tile map) -> one
        pinned upload; workspace, tags, verdicts."""
        import numpy as np
        self.n = n = desc.shape[0]
        nkeys = len(self._keys)
        if key_index is None and nkeys == 1:
            kidx = np.zeros(n, dtype=np.int64)
        else:
            if key_index is not None:
                key_index = np.fromiter((int(k) for k in key_index), dtype=np.int64)
            kidx = _key_index(key_index, n, nkeys)
        if n == 0:
            return
        desc[:, 5] = kidx.astype(np.uint64)
        lib = _lib()
        desc = np.ascontiguousarray(desc)
        ntiles = lib.otc_chacha_batch_plan(desc.ctypes.data, n, nkeys, None, None)
        if ntiles < 0:
            raise ValueError((lib.otc_last_error() or b"").decode())
        first = np.zeros(n, dtype=np.uint64)
        tmap = np.zeros(max(ntiles, 1), dtype=np.uint32)
        if lib.otc_chacha_batch_plan(desc.ctypes.data, n, nkeys, tmap.ctypes.data, first.ctypes.data) != ntiles:
            raise RuntimeError("otc_chacha_batch_plan: the two passes disagree")
        if self.lanes is None:
            self.lanes = lib.otc_chacha_batch_lanes(desc.ctypes.data, n)
        blob = _Blob()
        self._o_keys = blob.add(b"".join(self._keys))
        self._o_desc = blob.add(desc.tobytes())
        self._o_first = blob.add(first.tobytes())
        self._o_map = blob.add(tmap.tobytes())
        self.ntiles = int(ntiles)
        dev = self.device
        with torch.cuda.device(dev):
            self._plan = blob.upload(dev)
            self._ws = torch.empty(lib.otc_chacha_batch_ws_bytes(n), dtype=torch.uint8, device=dev)
            self.tags = torch.empty((n, 16), dtype=torch.uint8, device=dev)
            self.ok = torch.zeros(n, dtype=torch.uint8, device=dev)
            # planning may wait; the runs never do, on whatever stream (or capture) they go
            torch.cuda.current_stream(dev).synchronize()

    def _check_nonces(self, nonces):
        if not isinstance(nonces, torch.Tensor) or (self.n and nonces.device.type != "cuda"):
            raise ValueError("nonces must be a GPU tensor, uint8 [n, 12]")
        if nonces.dtype != torch.uint8 or nonces.dim() != 2 or not nonces.is_contiguous():
            raise ValueError("nonces must be a contiguous uint8 [n, 12] tensor")
        if nonces.shape[1] != 12:
            raise ValueError(f"a ChaCha20-Poly1305 nonce has 12 bytes (got {nonces.shape[1]})")
        if nonces.shape[0] != self.n:
            raise ValueError(f"one nonce per record: nonces must be [{self.n}, 12]")
        if self.n and nonces.device != self.device:
            raise ValueError("nonces must be on the records' device")

    def _launch(self, decrypt, nonces, expect, stream):
        if self.n == 0:
            return
        st = stream or torch.cuda.current_stream(self.device)
        base = self._plan.data_ptr()
        with torch.cuda.device(self.device):
            rc = _lib().otc_chacha20_poly1305_batch(
                base + self._o_desc, base + self._o_map, base + self._o_first, self.ntiles, self.n,
                base + self._o_keys, DECRYPT if decrypt else ENCRYPT, nonces.data_ptr(), self.tags.data_ptr(),
                expect.data_ptr() if decrypt else None, self.ok.data_ptr() if decrypt else None,
                self._ws.data_ptr(), self.lanes, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_chacha20_poly1305_batch")

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device or "cpu")

    def encrypt(self, nonces: torch.Tensor, stream=None):
        """Seal every record under ``nonces`` (device uint8 [n, 12]):
        ``(outs, tags)``, the tags a device uint8 [n, 16] tensor.  Only
        launches; every call must bring nonces never used under their keys."""
        self._check_nonces(nonces)
        self._launch(False, nonces, None, stream)
        return self.outs, (self.tags if self.n else self._empty((0, 16), torch.uint8))

    def decrypt(self, nonces: torch.Tensor, tags: torch.Tensor, stream=None):
        """Open every record: ``(outs, ok)`` with ``ok`` a device bool [n]
        tensor.  tags: the received tags, device uint8 [n, 16].  The
        comparison runs on the device; the output of every record whose tag
        does not match is zeroed (in place: the ciphertext with it) and so is
        its row of ``self.tags`` -- the computed tag of a forged record is the
        valid tag of that forgery and is not handed out; the others are
        unaffected.  Nothing is read back.  ``tags`` must not be (or overlap)
        the batch's own ``self.tags`` / ``self.ok``, which every run
        overwrites with what it computes: pass a copy (``ValueError``
        otherwise)."""
        if self.n and isinstance(tags, torch.Tensor):  # first: whatever else is wrong, never the batch's own
            e0, e1 = tags.data_ptr(), tags.data_ptr() + _nbytes(tags)
            for own in (self.tags, self.ok):
                if e0 < own.data_ptr() + _nbytes(own) and own.data_ptr() < e1:
                    raise ValueError("tags overlaps the batch's own tags / verdicts, which this run overwrites: "
                                     "pass a copy (tags.clone())")
        self._check_nonces(nonces)
        if not isinstance(tags, torch.Tensor) or (self.n and tags.device.type != "cuda"):
            raise ValueError("tags must be a GPU tensor, uint8 [n, 16]")
        if tags.dtype != torch.uint8 or tags.dim() != 2 or not tags.is_contiguous() or \
                tuple(tags.shape) != (self.n, 16):
            raise ValueError(f"tags must be a contiguous uint8 [{self.n}, 16] tensor")
        if self.n and tags.device != self.device:
            raise ValueError("tags must be on the records' device")
        self._launch(True, nonces, tags, stream)
        return self.outs, (self.ok.view(torch.bool) if self.n else self._empty((0,), torch.bool))

    def poly1305(self, onetime_keys, stream=None) -> torch.Tensor:
        """The hash half by itself (``otc_poly1305_batch``): a device uint8
        [n, 16] tensor, row m the Poly1305 tag under ``onetime_keys[m]``
        (r || s, 32 bytes; r is clamped on the device) of record m's
        ``pad16(AAD) || pad16(input) || lengths``.  onetime_keys: a device
        uint8 [n, 32] tensor (the call only launches), or a list of 32-byte
        keys (uploaded by this call, a synchronous copy)."""
        if not isinstance(onetime_keys, torch.Tensor):
            ks = [bytes(k) for k in onetime_keys]
            if len(ks) != self.n or any(len(k) != 32 for k in ks):
                raise ValueError("one 32-byte one-time key per record")
            if self.n == 0:
                return self._empty((0, 16), torch.uint8)
            onetime_keys = torch.frombuffer(bytearray(b"".join(ks)), dtype=torch.uint8).view(self.n, 32).to(self.device)
        otk = onetime_keys
        if otk.dtype != torch.uint8 or otk.dim() != 2 or not otk.is_contiguous() or tuple(otk.shape) != (self.n, 32):
            raise ValueError(f"onetime_keys must be a contiguous uint8 [{self.n}, 32] tensor")
        if self.n == 0:
            return self._empty((0, 16), torch.uint8)
        if otk.device != self.device:
            raise ValueError("onetime_keys must be on the records' device")
        if otk.data_ptr() % 4:
            raise ValueError("onetime_keys must be 4-byte aligned (clone a sliced tensor)")
        st = stream or torch.cuda.current_stream(self.device)
        tags = torch.empty((self.n, 16), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = _lib().otc_poly1305_batch(self._plan.data_ptr() + self._o_desc, self.n, otk.data_ptr(), tags.data_ptr(),
                                           self.lanes, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_poly1305_batch")
        return tags


def chacha_batch_spans() -> list[int]:
    """The batched Poly1305 kernel's own boundaries in hashed blocks (AAD,
    data and length block together), smallest first (otc.h
    otc_chacha_batch_spans)."""
    return _spans("otc_chacha_batch_spans")


def poly1305_batch(xs, onetime_keys, aads=None, lanes=None) -> torch.Tensor:
    """The AEAD's Poly1305 tag of every record of a batch under its own
    one-time key, AAD and length block included: device uint8 [n, 16] (the
    hash kernel of ``ChaChaBatch`` alone)."""
    xs = list(xs)
    return ChaChaBatch(xs, bytes(32), outs=xs, aads=aads, lanes=lanes).poly1305(onetime_keys)


def chacha20_poly1305_encrypt_batch(xs, keys, nonces: torch.Tensor, aads=None, outs=None, key_index=None):
    """Plan and run a ``ChaChaBatch`` once: ``(outs, tags)``."""
    return ChaChaBatch(xs, keys, outs=outs, aads=aads, key_index=key_index).encrypt(nonces)


def chacha20_poly1305_decrypt_batch(xs, keys, nonces: torch.Tensor, tags: torch.Tensor, aads=None, outs=None,
                                    key_index=None):
    """Plan and run a ``ChaChaBatch`` once: ``(outs, ok)``."""
    return ChaChaBatch(xs, keys, outs=outs, aads=aads, key_index=key_index).decrypt(nonces, tags)
