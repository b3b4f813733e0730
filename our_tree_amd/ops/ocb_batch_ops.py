"""``OcbBatch``: a planned batch of AES-OCB3 records (RFC 7253), all under one
key, each with its own 12-byte nonce, AAD and 16-byte tag, backed by the gfx950
kernels of ``csrc/hip/aes_ocb_batch.hip`` (``otc_aes_ocb_batch``), and the
plan-and-run-once functions around it.

The names of this module are not in ``ops.__all__`` yet (reach them as
``ops.ocb_batch_ops.OcbBatch`` or through ``models.AES``); the planning pieces
-- packed layout, descriptors, AAD columns, the pinned upload -- are
``batch_ops``'s."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from ._common import _check_dev, _lib, _nbytes, _spans
from .batch_ops import _Blob, _packed_buffers, _packed_layout, _set_aads, _tensor_descs
from .keys import DECRYPT, ENCRYPT
from .ocb_ops import _ocb_key

OCB_BATCH_MAX_BYTES = 1 << 20  # otc.h OTC_OCB_BATCH_MAX_BYTES


class OcbBatch:
    """A planned batch of AES-OCB3 records -- own buffers, own 12-byte nonce,
    own AAD and own 16-byte tag each, ONE key for the batch
    (``otc_aes_ocb_batch``).  Record ``m`` is RFC 7253 OCB3 with TAGLEN 128
    under ``(key, nonces[m], aads[m])`` and equals ``ocb_ops.ocb_encrypt`` on
    that record alone, byte for byte.  Other nonce and tag lengths stay with
    the single-message call.

    One ``ocb_encrypt`` per record pays two host AES blocks for ``Offset_0``, a
    host hash of the AAD and three launches each time; here planning --
    validation, descriptors, the bulk kernel's tile map, the workspace, one
    pinned upload -- happens once in the constructor, ``Offset_0`` and
    ``HASH(K, A)`` are made on the device, and ``encrypt`` / ``decrypt`` only
    launch one linear chain of kernels on one stream: no allocation, no host
    synchronisation, capturable in a ``torch.cuda.CUDAGraph``.  They can be
    replayed with new data in the same buffers.  The data is read once: OCB
    needs no second pass for the tag.

    **Nonce uniqueness under the key is the caller's duty, and a replay must
    bring new nonces**: that is why the nonces are no part of the plan but a
    device ``uint8 [n, 12]`` tensor handed to every run (a captured graph reads
    the tensor's contents at replay: change them in place).

    xs / outs: GPU tensors (contiguous, 16-byte aligned; ``outs[i] is xs[i]``
    for in place), 0 .. 1 MiB each, any byte count -- larger messages belong to
    ``ocb_encrypt``.  Distinct records must not overlap, and no input may
    overlap another record's output.  key: 16, 24 or 32 bytes.  aads: ``None``,
    a device ``uint8 [n, A]`` tensor (row m is record m's AAD), or a list with
    one entry per record: a device tensor or host bytes (uploaded once with the
    plan), 0 .. 64 KiB each, any alignment; no AAD may overlap any record's
    output.  A record of 0 bytes is valid, with AAD or without.

    ``tags`` and ``ok`` are the batch's own tensors, overwritten by the next
    run; ``decrypt`` therefore refuses ``self.tags`` as the expected tags."""

    def __init__(self, xs, key, outs=None, aads=None):
        import numpy as np
        self._init_common(key)
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
        for i, pi, po, nb in _tensor_descs(xs, outs, self.device, "record"):
            if nb > OCB_BATCH_MAX_BYTES:
                raise ValueError(f"record {i}: more than 1 MiB of data (use ocb_encrypt for large messages)")
            desc[i, :3] = (pi if nb else 0, po if nb else 0, nb)
        _set_aads(desc, aads, self.device, self._keep)
        self._build(desc)

    @classmethod
    def packed(cls, buf: torch.Tensor, lengths, key, out: torch.Tensor | None = None, offsets=None,
               aad=None) -> "OcbBatch":
        """Records packed in ONE device buffer, ``CtrBatch.packed``'s layout:
        record i is ``buf[offsets[i] : offsets[i] + lengths[i]]`` (offsets
        default to back-to-back 16-byte aligned slots) and lands at the same
        offset of ``out`` (default: a new buffer; ``out is buf`` for in
        place).  aad: ``None`` or a device ``uint8 [n, A]`` tensor.  Bytes of
        ``out`` outside the records are not written.  The output is
        ``self.out``."""
        self = cls.__new__(cls)
        self._init_common(key)
        _check_dev(buf, "buf")
        lens, offs = _packed_layout(buf, lengths, offsets, "record")
        if lens.size and (lens > OCB_BATCH_MAX_BYTES).any():
            raise ValueError("a record has at most 1 MiB of data (use ocb_encrypt for large messages)")
        out, desc = _packed_buffers(buf, out, lens, offs)
        self.out = out
        self.outs = [out]
        self._keep = [buf]
        self.device = buf.device
        if aad is not None and not isinstance(aad, torch.Tensor):
            raise ValueError("aad must be a device uint8 [n, A] tensor")
        _set_aads(desc, aad, self.device, self._keep)
        self._build(desc)
        return self

    def _init_common(self, key):
        key = bytes(key)
        if len(key) not in (16, 24, 32):
            raise ValueError(f"AES key must be 16, 24 or 32 bytes, got {len(key)}")
        self._key = _ocb_key(key)
        self.n = 0
        self.ntiles = 0
        self.tags = self.ok = None

    def _build(self, desc):
        """Planner (validation + the bulk kernel's tile map) -> one pinned
        upload; workspace, tags, verdicts."""
        import numpy as np
        self.n = n = desc.shape[0]
        if n == 0:
            return
        lib = _lib()
        desc = np.ascontiguousarray(desc)
        ntiles = lib.otc_ocb_batch_plan(desc.ctypes.data, n, None, None)
        if ntiles < 0:
            raise ValueError((lib.otc_last_error() or b"").decode())
        first = np.zeros(n, dtype=np.uint64)
        tmap = np.zeros(max(ntiles, 1), dtype=np.uint32)
        if lib.otc_ocb_batch_plan(desc.ctypes.data, n, tmap.ctypes.data, first.ctypes.data) != ntiles:
            raise RuntimeError("otc_ocb_batch_plan: the two passes disagree")
        blob = _Blob()
        self._o_desc = blob.add(desc.tobytes())
        self._o_first = blob.add(first.tobytes())
        self._o_map = blob.add(tmap.tobytes())
        self.ntiles = int(ntiles)
        dev = self.device
        with torch.cuda.device(dev):
            self._plan = blob.upload(dev)
            self._ws = torch.empty(lib.otc_ocb_batch_ws_bytes(n), dtype=torch.uint8, device=dev)
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
            raise ValueError(f"a batched OCB nonce has 12 bytes (got {nonces.shape[1]}; other lengths: ocb_encrypt)")
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
            rc = _lib().otc_aes_ocb_batch(
                base + self._o_desc, base + self._o_map, base + self._o_first, self.ntiles, self.n,
                ctypes.byref(self._key), DECRYPT if decrypt else ENCRYPT, nonces.data_ptr(), self.tags.data_ptr(),
                expect.data_ptr() if decrypt else None, self.ok.data_ptr() if decrypt else None,
                self._ws.data_ptr(), ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_aes_ocb_batch")

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device or "cpu")

    def encrypt(self, nonces: torch.Tensor, stream=None):
        """Seal every record under ``nonces`` (device uint8 [n, 12]):
        ``(outs, tags)``, the tags a device uint8 [n, 16] tensor.  Only
        launches; every call must bring nonces never used under the key."""
        self._check_nonces(nonces)
        self._launch(False, nonces, None, stream)
        return self.outs, (self.tags if self.n else self._empty((0, 16), torch.uint8))

    def decrypt(self, nonces: torch.Tensor, tags: torch.Tensor, stream=None):
        """Open every record: ``(outs, ok)`` with ``ok`` a device bool [n]
        tensor.  tags: the received tags, device uint8 [n, 16].  OCB's
        checksum is over the plaintext, so every record is decrypted first;
        the comparison runs on the device, and the output of every record
        whose tag does not match is zeroed (in place: the ciphertext with it)
        and so is its row of ``self.tags``; the others are unaffected.
        Nothing is read back.  ``tags`` must not be (or overlap) the batch's
        own ``self.tags`` / ``self.ok``, which every run overwrites with what
        it computes: pass a copy (``ValueError`` otherwise)."""
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

    @staticmethod
    def spans() -> list[int]:
        """The bulk kernel's boundaries in bytes, smallest first (otc.h
        otc_ocb_batch_spans): a block, a slot, a wave pass, a workgroup step
        and the full grid's first step."""
        return _spans("otc_ocb_batch_spans")


def ocb_batch_spans() -> list[int]:
    """``OcbBatch.spans()``."""
    return OcbBatch.spans()


def ocb_encrypt_batch(xs, key, nonces: torch.Tensor, aads=None, outs=None):
    """Plan and run an ``OcbBatch`` once: ``(outs, tags)``."""
    return OcbBatch(xs, key, outs=outs, aads=aads).encrypt(nonces)


def ocb_decrypt_batch(xs, key, nonces: torch.Tensor, tags: torch.Tensor, aads=None, outs=None):
    """Plan and run an ``OcbBatch`` once: ``(outs, ok)``."""
    return OcbBatch(xs, key, outs=outs, aads=aads).decrypt(nonces, tags)
