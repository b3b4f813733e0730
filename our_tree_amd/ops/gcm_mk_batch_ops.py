"""``GcmMkBatch``: a planned batch of AES-GCM records with a KEY PER RECORD
("mk": many keys) -- own 12-byte IV, own AAD and own tag each -- backed by the
gfx950 kernels of ``csrc/hip/aes_gcm_mk_batch.hip`` (``otc_aes_gcm_mk_batch``),
the plan-and-run-once functions around it, and the hash half by itself
(``ghash_mk_batch``).

The names of this module are not in ``ops.__all__`` yet (reach them as
``ops.gcm_mk_batch_ops.GcmMkBatch``).  The contract, the checks and their error
texts are ``GcmBatch``'s -- the class derives from it -- and the planning pieces
(packed layout, descriptors, key index, AAD columns, the pinned upload) are
``batch_ops``'s."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from ._common import _check_dev, _lib, _spans
from .batch_ops import (GCM_BATCH_MAX_BYTES, GcmBatch, _Blob, _key_index, _packed_buffers, _packed_layout, _set_aads,
                        _tensor_descs, _tile_blocks)
from .keys import DECRYPT, ENCRYPT, expand_key


def _schedules(keys):
    """The expanded encryption keys of a batch: one size for all of them."""
    keys = [bytes(k) for k in keys]
    if not keys:
        raise ValueError("a batch needs at least one key")
    if any(len(k) not in (16, 24, 32) for k in keys):
        raise ValueError("an AES key has 16, 24 or 32 bytes")
    if len({len(k) for k in keys}) > 1:
        raise ValueError("the keys of a batch have one size (16, 24 or 32 bytes): make one batch per key size")
    return [expand_key(k) for k in keys]


class GcmMkBatch(GcmBatch):
    """A planned batch of AES-GCM records, each under its OWN key -- own
    buffers, own 12-byte IV, own AAD and own tag each
    (``otc_aes_gcm_mk_batch``).  Record ``m`` is SP 800-38D GCM under
    ``(keys[key_index[m]], ivs[m], aads[m])`` and equals ``gcm_encrypt`` on
    that record alone, byte for byte, tag included.

    The serving shape of ``GcmBatch`` -- TLS records, ESP / QUIC packets,
    sealed sectors -- as a server sees it: from many connections, a key each.
    ``GcmBatch`` stays the faster class where one key covers the batch.
    Planning -- validation, descriptors, the CTR half's tile map, the key
    schedules, every key's hash tables (1792 bytes per key, built on the
    device), the workspace, one pinned upload -- happens once in the
    constructor; ``encrypt`` / ``decrypt`` only launch one linear chain of
    kernels on one stream: no allocation, no host synchronisation, capturable
    in a ``torch.cuda.CUDAGraph``.

    keys: AES keys of ONE size (16, 24 or 32 bytes; anything else is a
    ``ValueError`` -- a caller with two sizes makes two batches), selected per
    record by ``key_index`` (default: ``keys[i]`` for record i).  Everything
    else -- xs / outs, aads, ``tag_bytes``, ``tile_blocks``, ``lanes``, the IVs
    as a device ``uint8 [n, 12]`` tensor handed to every run, ``tags`` and
    ``ok`` as the batch's own tensors -- is ``GcmBatch``'s.  **IV uniqueness
    under each key is the caller's duty.**

    The plan's schedule array and the table image on the device hold key
    material; ``wipe_keys()`` zeroes them."""

    def __init__(self, xs, keys, key_index=None, outs=None, aads=None, tag_bytes: int = 16, tile_blocks=None,
                 lanes=None):
        import numpy as np
        self._init_common(keys, tag_bytes, lanes)
        xs = list(xs)
        n = len(xs)
        kidx = _key_index(key_index, n, self.nkeys)
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
            if nb > GCM_BATCH_MAX_BYTES:
                raise ValueError(f"record {i}: more than 1 MiB of data (use gcm_encrypt for large messages)")
            desc[i, :3] = (pi if nb else 0, po if nb else 0, nb)
        desc[:, 5] = kidx.astype(np.uint64)
        self._set_aads(desc, aads)
        self._build(desc, tile_blocks)

    @classmethod
    def packed(cls, buf: torch.Tensor, lengths, keys, key_index=None, out: torch.Tensor | None = None, offsets=None,
               aad=None, tag_bytes: int = 16, tile_blocks=None, lanes=None) -> "GcmMkBatch":
        """Records packed in ONE device buffer, ``GcmBatch.packed``'s layout
        and arguments, with ``keys`` / ``key_index`` as in the constructor."""
        import numpy as np
        self = cls.__new__(cls)
        self._init_common(keys, tag_bytes, lanes)
        kidx = _key_index(key_index, np.asarray(lengths).size, self.nkeys)
        _check_dev(buf, "buf")
        lens, offs = _packed_layout(buf, lengths, offsets, "record")
        if lens.size and (lens > GCM_BATCH_MAX_BYTES).any():
            raise ValueError("a record has at most 1 MiB of data (use gcm_encrypt for large messages)")
        out, desc = _packed_buffers(buf, out, lens, offs)
        desc[:, 5] = kidx.astype(np.uint64)
        self.out = out
        self.outs = [out]
        self._keep = [buf]
        self.device = buf.device
        if aad is not None and not isinstance(aad, torch.Tensor):
            raise ValueError("aad must be a device uint8 [n, A] tensor")
        self._set_aads(desc, aad)
        self._build(desc, tile_blocks)
        return self

    def _init_common(self, keys, tag_bytes, lanes):
        if not isinstance(tag_bytes, int) or not 4 <= tag_bytes <= 16:
            raise ValueError("a GCM tag has 4 to 16 bytes")
        if lanes not in (None, 16, 64):
            raise ValueError("lanes must be 16 or 64 (default: picked from the record sizes)")
        self.tag_bytes = tag_bytes
        self.lanes = lanes
        self._sched = _schedules(keys)
        self.nkeys = len(self._sched)
        self.nr = self._sched[0].nr
        self.n = 0
        self.ntiles = 0
        self.tags = self.ok = None

    def _build(self, desc, tile_blocks):
        """Planner (validation + the CTR half's tile map) -> one pinned upload;
        the keys' hash tables; workspace, tags, verdicts."""
        import numpy as np
        self.n = n = desc.shape[0]
        self.tile_blocks = tile_blocks = _tile_blocks(tile_blocks, desc[:, 2])
        if n == 0:
            return
        lib = _lib()
        desc = np.ascontiguousarray(desc)
        ntiles = lib.otc_gcm_mk_batch_plan(desc.ctypes.data, n, self.nkeys, tile_blocks, None, None, None)
        if ntiles < 0:
            raise ValueError((lib.otc_last_error() or b"").decode())
        ctr = np.zeros((n, 6), dtype=np.uint64)
        first = np.zeros(n, dtype=np.uint64)
        tmap = np.zeros(max(ntiles, 1), dtype=np.uint32)
        if lib.otc_gcm_mk_batch_plan(desc.ctypes.data, n, self.nkeys, tile_blocks, ctr.ctypes.data, tmap.ctypes.data,
                                     first.ctypes.data) != ntiles:
            raise RuntimeError("otc_gcm_mk_batch_plan: the two passes disagree")
        if self.lanes is None:
            self.lanes = lib.otc_gcm_mk_batch_lanes(desc.ctypes.data, n)
        blob = _Blob()
        self._o_desc = blob.add(desc.tobytes())
        self._o_ctr = blob.add(ctr.tobytes())
        self._o_first = blob.add(first.tobytes())
        self._o_map = blob.add(tmap.tobytes())
        self.ntiles = int(ntiles)
        dev = self.device
        with torch.cuda.device(dev):
            self._plan = blob.upload(dev)
            # otc_aes_key[nkeys]: the CTR half and the finisher read round keys from memory
            self._keys = torch.empty(256 * self.nkeys, dtype=torch.uint8, device=dev)
            self._tab = torch.empty(lib.otc_gcm_mk_batch_table_bytes(self.nkeys), dtype=torch.uint8, device=dev)
            self._ws = torch.empty(lib.otc_gcm_mk_batch_ws_bytes(n), dtype=torch.uint8, device=dev)
            self.tags = torch.empty((n, 16), dtype=torch.uint8, device=dev)
            self.ok = torch.zeros(n, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev)
            self._upload_keys(st)
            # planning may wait; the runs never do, on whatever stream (or capture) they go
            st.synchronize()

    def _upload_keys(self, st):
        """The schedules by one copy, then the table kernel, in the order of ``st``."""
        host = torch.frombuffer(bytearray(b"".join(bytes(k) for k in self._sched)), dtype=torch.uint8).pin_memory()
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            self._keys.copy_(host, non_blocking=True)
            rc = _lib().otc_gcm_mk_batch_tables(self._keys.data_ptr(), self.nkeys, self.nr, self._tab.data_ptr(),
                                                ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_gcm_mk_batch_tables")
        self._keys_host = host  # pinned: alive until the copy has run

    def rekey(self, keys, stream=None):
        """New keys for the same plan: as many as before and of the same size
        (``ValueError`` otherwise).  One copy of the schedules and the table
        kernel, in stream order; nothing is replanned, and runs queued on the
        stream before this call still use the old keys."""
        sched = _schedules(keys)
        if len(sched) != self.nkeys or sched[0].nr != self.nr:
            raise ValueError(f"rekey takes {self.nkeys} keys of the batch's size")
        self._sched = sched
        if self.n:
            self._upload_keys(stream or torch.cuda.current_stream(self.device))

    def wipe_keys(self):
        """Zero the schedule array and the table image on the device, in stream order."""
        if self.n:
            self._keys.zero_()
            self._tab.zero_()

    def _launch(self, decrypt, ivs, expect, stream):
        if self.n == 0:
            return
        st = stream or torch.cuda.current_stream(self.device)
        base = self._plan.data_ptr()
        with torch.cuda.device(self.device):
            rc = _lib().otc_aes_gcm_mk_batch(
                base + self._o_desc, base + self._o_ctr, base + self._o_map, base + self._o_first, self.ntiles,
                self.tile_blocks, self.n, self._keys.data_ptr(), self.nkeys, self.nr, self._tab.data_ptr(),
                DECRYPT if decrypt else ENCRYPT, ivs.data_ptr(), self.tags.data_ptr(),
                expect.data_ptr() if decrypt else None, self.tag_bytes, self.ok.data_ptr() if decrypt else None,
                self._ws.data_ptr(), self.lanes, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_aes_gcm_mk_batch")

    def ghash(self, stream=None) -> torch.Tensor:
        """The hash half by itself (``otc_ghash_mk_batch``): a device uint8
        [n, 16] tensor, row m the GHASH under the hash subkey of record m's
        key of ``pad16(AAD) || pad16(input) || lengths``."""
        if self.n == 0:
            return self._empty((0, 16), torch.uint8)
        st = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            s = torch.empty((self.n, 16), dtype=torch.uint8, device=self.device)
            rc = _lib().otc_ghash_mk_batch(self._plan.data_ptr() + self._o_desc, self.n, self._tab.data_ptr(),
                                           s.data_ptr(), self.lanes, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_ghash_mk_batch")
        return s

    @staticmethod
    def spans() -> list[int]:
        """The batched hash kernel's own boundaries in hashed blocks (AAD, data
        and length block together), smallest first (otc.h
        otc_gcm_mk_batch_spans)."""
        return _spans("otc_gcm_mk_batch_spans")


def gcm_mk_batch_spans() -> list[int]:
    """``GcmMkBatch.spans()``."""
    return GcmMkBatch.spans()


def ghash_mk_batch(xs, keys, key_index=None, aads=None, lanes=None) -> torch.Tensor:
    """GHASH of every record of a batch under its own key's hash subkey,
    length block included: device uint8 [n, 16] (the hash kernel of
    ``GcmMkBatch`` alone)."""
    xs = list(xs)
    return GcmMkBatch(xs, keys, key_index=key_index, outs=xs, aads=aads, lanes=lanes).ghash()


def gcm_mk_encrypt_batch(xs, keys, ivs: torch.Tensor, key_index=None, aads=None, outs=None):
    """Plan and run a ``GcmMkBatch`` once: ``(outs, tags)``."""
    return GcmMkBatch(xs, keys, key_index=key_index, outs=outs, aads=aads).encrypt(ivs)


def gcm_mk_decrypt_batch(xs, keys, ivs: torch.Tensor, tags: torch.Tensor, key_index=None, aads=None, outs=None):
    """Plan and run a ``GcmMkBatch`` once: ``(outs, ok)``; the tag length is
    ``tags.shape[1]``."""
    tb = int(tags.shape[1]) if isinstance(tags, torch.Tensor) and tags.dim() == 2 else 16
    return GcmMkBatch(xs, keys, key_index=key_index, outs=outs, aads=aads, tag_bytes=tb).decrypt(ivs, tags)
