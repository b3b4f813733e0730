"""``GcmSivBatch``: a planned batch of AES-GCM-SIV records (RFC 8452), all under
one key-generating key, each with its own 12-byte nonce, AAD and 16-byte tag,
backed by the gfx950 kernels of ``csrc/hip/aes_gcm_siv_batch.hip``
(``otc_aes_gcm_siv_batch``), the plan-and-run-once functions around it, and the
two halves by themselves (``polyval_batch``, ``ctr_le32_batch``).

The names of this module are not in ``ops.__all__`` yet (reach them as
``ops.gcm_siv_batch_ops.GcmSivBatch`` or through ``models.AES``).  The contract,
the checks and their error texts are ``OcbBatch``'s -- the class derives from it
-- and the planning pieces (packed layout, descriptors, AAD columns, the pinned
upload) are ``batch_ops``'s."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from ._common import _check_dev, _lib, _spans
from .batch_ops import _Blob, _packed_buffers, _packed_layout, _set_aads, _tensor_descs
from .gcm_siv_ops import _siv_key
from .keys import DECRYPT, ENCRYPT, expand_key
from .ocb_batch_ops import OcbBatch

GCM_SIV_BATCH_MAX_BYTES = 1 << 20  # otc.h OTC_GCM_SIV_BATCH_MAX_BYTES


def _plan(desc):
    """Planner (validation + the counter kernel's tile map) over host descriptors: ``(ntiles, tile_msg, tile_first)``."""
    import numpy as np
    lib = _lib()
    n = desc.shape[0]
    ntiles = lib.otc_gcm_siv_batch_plan(desc.ctypes.data, n, None, None)
    if ntiles < 0:
        raise ValueError((lib.otc_last_error() or b"").decode())
    first = np.zeros(n, dtype=np.uint64)
    tmap = np.zeros(max(ntiles, 1), dtype=np.uint32)
    if lib.otc_gcm_siv_batch_plan(desc.ctypes.data, n, tmap.ctypes.data, first.ctypes.data) != ntiles:
        raise RuntimeError("otc_gcm_siv_batch_plan: the two passes disagree")
    return int(ntiles), tmap, first


class GcmSivBatch(OcbBatch):
    """A planned batch of AES-GCM-SIV records -- own buffers, own 12-byte
    nonce, own AAD and own 16-byte tag each, ONE key-generating key for the
    batch (``otc_aes_gcm_siv_batch``).  Record ``m`` is RFC 8452 AES-GCM-SIV
    under ``(key, nonces[m], aads[m])`` and equals
    ``gcm_siv_ops.gcm_siv_encrypt`` on that record alone, byte for byte, tag
    included.

    One ``gcm_siv_encrypt`` per record pays the key derivation, a key expansion
    and the AAD's hash on the host, an allocation, the hash tables and four or
    more launches each time; here planning -- validation, descriptors, the
    counter kernel's tile map, the workspace, one pinned upload -- happens once
    in the constructor, every record's two keys are derived and expanded on the
    device, and ``encrypt`` / ``decrypt`` only launch one linear chain of
    kernels on one stream: no allocation, no host synchronisation, capturable
    in a ``torch.cuda.CUDAGraph``.  They can be replayed with new data in the
    same buffers.

    GCM-SIV keeps its promise when a nonce repeats (a repeat shows only whether
    two records were equal), but fresh nonces are still what a caller should
    bring: the nonces are no part of the plan but a device ``uint8 [n, 12]``
    tensor handed to every run (a captured graph reads the tensor's contents at
    replay: change them in place).

    xs / outs: GPU tensors (contiguous, 16-byte aligned; ``outs[i] is xs[i]``
    for in place), 0 .. 1 MiB each, any byte count -- larger messages belong to
    ``gcm_siv_encrypt``.  Distinct records must not overlap, and no input may
    overlap another record's output.  key: 16 or 32 bytes.  aads: as
    ``OcbBatch``'s.  A record of 0 bytes is valid, with AAD or without.  lanes:
    16 or 64 lanes of the hash kernel per record (``None``: chosen from the
    record sizes, ``otc_gcm_siv_batch_lanes``); both compute the same.

    ``tags`` and ``ok`` are the batch's own tensors, overwritten by the next
    run; ``decrypt`` therefore refuses ``self.tags`` as the expected tags.  The
    workspace holds every record's derived keys after a run; it is zeroed when
    the batch is collected only if the caller calls ``wipe_keys()``."""

    def __init__(self, xs, key, outs=None, aads=None, lanes=None):
        import numpy as np
        self._init_common(key, lanes)
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
            if nb > GCM_SIV_BATCH_MAX_BYTES:
                raise ValueError(f"record {i}: more than 1 MiB of data (use gcm_siv_encrypt for large messages)")
            desc[i, :3] = (pi if nb else 0, po if nb else 0, nb)
        _set_aads(desc, aads, self.device, self._keep)
        self._build(desc)

    @classmethod
    def packed(cls, buf: torch.Tensor, lengths, key, out: torch.Tensor | None = None, offsets=None,
               aad=None, lanes=None) -> "GcmSivBatch":
        """Records packed in ONE device buffer, ``CtrBatch.packed``'s layout:
        record i is ``buf[offsets[i] : offsets[i] + lengths[i]]`` (offsets
        default to back-to-back 16-byte aligned slots) and lands at the same
        offset of ``out`` (default: a new buffer; ``out is buf`` for in
        place).  aad: ``None`` or a device ``uint8 [n, A]`` tensor.  Bytes of
        ``out`` outside the records are not written.  The output is
        ``self.out``."""
        self = cls.__new__(cls)
        self._init_common(key, lanes)
        _check_dev(buf, "buf")
        lens, offs = _packed_layout(buf, lengths, offsets, "record")
        if lens.size and (lens > GCM_SIV_BATCH_MAX_BYTES).any():
            raise ValueError("a record has at most 1 MiB of data (use gcm_siv_encrypt for large messages)")
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

    def _init_common(self, key, lanes=None):
        key = bytes(key)
        if len(key) not in (16, 32):
            raise ValueError(f"an AES-GCM-SIV key has 16 or 32 bytes, got {len(key)}")
        if lanes not in (None, 16, 64):
            raise ValueError("lanes must be 16 or 64")
        self._key = _siv_key(key)
        self.lanes = lanes
        self.n = 0
        self.ntiles = 0
        self.tags = self.ok = None

    def _build(self, desc):
        """Planner -> one pinned upload; workspace, tags, verdicts."""
        import numpy as np
        self.n = n = desc.shape[0]
        if n == 0:
            return
        lib = _lib()
        desc = np.ascontiguousarray(desc)
        ntiles, tmap, first = _plan(desc)
        if self.lanes is None:
            self.lanes = lib.otc_gcm_siv_batch_lanes(desc.ctypes.data, n)
        blob = _Blob()
        self._o_desc = blob.add(desc.tobytes())
        self._o_first = blob.add(first.tobytes())
        self._o_map = blob.add(tmap.tobytes())
        self.ntiles = ntiles
        dev = self.device
        with torch.cuda.device(dev):
            self._plan = blob.upload(dev)
            self._ws = torch.empty(lib.otc_gcm_siv_batch_ws_bytes(n), dtype=torch.uint8, device=dev)
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
            raise ValueError(f"an AES-GCM-SIV nonce has exactly 12 bytes (got {nonces.shape[1]})")
        if nonces.shape[0] != self.n:
            raise ValueError(f"one nonce per record: nonces must be [{self.n}, 12]")
        if self.n and nonces.device != self.device:
            raise ValueError("nonces must be on the records' device")

    def _launch(self, decrypt, nonces, expect, stream):
        if self.n == 0:
            return
        if decrypt and expect.data_ptr() % 4:
            raise ValueError("tags must be 4-byte aligned: the counter kernel reads them where they lie")
        st = stream or torch.cuda.current_stream(self.device)
        base = self._plan.data_ptr()
        with torch.cuda.device(self.device):
            rc = _lib().otc_aes_gcm_siv_batch(
                base + self._o_desc, base + self._o_map, base + self._o_first, self.ntiles, self.n,
                ctypes.byref(self._key), DECRYPT if decrypt else ENCRYPT, nonces.data_ptr(), self.tags.data_ptr(),
                expect.data_ptr() if decrypt else None, self.ok.data_ptr() if decrypt else None,
                self._ws.data_ptr(), self.lanes, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_aes_gcm_siv_batch")

    def encrypt(self, nonces: torch.Tensor, stream=None):
        """Seal every record under ``nonces`` (device uint8 [n, 12]):
        ``(outs, tags)``, the tags a device uint8 [n, 16] tensor.  Only
        launches.  The hash runs over the plaintext first; the tags it ends in
        are the counter kernel's starting blocks and stay on the device."""
        return super().encrypt(nonces, stream)

    def decrypt(self, nonces: torch.Tensor, tags: torch.Tensor, stream=None):
        """Open every record: ``(outs, ok)`` with ``ok`` a device bool [n]
        tensor.  tags: the received tags, device uint8 [n, 16]; the counter
        kernel starts from them.  GCM-SIV's hash is over the plaintext, so
        every record is decrypted first; the comparison runs on the device, and
        the output of every record whose tag does not match is zeroed (in
        place: the ciphertext with it) and so is its row of ``self.tags``; the
        others are unaffected.  Nothing is read back.  ``tags`` must not be (or
        overlap) the batch's own ``self.tags`` / ``self.ok``, which every run
        overwrites with what it computes: pass a copy (``ValueError``
        otherwise)."""
        return super().decrypt(nonces, tags, stream)

    def wipe_keys(self):
        """Zero the workspace (every record's derived keys), in stream order."""
        if self.n:
            self._ws.zero_()

    @staticmethod
    def spans() -> list[int]:
        """The batched POLYVAL kernel's own boundaries in hashed blocks (AAD,
        data and length block together), smallest first (otc.h
        otc_gcm_siv_batch_spans)."""
        return _spans("otc_gcm_siv_batch_spans")


def gcm_siv_batch_spans() -> list[int]:
    """``GcmSivBatch.spans()``."""
    return GcmSivBatch.spans()


def gcm_siv_encrypt_batch(xs, key, nonces: torch.Tensor, aads=None, outs=None):
    """Plan and run a ``GcmSivBatch`` once: ``(outs, tags)``."""
    return GcmSivBatch(xs, key, outs=outs, aads=aads).encrypt(nonces)


def gcm_siv_decrypt_batch(xs, key, nonces: torch.Tensor, tags: torch.Tensor, aads=None, outs=None):
    """Plan and run a ``GcmSivBatch`` once: ``(outs, ok)``."""
    return GcmSivBatch(xs, key, outs=outs, aads=aads).decrypt(nonces, tags)


def _descs(xs, outs, aads, keep):
    """Host descriptors of records that are only read (outs None) or run through the counter mode."""
    import numpy as np
    xs = list(xs)
    device = xs[0].device if xs else None
    desc = np.zeros((len(xs), 6), dtype=np.uint64)
    for i, pi, po, nb in _tensor_descs(xs, xs if outs is None else outs, device, "record"):
        if nb > GCM_SIV_BATCH_MAX_BYTES:
            raise ValueError(f"record {i}: more than 1 MiB of data")
        desc[i, :3] = (pi if nb else 0, po if nb else 0, nb)
    _set_aads(desc, aads, device, keep)
    return np.ascontiguousarray(desc), device


def _rows(t, n, width, name, device, align):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{name} must be a GPU tensor, uint8 [n, {width}]")
    if t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (n, width):
        raise ValueError(f"{name} must be a contiguous uint8 [{n}, {width}] tensor")
    if n and t.device != device:
        raise ValueError(f"{name} must be on the records' device")
    if t.data_ptr() % align:
        raise ValueError(f"{name} must be {align}-byte aligned")


def polyval_batch(xs, hs: torch.Tensor, aads=None, lanes=None) -> torch.Tensor:
    """The hash half by itself (``otc_polyval_batch``): a device uint8 [n, 16]
    tensor, row m the POLYVAL under the key ``hs[m]`` (device uint8 [n, 16]) of
    record m's ``pad16(AAD) || pad16(data) || le64(8 aad) le64(8 n)``.  lanes:
    16 or 64 per record (``None``: chosen from the sizes)."""
    keep = []
    desc, device = _descs(xs, None, aads, keep)
    n = desc.shape[0]
    if lanes not in (None, 16, 64):
        raise ValueError("lanes must be 16 or 64")
    _rows(hs, n, 16, "hs", device, 16)
    if n == 0:
        return torch.empty((0, 16), dtype=torch.uint8)
    lib = _lib()
    _plan(desc)  # the planner's checks
    if lanes is None:
        lanes = lib.otc_gcm_siv_batch_lanes(desc.ctypes.data, n)
    blob = _Blob()
    o = blob.add(desc.tobytes())
    with torch.cuda.device(device):
        plan = blob.upload(device)
        s = torch.empty((n, 16), dtype=torch.uint8, device=device)
        st = torch.cuda.current_stream(device)
        rc = lib.otc_polyval_batch(plan.data_ptr() + o, n, hs.data_ptr(), s.data_ptr(), lanes,
                                   ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_polyval_batch")
        plan.record_stream(st)
    return s


def ctr_le32_batch(xs, keys, ctrs: torch.Tensor, outs=None):
    """The counter half by itself (``otc_aes_ctr_le32_batch``): record m's
    output is its input XOR the keystream of GCM-SIV's counter mode under
    ``keys[m]`` (a list of n keys of ONE size, 16, 24 or 32 bytes) from the
    counter block ``ctrs[m]`` (device uint8 [n, 16], read where it lies in
    stream order): bytes 0..3 count little-endian modulo 2**32 without carry,
    bit 7 of byte 15 is forced on.  Returns ``outs`` (new tensors by default;
    ``outs[i] is xs[i]`` for in place)."""
    import numpy as np
    xs = list(xs)
    keys = [bytes(k) for k in keys]
    if len(keys) != len(xs):
        raise ValueError("one key per record")
    if len({len(k) for k in keys}) > 1 or any(len(k) not in (16, 24, 32) for k in keys):
        raise ValueError("the keys of a batch have one size: 16, 24 or 32 bytes")
    if outs is None:
        outs = [torch.empty_like(x) for x in xs]
    outs = list(outs)
    if len(outs) != len(xs):
        raise ValueError("one output per record")
    keep = []
    desc, device = _descs(xs, outs, None, keep)
    n = desc.shape[0]
    _rows(ctrs, n, 16, "ctrs", device, 4)
    if n == 0:
        return outs
    ntiles, tmap, first = _plan(desc)
    sched = [expand_key(k) for k in keys]
    blob = _Blob()
    o_desc = blob.add(desc.tobytes())
    o_keys = blob.add(b"".join(bytes(s) for s in sched))
    o_first = blob.add(first.tobytes())
    o_map = blob.add(tmap.tobytes())
    with torch.cuda.device(device):
        plan = blob.upload(device)
        base = plan.data_ptr()
        st = torch.cuda.current_stream(device)
        rc = _lib().otc_aes_ctr_le32_batch(base + o_desc, base + o_keys, ctrs.data_ptr(), base + o_map, base + o_first,
                                           ntiles, n, sched[0].nr, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_aes_ctr_le32_batch")
        plan.record_stream(st)
    return outs
