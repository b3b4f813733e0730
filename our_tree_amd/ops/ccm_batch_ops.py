"""``CcmBatch``: a planned batch of AES-CCM records (NIST SP 800-38C, RFC 3610),
all under one key, each with its own nonce, AAD and tag, backed by the gfx950
kernel of ``csrc/hip/aes_ccm_batch.hip`` (``otc_aes_ccm_batch``), the
plan-and-run-once functions around it and the single-message calls, which are a
batch of one.

The names of this module are not in ``ops.__all__`` yet (reach them as
``ops.ccm_batch_ops.CcmBatch`` or through ``models.AES``); the planning pieces
-- packed layout, descriptors, AAD columns, the pinned upload -- are
``batch_ops``'s."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from ..models.cpu_ref import CcmTagError, ccm_check
from ._common import _check_dev, _lib, _nbytes, _spans
from .batch_ops import _Blob, _packed_buffers, _packed_layout, _set_aads, _tensor_descs
from .keys import DECRYPT, ENCRYPT, expand_key

CCM_BATCH_MAX_BYTES = 1 << 20  # otc.h OTC_CCM_BATCH_MAX_BYTES


class CcmBatch:
    """A planned batch of AES-CCM records -- own buffers, own nonce, own AAD and
    own tag each; ONE key, ONE nonce length (``nonce_bytes``, 7 .. 13) and ONE
    tag length (``tag_bytes``: 4, 6, .., 16) for the batch
    (``otc_aes_ccm_batch``).  Record ``m`` is SP 800-38C / RFC 3610 CCM under
    ``(key, nonces[m], aads[m])`` and equals ``cpu_ref.ccm`` on that record
    alone, byte for byte.

    CCM's tag is a CBC-MAC, one serial chain per record, so the kernel runs ONE
    RECORD PER LANE -- the only parallelism is across records -- with the MAC's
    and the counter mode's cipher calls as two blocks in flight, and reads the
    data once.  The planner sorts the records by block count, longest first, so
    that the lanes of a wave end together (``self.order``; the records, their
    outputs, tags and verdicts keep the caller's order).  Planning --
    validation, descriptors, the order, one pinned upload -- happens once in the
    constructor; ``encrypt`` / ``decrypt`` only launch one linear chain of
    kernels on one stream: no allocation, no host synchronisation, capturable
    in a ``torch.cuda.CUDAGraph``.  They can be replayed with new data in the
    same buffers.

    **Nonce uniqueness under the key is the caller's duty, and a replay must
    bring new nonces**: that is why the nonces are no part of the plan but a
    device ``uint8 [n, nonce_bytes]`` tensor handed to every run (a captured
    graph reads the tensor's contents at replay: change them in place).

    xs / outs: GPU tensors (contiguous, 16-byte aligned; ``outs[i] is xs[i]``
    for in place), 0 .. 1 MiB each and fewer than ``2**(8 * (15 -
    nonce_bytes))`` bytes (65535 at most under a 13-byte nonce), any byte
    count.  Distinct records must not overlap, and no input may overlap another
    record's output.  key: 16, 24 or 32 bytes.  aads: ``None``, a device
    ``uint8 [n, A]`` tensor (row m is record m's AAD), or a list with one entry
    per record: a device tensor or host bytes (uploaded once with the plan),
    0 .. 64 KiB each, any alignment; no AAD may overlap any record's output.  A
    record of 0 bytes is valid, with AAD or without.

    ``tags`` and ``ok`` are the batch's own tensors, overwritten by the next
    run; ``decrypt`` therefore refuses ``self.tags`` as the expected tags."""

    def __init__(self, xs, key, outs=None, aads=None, nonce_bytes: int = 12, tag_bytes: int = 16, _sort: bool = True):
        import numpy as np
        self._init_common(key, nonce_bytes, tag_bytes, _sort)
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
            if nb > CCM_BATCH_MAX_BYTES:
                raise ValueError(f"record {i}: more than 1 MiB of data")
            desc[i, :3] = (pi if nb else 0, po if nb else 0, nb)
        _set_aads(desc, aads, self.device, self._keep)
        self._build(desc)

    @classmethod
    def packed(cls, buf: torch.Tensor, lengths, key, out: torch.Tensor | None = None, offsets=None, aad=None,
               nonce_bytes: int = 12, tag_bytes: int = 16, _sort: bool = True) -> "CcmBatch":
        """Records packed in ONE device buffer, ``CtrBatch.packed``'s layout:
        record i is ``buf[offsets[i] : offsets[i] + lengths[i]]`` (offsets
        default to back-to-back 16-byte aligned slots) and lands at the same
        offset of ``out`` (default: a new buffer; ``out is buf`` for in
        place).  aad: ``None`` or a device ``uint8 [n, A]`` tensor.  Bytes of
        ``out`` outside the records are not written.  The output is
        ``self.out``."""
        self = cls.__new__(cls)
        self._init_common(key, nonce_bytes, tag_bytes, _sort)
        _check_dev(buf, "buf")
        lens, offs = _packed_layout(buf, lengths, offsets, "record")
        if lens.size and (lens > CCM_BATCH_MAX_BYTES).any():
            raise ValueError("a record has at most 1 MiB of data")
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

    def _init_common(self, key, nonce_bytes, tag_bytes, sort):
        key = bytes(key)
        if len(key) not in (16, 24, 32):
            raise ValueError(f"AES key must be 16, 24 or 32 bytes, got {len(key)}")
        ccm_check(nonce_bytes, tag_bytes)
        self.nonce_bytes, self.tag_bytes = nonce_bytes, tag_bytes
        self._key = expand_key(key)  # the encryption schedule: CCM never runs the inverse cipher
        self._sort = bool(sort)
        self.n = 0
        self.order = None
        self.tags = self.ok = None

    def _build(self, desc):
        """Planner (validation + the order) -> one pinned upload; tags, verdicts."""
        import numpy as np
        self.n = n = desc.shape[0]
        if n == 0:
            return
        lib = _lib()
        desc = np.ascontiguousarray(desc)
        order = np.zeros(n, dtype=np.uint32)
        if lib.otc_ccm_batch_plan(desc.ctypes.data, n, self.nonce_bytes, order.ctypes.data):
            raise ValueError((lib.otc_last_error() or b"").decode())
        if not self._sort:  # the A/B arm of benchmarks/ccm_batch.py: the records as given
            order = np.arange(n, dtype=np.uint32)
        self.order = order
        blob = _Blob()
        self._o_desc = blob.add(desc.tobytes())
        self._o_order = blob.add(order.tobytes())
        dev = self.device
        with torch.cuda.device(dev):
            self._plan = blob.upload(dev)
            self._ws = torch.empty(lib.otc_ccm_batch_ws_bytes(n), dtype=torch.uint8, device=dev)
            self.tags = torch.empty((n, self.tag_bytes), dtype=torch.uint8, device=dev)
            self.ok = torch.zeros(n, dtype=torch.uint8, device=dev)
            # planning may wait; the runs never do, on whatever stream (or capture) they go
            torch.cuda.current_stream(dev).synchronize()

    def _check_rows(self, t, width, what):
        if not isinstance(t, torch.Tensor) or (self.n and t.device.type != "cuda"):
            raise ValueError(f"{what} must be a GPU tensor, uint8 [n, {width}]")
        if t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous uint8 [n, {width}] tensor")
        if t.shape[1] != width:
            raise ValueError(f"this batch's {what} have {width} bytes each (got {t.shape[1]})")
        if t.shape[0] != self.n:
            raise ValueError(f"one row per record: {what} must be [{self.n}, {width}]")
        if self.n and t.device != self.device:
            raise ValueError(f"{what} must be on the records' device")

    def _launch(self, decrypt, nonces, expect, stream):
        if self.n == 0:
            return
        st = stream or torch.cuda.current_stream(self.device)
        base = self._plan.data_ptr()
        with torch.cuda.device(self.device):
            rc = _lib().otc_aes_ccm_batch(
                base + self._o_desc, base + self._o_order, self.n, ctypes.byref(self._key),
                DECRYPT if decrypt else ENCRYPT, nonces.data_ptr(), self.nonce_bytes, self.tags.data_ptr(),
                self.tag_bytes, expect.data_ptr() if decrypt else None, self.ok.data_ptr() if decrypt else None,
                self._ws.data_ptr() if self._ws.numel() else None, ctypes.c_void_p(st.cuda_stream))
        _native.check(rc, "otc_aes_ccm_batch")

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device or "cpu")

    def encrypt(self, nonces: torch.Tensor, stream=None):
        """Seal every record under ``nonces`` (device uint8 [n, nonce_bytes]):
        ``(outs, tags)``, the tags a device uint8 [n, tag_bytes] tensor.  Only
        launches; every call must bring nonces never used under the key."""
        self._check_rows(nonces, self.nonce_bytes, "nonces")
        self._launch(False, nonces, None, stream)
        return self.outs, (self.tags if self.n else self._empty((0, self.tag_bytes), torch.uint8))

    def decrypt(self, nonces: torch.Tensor, tags: torch.Tensor, stream=None):
        """Open every record: ``(outs, ok)`` with ``ok`` a device bool [n]
        tensor.  tags: the received tags, device uint8 [n, tag_bytes].  CCM's
        MAC is over the plaintext, so every record is decrypted first; the
        comparison runs on the device, and the output of every record whose
        tag does not match is zeroed (in place: the ciphertext with it) and so
        is its row of ``self.tags``; the others are unaffected.  Nothing is
        read back.  ``tags`` must not be (or overlap) the batch's own
        ``self.tags`` / ``self.ok``, which every run overwrites with what it
        computes: pass a copy (``ValueError`` otherwise)."""
        if self.n and isinstance(tags, torch.Tensor):  # first: whatever else is wrong, never the batch's own
            e0, e1 = tags.data_ptr(), tags.data_ptr() + _nbytes(tags)
            for own in (self.tags, self.ok):
                if e0 < own.data_ptr() + _nbytes(own) and own.data_ptr() < e1:
                    raise ValueError("tags overlaps the batch's own tags / verdicts, which this run overwrites: "
                                     "pass a copy (tags.clone())")
        self._check_rows(nonces, self.nonce_bytes, "nonces")
        self._check_rows(tags, self.tag_bytes, "tags")
        self._launch(True, nonces, tags, stream)
        return self.outs, (self.ok.view(torch.bool) if self.n else self._empty((0,), torch.bool))

    @staticmethod
    def spans() -> list[int]:
        """The kernel's boundaries, smallest first (otc.h otc_ccm_batch_spans):
        a block and a lane's burst in bytes; a wave, a workgroup and the full
        grid's first step in records."""
        return _spans("otc_ccm_batch_spans")


def ccm_batch_spans() -> list[int]:
    """``CcmBatch.spans()``."""
    return CcmBatch.spans()


def ccm_encrypt_batch(xs, key, nonces: torch.Tensor, aads=None, outs=None, tag_bytes: int = 16):
    """Plan and run a ``CcmBatch`` once: ``(outs, tags)``.  The nonce length is
    the width of ``nonces``."""
    return CcmBatch(xs, key, outs=outs, aads=aads, nonce_bytes=_width(nonces, "nonces"),
                    tag_bytes=tag_bytes).encrypt(nonces)


def ccm_decrypt_batch(xs, key, nonces: torch.Tensor, tags: torch.Tensor, aads=None, outs=None):
    """Plan and run a ``CcmBatch`` once: ``(outs, ok)``.  The nonce and tag
    lengths are the widths of ``nonces`` and ``tags``."""
    return CcmBatch(xs, key, outs=outs, aads=aads, nonce_bytes=_width(nonces, "nonces"),
                    tag_bytes=_width(tags, "tags")).decrypt(nonces, tags)


def _width(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{what} must be a GPU tensor, uint8 [n, bytes per record]")
    return int(t.shape[1])


def _one(x, key, nonce, aad, out, tag_bytes):
    _check_dev(x, "x")
    nonce = bytes(nonce)
    ccm_check(len(nonce), tag_bytes, _nbytes(x))
    if _nbytes(x) > CCM_BATCH_MAX_BYTES:
        raise ValueError("a CCM message has at most 1 MiB here: its MAC is one serial chain on one lane")
    b = CcmBatch([x], key, outs=None if out is None else [out], aads=[bytes(aad)], nonce_bytes=len(nonce),
                 tag_bytes=tag_bytes)
    n = torch.frombuffer(bytearray(nonce), dtype=torch.uint8).to(x.device).view(1, len(nonce))
    return b, n


def ccm_encrypt(x: torch.Tensor, key, nonce: bytes, aad: bytes = b"", out: torch.Tensor | None = None,
                tag_bytes: int = 16):
    """AES-CCM of ONE message on the GPU: ``(ciphertext, tag)``, the tag as
    ``tag_bytes`` host bytes.  A batch of one: a CCM message is one serial
    chain (its CBC-MAC), so it runs on one lane and nothing spreads it over
    the chip -- the limit is 1 MiB, and many messages belong in one
    ``CcmBatch``.  The nonce (7 .. 13 bytes) must never repeat under the key."""
    b, n = _one(x, key, nonce, aad, out, tag_bytes)
    outs, tags = b.encrypt(n)
    return outs[0], bytes(tags[0].cpu().numpy().tobytes())


def ccm_decrypt(x: torch.Tensor, key, nonce: bytes, tag: bytes, aad: bytes = b"", out: torch.Tensor | None = None):
    """Authenticated decryption of ONE message: the plaintext, or
    ``CcmTagError`` -- with the output zeroed -- when the received ``tag`` (its
    length is the message's tag length) does not match.  A batch of one, as
    ``ccm_encrypt``: one serial chain on one lane, 1 MiB at most; reads the
    verdict back."""
    tag = bytes(tag)
    b, n = _one(x, key, nonce, aad, out, len(tag))
    t = torch.frombuffer(bytearray(tag), dtype=torch.uint8).to(x.device).view(1, len(tag))
    outs, ok = b.decrypt(n, t)
    if not bool(ok[0].item()):
        err = CcmTagError("CCM tag mismatch")
        err.output = outs[0]
        raise err
    return outs[0]
