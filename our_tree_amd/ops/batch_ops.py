"""Planned batches of small messages: ``CtrBatch`` (AES-CTR, own key and
counter each, ``csrc/hip/aes_tt.hip``) and ``GcmBatch`` (AES-GCM records under
one key, ``csrc/hip/aes_gcm_batch.hip``), and the planning pieces they share:
the packed-buffer layout, the per-tensor descriptors, the key index, the AAD
columns and the plan's pinned upload (``chacha_batch_ops`` uses them too)."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from ._common import _check_dev, _lib, _nbytes, _out_like, _spans
from .gcm_ops import _gcm_key
from .keys import DECRYPT, ENCRYPT, expand_key

BATCH_TILES = (256, 128, 64)  # tile sizes in blocks the batch kernel supports (otc.h)
BATCH_ALIGNED = 0x80000000  # otc.h OTC_BATCH_ALIGNED
BATCH_ALIGN_MIN_TILES = 6  # counter-aligned tiling pays once (n+1) x 133 < n x 160 lookups
# relative cost per tile block slot, measured on MI355X with 16384 x 4 KiB
# messages (960 / 946 / 910 GB/s at 256 / 128 / 64 blocks per tile,
# profiles/r1/batch_ctr_tiles.jsonl): fewer blocks per lane hide less LDS latency
BATCH_TILE_COST = {256: 1.0, 128: 1.015, 64: 1.055}

GCM_BATCH_MAX_BYTES = 1 << 20  # otc.h OTC_GCM_BATCH_MAX_BYTES
GCM_BATCH_MAX_AAD = 1 << 16  # otc.h OTC_GCM_BATCH_MAX_AAD


def _pick_tile(nbytes) -> int:
    """Tile size minimising (tile slots issued) x (cost per slot)."""
    best, best_cost = 256, None
    for t in BATCH_TILES:
        slots = int(((nbytes + 16 * t - 1) // (16 * t)).sum()) * t
        cost = slots * BATCH_TILE_COST[t]
        if best_cost is None or cost < best_cost:
            best, best_cost = t, cost
    return best


def _tile_blocks(tile_blocks, nbytes) -> int:
    """The caller's tile size, checked, or the one picked from the message sizes."""
    if tile_blocks is None:
        tile_blocks = _pick_tile(nbytes) if len(nbytes) else 256
    if tile_blocks not in BATCH_TILES:
        raise ValueError(f"tile_blocks must be one of {BATCH_TILES}")
    return tile_blocks


class _Blob:
    """A plan's host image: pieces at aligned offsets, sent to the device by one pinned copy."""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, b: bytes, align: int = 16) -> int:
        pad = (-self.size) % align
        if pad:
            self.parts.append(bytes(pad))
        at = self.size + pad
        self.parts.append(b)
        self.size = at + len(b)
        return at

    def upload(self, device) -> torch.Tensor:
        host = torch.frombuffer(bytearray(b"".join(self.parts)), dtype=torch.uint8).pin_memory()
        return host.to(device, non_blocking=True)


def _packed_layout(buf: torch.Tensor, lengths, offsets, noun: str):
    """``(lengths, offsets)`` as int64 arrays of the ``noun``s ("message" /
    "record") packed in ``buf``: offsets default to back-to-back 16-byte
    aligned slots; every one lies inside the buffer at a multiple of 16."""
    import numpy as np
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    n = lens.size
    if offsets is None:
        offs = np.zeros(n, dtype=np.int64)
        if n > 1:
            offs[1:] = np.cumsum((lens[:-1] + 15) // 16 * 16)
    else:
        offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offs.size != n:
        raise ValueError(f"one offset per {noun}")
    if n and ((lens < 0).any() or (offs < 0).any() or (offs + lens > _nbytes(buf)).any()):
        raise ValueError(f"{noun}s must lie inside the buffer")
    if n and (offs % 16).any():
        raise ValueError(f"{noun} offsets must be multiples of 16")
    return lens, offs


def _packed_buffers(buf: torch.Tensor, out, lens, offs):
    """``(out, descriptors)`` of a packed batch: ``out`` defaults to a new
    buffer; both buffers are 16-byte aligned and the same or disjoint; the
    (n, 6) uint64 descriptors have their columns in, out, nbytes filled.
    Apart from ``_packed_layout`` because ``CtrBatch.packed`` checks its
    counters and key index between the two."""
    import numpy as np
    out = _out_like(buf, out)
    pi, po, nb = buf.data_ptr(), out.data_ptr(), _nbytes(buf)
    if (pi | po) % 16:
        raise ValueError("buf / out must be 16-byte aligned")
    if pi != po and pi < po + nb and po < pi + nb:
        raise ValueError("buf and out overlap partially")
    desc = np.zeros((lens.size, 6), dtype=np.uint64)
    desc[:, 0] = np.uint64(pi) + offs.astype(np.uint64)
    desc[:, 1] = np.uint64(po) + offs.astype(np.uint64)
    desc[:, 2] = lens.astype(np.uint64)
    return out, desc


def _key_index(key_index, n: int, nkeys: int):
    """The key of every message as an int64 array (default: key i for message i)."""
    import numpy as np
    if key_index is None:
        if nkeys != n:
            raise ValueError("one key per message, or pass key_index")
        kidx = np.arange(n, dtype=np.int64)
    else:
        kidx = np.asarray(key_index, dtype=np.int64).reshape(-1)
        if kidx.size != n:
            raise ValueError("one key index per message")
    if n and (kidx.min() < 0 or kidx.max() >= nkeys):
        raise ValueError("key_index out of range")
    return kidx


def _tensor_descs(xs, outs, device, noun: str):
    """Yields ``(i, in address, out address, bytes)`` of every input / output
    pair after the checks both batches make: GPU tensors, contiguous, all on
    ``device``, ``outs[i]`` of ``xs[i]``'s byte size."""
    for i, (x, o) in enumerate(zip(xs, outs)):
        _check_dev(x, f"xs[{i}]")
        _check_dev(o, f"outs[{i}]")
        if x.device != device or o.device != device:
            raise ValueError(f"all {noun}s must be on one device")
        nb = _nbytes(x)
        if _nbytes(o) != nb:
            raise ValueError(f"outs[{i}] must have the byte size of xs[{i}]")
        yield i, x.data_ptr(), o.data_ptr(), nb


def _set_aads(desc, aads, device, keep):
    """Columns 3 and 4 of a batched AEAD's descriptors (``GcmBatch`` and
    ``chacha_batch_ops.ChaChaBatch``, whose AAD cap is the same); host AADs go
    to one device buffer.  ``keep`` collects what must stay alive."""
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
        if aads.device != device:
            raise ValueError("aads must be on the records' device")
        a = int(aads.shape[1])
        if a > GCM_BATCH_MAX_AAD:
            raise ValueError("a record has at most 64 KiB of AAD")
        keep.append(aads)
        if a:
            desc[:, 3] = np.uint64(aads.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(a)
            desc[:, 4] = a
        return
    aads = list(aads)
    if len(aads) != n:
        raise ValueError("one AAD per record")
    host, blob = [], _Blob()
    for i, a in enumerate(aads):
        if isinstance(a, torch.Tensor):
            _check_dev(a, f"aads[{i}]")
            if a.device != device:
                raise ValueError("aads must be on the records' device")
            na = _nbytes(a)
            addr = a.data_ptr()
        else:
            a = b"" if a is None else bytes(a)
            na, addr = len(a), None
        if na > GCM_BATCH_MAX_AAD:
            raise ValueError(f"record {i}: more than 64 KiB of AAD")
        if na and addr is None:
            host.append((i, blob.add(a, 1)))  # back to back: an AAD takes any alignment
        elif na:
            desc[i, 3] = addr
        desc[i, 4] = na
    keep.append(aads)
    if host:
        dev = blob.upload(device)
        keep.append(dev)
        for i, off in host:
            desc[i, 3] = dev.data_ptr() + off


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
        if key_index is not None:  # any iterable of int-likes; its first n entries count
            key_index = np.fromiter((int(k) for k in key_index), dtype=np.int64, count=n)
        kidx = _key_index(key_index, n, len(keys))
        self._start(list(outs), list(xs), xs[0].device if n else None, tile_blocks)
        if n == 0:
            return
        desc = np.zeros((n, 6), dtype=np.uint64)  # in, out, nbytes, ctr_hi, ctr_lo, key
        for i, pi, po, nb in _tensor_descs(xs, outs, self.device, "message"):
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

    def _start(self, outs, keep, device, tile_blocks):
        self.outs = outs
        self._keep = keep  # descriptors hold raw addresses: keep the tensors alive
        self._launches = []
        self.device = device
        self.ntiles, self.tile_blocks = 0, tile_blocks or 256  # an empty batch's; _build sets the real ones

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
        lens, offs = _packed_layout(buf, lengths, offsets, "message")
        n = lens.size
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
        kidx = _key_index(key_index, n, len(keys))
        _check_dev(buf, "buf")  # after the layout: a bad layout is reported without a device
        out, desc = _packed_buffers(buf, out, lens, offs)
        self = cls.__new__(cls)
        self.out = out
        self._start([out], [buf], buf.device, tile_blocks)
        if n == 0:
            return self
        desc[:, 3] = c[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
        desc[:, 4] = c[:, 8:].copy().view(">u8").reshape(-1).astype(np.uint64)
        desc[:, 5] = kidx.astype(np.uint64)
        self._build(desc, keys, kidx, tile_blocks)
        return self

    def _build(self, desc, keys, kidx, tile_blocks):
        """Tile map + key schedules + descriptors -> one pinned upload."""
        import numpy as np
        self.tile_blocks = tile_blocks = _tile_blocks(tile_blocks, desc[:, 2])
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
        nr_msg = np.array([k.nr for k in ek], dtype=np.int64)[kidx]
        blob, launches = _Blob(), []
        blob.add(b"".join(bytes(k) for k in ek))  # otc_aes_key[] (256 B each), at offset 0
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
            launches.append((blob.add(d.tobytes()), blob.add(first.tobytes()), blob.add(tmap.tobytes()), ntiles, nr))
        self._plan = blob.upload(self.device)
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
        for i, pi, po, nb in _tensor_descs(xs, outs, self.device, "record"):
            if nb > GCM_BATCH_MAX_BYTES:
                raise ValueError(f"record {i}: more than 1 MiB of data (use gcm_encrypt for large messages)")
            desc[i, :3] = (pi if nb else 0, po if nb else 0, nb)
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
        self = cls.__new__(cls)
        self._init_common(key, tag_bytes, lanes)
        _check_dev(buf, "buf")  # before the layout, unlike CtrBatch.packed
        lens, offs = _packed_layout(buf, lengths, offsets, "record")
        if lens.size and (lens > GCM_BATCH_MAX_BYTES).any():
            raise ValueError("a record has at most 1 MiB of data (use gcm_encrypt for large messages)")
        out, desc = _packed_buffers(buf, out, lens, offs)
        self.out = out
        self.outs = [out]
        self._keep = [buf]
        self.device = buf.device
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
        _set_aads(desc, aads, self.device, self._keep)

    def _build(self, desc, tile_blocks):
        """Planner (validation + the CTR half's tile map) -> one pinned upload;
        the key's hash tables; workspace, tags, verdicts."""
        import numpy as np
        self.n = n = desc.shape[0]
        self.tile_blocks = tile_blocks = _tile_blocks(tile_blocks, desc[:, 2])
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
        if self.lanes is None:
            self.lanes = lib.otc_gcm_batch_lanes(desc.ctypes.data, n)
        blob = _Blob()
        self._o_key = blob.add(bytes(self._k.enc))  # otc_aes_key[1]: the CTR half reads round keys from memory
        self._o_desc = blob.add(desc.tobytes())
        self._o_ctr = blob.add(ctr.tobytes())
        self._o_first = blob.add(first.tobytes())
        self._o_map = blob.add(tmap.tobytes())
        self.ntiles = int(ntiles)
        dev = self.device
        with torch.cuda.device(dev):
            self._plan = blob.upload(dev)
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
    return _spans("otc_gcm_batch_spans")


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
