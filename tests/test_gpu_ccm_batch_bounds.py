"""Guard bands around every buffer of a batched AES-CCM run
(csrc/hip/aes_ccm_batch.hip), by the arena method of
tests/test_gpu_ocb_batch_bounds.py: records, outputs, AADs, nonces, expected
tags, computed tags and verdicts each sit in one arena between guard bands of a
known fill.  After an encryption, a decryption with one forged record (which
runs the wipe) and a decryption in place, under two fills (0x00 and 0xFF) and
two tag lengths: every result equals the oracle, so no byte outside an input
reached it; no guard byte changed; the inputs of an out-of-place run are
intact.  A packed batch with gaps between its records runs in an arena of its
own: the gaps are guards too.

The kernel's widest store is a lane's burst, 8 blocks of 16 bytes back to back
(a partial block goes out byte by byte, tags and verdicts byte by byte; the
wipe stores 16 bytes per lane); the guards are 4 KiB + 64 bytes, far wider, so
a wrong range check shows as a changed guard byte and never as a fault."""
import numpy as np
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

CB = ops.ccm_batch_ops
BURST = 128  # aes_ccm_batch.hip: a lane's burst in bytes
GUARD = 4096 + 64
KEY = bytes(range(7, 39))
# around a block, a burst and two, and partial tail blocks first, in the middle and last in a burst
LENS = [0, 1, 15, 16, 17, 127, 128, 129, 255, 256 + 17, 1024 + 113, 4096 + 17]
AADS = [0, 13, 1, 16, 17, 0, 40, 13, 5, 14, 30, 13]
FORGED = 9


class Arena:
    """One device buffer of ``fill`` bytes in which regions are handed out
    from front to back, every one behind a guard band and 16-byte aligned plus
    ``shift``; ``assert_guards`` compares every byte outside the regions."""

    def __init__(self, gpu, size, fill):
        self.t = torch.full((size,), fill, dtype=torch.uint8, device=gpu)
        self.fill, self.at, self.regions = fill, 0, []

    def region(self, n, shift=0):
        start = (self.at + GUARD + 15) // 16 * 16 + shift
        self.at = start + n
        assert self.at + GUARD <= self.t.numel()
        self.regions.append((start, n))
        return self.t[start:start + n]

    def put(self, b: bytes, shift=0):
        r = self.region(len(b), shift)
        if b:
            r.copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
        return r

    def assert_guards(self, what):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy().copy()
        for start, n in self.regions:
            h[start:start + n] = self.fill
        bad = np.nonzero(h != self.fill)[0]
        assert bad.size == 0, f"{what}: {bad.size} guard bytes changed, from +{int(bad[0])} to +{int(bad[-1])}"


def host(t):
    torch.cuda.synchronize()
    return t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


_data = {}


def records(tb):
    """Seeded plaintexts, AADs, nonces and the oracle's ciphertexts and tags, once per tag length."""
    if tb not in _data:
        rng = np.random.default_rng(61)
        pts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENS]
        aads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in AADS]
        nonces = [rng.integers(0, 256, 13, dtype=np.uint8).tobytes() for _ in LENS]
        sealed = cpu_ref.ccm_batch(KEY, nonces, pts, aads, tag_bytes=tb)
        _data[tb] = dict(pts=pts, aads=aads, nonces=nonces, cts=[c for c, _ in sealed], tags=[t for _, t in sealed])
    return _data[tb]


def in_arena(batch, ar):
    """The batch's own tensors -- computed tags, verdicts -- moved between guard bands (there is no workspace)."""
    n = batch.n
    assert batch._ws.numel() == 0
    batch.tags = ar.region(batch.tag_bytes * n, shift=1).view(n, batch.tag_bytes)  # rows at odd addresses
    batch.ok = ar.region(n, shift=3)
    torch.cuda.synchronize()
    return batch


@pytest.mark.parametrize("tb", [4, 16], ids=["tag-4", "tag-16"])
@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["fill-00", "fill-ff"])
def test_batch_guarded(gpu, fill, tb):
    assert CB.CcmBatch.spans()[1] == BURST  # the guards are sized for the kernel as it is
    d = records(tb)
    n = len(LENS)
    ar = Arena(gpu, (5 * n + 16) * (GUARD + 32) + 5 * sum(LENS) + sum(AADS), fill)
    xs = [ar.put(p) for p in d["pts"]]
    outs = [ar.region(len(p)) for p in d["pts"]]
    aads = [ar.put(a, shift=1) for a in d["aads"]]       # AADs start at odd addresses
    nonces = ar.put(b"".join(d["nonces"]), shift=3).view(n, 13)
    expect = ar.put(b"".join(d["tags"]), shift=5).view(n, tb)
    kw = dict(nonce_bytes=13, tag_bytes=tb)

    # encryption, out of place
    e = in_arena(CB.CcmBatch(xs, KEY, outs=outs, aads=aads, **kw), ar)
    e.encrypt(nonces)
    assert [host(o) for o in outs] == d["cts"] and host(e.tags) == b"".join(d["tags"])
    assert [host(x) for x in xs] == d["pts"] and [host(a) for a in aads] == d["aads"], "an input changed"
    assert host(nonces) == b"".join(d["nonces"])
    ar.assert_guards("encrypt")

    # one forged record, out of place from a copy of the ciphertexts: the wipe runs inside the guards
    cts = [ar.put(c) for c in d["cts"]]
    cts[FORGED][LENS[FORGED] - 1] ^= 1
    pts = [ar.region(len(p)) for p in d["pts"]]
    f = in_arena(CB.CcmBatch(cts, KEY, outs=pts, aads=aads, **kw), ar)
    _, ok = f.decrypt(nonces, expect)
    assert ok.tolist() == [m != FORGED for m in range(n)]
    assert [host(p) for p in pts] == [bytes(len(p)) if m == FORGED else p for m, p in enumerate(d["pts"])]
    assert host(f.tags) == b"".join(bytes(tb) if m == FORGED else t for m, t in enumerate(d["tags"]))
    assert host(expect) == b"".join(d["tags"])
    ar.assert_guards("decrypt with a forged record")

    # decryption in place over the encryption's outputs
    dd = in_arena(CB.CcmBatch(outs, KEY, outs=outs, aads=aads, **kw), ar)
    _, ok = dd.decrypt(nonces, expect)
    assert bool(ok.all()) and [host(o) for o in outs] == d["pts"] and host(dd.tags) == b"".join(d["tags"])
    ar.assert_guards("decrypt in place")


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_packed_offsets_with_gaps_guarded(gpu, inplace):
    """Records at packed offsets with gaps of 16 .. 48 bytes (and the partial
    blocks' own padding) between them: nothing between the records changes, in
    the output of an encryption, of a decryption with a forged record, and of a
    clean one."""
    d = records(16)
    n = len(LENS)
    fill = 0x3C
    offs, at = [], 0
    for i, k in enumerate(LENS):
        offs.append(at)
        at += (k + 15) // 16 * 16 + 16 * (1 + i % 3)
    ar = Arena(gpu, 16 * (GUARD + 32) + 3 * at, fill)
    buf = ar.region(at)
    for o, p in zip(offs, d["pts"]):
        if p:
            buf[o:o + len(p)].copy_(torch.frombuffer(bytearray(p), dtype=torch.uint8))
    out = buf if inplace else ar.region(at)
    aad = ar.put(bytes(range(13)) * n, shift=1).view(n, 13)
    ha = [bytes(range(13))] * n
    nonces = ar.put(b"".join(d["nonces"]), shift=3).view(n, 13)
    want = cpu_ref.ccm_batch(KEY, d["nonces"], d["pts"], ha)
    expect = ar.put(b"".join(t for _, t in want), shift=5).view(n, 16)

    def recs(t):
        h = host(t)
        return [h[o:o + k] for o, k in zip(offs, LENS)]

    def gaps_intact(t, what):
        h = np.frombuffer(host(t), dtype=np.uint8).copy()
        for o, k in zip(offs, LENS):
            h[o:o + k] = fill
        assert (h == fill).all(), f"{what}: bytes between the records changed"

    e = in_arena(CB.CcmBatch.packed(buf, LENS, KEY, out=out, offsets=offs, aad=aad, nonce_bytes=13), ar)
    e.encrypt(nonces)
    assert recs(out) == [c for c, _ in want] and host(e.tags) == b"".join(t for _, t in want)
    gaps_intact(out, "encrypt")
    if not inplace:
        assert recs(buf) == d["pts"]
        gaps_intact(buf, "encrypt (input)")
    ar.assert_guards("packed encrypt")

    out[offs[FORGED] + 5] ^= 0x40
    f = in_arena(CB.CcmBatch.packed(out, LENS, KEY, out=out, offsets=offs, aad=aad, nonce_bytes=13), ar)
    _, ok = f.decrypt(nonces, expect)
    assert ok.tolist() == [m != FORGED for m in range(n)]
    assert recs(out) == [bytes(len(p)) if m == FORGED else p for m, p in enumerate(d["pts"])]
    gaps_intact(out, "decrypt with a forged record")
    ar.assert_guards("packed decrypt")
