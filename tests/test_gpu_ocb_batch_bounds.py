"""Guard bands around every buffer of a batched AES-OCB3 run
(csrc/hip/aes_ocb_batch.hip), by the arena method of
tests/test_gpu_chacha_batch_bounds.py: records, outputs, AADs, nonces, expected
tags, computed tags, verdicts and the workspace each sit in one arena between
guard bands of a known fill.  After an encryption, a decryption with one
forged record (which runs the wipe) and a decryption in place, under two fills
(0x00 and 0xFF): every result equals the oracle, so no byte outside an input
reached it; no guard byte changed; the inputs of an out-of-place run are
intact.

The widest store step is one workgroup step of the bulk kernel: 16 waves x 4
slots x 1 KiB = 64 KiB when all its tiles belong to one record (one store
instruction of a wave covers 1 KiB; the finisher stores single bytes, 16-byte
tags and single verdict bytes; prep stores 16-byte rows of the workspace; the
checksum atomics touch 16 bytes of it; the wipe stores 16 bytes per lane).
The guards are 64 KiB + 64 bytes, wider than that, so a wrong range check
shows as a changed guard byte and never as a fault."""
import numpy as np
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

OB = ops.ocb_batch_ops
STORE_STEP = 16 * 4 * 1024  # aes_ocb_batch.hip: waves x slots x a tile's bytes
GUARD = STORE_STEP + 64
KEY = bytes(range(7, 39))
# around a lane's block, a tile, a wave pass and the workgroup's store step
LENS = [0, 1, 15, 16, 17, 1023, 1024, 1040, 4096 + 17, STORE_STEP + 16]
AADS = [0, 13, 1, 16, 17, 0, 40, 13, 5, 13]
FORGED = 7


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


def records():
    """Seeded plaintexts, AADs, nonces and the oracle's ciphertexts and tags, once."""
    if not _data:
        rng = np.random.default_rng(61)
        pts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENS]
        aads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in AADS]
        nonces = [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in LENS]
        sealed = cpu_ref.ocb_batch(KEY, nonces, pts, aads)
        _data.update(pts=pts, aads=aads, nonces=nonces, cts=[c for c, _ in sealed], tags=[t for _, t in sealed])
    return _data


def in_arena(batch, ar):
    """The batch's own tensors -- workspace, computed tags, verdicts -- moved between guard bands."""
    n = batch.n
    batch._ws = ar.region(48 * n)
    batch.tags = ar.region(16 * n).view(n, 16)
    batch.ok = ar.region(n)
    torch.cuda.synchronize()
    return batch


@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["fill-00", "fill-ff"])
def test_batch_guarded(gpu, fill):
    assert OB.OcbBatch.spans()[3] == STORE_STEP  # the guards are sized for the kernel as it is
    d = records()
    n = len(LENS)
    ar = Arena(gpu, (5 * n + 16) * (GUARD + 32) + 5 * sum(LENS) + sum(AADS), fill)
    xs = [ar.put(p) for p in d["pts"]]
    outs = [ar.region(len(p)) for p in d["pts"]]
    aads = [ar.put(a, shift=1) for a in d["aads"]]       # AADs start at odd addresses
    nonces = ar.put(b"".join(d["nonces"]), shift=3).view(n, 12)
    expect = ar.put(b"".join(d["tags"]), shift=5).view(n, 16)

    # encryption, out of place
    e = in_arena(OB.OcbBatch(xs, KEY, outs=outs, aads=aads), ar)
    e.encrypt(nonces)
    assert [host(o) for o in outs] == d["cts"] and host(e.tags) == b"".join(d["tags"])
    assert [host(x) for x in xs] == d["pts"] and [host(a) for a in aads] == d["aads"], "an input changed"
    assert host(nonces) == b"".join(d["nonces"])
    ar.assert_guards("encrypt")

    # one forged record, out of place from a copy of the ciphertexts: the wipe runs inside the guards
    cts = [ar.put(c) for c in d["cts"]]
    cts[FORGED][LENS[FORGED] - 1] ^= 1
    pts = [ar.region(len(p)) for p in d["pts"]]
    f = in_arena(OB.OcbBatch(cts, KEY, outs=pts, aads=aads), ar)
    _, ok = f.decrypt(nonces, expect)
    assert ok.tolist() == [m != FORGED for m in range(n)]
    assert [host(p) for p in pts] == [bytes(len(p)) if m == FORGED else p for m, p in enumerate(d["pts"])]
    assert host(f.tags) == b"".join(bytes(16) if m == FORGED else t for m, t in enumerate(d["tags"]))
    assert host(expect) == b"".join(d["tags"])
    ar.assert_guards("decrypt with a forged record")

    # decryption in place over the encryption's outputs
    dd = in_arena(OB.OcbBatch(outs, KEY, outs=outs, aads=aads), ar)
    _, ok = dd.decrypt(nonces, expect)
    assert bool(ok.all()) and [host(o) for o in outs] == d["pts"] and host(dd.tags) == b"".join(d["tags"])
    ar.assert_guards("decrypt in place")
