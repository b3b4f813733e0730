"""Guard bands around every buffer of a batched AES-GCM-SIV run
(csrc/hip/aes_gcm_siv_batch.hip), by the arena method of
tests/test_gpu_ocb_batch_bounds.py (its ``Arena``): records, outputs, AADs,
nonces, expected tags, computed tags, verdicts, the workspace with the derived
keys, and for the two halves the hash keys, hashes, schedules and counter rows
each sit in one arena between guard bands of a known fill.  After an
encryption, a decryption with one forged record (which runs the wipe), a
decryption in place and the two halves alone, under two fills (0x00 and 0xFF):
every result equals the oracle, so no byte outside an input reached it; no
guard byte changed; the inputs of an out-of-place run are intact.

The widest store step is one pass of the counter kernel's workgroup: 16 waves x
one tile of 4 KiB = 64 KiB when all its tiles belong to one record (one store
instruction of a wave covers 1 KiB; the partial last block is stored byte by
byte; derive stores 16-byte rows of the workspace, the hash and the finisher
16-byte rows and single verdict bytes; the wipe 16 bytes per lane).  The
helper's guards are 64 KiB + 64 bytes, wider than that, so a wrong range check
shows as a changed guard byte and never as a fault."""
import numpy as np
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref
from test_gpu_ocb_batch_bounds import GUARD, Arena, host

pytestmark = pytest.mark.gpu

SB = ops.gcm_siv_batch_ops
TILE = 4096
STORE_STEP = 16 * TILE  # aes_gcm_siv_batch.hip: the waves of a workgroup, one tile each
assert GUARD > STORE_STEP
KEY = bytes(range(9, 41))
# around a lane's block, the hash kernel's spans (16, 64, 256 hashed blocks behind a 13-byte AAD), a tile and the store step
LENS = [0, 1, 15, 16, 17, 14 * 16, 62 * 16 - 1, 254 * 16 + 1, TILE - 1, TILE, TILE + 17, STORE_STEP + 16]
AADS = [0, 13, 1, 16, 17, 13, 13, 13, 40, 0, 5, 13]
FORGED = 8
WS_PER_RECORD = 288  # otc_gcm_siv_batch_ws_bytes: H, S and an expanded key


def records():
    rng = np.random.default_rng(67)
    pts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENS]
    aads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in AADS]
    nonces = [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in LENS]
    sealed = cpu_ref.gcm_siv_batch(KEY, nonces, pts, aads)
    return dict(pts=pts, aads=aads, nonces=nonces, cts=[c for c, _ in sealed], tags=[t for _, t in sealed])


_data = {}


def data():
    if not _data:
        _data.update(records())
    return _data


def in_arena(batch, ar):
    """The batch's own tensors -- workspace, computed tags, verdicts -- moved between guard bands."""
    n = batch.n
    assert batch._ws.numel() == WS_PER_RECORD * n
    batch._ws = ar.region(WS_PER_RECORD * n)
    batch.tags = ar.region(16 * n).view(n, 16)
    batch.ok = ar.region(n)
    torch.cuda.synchronize()
    return batch


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["fill-00", "fill-ff"])
def test_batch_guarded(gpu, fill, lanes):
    d = data()
    n = len(LENS)
    ar = Arena(gpu, (5 * n + 16) * (GUARD + 32) + 5 * sum(LENS) + sum(AADS) + 3 * WS_PER_RECORD * n, fill)
    xs = [ar.put(p) for p in d["pts"]]
    outs = [ar.region(len(p)) for p in d["pts"]]
    aads = [ar.put(a, shift=1) for a in d["aads"]]       # AADs start at odd addresses
    nonces = ar.put(b"".join(d["nonces"]), shift=3).view(n, 12)
    expect = ar.put(b"".join(d["tags"]), shift=4).view(n, 16)  # 4-byte aligned: the counter kernel reads it

    # encryption, out of place
    e = in_arena(SB.GcmSivBatch(xs, KEY, outs=outs, aads=aads, lanes=lanes), ar)
    e.encrypt(nonces)
    assert [host(o) for o in outs] == d["cts"] and host(e.tags) == b"".join(d["tags"])
    assert [host(x) for x in xs] == d["pts"] and [host(a) for a in aads] == d["aads"], "an input changed"
    assert host(nonces) == b"".join(d["nonces"])
    ar.assert_guards("encrypt")

    # one forged record, out of place from a copy of the ciphertexts: the wipe runs inside the guards
    cts = [ar.put(c) for c in d["cts"]]
    cts[FORGED][LENS[FORGED] - 1] ^= 1
    pts = [ar.region(len(p)) for p in d["pts"]]
    f = in_arena(SB.GcmSivBatch(cts, KEY, outs=pts, aads=aads, lanes=lanes), ar)
    _, ok = f.decrypt(nonces, expect)
    assert ok.tolist() == [m != FORGED for m in range(n)]
    assert [host(p) for p in pts] == [bytes(len(p)) if m == FORGED else p for m, p in enumerate(d["pts"])]
    assert host(f.tags) == b"".join(bytes(16) if m == FORGED else t for m, t in enumerate(d["tags"]))
    assert host(expect) == b"".join(d["tags"])
    ar.assert_guards("decrypt with a forged record")

    # decryption in place over the encryption's outputs
    dd = in_arena(SB.GcmSivBatch(outs, KEY, outs=outs, aads=aads, lanes=lanes), ar)
    _, ok = dd.decrypt(nonces, expect)
    assert bool(ok.all()) and [host(o) for o in outs] == d["pts"] and host(dd.tags) == b"".join(d["tags"])
    ar.assert_guards("decrypt in place")


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["fill-00", "fill-ff"])
def test_polyval_batch_guarded(gpu, fill, lanes):
    """The hash half: the keys are a guarded input, the records and AADs too; the result is copied into a guarded region."""
    d = data()
    n = len(LENS)
    rng = np.random.default_rng(68)
    hs = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in LENS]
    ar = Arena(gpu, (2 * n + 8) * (GUARD + 32) + sum(LENS) + sum(AADS), fill)
    xs = [ar.put(p) for p in d["pts"]]
    aads = [ar.put(a, shift=1) for a in d["aads"]]
    hv = ar.put(b"".join(hs)).view(n, 16)
    s = SB.polyval_batch(xs, hv, aads=aads, lanes=lanes)
    want = []
    for h, a, p in zip(hs, d["aads"], d["pts"]):
        want.append(cpu_ref.polyval(h, a + bytes(-len(a) % 16) + p + bytes(-len(p) % 16) +
                                    (8 * len(a)).to_bytes(8, "little") + (8 * len(p)).to_bytes(8, "little")))
    assert host(s) == b"".join(want)
    assert [host(x) for x in xs] == d["pts"] and host(hv) == b"".join(hs)
    ar.assert_guards("polyval_batch")


@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["fill-00", "fill-ff"])
def test_ctr_le32_batch_guarded(gpu, fill, bits):
    """The counter half, out of place and in place; the counter rows wrap inside the records."""
    d = data()
    n = len(LENS)
    rng = np.random.default_rng(69)
    keys = [rng.integers(0, 256, bits // 8, dtype=np.uint8).tobytes() for _ in LENS]
    ctrs = [((1 << 32) - 3 - 67 * m).to_bytes(4, "little") + b"\xff" + rng.integers(0, 256, 10, dtype=np.uint8).tobytes() +
            bytes([m]) for m in range(n)]
    want = [cpu_ref.ctr_le32(k, c[:15] + bytes([c[15] | 0x80]), p) for k, c, p in zip(keys, ctrs, d["pts"])]
    ar = Arena(gpu, (3 * n + 8) * (GUARD + 32) + 3 * sum(LENS), fill)
    xs = [ar.put(p) for p in d["pts"]]
    outs = [ar.region(len(p)) for p in d["pts"]]
    cv = ar.put(b"".join(ctrs)).view(n, 16)
    SB.ctr_le32_batch(xs, keys, cv, outs=outs)
    assert [host(o) for o in outs] == want and [host(x) for x in xs] == d["pts"] and host(cv) == b"".join(ctrs)
    ar.assert_guards("ctr_le32_batch")
    SB.ctr_le32_batch(outs, keys, cv, outs=outs)  # in place: back to the plaintexts
    assert [host(o) for o in outs] == d["pts"]
    ar.assert_guards("ctr_le32_batch in place")
