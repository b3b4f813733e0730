"""Guard bands around every buffer of a many-key batched AES-GCM run
(csrc/hip/aes_gcm_mk_batch.hip), by the arena method of
tests/test_gpu_ocb_batch_bounds.py (its ``Arena``): records, outputs, AADs,
IVs, expected tags, computed tags, verdicts, the workspace, the schedule array
and the table image each sit in one arena between guard bands of a known fill.
After an encryption, a decryption with one forged record (which runs the wipe),
a decryption in place, the hash alone and the table kernel alone, under two
fills (0x00 and 0xFF): every result equals the oracle, so no byte outside an
input reached it; no guard byte changed; the inputs of an out-of-place run are
intact.

The widest store step is one pass of the CTR kernel's workgroup: 16 waves x one
tile of 4 KiB = 64 KiB when all its tiles belong to one record (the hash and
the finisher store 16-byte rows and single verdict bytes, the table kernel
16-byte table entries, prep 8-byte words of the CTR descriptors and 16-byte
rows, the wipe 16 bytes per lane).  The helper's guards are 64 KiB + 64 bytes,
wider than that, so a wrong range check shows as a changed guard byte and never
as a fault."""
import ctypes

import numpy as np
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref
from test_gpu_ocb_batch_bounds import GUARD, Arena, host

pytestmark = pytest.mark.gpu

MK = ops.gcm_mk_batch_ops
TILE = 4096
STORE_STEP = 16 * TILE  # aes_tt.hip's batch kernel: the waves of a workgroup, one tile each
assert GUARD > STORE_STEP
# around a lane's block, the hash kernel's spans (16, 64, 256 hashed blocks behind a 13-byte AAD), a tile and the store step
LENS = [0, 1, 15, 16, 17, 14 * 16, 62 * 16 - 1, 254 * 16 + 1, TILE - 1, TILE, TILE + 17, STORE_STEP + 16]
AADS = [0, 13, 1, 16, 17, 13, 13, 13, 40, 0, 5, 13]
NKEYS = 5
KIDX = [(3 * m + 2) % NKEYS for m in range(len(LENS))]
FORGED = 8
WS_PER_RECORD = 32     # otc_gcm_mk_batch_ws_bytes: J0 and the hash
TABLE_PER_KEY = 7 * 256


def records(bits):
    rng = np.random.default_rng(71 + bits)
    keys = [rng.integers(0, 256, bits // 8, dtype=np.uint8).tobytes() for _ in range(NKEYS)]
    pts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENS]
    aads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in AADS]
    ivs = [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in LENS]
    sealed = cpu_ref.gcm_mk_batch(keys, KIDX, ivs, pts, aads)
    return dict(keys=keys, pts=pts, aads=aads, ivs=ivs, cts=[c for c, _ in sealed], tags=[t for _, t in sealed])


_data = {}


def data(bits):
    if bits not in _data:
        _data[bits] = records(bits)
    return _data[bits]


def in_arena(batch, ar):
    """The batch's own tensors -- schedules, table image, workspace, computed tags, verdicts -- moved between
    guard bands; the table kernel then runs again, into the guarded image."""
    n = batch.n
    assert batch._ws.numel() == WS_PER_RECORD * n and batch._tab.numel() == TABLE_PER_KEY * NKEYS
    assert batch._keys.numel() == 256 * NKEYS
    batch._keys = ar.region(256 * NKEYS)
    batch._tab = ar.region(TABLE_PER_KEY * NKEYS)
    batch._ws = ar.region(WS_PER_RECORD * n)
    batch.tags = ar.region(16 * n).view(n, 16)
    batch.ok = ar.region(n)
    batch._upload_keys(torch.cuda.current_stream())
    torch.cuda.synchronize()
    return batch


@pytest.mark.parametrize("lanes,bits", [(16, 128), (64, 256), (16, 192)])
@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["fill-00", "fill-ff"])
def test_batch_guarded(gpu, fill, lanes, bits):
    d = data(bits)
    n = len(LENS)
    own = 256 * NKEYS + TABLE_PER_KEY * NKEYS + WS_PER_RECORD * n + 17 * n
    ar = Arena(gpu, (5 * n + 32) * (GUARD + 32) + 5 * sum(LENS) + sum(AADS) + 4 * own, fill)
    xs = [ar.put(p) for p in d["pts"]]
    outs = [ar.region(len(p)) for p in d["pts"]]
    aads = [ar.put(a, shift=1) for a in d["aads"]]       # AADs start at odd addresses
    ivs = ar.put(b"".join(d["ivs"]), shift=3).view(n, 12)
    expect = ar.put(b"".join(d["tags"]), shift=5).view(n, 16)

    # encryption, out of place
    e = in_arena(MK.GcmMkBatch(xs, d["keys"], key_index=KIDX, outs=outs, aads=aads, lanes=lanes), ar)
    e.encrypt(ivs)
    assert [host(o) for o in outs] == d["cts"] and host(e.tags) == b"".join(d["tags"])
    assert [host(x) for x in xs] == d["pts"] and [host(a) for a in aads] == d["aads"], "an input changed"
    assert host(ivs) == b"".join(d["ivs"])
    ar.assert_guards("encrypt")

    # the hash alone, over the plaintexts: the result is the batch's own allocation, copied into a guarded region
    hs = [cpu_ref.gcm_h(k) for k in d["keys"]]
    s = ar.region(16 * n)
    s.copy_(e.ghash().view(-1))
    want = [cpu_ref.ghash(hs[k], a + bytes(-len(a) % 16) + p + bytes(-len(p) % 16) + (8 * len(a)).to_bytes(8, "big") +
                          (8 * len(p)).to_bytes(8, "big")) for k, a, p in zip(KIDX, d["aads"], d["pts"])]
    assert host(s) == b"".join(want)
    ar.assert_guards("ghash")

    # one forged record, out of place from a copy of the ciphertexts: the wipe runs inside the guards
    cts = [ar.put(c) for c in d["cts"]]
    cts[FORGED][LENS[FORGED] - 1] ^= 1
    pts = [ar.region(len(p)) for p in d["pts"]]
    f = in_arena(MK.GcmMkBatch(cts, d["keys"], key_index=KIDX, outs=pts, aads=aads, lanes=lanes), ar)
    _, ok = f.decrypt(ivs, expect)
    assert ok.tolist() == [m != FORGED for m in range(n)]
    assert [host(p) for p in pts] == [bytes(len(p)) if m == FORGED else p for m, p in enumerate(d["pts"])]
    assert host(f.tags) == b"".join(bytes(16) if m == FORGED else t for m, t in enumerate(d["tags"]))
    assert host(expect) == b"".join(d["tags"])
    ar.assert_guards("decrypt with a forged record")

    # decryption in place over the encryption's outputs
    dd = in_arena(MK.GcmMkBatch(outs, d["keys"], key_index=KIDX, outs=outs, aads=aads, lanes=lanes), ar)
    _, ok = dd.decrypt(ivs, expect)
    assert bool(ok.all()) and [host(o) for o in outs] == d["pts"] and host(dd.tags) == b"".join(d["tags"])
    ar.assert_guards("decrypt in place")


@pytest.mark.parametrize("nkeys", [1, 4, 5, 67])
@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["fill-00", "fill-ff"])
def test_table_kernel_guarded(gpu, fill, nkeys):
    """The table kernel alone: 1792 bytes per key, nothing past the last key's
    image (a workgroup takes four keys: 1, 5 and 67 leave lanes without one), the
    schedules intact; the image serves a hash that equals the oracle."""
    rng = np.random.default_rng(73)
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(nkeys)]
    ar = Arena(gpu, 8 * (GUARD + 32) + (256 + TABLE_PER_KEY + 208) * nkeys + 4096, fill)
    datas = [bytes((k + 3 * i) & 0xFF for i in range(200)) for k in range(nkeys)]
    slab = ar.put(b"".join(d + bytes(8) for d in datas))  # 16-byte aligned slots in one region
    xs = [slab[208 * k:208 * k + 200] for k in range(nkeys)]
    b = MK.GcmMkBatch(xs, keys, outs=xs, lanes=16)
    sched = host(b._keys)
    b._keys = ar.put(sched)
    b._tab = ar.region(TABLE_PER_KEY * nkeys)
    rc = ops._common._lib().otc_gcm_mk_batch_tables(b._keys.data_ptr(), nkeys, 14, b._tab.data_ptr(),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    ar.assert_guards("tables")
    assert host(b._keys) == sched
    image = host(b._tab)
    assert all(image[TABLE_PER_KEY * k:TABLE_PER_KEY * k + 16] == bytes(16) for k in range(nkeys))  # entry 0 of a table
    assert len({image[TABLE_PER_KEY * k:TABLE_PER_KEY * (k + 1)] for k in range(nkeys)}) == nkeys
    got = host(b.ghash())
    for k in range(nkeys):
        assert got[16 * k:16 * k + 16] == cpu_ref.ghash(cpu_ref.gcm_h(keys[k]), datas[k] + bytes(8) + bytes(8) +
                                                         (1600).to_bytes(8, "big")), k
    ar.assert_guards("ghash on the guarded image")
