"""Batched AES-OCB3 on the device (csrc/hip/aes_ocb_batch.hip through
ops.ocb_batch_ops.OcbBatch): many records under one key, each with its own
12-byte nonce, AAD and 16-byte tag.  Every byte and every tag is compared with
the C oracle per record (cpu_ref.ocb, pinned to RFC 7253 in
tests/test_ocb_cpu.py), and the 48 golden vectors with 12-byte nonces and
16-byte tags of tests/golden/ocb_vectors.json run as three batches.

The shapes come from the bulk kernel's own decomposition (otc_ocb_batch_spans,
in bytes).  Data and AADs are slices of one seeded pool; the AADs start at odd
addresses on purpose."""
import json
import os
import time

import numpy as np
import pytest
import torch

from our_tree_amd import models, ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

OB = ops.ocb_batch_ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = [v for v in json.load(open(os.path.join(ROOT, "tests", "golden", "ocb_vectors.json")))["ocb"]
           if len(v["nonce"]) == 24 and v["tag_bytes"] == 16]

MIB = 1 << 20
DATA = 3 * MIB                # the pool's data region: records are cut from its front, 16-byte aligned
AAD_AT = DATA + 1             # the AAD region starts at an odd address
POOL = DATA + 256 * 1024
KEYS = {128: bytes(range(3, 19)), 192: bytes(range(60, 84)), 256: bytes(range(201, 233))}
KEY = KEYS[128]
ONE_LENS = [0, 1, 15, 16, 17, 1008, 1023, 1024, 1025, 1039, 1040, 1056]

_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host.  Never written."""
    if not _pool:
        g = torch.Generator(device=gpu).manual_seed(47)
        dev = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes())
    return _pool


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def cut(pool, lens, aad_lens=None):
    """Records of these lengths from the pool: (device views, host bytes,
    device AAD views, host AADs).  Data slots are 16-byte aligned and back to
    back; AADs are packed byte by byte from an odd address."""
    xs, hx, at = [], [], 0
    for n in lens:
        xs.append(pool["dev"][at:at + n])
        hx.append(pool["host"][at:at + n])
        at += (n + 15) // 16 * 16
    assert at <= DATA
    aad_lens = aad_lens or [0] * len(lens)
    ad, ha, at = [], [], AAD_AT
    for n in aad_lens:
        ad.append(pool["dev"][at:at + n])
        ha.append(pool["host"][at:at + n])
        at += n
    assert at <= POOL
    return xs, hx, ad, ha


def make_nonces(gpu, n, seed):
    b = np.random.default_rng(seed).integers(0, 256, (n, 12), dtype=np.uint8)
    return torch.from_numpy(b).to(gpu), [r.tobytes() for r in b]


def rows(t: torch.Tensor, width=16):
    b = host(t)
    return [b[i:i + width] for i in range(0, len(b), width)]


def dev_bytes(gpu, b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)


def check_both_ways(gpu, key, xs, hx, ad, ha, seed, inplace=False):
    """Encrypt the records, compare every ciphertext and tag with the oracle;
    decrypt them again, compare every plaintext, tag and verdict."""
    n = len(xs)
    nv, hn = make_nonces(gpu, n, seed)
    want = cpu_ref.ocb_batch(key, hn, hx, ha)
    if inplace:
        xs = [x.clone() for x in xs]
    b = OB.OcbBatch(xs, key, outs=xs if inplace else None, aads=ad)
    outs, tags = b.encrypt(nv)
    got_t = rows(tags)
    for m, (ct, tag) in enumerate(want):
        assert host(outs[m]) == ct, (m, len(hx[m]), "ciphertext")
        assert got_t[m] == tag, (m, len(hx[m]), len(ha[m]), "tag", got_t[m].hex(), tag.hex())
    d = b if inplace else OB.OcbBatch(outs, key, aads=ad)
    pts, ok = d.decrypt(nv, tags.clone())
    assert ok.dtype == torch.bool and ok.tolist() == [True] * n
    got_t = rows(d.tags)
    for m in range(n):
        assert host(pts[m]) == hx[m], (m, len(hx[m]), "plaintext")
        assert got_t[m] == want[m][1], (m, "tag of the decryption")
    return b


# ---- the golden vectors ----------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_rfc_7253_vectors_as_one_batch(gpu, bits):
    vs = [v for v in VECTORS if len(v["key"]) == bits // 4]
    assert len(vs) == 16 and len(VECTORS) == 48
    key = bytes.fromhex(vs[0]["key"])
    assert all(v["key"] == vs[0]["key"] for v in vs)
    xs = [dev_bytes(gpu, bytes.fromhex(v["pt"])) for v in vs]
    aads = [bytes.fromhex(v["aad"]) for v in vs]
    nv = dev_bytes(gpu, b"".join(bytes.fromhex(v["nonce"]) for v in vs)).view(16, 12)
    outs, tags = OB.ocb_encrypt_batch(xs, key, nv, aads=aads)
    for m, v in enumerate(vs):
        assert host(outs[m]).hex() == v["ct"] and rows(tags)[m].hex() == v["tag"], v["name"]
    pts, ok = OB.ocb_decrypt_batch(outs, key, nv, tags.clone(), aads=aads)
    assert bool(ok.all()) and [host(p).hex() for p in pts] == [v["pt"] for v in vs]


# ---- one record ------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_one_record_at_every_edge(pool, gpu, bits):
    """The lengths around a block and a tile, then every span of the bulk kernel
    up to the workgroup step - 16, + 0 and + 16, each as a batch of ONE record
    behind a 13-byte AAD, both directions."""
    spans = OB.OcbBatch.spans()
    assert len(spans) == 5 and spans == sorted(set(spans))
    lens = list(ONE_LENS)
    for s in spans[:4]:
        lens += [s - 16, s, s + 16]
    for i, n in enumerate(sorted(set(lens))):
        xs, hx, ad, ha = cut(pool, [n], [13])
        b = check_both_ways(gpu, KEYS[bits], xs, hx, ad, ha, seed=1000 + n)
        assert b.ntiles == (n // 16 + 63) // 64


def test_one_mib_record(pool, gpu):
    """The cap: 1024 tiles, block index 2^16 and L_16, in place."""
    xs, hx, ad, ha = cut(pool, [MIB], [5])
    check_both_ways(gpu, KEYS[256], xs, hx, ad, ha, seed=5, inplace=True)
    xs, hx, ad, ha = cut(pool, [MIB - 1], [0])
    check_both_ways(gpu, KEYS[128], xs, hx, ad, ha, seed=6)


# ---- several records -------------------------------------------------------------------
def test_four_slots_of_a_wave_on_four_records(pool, gpu):
    """Tiles 0..3 -- the four slots of the first wave's first pass -- belong to
    four different records; record 2 ends in the middle of its slot, records 4
    and 6 span several slots and end in the middle of one; record 1 has no
    tile at all."""
    lens = [1024, 7, 1024, 16 * 37 + 3, 1024, 2048 + 16 * 11, 1040, 4096 + 512 + 9]
    spans = OB.OcbBatch.spans()
    assert spans[1] == 1024 and spans[2] == 4 * spans[1]  # a slot is a tile of 1 KiB, a wave pass four of them
    xs, hx, ad, ha = cut(pool, lens, [0, 13, 16, 17, 0, 1, 40, 13])
    b = check_both_ways(gpu, KEY, xs, hx, ad, ha, seed=71)
    assert b.ntiles == 1 + 0 + 1 + 1 + 1 + 3 + 2 + 5
    check_both_ways(gpu, KEYS[192], xs, hx, ad, ha, seed=72, inplace=True)


def test_a_batch_past_the_grids_first_step(gpu):
    """A little more than the full grid's first step (one workgroup step per
    CU), so that a workgroup takes a second step: records of 1 MiB - 16 bytes
    built from the span, not from a constant."""
    first_step = OB.OcbBatch.spans()[-1]
    rec = MIB - 16
    n = first_step // rec + 2
    total = n * MIB
    assert n * rec > first_step + 4096
    g = torch.Generator(device=gpu).manual_seed(48)
    buf = torch.randint(0, 256, (total,), dtype=torch.uint8, device=gpu, generator=g)
    hb = host(buf)
    lens, offs = [rec] * n, [m * MIB for m in range(n)]
    nv, hn = make_nonces(gpu, n, 81)
    want = cpu_ref.ocb_batch(KEY, hn, [hb[o:o + rec] for o in offs])
    b = OB.OcbBatch.packed(buf, lens, KEY, out=buf, offsets=offs)
    assert b.ntiles * 1024 > first_step
    _, tags = b.encrypt(nv)
    out = host(buf)
    for m, o in enumerate(offs):
        assert out[o:o + rec] == want[m][0], m
        assert out[o + rec:o + MIB] == hb[o + rec:o + MIB], (m, "bytes outside the record")
    assert rows(tags) == [t for _, t in want]
    _, ok = b.decrypt(nv, tags.clone())
    assert bool(ok.all()) and host(buf) == hb


def mixed(pool, gpu):
    lens, aads = [], []
    for i in range(200):
        lens.append(0 if i % 5 == 1 else ONE_LENS[(i // 3 * 7 + i) % len(ONE_LENS)] + (4096 if i % 11 == 0 else 0))
        aads.append([0, 13, 16, 17, 1, 40][i % 6] if i % 4 else 0)
    xs, hx, ad, ha = cut(pool, lens, aads)
    nv, hn = make_nonces(gpu, 200, 77)
    want = cpu_ref.ocb_batch(KEY, hn, hx, ha)
    return lens, xs, hx, ad, ha, nv, hn, want


_mixed = {}


@pytest.fixture(scope="module")
def mix(pool, gpu):
    """200 records, the edge lengths interleaved with empty ones, AADs on some; the oracle once."""
    if not _mixed:
        _mixed["v"] = mixed(pool, gpu)
    return _mixed["v"]


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_mixed_batch_of_tensors(mix, gpu, inplace):
    lens, xs, hx, ad, ha, nv, hn, want = mix
    xs = [x.clone() for x in xs]  # the pool is never written
    b = OB.OcbBatch(xs, KEY, outs=xs if inplace else None, aads=ad)
    assert b.ntiles == sum((n // 16 + 63) // 64 for n in lens)
    _, tags = b.encrypt(nv)
    got_t = rows(tags)
    for m, (ct, tag) in enumerate(want):
        assert host(b.outs[m]) == ct and got_t[m] == tag, (m, lens[m])
    d = b if inplace else OB.OcbBatch(b.outs, KEY, outs=b.outs, aads=ad)
    pts, ok = d.decrypt(nv, tags.clone())
    assert bool(ok.all())
    for m, p in enumerate(pts):
        assert host(p) == hx[m], (m, lens[m])


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_mixed_batch_packed(mix, pool, gpu, inplace):
    lens, xs, hx, ad, ha, nv, hn, want = mix
    total = sum((n + 15) // 16 * 16 for n in lens)
    buf = pool["dev"][:total].clone()
    # the packed form takes one AAD length for all: 13 bytes each, rows of a [n, 13] tensor at an odd address
    aad = pool["dev"][AAD_AT:AAD_AT + 13 * len(lens)].view(len(lens), 13)
    ha13 = [pool["host"][AAD_AT + 13 * m:AAD_AT + 13 * m + 13] for m in range(len(lens))]
    want13 = cpu_ref.ocb_batch(KEY, hn, hx, ha13)
    b = OB.OcbBatch.packed(buf, lens, KEY, out=buf if inplace else None, aad=aad)
    offs = np.concatenate([[0], np.cumsum([(n + 15) // 16 * 16 for n in lens])[:-1]])
    before = host(b.out) if not inplace else None

    def outs_bytes():
        o = host(b.out)
        return [o[at:at + n] for at, n in zip(offs, lens)]

    _, tags = b.encrypt(nv)
    assert outs_bytes() == [c for c, _ in want13] and rows(tags) == [t for _, t in want13]
    if not inplace:  # bytes of out outside the records are not written
        after = host(b.out)
        for at, n in zip(offs, lens):
            pad = (n + 15) // 16 * 16 - n
            assert after[at + n:at + n + pad] == before[at + n:at + n + pad]
    d = OB.OcbBatch.packed(b.out, lens, KEY, out=b.out, aad=aad)
    _, ok = d.decrypt(nv, tags.clone())
    assert bool(ok.all()) and outs_bytes() == hx


def test_aad_lengths_at_misaligned_addresses(pool, gpu):
    """0 .. 64 KiB of AAD (the cap: 4096 blocks, the 16-lane group strides 256
    times), each from an odd address; a record of no data behind an AAD."""
    aads = [0, 1, 15, 16, 17, 255, 4096, 65536, 13, 65535]
    lens = [100, 100, 16, 0, 1040, 33, 100, 100, 0, 0]
    xs, hx, ad, ha = cut(pool, lens, aads)
    assert ad[1].data_ptr() % 2 == 1 and all(a.data_ptr() % 16 for a in ad[1:8])
    check_both_ways(gpu, KEYS[256], xs, hx, ad, ha, seed=91)


# ---- forgery --------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("what", ["ciphertext", "tag", "aad", "nonce"])
def test_a_forged_record_fails_alone(pool, gpu, what, inplace):
    lens = [1040, 0, 100, 5000, 64, 1, 2049]
    F = 3  # the forged record, in the middle
    xs, hx, ad, ha = cut(pool, lens, [13] * len(lens))
    nv, hn = make_nonces(gpu, len(lens), 31)
    outs, tags = OB.ocb_encrypt_batch(xs, KEY, nv, aads=ad)
    cts = [o.clone() for o in outs]
    tags, nv, ad = tags.clone(), nv.clone(), [a.clone() for a in ad]
    {"ciphertext": cts[F], "tag": tags[F], "aad": ad[F], "nonce": nv[F]}[what][5] ^= 0x10
    d = OB.OcbBatch(cts, KEY, outs=cts if inplace else None, aads=ad)
    pts, ok = d.decrypt(nv, tags)
    assert ok.tolist() == [m != F for m in range(len(lens))]
    got_tags = rows(d.tags)
    for m, p in enumerate(pts):
        if m == F:
            assert host(p) == bytes(lens[m]) and got_tags[m] == bytes(16)  # zeroed, and its tag is not handed out
        else:
            assert host(p) == hx[m] and got_tags[m] == rows(tags)[m]


# ---- nonces are run-time data ----------------------------------------------------------
def test_one_plan_two_nonce_sets(pool, gpu):
    lens = [100, 1024, 0, 5000]
    xs, hx, ad, ha = cut(pool, lens, [13] * 4)
    b = OB.OcbBatch(xs, KEY, aads=ad)
    seen = []
    for seed in (1, 2):
        nv, hn = make_nonces(gpu, 4, seed)
        outs, tags = b.encrypt(nv)
        got = [host(o) for o in outs]
        want = cpu_ref.ocb_batch(KEY, hn, hx, ha)
        assert got == [c for c, _ in want] and rows(tags) == [t for _, t in want]
        seen.append(got)
    assert seen[0][0] != seen[1][0] and seen[0][3] != seen[1][3]


def test_the_batch_against_the_single_message_op(pool, gpu):
    lens = [100, 0, 5000, 1024]
    xs, hx, _, _ = cut(pool, lens)
    aads = [b"header-0", b"", b"header-2 is longer", b"x" * 40]
    nv, hn = make_nonces(gpu, 4, 15)
    m = models.aes.AES(KEYS[192])
    outs, tags = m.ocb_encrypt_batch(xs, nv, aads=aads)
    for i in range(4):
        ct, tag = ops.ocb_ops.ocb_encrypt(xs[i], KEYS[192], hn[i], aads[i])
        assert host(outs[i]) == host(ct) and rows(tags)[i] == host(tag)
    pts, ok = m.ocb_decrypt_batch(outs, nv, tags.clone(), aads=aads)
    assert bool(ok.all())
    for i in range(4):
        assert host(pts[i]) == hx[i]
        assert host(ops.ocb_ops.ocb_decrypt(outs[i], KEYS[192], hn[i], rows(tags)[i], aads[i])) == hx[i]


# ---- graph ---------------------------------------------------------------------------
def test_encrypt_and_decrypt_replay_in_a_graph(pool, gpu):
    """The chain is linear on one stream: captured once, replayed after nonces and inputs changed in place."""
    lens = [1040, 0, 100, 64, 4100]
    n = len(lens)
    xs = [x.clone() for x in cut(pool, lens)[0]]
    nv, _ = make_nonces(gpu, n, 11)
    b = OB.OcbBatch(xs, KEY)
    d = OB.OcbBatch(b.outs, KEY)
    expect = torch.zeros((n, 16), dtype=torch.uint8, device=gpu)
    b.encrypt(nv)  # warm: code objects are loaded outside the capture
    d.decrypt(nv, expect)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.encrypt(nv)
        expect.copy_(b.tags)
        d.decrypt(nv, expect)
    nv2, hn2 = make_nonces(gpu, n, 12)
    nv.copy_(nv2)
    new = [pool["dev"][MIB + 16 * m:MIB + 16 * m + k] for m, k in enumerate(lens)]
    hnew = [pool["host"][MIB + 16 * m:MIB + 16 * m + k] for m, k in enumerate(lens)]
    for x, y in zip(xs, new):
        x.copy_(y)
    g.replay()
    want = cpu_ref.ocb_batch(KEY, hn2, hnew)
    for m in range(n):
        assert host(b.outs[m]) == want[m][0] and rows(b.tags)[m] == want[m][1], m
        assert host(d.outs[m]) == hnew[m] and rows(d.tags)[m] == want[m][1], m
    assert d.ok.tolist() == [1] * n


# ---- the stream contract ---------------------------------------------------------------
DELAY = 0.3      # seconds the pending work in front of every case runs
WINDOW = 0.001   # clock_probe's measuring window behind the delay
A5, Z5 = 0xA5, 0x5A


def independent_stream(gpu, tries=12):
    """A fresh stream that does not share its hardware queue with the default
    stream: work on the default stream finishes while a 5 ms delay still holds
    the candidate."""
    default = torch.cuda.default_stream(gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    for _ in range(tries):
        s = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(s):
            probe = ops.clock_probe(0.005, WINDOW, stream=s)
        behind = torch.cuda.Event()
        behind.record(s)
        with torch.cuda.stream(default):
            flag.add_(1)
        done = torch.cuda.Event()
        done.record(default)
        done.synchronize()
        independent = not behind.query()
        s.synchronize()
        del probe
        if independent:
            return s
    raise AssertionError("no fresh stream runs independently of the default stream: the order check proves nothing here")


def run_contract(gpu, inputs, fresh, outs, call, expect):
    """The method of tests/test_gpu_async_contract.py: behind a delay on a fresh
    independent stream go, with no host wait in between, the copies that
    PRODUCE the op's inputs (``fresh`` into ``inputs``), the op, and copies
    that CONSUME its results.  The event behind the delay has not fired when
    the enqueue returns, and the consumed bytes equal ``expect`` (the oracle
    over the fresh inputs)."""
    stale = [t.clone() for t in inputs]
    zs = [torch.empty(len(e), dtype=torch.uint8, device=gpu) for e in expect]
    s = independent_stream(gpu)

    def enqueue(delay):
        with torch.cuda.stream(s):
            probe = ops.clock_probe(delay, WINDOW, stream=s)
            e_d = torch.cuda.Event()
            e_d.record(s)
            for inp, f in zip(inputs, fresh):
                inp.copy_(f)
            res = call(s)
            assert len(res) == len(expect)
            for r, z in zip(res, zs):
                z.copy_(r.reshape(-1).view(torch.uint8))
            return not e_d.query(), probe

    try:
        t0 = time.perf_counter()
        enqueue(0.0)  # warm-up: code objects, allocator caches
        s.synchronize()
        t0 = time.perf_counter()
        enqueue(0.0)
        t_enqueue = time.perf_counter() - t0
        s.synchronize()
        assert t_enqueue < DELAY / 4, f"inconclusive: the host enqueue took {t_enqueue * 1e3:.1f} ms"
        for inp, o in zip(inputs, stale):
            inp.copy_(o)
        for o in outs:
            o.fill_(A5)
        for z in zs:
            z.fill_(Z5)
        torch.cuda.synchronize()
        waiting, probe = enqueue(DELAY)
        s.synchronize()
        for i, (z, e) in enumerate(zip(zs, expect)):
            assert host(z) == e, f"order: result {i} differs from the oracle over the late inputs"
        assert waiting, "host wait: the delay in front of the call had finished when the enqueue returned"
    finally:
        torch.cuda.synchronize()


def contract_setup(pool, gpu):
    lens = [1040, 0, 100, 8193]
    xs = [x.clone() for x in cut(pool, lens)[0]]
    fresh = [pool["dev"][MIB + 16 * m:MIB + 16 * m + n].clone() for m, n in enumerate(lens)]
    hf = [pool["host"][MIB + 16 * m:MIB + 16 * m + n] for m, n in enumerate(lens)]
    aad = pool["dev"][AAD_AT:AAD_AT + 13 * 4].clone().view(4, 13)
    faad = pool["dev"][AAD_AT + 100:AAD_AT + 100 + 13 * 4].clone().view(4, 13)
    hfa = [pool["host"][AAD_AT + 100 + 13 * m:AAD_AT + 113 + 13 * m] for m in range(4)]
    nv, _ = make_nonces(gpu, 4, 21)
    fnv, hn = make_nonces(gpu, 4, 22)
    return lens, xs, fresh, hf, aad, faad, hfa, nv, fnv, hn


def test_stream_contract_encrypt(pool, gpu):
    lens, xs, fresh, hf, aad, faad, hfa, nv, fnv, hn = contract_setup(pool, gpu)
    b = OB.OcbBatch(xs, KEY, aads=aad)
    want = cpu_ref.ocb_batch(KEY, hn, hf, hfa)

    def call(s):
        outs, tags = b.encrypt(nv, stream=s)
        return list(outs) + [tags]

    run_contract(gpu, xs + [aad, nv], fresh + [faad, fnv], b.outs + [b.tags], call,
                 [w[0] for w in want] + [b"".join(w[1] for w in want)])


def test_stream_contract_decrypt(pool, gpu):
    lens, xs, fresh, hf, aad, faad, hfa, nv, fnv, hn = contract_setup(pool, gpu)
    # the late inputs are ciphertexts with their tags: decrypt returns the plaintexts and all-true verdicts
    sealed = cpu_ref.ocb_batch(KEY, hn, hf, hfa)
    fresh = [dev_bytes(gpu, c) if c else f for (c, _), f in zip(sealed, fresh)]
    ftags = dev_bytes(gpu, b"".join(t for _, t in sealed)).view(4, 16)
    tags = torch.zeros_like(ftags)
    b = OB.OcbBatch(xs, KEY, aads=aad)

    def call(s):
        outs, ok = b.decrypt(nv, tags, stream=s)
        return list(outs) + [ok.view(torch.uint8)]

    run_contract(gpu, xs + [aad, nv, tags], fresh + [faad, fnv, ftags], b.outs + [b.ok], call, hf + [b"\x01" * 4])
