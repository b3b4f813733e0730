"""Batched AES-CCM on the device (csrc/hip/aes_ccm_batch.hip through
ops.ccm_batch_ops.CcmBatch): many records under one key, one nonce length and
one tag length per batch, each record with its own nonce, AAD and tag.  Every
byte and every tag is compared with the C oracle per record (cpu_ref.ccm,
pinned to SP 800-38C / RFC 3610 and to a Python model in tests/test_ccm_cpu.py),
and the vectors of tests/golden/ccm_vectors.json run as batches, one per nonce
and tag length.

The kernel runs one record per lane, so the shapes are counts of records -- a
wave and one more, past a workgroup, past the grid's first step
(otc_ccm_batch_spans) -- and lengths around a block, a burst of 8 blocks and
the counter's first carry at block 256.  Data and AADs are slices of one seeded
pool; the AADs start at odd addresses on purpose."""
import json
import os

import numpy as np
import pytest
import torch

from our_tree_amd import models, ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

CB = ops.ccm_batch_ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ccm_vectors.json")) as f:
    _V = json.load(f)
VECTORS = _V["published"] + _V["cross_checks"]

MIB = 1 << 20
DATA = 3 * MIB                # the pool's data region: records are cut from its front, 16-byte aligned
AAD_AT = DATA + 1             # the AAD region starts at an odd address
POOL = DATA + 512 * 1024
KEYS = {128: bytes(range(3, 19)), 192: bytes(range(60, 84)), 256: bytes(range(201, 233))}
KEY = KEYS[128]
# around a block, two blocks, a burst of 8 blocks (128 bytes), 256 blocks, and 4113: block 257, behind the carry
EDGES = [0, 1, 15, 16, 17, 31, 32, 127, 128, 129, 4096, 4097, 4113]

_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host.  Never written."""
    if not _pool:
        g = torch.Generator(device=gpu).manual_seed(53)
        dev = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes())
    return _pool


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def cut(pool, lens, aad_lens=None, aad_shift=0):
    """Records of these lengths from the pool: (device views, host bytes,
    device AAD views, host AADs).  Data slots are 16-byte aligned and back to
    back; AADs are packed byte by byte from an odd address (+ aad_shift)."""
    xs, hx, at = [], [], 0
    for n in lens:
        xs.append(pool["dev"][at:at + n])
        hx.append(pool["host"][at:at + n])
        at += (n + 15) // 16 * 16
    assert at <= DATA
    aad_lens = aad_lens or [0] * len(lens)
    ad, ha, at = [], [], AAD_AT + aad_shift
    for n in aad_lens:
        ad.append(pool["dev"][at:at + n])
        ha.append(pool["host"][at:at + n])
        at += n
    assert at <= POOL
    return xs, hx, ad, ha


def make_nonces(gpu, n, seed, width=12):
    b = np.random.default_rng(seed).integers(0, 256, (n, width), dtype=np.uint8)
    return torch.from_numpy(b).to(gpu), [r.tobytes() for r in b]


def rows(t: torch.Tensor, width=16):
    b = host(t)
    return [b[i:i + width] for i in range(0, len(b), width)]


def dev_bytes(gpu, b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)


def check_both_ways(gpu, key, xs, hx, ad, ha, seed, inplace=False, nb=12, tb=16):
    """Encrypt the records, compare every ciphertext and tag with the oracle;
    decrypt them again, compare every plaintext, tag and verdict."""
    n = len(xs)
    nv, hn = make_nonces(gpu, n, seed, nb)
    want = cpu_ref.ccm_batch(key, hn, hx, ha, tag_bytes=tb)
    if inplace:
        xs = [x.clone() for x in xs]
    b = CB.CcmBatch(xs, key, outs=xs if inplace else None, aads=ad, nonce_bytes=nb, tag_bytes=tb)
    outs, tags = b.encrypt(nv)
    assert tuple(tags.shape) == (n, tb)
    got_t = rows(tags, tb)
    for m, (ct, tag) in enumerate(want):
        assert host(outs[m]) == ct, (m, len(hx[m]), "ciphertext")
        assert got_t[m] == tag, (m, len(hx[m]), len(ha[m]), "tag", got_t[m].hex(), tag.hex())
    d = b if inplace else CB.CcmBatch(outs, key, aads=ad, nonce_bytes=nb, tag_bytes=tb)
    pts, ok = d.decrypt(nv, tags.clone())
    assert ok.dtype == torch.bool and ok.tolist() == [True] * n
    got_t = rows(d.tags, tb)
    for m in range(n):
        assert host(pts[m]) == hx[m], (m, len(hx[m]), "plaintext")
        assert got_t[m] == want[m][1], (m, "tag of the decryption")
    return b


# ---- the golden vectors ----------------------------------------------------------------
def vec_fields(v):
    count = lambda n: bytes(i & 255 for i in range(n))
    H = bytes.fromhex
    return (H(v["key"]), H(v["nonce"]), count(v["aad_count"]) if "aad_count" in v else H(v["aad"]),
            count(v["pt_count"]) if "pt_count" in v else H(v["pt"]), H(v["ct"]) if "ct" in v else None,
            H(v["ct_tail"]) if "ct_tail" in v else None, H(v["tag"]))


def test_vectors_as_batches_one_per_key_nonce_and_tag_length(gpu):
    groups = {}
    for v in VECTORS:
        f = vec_fields(v)
        groups.setdefault((f[0], len(f[1]), len(f[6])), []).append((v["name"], f))
    assert len(VECTORS) == 12 and len(groups) >= 7
    assert {(nl, tl) for _, nl, tl in groups} >= {(7, 4), (8, 6), (12, 8), (13, 14), (13, 8), (12, 16), (13, 16)}
    for (key, nl, tl), vs in groups.items():
        xs = [dev_bytes(gpu, f[3]) for _, f in vs]
        aads = [f[2] for _, f in vs]
        nv = dev_bytes(gpu, b"".join(f[1] for _, f in vs)).view(len(vs), nl)
        outs, tags = CB.ccm_encrypt_batch(xs, key, nv, aads=aads, tag_bytes=tl)
        for m, (name, f) in enumerate(vs):
            got = host(outs[m])
            assert rows(tags, tl)[m] == f[6], name
            if f[4] is not None:
                assert got == f[4], name
            if f[5] is not None:
                assert got[-len(f[5]):] == f[5], name
        pts, ok = CB.ccm_decrypt_batch(outs, key, nv, tags.clone(), aads=aads)
        assert bool(ok.all()) and [host(p) for p in pts] == [f[3] for _, f in vs]


# ---- one record ------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_one_record_at_every_edge(pool, gpu, bits):
    """Each edge length as a batch of ONE record (one live lane) behind a
    13-byte AAD, both directions, for the shortest, the usual and the longest
    nonce and tag."""
    spans = CB.CcmBatch.spans()
    assert spans[:2] == [16, 128] and 129 in EDGES and 4113 // 16 == 257
    for nb in (7, 12, 13):
        for tb in (4, 8, 16):
            for n in EDGES:
                xs, hx, ad, ha = cut(pool, [n], [13])
                check_both_ways(gpu, KEYS[bits], xs, hx, ad, ha, seed=1000 + n, nb=nb, tb=tb)


def test_the_length_fields_limit_under_a_13_byte_nonce(pool, gpu):
    """L = 2: 65535 bytes run, 65536 are refused at planning."""
    xs, hx, ad, ha = cut(pool, [65535], [7])
    check_both_ways(gpu, KEYS[192], xs, hx, ad, ha, seed=3, nb=13, tb=8)
    xs, _, _, _ = cut(pool, [100, 65536])
    with pytest.raises(ValueError, match="record 1.*length field"):
        CB.CcmBatch(xs, KEY, nonce_bytes=13)
    CB.CcmBatch(xs, KEY, nonce_bytes=12)


def test_one_mib_record(pool, gpu):
    """The cap: one lane, 65536 steps, counters up to 2^16; in place."""
    xs, hx, ad, ha = cut(pool, [MIB], [5])
    check_both_ways(gpu, KEYS[256], xs, hx, ad, ha, seed=5, inplace=True)
    xs, hx, ad, ha = cut(pool, [MIB - 1], [0])
    check_both_ways(gpu, KEYS[128], xs, hx, ad, ha, seed=6, nb=7, tb=4)
    big = torch.zeros(MIB + 16, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="1 MiB"):
        CB.CcmBatch([big], KEY)


# ---- lanes and the order -----------------------------------------------------------------
def test_a_full_wave_and_one_more_lane(pool, gpu):
    lens = [(37 * i) % 300 for i in range(65)]
    xs, hx, ad, ha = cut(pool, lens, [(i * 5) % 23 for i in range(65)])
    check_both_ways(gpu, KEY, xs, hx, ad, ha, seed=65)
    check_both_ways(gpu, KEYS[256], xs, hx, ad, ha, seed=66, inplace=True, nb=13, tb=4)


def test_shuffled_distinct_lengths_land_in_their_own_buffers(pool, gpu):
    """130 records of distinct lengths 0, 7, .., 129 * 7 in a shuffled order:
    the planner's order is a real permutation, and a wrong one would put a
    record's output (or tag) in another's place."""
    lens = [7 * i for i in range(130)]
    np.random.default_rng(130).shuffle(lens)
    xs, hx, ad, ha = cut(pool, lens, [13] * 130)
    b = check_both_ways(gpu, KEYS[192], xs, hx, ad, ha, seed=130)
    blocks = [(n + 15) // 16 for n in lens]
    assert b.order.tolist() == sorted(range(130), key=lambda m: -blocks[m])
    assert b.order.tolist() != list(range(130))
    # any permutation is a valid order: the records as given compute the same
    nv, hn = make_nonces(gpu, 130, 131)
    ident = CB.CcmBatch(xs, KEYS[192], aads=ad, _sort=False)
    assert ident.order.tolist() == list(range(130))
    outs, tags = ident.encrypt(nv)
    want = cpu_ref.ccm_batch(KEYS[192], hn, hx, ha)
    assert [host(o) for o in outs] == [c for c, _ in want] and rows(tags) == [t for _, t in want]


def test_past_one_workgroup(pool, gpu):
    assert CB.CcmBatch.spans()[3] == 1024
    lens = [(i * 13) % 90 for i in range(1025)]
    total = sum((n + 15) // 16 * 16 for n in lens)
    buf = pool["dev"][:total].clone()
    offs = np.concatenate([[0], np.cumsum([(n + 15) // 16 * 16 for n in lens])[:-1]])
    hx = [pool["host"][o:o + n] for o, n in zip(offs, lens)]
    nv, hn = make_nonces(gpu, 1025, 1025, 11)
    want = cpu_ref.ccm_batch(KEY, hn, hx, tag_bytes=10)
    b = CB.CcmBatch.packed(buf, lens, KEY, nonce_bytes=11, tag_bytes=10)
    _, tags = b.encrypt(nv)
    o = host(b.out)
    assert [o[at:at + n] for at, n in zip(offs, lens)] == [c for c, _ in want]
    assert rows(tags, 10) == [t for _, t in want]
    d = CB.CcmBatch.packed(b.out, lens, KEY, out=b.out, nonce_bytes=11, tag_bytes=10)
    _, ok = d.decrypt(nv, tags.clone())
    o = host(d.out)
    assert bool(ok.all()) and [o[at:at + n] for at, n in zip(offs, lens)] == hx


def test_a_batch_past_the_grids_first_step(gpu):
    """spans()[-1] + 65 records of 16 .. 32 bytes in 32-byte slots: a wave takes a
    second record per lane, the last wave has one live lane.  The oracle runs
    on the first, the last and 1500 random places of the order (the records past
    the first step are the order's last); every record is then opened on the
    device and compared with its plaintext."""
    first_step = CB.CcmBatch.spans()[-1]
    n = first_step + 65
    rng = np.random.default_rng(99)
    lens = rng.integers(16, 33, n)
    offs = np.arange(n, dtype=np.int64) * 32
    g = torch.Generator(device=gpu).manual_seed(98)
    buf = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device=gpu, generator=g)
    hb = host(buf)
    nv = torch.randint(0, 256, (n, 12), dtype=torch.uint8, device=gpu, generator=g)
    hn = host(nv)
    b = CB.CcmBatch.packed(buf, lens, KEY, offsets=offs, tag_bytes=8)
    assert b.n == first_step + 65 and int(lens[b.order[-1]]) == 16  # the one-block records are the order's last
    _, tags = b.encrypt(nv)
    out, ht = host(b.out), host(tags)
    picks = np.concatenate([b.order[:500], b.order[-1500:], rng.integers(0, n, 1500)])
    for m in picks.tolist():
        o, k = int(offs[m]), int(lens[m])
        ct, tag = cpu_ref.ccm(KEY, hn[12 * m:12 * m + 12], hb[o:o + k], tag_bytes=8)
        assert out[o:o + k] == ct and ht[8 * m:8 * m + 8] == tag, m
    d = CB.CcmBatch.packed(b.out, lens, KEY, out=b.out, offsets=offs, tag_bytes=8)
    _, ok = d.decrypt(nv, tags.clone())
    assert bool(ok.all())
    keep = (torch.arange(32, device=gpu)[None, :] < torch.from_numpy(lens).to(gpu)[:, None]).reshape(-1)
    assert torch.equal(d.out[keep], buf[keep])


# ---- the AAD -----------------------------------------------------------------------------
AAD_LENS = [0, 1, 13, 14, 15, 16, 29, 30, 31, 65279, 65280, 65536]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_aad_lengths_at_every_misalignment(pool, gpu, shift):
    """Around one and two MAC blocks behind the 2-byte length (14 and 30 fill
    them), either side of the encodings' switch at 0xFF00 and at the cap, each
    at an address misaligned by shift + 1 .. (the AADs are packed byte by byte);
    then the same AADs over records of NO data."""
    lens = [100, 17, 16, 0, 129, 33, 100, 1, 0, 17, 17, 40]
    xs, hx, ad, ha = cut(pool, lens, AAD_LENS, aad_shift=shift)
    assert {a.data_ptr() % 4 for a in ad[1:]} == {0, 1, 2, 3}
    check_both_ways(gpu, KEYS[256], xs, hx, ad, ha, seed=91 + shift)
    xs, hx, ad, ha = cut(pool, [0] * len(AAD_LENS), AAD_LENS, aad_shift=shift)
    check_both_ways(gpu, KEY, xs, hx, ad, ha, seed=95 + shift, nb=13, tb=8)


def test_aads_as_a_tensor_and_as_host_bytes(pool, gpu):
    lens = [100, 0, 129, 16]
    xs, hx, _, _ = cut(pool, lens)
    nv, hn = make_nonces(gpu, 4, 17)
    aad = pool["dev"][AAD_AT:AAD_AT + 4 * 21].view(4, 21)
    ha = [pool["host"][AAD_AT + 21 * m:AAD_AT + 21 * m + 21] for m in range(4)]
    want = cpu_ref.ccm_batch(KEY, hn, hx, ha)
    for aads in (aad, ha, [aad[0], ha[1], aad[2], bytearray(ha[3])]):
        outs, tags = CB.CcmBatch(xs, KEY, aads=aads).encrypt(nv)
        assert [host(o) for o in outs] == [c for c, _ in want] and rows(tags) == [t for _, t in want]


# ---- layouts ---------------------------------------------------------------------------
def mixed(pool, gpu):
    lens, aads = [], []
    for i in range(200):
        lens.append(0 if i % 5 == 1 else EDGES[(i // 3 * 7 + i) % len(EDGES)] + (2048 if i % 11 == 0 else 0))
        aads.append([0, 13, 16, 14, 1, 40][i % 6] if i % 4 else 0)
    xs, hx, ad, ha = cut(pool, lens, aads)
    nv, hn = make_nonces(gpu, 200, 77)
    want = cpu_ref.ccm_batch(KEY, hn, hx, ha)
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
    b = CB.CcmBatch(xs, KEY, outs=xs if inplace else None, aads=ad)
    _, tags = b.encrypt(nv)
    got_t = rows(tags)
    for m, (ct, tag) in enumerate(want):
        assert host(b.outs[m]) == ct and got_t[m] == tag, (m, lens[m])
    d = b if inplace else CB.CcmBatch(b.outs, KEY, outs=b.outs, aads=ad)
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
    want13 = cpu_ref.ccm_batch(KEY, hn, hx, ha13)
    b = CB.CcmBatch.packed(buf, lens, KEY, out=buf if inplace else None, aad=aad)
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
    d = CB.CcmBatch.packed(b.out, lens, KEY, out=b.out, aad=aad)
    _, ok = d.decrypt(nv, tags.clone())
    assert bool(ok.all()) and outs_bytes() == hx


# ---- forgery --------------------------------------------------------------------------
@pytest.mark.parametrize("tb", [4, 16])
@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("what", ["ciphertext", "tag", "aad", "nonce"])
def test_a_forged_record_fails_alone(pool, gpu, what, inplace, tb):
    lens = [1040, 0, 100, 5000, 64, 1, 2049]
    F = 3  # the forged record, in the middle
    xs, hx, ad, ha = cut(pool, lens, [13] * len(lens))
    nv, hn = make_nonces(gpu, len(lens), 31)
    outs, tags = CB.ccm_encrypt_batch(xs, KEY, nv, aads=ad, tag_bytes=tb)
    cts = [o.clone() for o in outs]
    tags, nv, ad = tags.clone(), nv.clone(), [a.clone() for a in ad]
    {"ciphertext": cts[F], "tag": tags[F], "aad": ad[F], "nonce": nv[F]}[what][3] ^= 0x10
    d = CB.CcmBatch(cts, KEY, outs=cts if inplace else None, aads=ad, tag_bytes=tb)
    pts, ok = d.decrypt(nv, tags)
    assert ok.tolist() == [m != F for m in range(len(lens))]
    got_tags = rows(d.tags, tb)
    for m, p in enumerate(pts):
        if m == F:
            assert host(p) == bytes(lens[m]) and got_tags[m] == bytes(tb)  # zeroed, and its tag is not handed out
        else:
            assert host(p) == hx[m] and got_tags[m] == rows(tags, tb)[m]


# ---- nonces are run-time data ----------------------------------------------------------
def test_one_plan_two_nonce_sets(pool, gpu):
    lens = [100, 1024, 0, 5000]
    xs, hx, ad, ha = cut(pool, lens, [13] * 4)
    b = CB.CcmBatch(xs, KEY, aads=ad)
    seen = []
    for seed in (1, 2):
        nv, hn = make_nonces(gpu, 4, seed)
        outs, tags = b.encrypt(nv)
        got = [host(o) for o in outs]
        want = cpu_ref.ccm_batch(KEY, hn, hx, ha)
        assert got == [c for c, _ in want] and rows(tags) == [t for _, t in want]
        seen.append(got)
    assert seen[0][0] != seen[1][0] and seen[0][3] != seen[1][3]


def test_the_batch_against_the_single_message_op(pool, gpu):
    lens = [100, 0, 5000, 1024]
    xs, hx, _, _ = cut(pool, lens)
    aads = [b"header-0", b"", b"header-2 is longer", b"x" * 40]
    nv, hn = make_nonces(gpu, 4, 15, 13)
    m = models.aes.AES(KEYS[192])
    outs, tags = m.ccm_encrypt_batch(xs, nv, aads=aads, tag_bytes=12)
    for i in range(4):
        ct, tag = CB.ccm_encrypt(xs[i], KEYS[192], hn[i], aads[i], tag_bytes=12)
        assert host(outs[i]) == host(ct) and rows(tags, 12)[i] == tag
    pts, ok = m.ccm_decrypt_batch(outs, nv, tags.clone(), aads=aads)
    assert bool(ok.all())
    for i in range(4):
        assert host(pts[i]) == hx[i]
        assert host(CB.ccm_decrypt(outs[i], KEYS[192], hn[i], rows(tags, 12)[i], aads[i])) == hx[i]
    bad = bytearray(rows(tags, 12)[2])
    bad[11] ^= 1
    with pytest.raises(cpu_ref.CcmTagError) as e:
        CB.ccm_decrypt(outs[2], KEYS[192], hn[2], bytes(bad), aads[2])
    assert host(e.value.output) == bytes(5000)
    with pytest.raises(ValueError, match="7 to 13"):
        CB.ccm_encrypt(xs[0], KEY, bytes(14))
    with pytest.raises(ValueError, match="fewer than"):
        CB.ccm_encrypt(pool["dev"][:65536], KEY, bytes(13))
