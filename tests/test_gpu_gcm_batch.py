"""Batched AES-GCM on the device (csrc/hip/aes_gcm_batch.hip through
ops.GcmBatch): many records under one key, each with its own 12-byte IV, AAD
and tag.  Everything is compared exactly against the C oracle (cpu_ref.gcm /
cpu_ref.ghash, pinned to known answers in tests/test_gcm_cpu.py).

The hash shapes come from the kernel's own decomposition
(otc_gcm_batch_spans, in HASHED blocks: AAD blocks + data blocks + the length
block), so the data lengths are derived from the hashed block count wanted,
with and without an AAD block in front.  Data and AADs are slices of one
seeded pool; the AADs start at odd addresses on purpose."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from our_tree_amd import _native, models, ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "gcm_vectors.json")))["vectors"]

MIB = 1 << 20
DATA = 3 * MIB                # the pool's data region: records are cut from its front, 16-byte aligned
AAD_AT = DATA + 1             # the AAD region starts at an odd address
POOL = DATA + 256 * 1024
KEYS = {16: bytes(range(3, 19)), 24: bytes(range(40, 64)), 32: bytes(range(101, 133))}
KEY = KEYS[16]

_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host.  Never written."""
    if not _pool:
        g = torch.Generator(device=gpu).manual_seed(41)
        dev = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes())
    return _pool


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


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


def make_ivs(gpu, n, seed):
    b = np.random.default_rng(seed).integers(0, 256, (n, 12), dtype=np.uint8)
    return torch.from_numpy(b).to(gpu), [r.tobytes() for r in b]


# ---- the hash alone ---------------------------------------------------------------
def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


@functools.lru_cache(maxsize=None)
def _h(key):
    return cpu_ref.gcm_h(key)


def ref_hash(key, data, aad):
    return cpu_ref.ghash(_h(key), pad16(aad) + pad16(data) + (8 * len(aad)).to_bytes(8, "big") +
                         (8 * len(data)).to_bytes(8, "big"))


def check_hash(pool, lens, aad_lens=None, key=KEY, lanes=(16, 64)):
    """Both forms of the kernel: 16 and 64 lanes per record."""
    xs, hx, ad, ha = cut(pool, lens, aad_lens)
    want = [ref_hash(key, d, a) for d, a in zip(hx, ha)]
    for ln in lanes:
        got = host(ops.ghash_batch(xs, key, aads=ad if aad_lens else None, lanes=ln))
        for m, w in enumerate(want):
            assert got[16 * m:16 * m + 16] == w, (ln, m, lens[m], len(ha[m]), got[16 * m:16 * m + 16].hex(), w.hex())


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1007, 1008, 1009])
def test_hash_one_record(pool, n, lanes):
    """The narrowest case: one record, no AAD."""
    check_hash(pool, [n], lanes=(lanes,))


def test_hash_byte_lengths_with_aad(pool):
    check_hash(pool, [0, 1, 15, 16, 17, 1007, 1008, 1009], [13] * 8)


def test_spans_are_reported(gpu):
    spans = ops.gcm_batch_spans()
    assert spans and spans[0] == 16 and 64 in spans and spans == sorted(set(spans))


def test_hash_around_every_span(pool):
    """Records whose HASHED block count is S-1, S, S+1, 2S+1 for every span,
    reached once by data alone (nb = data blocks + 1) and once behind a
    13-byte AAD (nb = 1 + data blocks + 1); the last data block once full and
    once holding a single byte."""
    spans = [s for s in ops.gcm_batch_spans() if s <= 4096]
    assert spans
    lens, aads = [], []
    for s in spans:
        for nb in (s - 1, s, s + 1, 2 * s + 1):
            for aad, nd in ((0, nb - 1), (13, nb - 2)):
                for n in (16 * nd, 16 * nd - 15):
                    lens.append(n)
                    aads.append(aad)
    check_hash(pool, lens, aads)


MIX_LENS = [0, 1, 16, 17, 63 * 16, 64 * 16 + 1, 4111]
MIX_AADS = [0, 1, 13, 16, 17, 1040]


@pytest.mark.parametrize("n", [16, 17, 33, 64, 65])
def test_hash_mixed_lengths_in_one_workgroup(pool, n):
    """Short and long records side by side: the shared fold starts at the first
    lane ANY of a group's 16 records uses."""
    check_hash(pool, [MIX_LENS[i % 7] for i in range(n)], [MIX_AADS[i % 6] for i in range(n)])


@pytest.mark.parametrize("where", ["first", "last", "none"])
def test_hash_one_long_record_in_a_group(pool, where):
    for group in (16, 64):  # the records of a workgroup with 64 and with 16 lanes per record
        lens = [5 + i % 11 for i in range(group)]  # 2 hashed blocks each: the fold would start at the last lane but one
        if where != "none":
            lens[0 if where == "first" else group - 1] = 64 * 16 + 1
        check_hash(pool, lens)
        check_hash(pool, lens + [3], [0] * group + [17])


@pytest.mark.parametrize("n", [1, 2, 15])
def test_hash_small_batches(pool, n):
    check_hash(pool, [16 + 5 * i for i in range(n)], [5] * n)


def test_hash_grid_wrap(pool, gpu):
    """More groups of records than workgroups: with 16 lanes per record (64
    records per workgroup) the grid-stride loop runs twice and the last group
    is partial, with 64 lanes (16 records) eight times.  Packed layout, AADs as
    one [n, 5] tensor."""
    n = 2 * 64 * _native.require_gpu_lib().otc_device_cus(0) + 5
    lens = [16 + (i * 37) % 81 for i in range(n)]
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum([(v + 15) // 16 * 16 for v in lens[:-1]])
    assert offs[-1] + lens[-1] <= DATA and 5 * n <= POOL - AAD_AT
    aad = pool["dev"][AAD_AT:AAD_AT + 5 * n].view(n, 5)
    want = [ref_hash(KEY, pool["host"][offs[m]:offs[m] + lens[m]], pool["host"][AAD_AT + 5 * m:AAD_AT + 5 * m + 5])
            for m in range(n)]
    for lanes in (16, 64):
        b = ops.GcmBatch.packed(pool["dev"][:DATA], lens, KEY, out=pool["dev"][:DATA], aad=aad, lanes=lanes)
        got = host(b.ghash())
        for m in range(n):
            assert got[16 * m:16 * m + 16] == want[m], (lanes, m)


# ---- full GCM ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(key, iv, at, n, aad_at, na):
    """(ciphertext, tag) of the pool's bytes [at, at + n) with the AAD [aad_at, aad_at + na)"""
    return cpu_ref.gcm(key, iv, _pool["host"][at:at + n], _pool["host"][aad_at:aad_at + na])


def check_gcm(pool, gpu, key, lens, aad_lens=None, inplace=False, ivs=None, seed=1):
    """Seal the records, compare with the oracle, open them again."""
    xs, hx, ad, ha = cut(pool, lens, aad_lens)
    n = len(lens)
    xs = [x.clone() for x in xs]  # 16-byte aligned fresh buffers (the pool stays read-only)
    outs = xs if inplace else [torch.full_like(x, 0xA5) for x in xs]
    iv_dev, iv_host = ivs if ivs is not None else make_ivs(gpu, n, seed)
    b = ops.GcmBatch(xs, key, outs=outs, aads=ad if aad_lens else None)
    got, tags = b.encrypt(iv_dev)
    tags_h = host(tags)
    want = [cpu_ref.gcm(key, iv_host[m], hx[m], ha[m]) for m in range(n)]
    for m in range(n):
        assert host(got[m]) == want[m][0], (m, lens[m])
        assert tags_h[16 * m:16 * m + 16] == want[m][1], (m, lens[m])
    # and back: the ciphertext as input, the computed tags as the expected ones
    cts = [o.clone() for o in got]
    pts = cts if inplace else [torch.full_like(c, 0xA5) for c in cts]
    d = ops.GcmBatch(cts, key, outs=pts, aads=ad if aad_lens else None)
    back, ok = d.decrypt(iv_dev, tags.clone())
    assert ok.dtype == torch.bool and bool(ok.all())
    assert host(d.tags) == tags_h
    for m in range(n):
        assert host(back[m]) == hx[m], (m, lens[m])


TILE_LENS = [v + d for v in (1024, 2048, 4096) for d in (-16, -1, 0, 1, 16)] + [65541]


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_gcm_around_the_ctr_tiles(pool, gpu, keylen, inplace):
    check_gcm(pool, gpu, KEYS[keylen], TILE_LENS, [(13 * i) % 40 for i in range(len(TILE_LENS))], inplace, seed=keylen)


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_gcm_the_cap_next_to_one_byte(pool, gpu, inplace):
    check_gcm(pool, gpu, KEYS[32], [MIB, 1], [0, 7], inplace, seed=5)


def test_gcm_gmac_and_empty_records(pool, gpu):
    check_gcm(pool, gpu, KEY, [0], [20], seed=6)                 # GMAC
    check_gcm(pool, gpu, KEY, [0, 0, 0], None, seed=7)           # all empty, no AAD: tag = E_K(J0)
    check_gcm(pool, gpu, KEY, [0, 33, 0, 0], [20, 0, 0, 1], seed=8)


def test_gcm_ivs_of_all_ff(pool, gpu):
    """The counter's low word starts at 2 whatever the IV: no carry out of it
    into the IV's bytes."""
    n = 4
    ivs = (torch.full((n, 12), 0xFF, dtype=torch.uint8, device=gpu), [b"\xff" * 12] * n)
    check_gcm(pool, gpu, KEYS[24], [4097, 17, 65541, 0], [3, 0, 0, 5], ivs=ivs)


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
def test_gcm_packed_keeps_slack_and_guard(pool, gpu, decrypt, inplace):
    """Back-to-back 16-byte slots, lengths no multiples of 16: the slack bytes
    of every slot and 64 guard bytes behind the buffer keep their fill."""
    lens = [1, 15, 17, 100, 4095, 4097, 33, 0, 1025, 7]
    n = len(lens)
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum([(v + 15) // 16 * 16 for v in lens[:-1]])
    total = int(offs[-1] + (lens[-1] + 15) // 16 * 16)
    key = KEYS[32]
    iv_dev, iv_host = make_ivs(gpu, n, 11)
    aad = pool["dev"][AAD_AT:AAD_AT + 13 * n].view(n, 13)
    refs = [_ref(key, iv_host[m], int(offs[m]), lens[m], AAD_AT + 13 * m, 13) for m in range(n)]
    src = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    for m in range(n):  # plaintext (encrypt) or ciphertext (decrypt) in the slots
        rec = refs[m][0] if decrypt else pool["host"][offs[m]:offs[m] + lens[m]]
        src[offs[m]:offs[m] + lens[m]] = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(gpu) if lens[m] else src[0:0]
    dst = src if inplace else torch.full_like(src, 0xA5)
    b = ops.GcmBatch.packed(src[:total], lens, key, out=dst[:total], aad=aad)
    if decrypt:
        tags = torch.frombuffer(bytearray(b"".join(r[1] for r in refs)), dtype=torch.uint8).to(gpu).view(n, 16)
        _, ok = b.decrypt(iv_dev, tags)
        assert bool(ok.all())
    else:
        _, tags = b.encrypt(iv_dev)
        assert host(tags) == b"".join(r[1] for r in refs)
    got = host(dst)
    for m in range(n):
        want = pool["host"][offs[m]:offs[m] + lens[m]] if decrypt else refs[m][0]
        assert got[offs[m]:offs[m] + lens[m]] == want, m
        end = int(offs[m + 1]) if m + 1 < n else total
        assert got[offs[m] + lens[m]:end] == b"\xa5" * (end - int(offs[m]) - lens[m]), f"slack of record {m}"
    assert got[total:] == b"\xa5" * 64, "guard bytes"


def test_golden_vectors_as_batches(gpu):
    """The known answers with 12-byte IVs, grouped by key: one batch per key."""
    groups = {}
    for v in VECTORS:
        if len(v["iv"]) == 24:
            groups.setdefault(v["key"], []).append(v)
    assert len(groups) >= 3 and any(len(g) > 1 for g in groups.values())
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)
    for key, vs in groups.items():
        f = [{k: bytes.fromhex(v[k]) for k in ("iv", "aad", "pt", "ct", "tag")} for v in vs]
        ivs = dev(b"".join(x["iv"] for x in f)).view(len(f), 12)
        aes = models.AESGCM(bytes.fromhex(key))
        outs, tags = aes.encrypt_batch([dev(x["pt"]) for x in f], ivs, aads=[x["aad"] for x in f])
        assert [host(o) for o in outs] == [x["ct"] for x in f]
        assert host(tags) == b"".join(x["tag"] for x in f)
        outs, ok = aes.decrypt_batch([dev(x["ct"]) for x in f], ivs, dev(b"".join(x["tag"] for x in f)).view(len(f), 16),
                                     aads=[dev(x["aad"]) for x in f])
        assert bool(ok.all()) and [host(o) for o in outs] == [x["pt"] for x in f]


# ---- replay -----------------------------------------------------------------------
def test_replay_with_new_data_and_new_ivs(pool, gpu):
    """One plan, two runs, then a captured graph replayed: new data in the same
    buffers and new IVs in the same tensor each time."""
    lens, aads = [4096, 777, 0, 12289, 16], [13, 0, 20, 1, 0]
    n = len(lens)
    _, _, ad, ha = cut(pool, lens, aads)
    xs = [torch.empty(v, dtype=torch.uint8, device=gpu) for v in lens]
    b = ops.GcmBatch(xs, KEYS[32], aads=ad)
    ivs = torch.empty((n, 12), dtype=torch.uint8, device=gpu)

    def load(shift, seed):
        iv_dev, iv_host = make_ivs(gpu, n, seed)
        ivs.copy_(iv_dev)
        data = []
        for x, v in zip(xs, lens):
            x.copy_(pool["dev"][shift:shift + v])
            data.append(pool["host"][shift:shift + v])
            shift += 32 + v
        return [cpu_ref.gcm(KEYS[32], iv_host[m], data[m], ha[m]) for m in range(n)]

    def check(want):
        assert [host(o) for o in b.outs] == [w[0] for w in want]
        assert host(b.tags) == b"".join(w[1] for w in want)

    want = load(0, 21)
    b.encrypt(ivs)
    check(want)
    want = load(4096, 22)
    b.encrypt(ivs)
    check(want)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up outside the capture
        b.encrypt(ivs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.encrypt(ivs)
    want = load(9000, 23)  # changes the ivs tensor's contents in place
    for o in b.outs:
        o.zero_()
    b.tags.zero_()
    graph.replay()
    check(want)


# ---- tampering --------------------------------------------------------------------
def sealed(pool, gpu, n, seed, key=KEY):
    """n sealed records (ciphertexts as fresh tensors) with a 9-byte AAD each."""
    lens = [48 + 37 * i for i in range(n)]
    xs, hx, ad, ha = cut(pool, lens, [9] * n)
    iv_dev, iv_host = make_ivs(gpu, n, seed)
    ref = [cpu_ref.gcm(key, iv_host[m], hx[m], ha[m]) for m in range(n)]
    cts = [torch.frombuffer(bytearray(r[0]), dtype=torch.uint8).to(gpu) for r in ref]
    tags = torch.frombuffer(bytearray(b"".join(r[1] for r in ref)), dtype=torch.uint8).to(gpu).view(n, 16)
    aad = torch.stack([a.clone() for a in ad])
    return cts, hx, tags, aad, iv_dev


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_tampered_records_fail_alone(pool, gpu, inplace):
    n = 40
    cts, hx, tags, aad, ivs = sealed(pool, gpu, n, 31)
    cts[7][5] ^= 0x10
    tags[19, 15] ^= 0x01
    aad[23, 0] ^= 0x80
    outs = cts if inplace else [torch.full_like(c, 0xA5) for c in cts]
    good = host(tags)
    good = good[:19 * 16 + 15] + bytes([good[19 * 16 + 15] ^ 0x01]) + good[20 * 16:]  # the tags as they were sealed
    b = ops.GcmBatch(cts, KEY, outs=outs, aads=aad)
    got, ok = b.decrypt(ivs, tags)
    okh = ok.cpu().tolist()
    assert okh == [m not in (7, 19, 23) for m in range(n)]
    computed = host(b.tags)
    for m in range(n):
        assert host(got[m]) == (hx[m] if okh[m] else bytes(len(hx[m]))), m
        # the computed tag of a record that failed is the valid tag of the forgery: it is not handed out
        assert computed[16 * m:16 * m + 16] == (good[16 * m:16 * m + 16] if okh[m] else bytes(16)), m


@pytest.mark.parametrize("tag_bytes", [16, 12])
def test_the_batchs_own_tags_are_refused_as_expected_tags(pool, gpu, tag_bytes):
    """encrypt() returns the batch's own tag tensor, which decrypt() overwrites
    with what it computes: handing it back as the expected tags would compare
    the computed tags with themselves.  It is refused, nothing runs, and with
    a copy the tampered record fails."""
    n = 8
    lens = [100 + 61 * i for i in range(n)]
    xs, hx, _, _ = cut(pool, lens)
    xs = [x.clone() for x in xs]
    ivs, _ = make_ivs(gpu, n, 61)
    b = ops.GcmBatch(xs, KEY, outs=xs, tag_bytes=tag_bytes)  # in place: the round trip on one batch
    _, tags = b.encrypt(ivs)
    assert tags is b.tags
    sealed_tags = tags.clone()
    xs[3][7] ^= 0x04
    before = [host(x) for x in xs]
    own = tags if tag_bytes == 16 else tags.view(-1)[5:5 + n * tag_bytes].view(n, tag_bytes)  # the same memory, another stride
    with pytest.raises(ValueError, match="overlaps the batch's own"):
        b.decrypt(ivs, own)
    assert [host(x) for x in xs] == before and host(b.tags) == host(sealed_tags)  # nothing ran
    got, ok = b.decrypt(ivs, sealed_tags[:, :tag_bytes].contiguous())
    assert ok.cpu().tolist() == [m != 3 for m in range(n)]
    assert [host(o) for o in got] == [hx[m] if m != 3 else bytes(lens[m]) for m in range(n)]
    assert host(b.tags) == b"".join(host(sealed_tags[m]) if m != 3 else bytes(16) for m in range(n))


@pytest.mark.parametrize("tag_bytes", [12, 4])
def test_truncated_tags(pool, gpu, tag_bytes):
    n = 6
    cts, hx, tags, aad, ivs = sealed(pool, gpu, n, 32)
    short = tags[:, :tag_bytes].contiguous()
    b = ops.GcmBatch(cts, KEY, aads=aad, tag_bytes=tag_bytes)
    got, ok = b.decrypt(ivs, short)
    assert ok.cpu().tolist() == [True] * n and [host(o) for o in got] == hx
    # A flipped bit in the last kept byte of record 2 fails.  The dropped bytes cannot be wrong here: the
    # expected tags are an [n, tag_bytes] tensor, so they never reach the device; that they play no part is
    # what the run above shows -- truncated tags verify, compared at a stride of tag_bytes.
    short[2, tag_bytes - 1] ^= 0x01
    got, ok = b.decrypt(ivs, short)
    assert ok.cpu().tolist() == [m != 2 for m in range(n)]
    assert [host(o) for o in got] == [hx[m] if m != 2 else bytes(len(hx[m])) for m in range(n)]


def test_agrees_with_the_one_message_path(pool, gpu):
    lens, aads = [0, 1, 16, 1000, 4096, 4097, 20000, 65541], [0, 3, 0, 16, 13, 0, 40, 1]
    xs, hx, ad, ha = cut(pool, lens, aads)
    xs = [x.clone() for x in xs]
    iv_dev, iv_host = make_ivs(gpu, len(lens), 41)
    outs, tags = ops.gcm_encrypt_batch(xs, KEYS[24], iv_dev, aads=ha)  # host AADs: uploaded with the plan
    tags_h = host(tags)
    for m, x in enumerate(xs):
        o, t = ops.gcm_encrypt(x, KEYS[24], iv_host[m], ha[m])
        assert host(o) == host(outs[m]) and host(t) == tags_h[16 * m:16 * m + 16], m
    assert ops.last_impl() == "ttable"


# ---- argument errors ----------------------------------------------------------------
def test_argument_errors_leave_the_output_untouched(pool, gpu):
    n = 3
    xs = [pool["dev"][4096 * i:4096 * i + 100].clone() for i in range(n)]
    outs = [torch.full_like(x, 0xA5) for x in xs]
    ivs, _ = make_ivs(gpu, n, 51)
    tags = torch.zeros((n, 16), dtype=torch.uint8, device=gpu)
    b = ops.GcmBatch(xs, KEY, outs=outs)
    big = torch.empty(MIB + 16, dtype=torch.uint8, device=gpu)
    bad = [
        lambda: b.encrypt(ivs[:, :11].contiguous()),                                   # 11-byte IVs
        lambda: b.encrypt(torch.zeros((n, 16), dtype=torch.uint8, device=gpu)),        # 16-byte IVs
        lambda: b.encrypt(ivs[:2].contiguous()),                                       # the wrong n
        lambda: b.encrypt(ivs.cpu()),                                                  # a CPU tensor
        lambda: b.encrypt(ivs.to(torch.int32)),                                        # the wrong dtype
        lambda: b.decrypt(ivs, tags[:, :12].contiguous()),                             # tags of the wrong width
        lambda: b.decrypt(ivs, tags[:2].contiguous()),
        lambda: b.decrypt(ivs, tags.cpu()),
        lambda: ops.GcmBatch([x.cpu() for x in xs], KEY, outs=outs),                   # CPU data
        lambda: ops.GcmBatch(xs[:2] + [big[:MIB + 1]], KEY, outs=outs[:2] + [big[:MIB + 1]]),   # over the cap
        lambda: ops.GcmBatch(xs, KEY, outs=outs, aads=[b"", bytes((1 << 16) + 1), b""]),       # AAD over the cap
        lambda: ops.GcmBatch(xs, KEY, outs=outs, aads=torch.zeros((n, (1 << 16) + 1), dtype=torch.uint8, device=gpu)),
        lambda: ops.GcmBatch(xs, KEY, outs=outs, aads=[b"a"]),                         # one AAD per record
        lambda: ops.GcmBatch([big[:100], xs[1]], KEY, outs=[big[16:116], outs[1]]),    # partial overlap
        lambda: ops.GcmBatch([xs[0], xs[1]], KEY, outs=[outs[0], outs[0]]),            # two records, one output
        lambda: ops.GcmBatch([big[1:101]], KEY, outs=[outs[0]]),                       # a misaligned data buffer
        lambda: ops.GcmBatch(xs, KEY, outs=outs, tag_bytes=3),
        lambda: ops.GcmBatch(xs, KEY, outs=outs, tag_bytes=17),
        lambda: ops.GcmBatch(xs, bytes(15), outs=outs),                                # a bad key
        lambda: ops.GcmBatch.packed(big, [100, 100], KEY, offsets=[0, 8]),             # a misaligned slot
        lambda: ops.GcmBatch.packed(big, [100, 100], KEY, offsets=[0, 64]),            # overlapping slots
        lambda: ops.GcmBatch.packed(big, [MIB + 1], KEY),
        lambda: ops.gcm_encrypt_batch(xs, KEY, ivs[:, :11].contiguous(), outs=outs),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} raised nothing")
    torch.cuda.synchronize()
    for o in outs:
        assert host(o) == b"\xa5" * 100
