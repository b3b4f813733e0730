"""Batched AES-GCM-SIV on the device (csrc/hip/aes_gcm_siv_batch.hip through
ops.gcm_siv_batch_ops.GcmSivBatch): many records under one key-generating key,
each with its own 12-byte nonce, AAD and 16-byte tag.  Every byte and every tag
is compared with the C oracle per record (cpu_ref.gcm_siv, cpu_ref.polyval,
cpu_ref.ctr_le32, pinned to RFC 8452 in tests/test_gcm_siv_cpu.py), and the
RFC's sealed vectors run as one batch per key size.

The shapes come from the kernels' own decomposition: the hash kernel's spans in
HASHED blocks (otc_gcm_siv_batch_spans: the AAD's blocks and the length block
count), the counter kernel's 4 KiB tile, the 1 MiB cap.  Data and AADs are
slices of one seeded pool; the AADs start at odd addresses on purpose.  The
oracle's results are computed once per key size and shared."""
import numpy as np
import pytest
import torch

from our_tree_amd import models, ops
from our_tree_amd.models import cpu_ref
from test_gcm_siv_cpu import SEALED

pytestmark = pytest.mark.gpu

SB = ops.gcm_siv_batch_ops
siv = ops.gcm_siv_ops

MIB = 1 << 20
TILE = 4096
DATA = 3 * MIB                # the pool's data region: records are cut from its front, 16-byte aligned
AAD_AT = DATA + 1             # the AAD region starts at an odd address
POOL = DATA + 512 * 1024
KEYS = {128: bytes(range(3, 19)), 256: bytes(range(201, 233))}
GUARD = 32                    # 0xA5 bytes behind every output
H_RFC = bytes.fromhex("25629347589242761d31f826ba4b757b")  # RFC 8452 appendix A
H_ENDS = bytes([0x01] + [0] * 14 + [0x80])                 # x^0 and x^127: a reflected convention shows here

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


def rows(t: torch.Tensor, width=16):
    b = host(t)
    return [b[i:i + width] for i in range(0, len(b), width)]


def dev_bytes(gpu, b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)


def cut(pool, lens, aad_lens):
    """Records of these lengths from the pool: (device views, host bytes, device
    AAD views, host AADs).  Data slots are 16-byte aligned and back to back;
    AADs are packed byte by byte from an odd address."""
    xs, hx, at = [], [], 0
    for n in lens:
        xs.append(pool["dev"][at:at + n])
        hx.append(pool["host"][at:at + n])
        at += (n + 15) // 16 * 16
    assert at <= DATA
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


def guarded(gpu, lens, fill=None):
    """One arena of 0xA5 with a slot per record and GUARD bytes behind each:
    (views, arena, check).  ``fill``: device tensors copied into the slots."""
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += (n + 15) // 16 * 16 + GUARD
    arena = torch.full((max(at, 16),), 0xA5, dtype=torch.uint8, device=gpu)
    views = [arena[o:o + n] for o, n in zip(offs, lens)]
    if fill is not None:
        for v, f in zip(views, fill):
            v.copy_(f)

    def check(what):
        h = np.frombuffer(host(arena), dtype=np.uint8).copy()
        for o, n in zip(offs, lens):
            h[o:o + n] = 0xA5
        bad = np.nonzero(h != 0xA5)[0]
        assert bad.size == 0, f"{what}: {bad.size} guard bytes changed, first at +{int(bad[0])}"

    return views, check


# ---- RFC 8452's vectors ----------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("lanes", [16, 64])
def test_rfc_8452_vectors_as_one_batch(gpu, bits, lanes):
    """Each sealed vector is a record with its own key-generating key in the RFC; here the
    vectors of one key size whose key is the same form one batch, the others a second one."""
    vs = [v for v in SEALED if len(v[0]) == bits // 8]
    assert len(vs) >= 3
    for key in sorted({v[0] for v in vs}):
        grp = [v for v in vs if v[0] == key]
        xs = [dev_bytes(gpu, pt) for _, _, _, pt, _ in grp]
        nv = dev_bytes(gpu, b"".join(n for _, n, _, _, _ in grp)).view(len(grp), 12)
        aads = [aad for _, _, aad, _, _ in grp]
        b = SB.GcmSivBatch(xs, key, aads=aads, lanes=lanes)
        outs, tags = b.encrypt(nv)
        for m, (_, _, _, pt, sealed) in enumerate(grp):
            assert (host(outs[m]) + rows(tags)[m]).hex() == sealed, (bits, m)
        pts, ok = SB.gcm_siv_decrypt_batch(outs, key, nv, tags.clone(), aads=aads)
        assert bool(ok.all()) and [host(p) for p in pts] == [pt for _, _, _, pt, _ in grp]


# ---- the mixed batch -------------------------------------------------------------------
def shapes(n):
    """(data bytes, AAD bytes) of a batch of n records."""
    if n == 1:
        return [TILE + 17], [13]
    if n == 5:  # not a multiple of the four records a wave takes in the 16-lane form
        return [0, 0, 17, TILE + 1, 255 * 16 - 3], [13, 0, 0, 4096, 13]
    spans = SB.GcmSivBatch.spans()
    assert spans == [16, 64, 256]
    cand = [(d, a) for d in (0, 1, 15, 16, 17) for a in (0, 13)]
    for a in (0, 13, 4096):
        na = (a + 15) // 16
        for s in spans:
            for nb in (s - 16, s - 1, s, s + 1, s + 16):  # hashed blocks: AAD blocks + data blocks + 1
                nd = nb - na - 1
                if nd >= 0:
                    cand += [(16 * nd, a), (max(16 * nd - 5, 0), a)]
    cand += [(d, a) for d in (TILE - 16, TILE - 1, TILE, TILE + 1, TILE + 16, 3 * TILE + 17) for a in (0, 13)]
    cand = list(dict.fromkeys(cand))
    assert len(cand) < n - 2
    lens = [cand[i % len(cand)][0] for i in range(n - 2)] + [MIB, 48]
    aads = [cand[i % len(cand)][1] for i in range(n - 2)] + [5, 1 << 16]  # the caps: 1 MiB of data, 64 KiB of AAD
    return lens, aads


_want = {}


def oracle(pool, gpu, bits, n):
    """The records of shapes(n), their nonces and the oracle's sealed records, once per (bits, n)."""
    if (bits, n) not in _want:
        lens, aad_lens = shapes(n)
        xs, hx, ad, ha = cut(pool, lens, aad_lens)
        nv, hn = make_nonces(gpu, n, 100 + n)
        _want[bits, n] = (xs, hx, ad, ha, nv, cpu_ref.gcm_siv_batch(KEYS[bits], hn, hx, ha))
    return _want[bits, n]


@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("bits", [128, 256])
def test_mixed_batch_both_ways(pool, gpu, bits, lanes, n):
    xs, hx, ad, ha, nv, want = oracle(pool, gpu, bits, n)
    lens = [len(h) for h in hx]
    key = KEYS[bits]
    assert (n == 1 or 0 in lens) and (n < 257 or {MIB, TILE, TILE + 1} <= set(lens))

    # out of place, 0xA5 behind every output
    outs, check = guarded(gpu, lens)
    b = SB.GcmSivBatch(xs, key, outs=outs, aads=ad, lanes=lanes)
    assert b.lanes == lanes and b.ntiles == sum((k + TILE - 1) // TILE for k in lens)
    _, tags = b.encrypt(nv)
    got_t = rows(tags)
    for m, (ct, tag) in enumerate(want):
        assert got_t[m] == tag, (m, lens[m], len(ha[m]), "tag", got_t[m].hex(), tag.hex())
        assert host(outs[m]) == ct, (m, lens[m], "ciphertext")
    check("encrypt")
    assert [host(x) for x in xs[:8]] == hx[:8]
    pts, check_p = guarded(gpu, lens)
    d = SB.GcmSivBatch(outs, key, outs=pts, aads=ad, lanes=lanes)
    _, ok = d.decrypt(nv, tags.clone())
    assert ok.dtype == torch.bool and ok.tolist() == [True] * n
    assert rows(d.tags) == [t for _, t in want]
    for m in range(n):
        assert host(pts[m]) == hx[m], (m, lens[m], "plaintext")
    check_p("decrypt")

    # in place, both ways, in one plan
    buf, check_i = guarded(gpu, lens, fill=xs)
    e = SB.GcmSivBatch(buf, key, outs=buf, aads=ad, lanes=lanes)
    _, tags = e.encrypt(nv)
    assert rows(tags) == [t for _, t in want] and [host(o) for o in buf] == [c for c, _ in want]
    _, ok = e.decrypt(nv, tags.clone())
    assert bool(ok.all()) and [host(o) for o in buf] == hx
    check_i("in place")


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_packed_with_gaps(pool, gpu, inplace):
    """Records at chosen offsets of one buffer: the bytes between them come back untouched."""
    lens = [100, 0, TILE + 1, 16, 255 * 16 + 3, 1]
    offs = [32, 256, 512, 3 * TILE, 3 * TILE + 64, 5 * TILE - 16]
    total = 5 * TILE + 64
    key = KEYS[256]
    src = pool["dev"][:total].clone()
    hs = host(src)
    aad = pool["dev"][AAD_AT:AAD_AT + 6 * 13].view(6, 13)
    ha = [pool["host"][AAD_AT + 13 * m:AAD_AT + 13 * m + 13] for m in range(6)]
    nv, hn = make_nonces(gpu, 6, 7)
    want = cpu_ref.gcm_siv_batch(key, hn, [hs[o:o + n] for o, n in zip(offs, lens)], ha)
    out = src if inplace else torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
    b = SB.GcmSivBatch.packed(src, lens, key, out=out, offsets=offs, aad=aad)
    assert b.out is out
    _, tags = b.encrypt(nv)
    exp = bytearray(hs if inplace else bytes([0xA5]) * total)
    for (ct, _), o, n in zip(want, offs, lens):
        exp[o:o + n] = ct
    assert host(out) == bytes(exp) and rows(tags) == [t for _, t in want]
    d = SB.GcmSivBatch.packed(out, lens, key, out=out, offsets=offs, aad=aad)
    _, ok = d.decrypt(nv, tags.clone())
    for o, n in zip(offs, lens):
        exp[o:o + n] = hs[o:o + n]
    assert bool(ok.all()) and host(out) == bytes(exp)


def test_each_record_equals_the_single_call(pool, gpu):
    xs, hx, ad, ha, nv, want = oracle(pool, gpu, 256, 5)
    key = KEYS[256]
    outs, tags = models.AES(key).gcm_siv_encrypt_batch(xs, nv, aads=ad)
    hn = rows(nv, 12)
    for m in range(5):
        ct, tag = siv.gcm_siv_encrypt(xs[m], key, hn[m], ha[m])
        assert host(ct) == host(outs[m]) == want[m][0] and host(tag) == rows(tags)[m] == want[m][1], m


def test_the_keys_are_per_record(pool, gpu):
    """The mode's defining property, on the device output: the nonce decides both keys.
    Records 0 and 1 share data and AAD and differ in the nonce: no 16-byte block of
    their ciphertexts is equal.  Records 1 and 2 share the nonce too: identical."""
    n = TILE + 48
    x = pool["dev"][:n]
    aad = pool["host"][AAD_AT:AAD_AT + 13]
    hn = [bytes(range(12)), bytes(range(1, 13)), bytes(range(1, 13))]
    nv = dev_bytes(gpu, b"".join(hn)).view(3, 12)
    outs, tags = SB.gcm_siv_encrypt_batch([x, x, x], KEYS[128], nv, aads=[aad] * 3)
    c = [host(o) for o in outs]
    t = rows(tags)
    assert c[1] == c[2] and t[1] == t[2]
    assert t[0] != t[1] and all(c[0][i:i + 16] != c[1][i:i + 16] for i in range(0, n, 16))
    assert (c[0], t[0]) == cpu_ref.gcm_siv(KEYS[128], hn[0], host(x), aad)
    assert (c[1], t[1]) == cpu_ref.gcm_siv(KEYS[128], hn[1], host(x), aad)


# ---- the two halves by themselves --------------------------------------------------------
def hashed(aad: bytes, data: bytes) -> bytes:
    return (aad + bytes(-len(aad) % 16) + data + bytes(-len(data) % 16) + (8 * len(aad)).to_bytes(8, "little") +
            (8 * len(data)).to_bytes(8, "little"))


@pytest.mark.parametrize("lanes", [16, 64])
def test_polyval_batch_alone(pool, gpu, lanes):
    """Own H per record, among them RFC 8452's example key and the key with only bits 0 and 127."""
    lens, aad_lens = shapes(257)
    lens, aad_lens = lens[:120] + [MIB], aad_lens[:120] + [13]
    xs, hx, ad, ha = cut(pool, lens, aad_lens)
    n = len(lens)
    assert all(any(h) for h in hx if h)  # distinct from the all-zero block
    hs = [H_RFC, H_ENDS] + [r.tobytes() for r in np.random.default_rng(3).integers(0, 256, (n - 2, 16), dtype=np.uint8)]
    hv = dev_bytes(gpu, b"".join(hs)).view(n, 16)
    s = SB.polyval_batch(xs, hv, aads=ad, lanes=lanes)
    got = rows(s)
    for m in range(n):
        assert got[m] == cpu_ref.polyval(hs[m], hashed(ha[m], hx[m])), (m, lens[m], aad_lens[m])
    assert host(hv) == b"".join(hs)
    # RFC 8452 appendix A: POLYVAL(H, X_1, X_2) = f7a3...; a record of X_1 X_2 continues it over its length block
    x12 = bytes.fromhex("4f4f95668c83dfb6401762bb2d01a262d1a24ddd2721d006bbe45f20d3c9f362")
    one = SB.polyval_batch([dev_bytes(gpu, x12)], dev_bytes(gpu, H_RFC).view(1, 16), lanes=lanes)
    assert host(one) == cpu_ref.polyval(H_RFC, (256).to_bytes(8, "little").rjust(16, b"\0"),
                                        y0=bytes.fromhex("f7a3b47b846119fae5b7866cf5e5b77e"))


@pytest.mark.parametrize("bits", [128, 256])
def test_ctr_le32_batch_alone_across_the_wrap(pool, gpu, bits):
    """The only place where the wrap can be steered: the AEAD's counter is its tag.  The counter rows
    start 3, 70 and 256 + 100 blocks before 2^32 -- the wrap falls inside the first tile's first load,
    across its lanes, and in the middle of a later tile.  Byte 4 is 0xff (a carry would show), byte 15
    below 0x80 (the forced bit shows).  A different key per record."""
    recs = [(n, back) for back in (3, 70, 356) for n in (1, 17, TILE + 5, 3 * TILE + 17)]
    lens = [n for n, _ in recs]
    xs, hx, _, _ = cut(pool, lens, [0] * len(lens))
    rng = np.random.default_rng(11)
    keys = [rng.integers(0, 256, bits // 8, dtype=np.uint8).tobytes() for _ in recs]
    ctrs = [((1 << 32) - back).to_bytes(4, "little") + b"\xff" + rng.integers(0, 256, 10, dtype=np.uint8).tobytes() +
            bytes([0x15 + i]) for i, (_, back) in enumerate(recs)]
    assert all(c[4] == 0xFF and c[15] < 0x80 for c in ctrs)
    cv = dev_bytes(gpu, b"".join(ctrs)).view(len(recs), 16)
    want = [cpu_ref.ctr_le32(k, c[:15] + bytes([c[15] | 0x80]), x) for k, c, x in zip(keys, ctrs, hx)]
    outs, check = guarded(gpu, lens)
    SB.ctr_le32_batch(xs, keys, cv, outs=outs)
    assert ops.last_impl() == "ttable"
    for m in range(len(recs)):
        assert host(outs[m]) == want[m], (m, recs[m])
    check("ctr_le32_batch")
    assert host(cv) == b"".join(ctrs)  # the kernel only reads its counter rows
    buf, check_i = guarded(gpu, lens, fill=xs)
    SB.ctr_le32_batch(buf, keys, cv, outs=buf)  # in place
    assert [host(o) for o in buf] == want
    check_i("ctr_le32_batch in place")


# ---- tampering ---------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_tampering_fails_exactly_the_tampered_records(pool, gpu, inplace):
    lens = [100, TILE + 1, 255 * 16, 17, 3 * TILE + 17, 16, 1000, 0, 64]
    key = KEYS[256]
    xs, hx, ad, ha = cut(pool, lens, [13] * 9)
    nv, hn = make_nonces(gpu, 9, 23)
    sealed = cpu_ref.gcm_siv_batch(key, hn, hx, ha)
    cts = [dev_bytes(gpu, c) for c, _ in sealed]
    tags = dev_bytes(gpu, b"".join(t for _, t in sealed)).view(9, 16)
    aads = torch.stack([a.clone() for a in ad])  # [9, 13], owned: one byte of it changes
    cts[2][lens[2] // 2] ^= 0x01                 # record 2: a ciphertext byte
    tags[4, 9] ^= 0x40                           # record 4: a tag bit
    aads[6, 0] ^= 0x80                           # record 6: an AAD byte
    nv = nv.clone()
    nv[8, 11] ^= 0x01                            # record 8: the nonce
    bad = {2, 4, 6, 8}
    outs, check = guarded(gpu, lens, fill=cts) if inplace else guarded(gpu, lens)
    b = SB.GcmSivBatch(outs if inplace else cts, key, outs=outs, aads=aads)
    _, ok = b.decrypt(nv, tags)
    assert ok.tolist() == [m not in bad for m in range(9)]
    got_t = rows(b.tags)
    for m in range(9):
        assert host(outs[m]) == (bytes(lens[m]) if m in bad else hx[m]), m
        assert got_t[m] == (bytes(16) if m in bad else sealed[m][1]), m
    check("decrypt with forged records")
    with pytest.raises(ValueError, match="own tags"):
        b.decrypt(nv, b.tags)


# ---- replay and graph -------------------------------------------------------------------
def test_replay_with_new_nonces_and_graph(pool, gpu):
    """Plan once; run twice with new nonces written in place into the same tensor; then capture
    encrypt in a graph and replay it after changing nonces and data in place."""
    lens = [100, TILE + 1, 0, 255 * 16 - 3, 17]
    key = KEYS[128]
    xs, hx, ad, ha = cut(pool, lens, [13, 0, 13, 4096, 1])
    ins, _ = guarded(gpu, lens, fill=xs)
    outs, check = guarded(gpu, lens)
    nv, hn = make_nonces(gpu, 5, 31)
    b = SB.GcmSivBatch(ins, key, outs=outs, aads=ad)

    def verify(hn, hx, what):
        want = cpu_ref.gcm_siv_batch(key, hn, hx, ha)
        assert [host(o) for o in outs] == [c for c, _ in want] and rows(b.tags) == [t for _, t in want], what

    b.encrypt(nv)
    verify(hn, hx, "first run")
    nv2, hn2 = make_nonces(gpu, 5, 32)
    nv.copy_(nv2)
    b.encrypt(nv)
    verify(hn2, hx, "second run, new nonces in the same tensor")

    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        b.encrypt(nv)  # warm: nothing is loaded or allocated inside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            b.encrypt(nv)
    nv3, hn3 = make_nonces(gpu, 5, 33)
    nv.copy_(nv3)
    hx3 = []
    for v, n in zip(ins, lens):  # new data in place: the pool from another offset
        v.copy_(pool["dev"][MIB:MIB + n])
        hx3.append(pool["host"][MIB:MIB + n])
    for o in outs:
        o.fill_(0xA5)
    b.tags.zero_()
    torch.cuda.synchronize()
    graph.replay()
    verify(hn3, hx3, "graph replay")
    check("replay")
