"""Batched AES-GCM with a key per record on the device
(csrc/hip/aes_gcm_mk_batch.hip through ops.gcm_mk_batch_ops.GcmMkBatch).
Everything is compared exactly against the C oracle (cpu_ref.gcm_mk_batch, a
loop over cpu_ref.gcm, and cpu_ref.ghash; pinned to known answers in
tests/test_gcm_cpu.py), and against the neighbouring device paths: ops.GcmBatch
where one key covers the batch, ops.gcm_encrypt record by record.

The shapes come from the kernels' boundaries: 16 / 64 / 256 hashed blocks (a
pass of the 16-lane form, a pass of the 64-lane form, its batch of passes), the
CTR half's 4 KiB tile, the 64 KiB a workgroup of the CTR kernel stores in one
step, the 1 MiB cap.  Data and AADs are slices of one seeded pool that is never
written; the AADs start at odd addresses on purpose.  The oracle's answer for a
batch is computed once and shared by the lane forms and the directions."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

MK = ops.gcm_mk_batch_ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "gcm_vectors.json")))["vectors"]

MIB = 1 << 20
DATA = 3 * MIB      # the pool's data region: records are cut from its front, 16-byte aligned
AAD_AT = DATA + 1   # the AAD region starts at an odd address
POOL = DATA + 64 * 1024
A5 = 0xA5
# a lane's block; 16, 64 and 256 hashed blocks behind a 13-byte AAD (1 + 14 + 1, 1 + 62 + 1, 1 + 255 + 1); the 4 KiB
# tile; the CTR workgroup's 64 KiB store step
LENS = [0, 1, 15, 16, 17, 14 * 16, 62 * 16 - 1, 254 * 16 + 1, 4095, 4096, 4113, 65536 + 16]
AADS = [0, 1, 13, 16, 17, 40]

_pool = {}


@pytest.fixture(scope="module")
def pool(gpu):
    """Random bytes, once: on the device and on the host.  Never written."""
    if not _pool:
        g = torch.Generator(device=gpu).manual_seed(43)
        dev = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device=gpu, generator=g)
        _pool.update(dev=dev, host=dev.cpu().numpy().tobytes())
    return _pool


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def dev(b: bytes, gpu, shape=None):
    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu)
    return t.view(*shape) if shape else t


def slots(lens):
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += (n + 15) // 16 * 16
    return offs, at


def cut(pool, lens, aad_lens):
    """Records of these lengths from the pool: (offsets, device views, host
    bytes, device AAD views, host AADs).  Data slots are 16-byte aligned and
    back to back; AADs are packed byte by byte from an odd address."""
    offs, total = slots(lens)
    assert total <= DATA
    xs = [pool["dev"][o:o + n] for o, n in zip(offs, lens)]
    hx = [pool["host"][o:o + n] for o, n in zip(offs, lens)]
    ad, ha, at = [], [], AAD_AT
    for n in aad_lens:
        ad.append(pool["dev"][at:at + n])
        ha.append(pool["host"][at:at + n])
        at += n
    assert at <= POOL
    return offs, xs, hx, ad, ha


def make_keys(nkeys, bits, seed=7):
    rng = np.random.default_rng(seed * 1000 + bits)
    return tuple(rng.integers(0, 256, bits // 8, dtype=np.uint8).tobytes() for _ in range(nkeys))


def make_ivs(n, seed):
    b = np.random.default_rng(seed).integers(0, 256, (n, 12), dtype=np.uint8)
    return b.tobytes(), [r.tobytes() for r in b]


def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def ref_hash(h, data, aad):
    return cpu_ref.ghash(h, pad16(aad) + pad16(data) + (8 * len(aad)).to_bytes(8, "big") + (8 * len(data)).to_bytes(8, "big"))


# ---- vectors ----------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_vectors_as_one_batch_with_a_key_each(gpu, bits, lanes):
    """The 12-byte-IV vectors of one key size: one batch, one key per vector."""
    vs = [v for v in VECTORS if len(bytes.fromhex(v["key"])) * 8 == bits and len(bytes.fromhex(v["iv"])) == 12]
    assert vs, "no 12-byte-IV vector of this key size"
    xs = [dev(bytes.fromhex(v["pt"]), gpu) if v["pt"] else torch.empty(0, dtype=torch.uint8, device=gpu) for v in vs]
    ivs = dev(b"".join(bytes.fromhex(v["iv"]) for v in vs), gpu, (len(vs), 12))
    b = MK.GcmMkBatch(xs, [bytes.fromhex(v["key"]) for v in vs], aads=[bytes.fromhex(v["aad"]) for v in vs], lanes=lanes)
    outs, tags = b.encrypt(ivs)
    assert [host(o).hex() for o in outs] == [v["ct"] for v in vs]
    assert [host(tags[m]).hex() for m in range(len(vs))] == [v["tag"] for v in vs]
    back, ok = MK.gcm_mk_decrypt_batch(outs, [bytes.fromhex(v["key"]) for v in vs], ivs, tags.clone(),
                                       aads=[bytes.fromhex(v["aad"]) for v in vs])
    assert bool(ok.all()) and [host(o).hex() for o in back] == [v["pt"] for v in vs]


# ---- mixed batches ----------------------------------------------------------------
def shape(n):
    return [LENS[m % len(LENS)] for m in range(n)], [AADS[(m + m // len(LENS)) % len(AADS)] for m in range(n)]


@functools.lru_cache(maxsize=None)
def mixed_ref(n, nk, bits):
    """Keys, key index, IVs and the oracle's sealed records of a mixed batch; the pool's host bytes come from _pool."""
    lens, aad_lens = shape(n)
    _, _, hx, _, ha = cut(_pool, lens, aad_lens)
    nkeys = n if nk == "n" else nk
    keys = make_keys(nkeys, bits)
    kidx = np.random.default_rng(100 * n + nkeys).integers(0, nkeys, n).tolist() if nk != "n" else list(range(n))
    iv_bytes, ivs = make_ivs(n, 11 * n + bits)
    sealed = cpu_ref.gcm_mk_batch(keys, kidx, ivs, hx, ha)
    return keys, kidx, iv_bytes, ivs, sealed


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("nk", [1, 3, "n"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_mixed_batch_both_ways(pool, gpu, n, nk, bits, lanes):
    lens, aad_lens = shape(n)
    offs, xs, hx, ad, ha = cut(pool, lens, aad_lens)
    total = slots(lens)[1]
    keys, kidx, iv_bytes, _, sealed = mixed_ref(n, nk, bits)
    ivs = dev(iv_bytes, gpu, (n, 12))
    want_ct = bytearray([A5]) * total
    for o, (c, _) in zip(offs, sealed):
        want_ct[o:o + len(c)] = c
    want_tags = b"".join(t for _, t in sealed)

    # out of place into an 0xA5 buffer: the gaps between the records stay
    out = torch.full((total,), A5, dtype=torch.uint8, device=gpu)
    b = MK.GcmMkBatch(xs, keys, key_index=kidx, outs=[out[o:o + k] for o, k in zip(offs, lens)], aads=ad, lanes=lanes)
    _, tags = b.encrypt(ivs)
    assert host(out) == bytes(want_ct) and host(tags) == want_tags
    if nk == 1:  # one key: the one-key batch's outputs and tags
        o1, t1 = ops.GcmBatch(xs, keys[0], aads=ad).encrypt(ivs)
        assert [host(o) for o in o1] == [c for c, _ in sealed] and host(t1) == want_tags

    # decryption in place over those outputs
    d = MK.GcmMkBatch([out[o:o + k] for o, k in zip(offs, lens)], keys, key_index=kidx,
                      outs=[out[o:o + k] for o, k in zip(offs, lens)], aads=ad, lanes=lanes)
    _, ok = d.decrypt(ivs, tags.clone())
    want_pt = bytearray([A5]) * total
    for o, p in zip(offs, hx):
        want_pt[o:o + len(p)] = p
    assert bool(ok.all()) and host(out) == bytes(want_pt) and host(d.tags) == want_tags

    # encryption in place, decryption out of place
    e = MK.GcmMkBatch([out[o:o + k] for o, k in zip(offs, lens)], keys, key_index=kidx,
                      outs=[out[o:o + k] for o, k in zip(offs, lens)], aads=ad, lanes=lanes)
    e.encrypt(ivs)
    assert host(out) == bytes(want_ct) and host(e.tags) == want_tags
    back = torch.full((total,), A5, dtype=torch.uint8, device=gpu)
    _, ok = MK.GcmMkBatch([out[o:o + k] for o, k in zip(offs, lens)], keys, key_index=kidx,
                          outs=[back[o:o + k] for o, k in zip(offs, lens)], aads=ad, lanes=lanes).decrypt(ivs, e.tags.clone())
    assert bool(ok.all()) and host(back) == bytes(want_pt) and host(out) == bytes(want_ct)
    assert host(pool["dev"][:total]) == pool["host"][:total], "an input changed"


def test_every_record_equals_gcm_encrypt_alone(pool, gpu):
    n = len(LENS)
    lens, aad_lens = shape(n)
    _, xs, hx, ad, ha = cut(pool, lens, aad_lens)
    keys = make_keys(3, 256, seed=9)
    kidx = [m % 3 for m in range(n)]
    iv_bytes, ivs = make_ivs(n, 77)
    outs, tags = MK.gcm_mk_encrypt_batch(xs, keys, dev(iv_bytes, gpu, (n, 12)), key_index=kidx, aads=ad)
    for m in range(n):
        o, t = ops.gcm_encrypt(xs[m].clone(), keys[kidx[m]], ivs[m], ha[m])
        assert host(outs[m]) == host(o) and host(tags[m]) == host(t), m


def test_packed_layout(pool, gpu):
    lens = [100, 0, 4096, 33]
    offs, total = slots(lens)
    keys = make_keys(2, 128, seed=3)
    kidx = [1, 0, 1, 0]
    iv_bytes, ivs = make_ivs(4, 5)
    aad = pool["dev"][AAD_AT:AAD_AT + 4 * 13].view(4, 13)
    ha = [pool["host"][AAD_AT + 13 * m:AAD_AT + 13 * m + 13] for m in range(4)]
    b = MK.GcmMkBatch.packed(pool["dev"][:total], lens, keys, key_index=kidx, aad=aad)
    _, tags = b.encrypt(dev(iv_bytes, gpu, (4, 12)))
    want = cpu_ref.gcm_mk_batch(keys, kidx, ivs, [pool["host"][o:o + k] for o, k in zip(offs, lens)], ha)
    got = host(b.out)
    assert [got[o:o + k] for o, k in zip(offs, lens)] == [c for c, _ in want] and host(tags) == b"".join(t for _, t in want)


@pytest.mark.parametrize("lanes", [16, 64])
def test_one_record_at_the_cap(pool, gpu, lanes):
    keys = make_keys(2, 128, seed=5)
    x = pool["dev"][:MIB]
    iv_bytes, ivs = make_ivs(2, 99)
    small = pool["dev"][MIB:MIB + 100]
    want = cpu_ref.gcm_mk_batch(keys, [1, 0], ivs, [pool["host"][:MIB], pool["host"][MIB:MIB + 100]], [b"", b""])
    outs, tags = MK.GcmMkBatch([x, small], keys, key_index=[1, 0], lanes=lanes).encrypt(dev(iv_bytes, gpu, (2, 12)))
    assert [host(o) for o in outs] == [c for c, _ in want] and host(tags) == b"".join(t for _, t in want)


# ---- the keys are per record ------------------------------------------------------
@pytest.mark.parametrize("lanes", [16, 64])
def test_the_key_is_per_record(pool, gpu, lanes):
    n = 8
    x, hx = pool["dev"][:1000], pool["host"][:1000]
    aad, ha = pool["dev"][AAD_AT:AAD_AT + 13], pool["host"][AAD_AT:AAD_AT + 13]
    keys = make_keys(2, 192, seed=21)
    iv = bytes(range(12))
    ivs = dev(iv * n, gpu, (n, 12))
    want = [cpu_ref.gcm(k, iv, hx, ha) for k in keys]
    assert want[0] != want[1]

    def run(kidx):
        outs, tags = MK.GcmMkBatch([x] * n, keys, key_index=kidx, aads=[aad] * n, lanes=lanes).encrypt(ivs)
        return [(host(o), host(tags[m])) for m, o in enumerate(outs)]

    kidx = [0, 1, 1, 0, 1, 0, 0, 1]
    got = run(kidx)
    # identical data / IV / AAD under two keys: two results, each the oracle's; records that share everything agree
    assert got == [want[k] for k in kidx]
    perm = [7, 2, 5, 0, 3, 6, 1, 4]
    assert run([kidx[p] for p in perm]) == [got[p] for p in perm]


# ---- the hash alone ---------------------------------------------------------------
@pytest.mark.parametrize("lanes", [16, 64])
def test_ghash_mk_batch_against_the_oracle(pool, gpu, lanes):
    n = 2 * len(LENS) + 3
    lens, aad_lens = shape(n)
    _, xs, hx, ad, ha = cut(pool, lens, aad_lens)
    keys = make_keys(5, 128, seed=31)
    kidx = [(3 * m + 1) % 5 for m in range(n)]
    hs = [cpu_ref.gcm_h(k) for k in keys]
    got = host(MK.ghash_mk_batch(xs, keys, key_index=kidx, aads=ad, lanes=lanes))
    for m in range(n):
        assert got[16 * m:16 * m + 16] == ref_hash(hs[kidx[m]], hx[m], ha[m]), (m, lens[m], aad_lens[m])


M128 = (1 << 128) - 1


def table_image(h: bytes) -> bytes:
    """A key's table image (otc.h: the nibble tables of C^(2^s), s = 0 .. 6, C =
    mulX_POLYVAL(ByteReverse(H))) for a CHOSEN H, from integers and the oracle's
    POLYVAL product: a key whose E_K(0) is a given H cannot be had."""
    def mulx(v):
        v <<= 1
        return (v & M128) ^ ((1 << 127) | (1 << 126) | (1 << 121) | 1) if v >> 128 else v

    c = mulx(int.from_bytes(h[::-1], "little"))
    img = bytearray()
    for _ in range(7):
        for nib in range(16):
            e, v = 0, c
            for k in range(4):
                if (nib >> k) & 1:
                    e ^= v
                v = mulx(v)
            img += e.to_bytes(16, "little")
        cb = c.to_bytes(16, "little")
        c = int.from_bytes(cpu_ref.polyval_dot(cb, cb), "little")
    return bytes(img)


def gf128_inverse(h: bytes) -> bytes:
    """h^(2^128 - 2) in GCM's field, by the oracle's product."""
    r, sq = None, h
    for _ in range(127):  # the exponent's bits 1 .. 127 are set
        sq = cpu_ref.gf128_mul(sq, sq)
        r = sq if r is None else cpu_ref.gf128_mul(r, sq)
    return r


@pytest.mark.parametrize("lanes", [16, 64])
def test_ghash_under_a_chosen_h(pool, gpu, lanes):
    """The hash kernel on table images of CHOSEN hash keys, written over the
    batch's own: H = 80 00 .. 00 01 -- only its first and last bit set, where a
    reflected bit order shows -- and RFC 8452 appendix A's H, under which
    GHASH(X_1, X_2) must be bd9b3997046731fb96251b91f9c99d7a."""
    hs = [bytes([0x80] + [0] * 14 + [0x01]), bytes.fromhex("25629347589242761d31f826ba4b757b")]
    x12 = bytes.fromhex("4f4f95668c83dfb6401762bb2d01a262" "d1a24ddd2721d006bbe45f20d3c9f362")
    lens = [32, 0, 16, 33, 1000, 4096]
    _, xs, hx, ad, ha = cut(pool, lens, [0] + [13] * (len(lens) - 1))
    xs[0], hx[0] = dev(x12, gpu), x12  # record 0: X_1 X_2 under the appendix's H, no AAD
    kidx = [1] + [m % 2 for m in range(1, len(lens))]
    b = MK.GcmMkBatch(xs, [bytes(16), bytes(16)], key_index=kidx, outs=xs, aads=ad, lanes=lanes)
    image = b"".join(table_image(h) for h in hs)
    assert len(image) == b._tab.numel()
    b._tab.copy_(dev(image, gpu))
    got = host(b.ghash())
    for m in range(len(lens)):
        assert got[16 * m:16 * m + 16] == ref_hash(hs[kidx[m]], hx[m], ha[m]), (m, lens[m])
    # the device's value is (Y ^ lengths) . H with Y = GHASH(H, X_1, X_2): take the last step off again
    lenblock = bytes(8) + (256).to_bytes(8, "big")
    y = bytes(a ^ c for a, c in zip(cpu_ref.gf128_mul(got[:16], gf128_inverse(hs[1])), lenblock))
    assert y.hex() == "bd9b3997046731fb96251b91f9c99d7a"


# ---- tampering --------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("tag_bytes", [4, 12, 16])
def test_tampering(pool, gpu, tag_bytes, inplace):
    """One record each with a flipped ciphertext byte, tag byte, AAD byte, IV
    byte and a swapped key index: exactly those fail, their outputs and tag rows
    are zero, all others equal the oracle."""
    n = 16
    lens = [48 + 37 * i for i in range(n)]
    lens[9] = 4096 + 100  # the forged ciphertext spans two tiles: the wipe covers both
    offs, xs, hx, ad, ha = cut(pool, lens, [9] * n)
    keys = make_keys(4, 128, seed=41)
    kidx = [m % 4 for m in range(n)]
    iv_bytes, ivs = make_ivs(n, 55)
    sealed = cpu_ref.gcm_mk_batch(keys, kidx, ivs, hx, ha)
    CT, TAG, AAD, IV, KEY = 9, 2, 5, 12, 14
    cts = [dev(c, gpu) for c, _ in sealed]
    cts[CT][lens[CT] - 1] ^= 0x01
    tags = bytearray(b"".join(t[:tag_bytes] for _, t in sealed))
    tags[TAG * tag_bytes + tag_bytes - 1] ^= 0x80  # the last byte that is compared
    aads = [a.clone() for a in ad]
    aads[AAD][3] ^= 0x04
    iv_t = bytearray(iv_bytes)
    iv_t[12 * IV + 11] ^= 0x01
    kidx_t = list(kidx)
    kidx_t[KEY] = (kidx[KEY] + 1) % 4
    bad = {CT, TAG, AAD, IV, KEY}
    outs = cts if inplace else [torch.full_like(c, A5) for c in cts]
    b = MK.GcmMkBatch(cts, keys, key_index=kidx_t, outs=outs, aads=aads, tag_bytes=tag_bytes)
    _, ok = b.decrypt(dev(bytes(iv_t), gpu, (n, 12)), dev(bytes(tags), gpu, (n, tag_bytes)))
    assert ok.tolist() == [m not in bad for m in range(n)]
    assert [host(o) for o in outs] == [bytes(lens[m]) if m in bad else hx[m] for m in range(n)]
    assert host(b.tags) == b"".join(bytes(16) if m in bad else sealed[m][1] for m in range(n))
    if tag_bytes < 16:  # a byte past the compared ones does not count
        tags[TAG * tag_bytes + tag_bytes - 1] ^= 0x80
        full = bytearray(b"".join(t for _, t in sealed))
        full[16 * TAG + tag_bytes] ^= 0xFF
        b2 = MK.GcmMkBatch([dev(c, gpu) for c, _ in sealed], keys, key_index=kidx, aads=ad, tag_bytes=tag_bytes)
        _, ok = b2.decrypt(dev(iv_bytes, gpu, (n, 12)),
                           dev(b"".join(bytes(full[16 * m:16 * m + tag_bytes]) for m in range(n)), gpu, (n, tag_bytes)))
        assert bool(ok.all())
    own = b.tags.view(-1)[:n * tag_bytes].view(n, tag_bytes)  # the batch's own tag rows as the expected tags
    with pytest.raises(ValueError, match="own tags"):
        b.decrypt(dev(iv_bytes, gpu, (n, 12)), own)


# ---- replay -------------------------------------------------------------------------
def test_replay_graph_and_rekey(pool, gpu):
    """The same plan with new data and new IVs, inside a captured graph, and after rekey."""
    n = 24
    lens = [LENS[m % len(LENS)] if LENS[m % len(LENS)] < 8192 else 777 for m in range(n)]
    offs, total = slots(lens)
    keys = make_keys(5, 256, seed=61)
    kidx = [(2 * m + 1) % 5 for m in range(n)]
    buf = torch.empty(total, dtype=torch.uint8, device=gpu)
    ivs = torch.empty((n, 12), dtype=torch.uint8, device=gpu)
    aad = pool["dev"][AAD_AT:AAD_AT + 13 * n].view(n, 13)
    ha = [pool["host"][AAD_AT + 13 * m:AAD_AT + 13 * m + 13] for m in range(n)]
    b = MK.GcmMkBatch.packed(buf, lens, keys, key_index=kidx, aad=aad)
    state = {"keys": keys}

    def load(at, seed):
        buf.copy_(pool["dev"][at:at + total])
        iv_bytes, iv_list = make_ivs(n, seed)
        ivs.copy_(dev(iv_bytes, gpu, (n, 12)))
        data = pool["host"][at:at + total]
        return cpu_ref.gcm_mk_batch(state["keys"], kidx, iv_list, [data[o:o + k] for o, k in zip(offs, lens)], ha)

    def check(want):
        got = host(b.out)
        assert [got[o:o + k] for o, k in zip(offs, lens)] == [c for c, _ in want]
        assert host(b.tags) == b"".join(t for _, t in want)

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
    b.out.zero_()
    b.tags.zero_()
    graph.replay()
    check(want)

    # new keys, same plan: the captured graph reads the schedules and tables where they lie
    state["keys"] = make_keys(5, 256, seed=62)
    b.rekey(state["keys"])
    want = load(5000, 24)
    b.encrypt(ivs)
    check(want)
    want = load(6000, 25)
    b.out.zero_()
    graph.replay()
    check(want)
    with pytest.raises(ValueError):
        b.rekey(make_keys(5, 128, seed=62))
    # and the key material on the device can be cleared
    b.wipe_keys()
    assert not host(b._keys).strip(b"\0") and not host(b._tab).strip(b"\0")
