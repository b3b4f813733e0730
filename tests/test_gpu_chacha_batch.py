"""Batched ChaCha20-Poly1305 on the device (csrc/hip/chacha_batch.hip through
ops.chacha_batch_ops.ChaChaBatch): many records, each with its own key,
12-byte nonce, AAD and tag.  Everything is compared exactly against the C
oracle per record (cpu_ref.chacha20_poly1305 / cpu_ref.poly1305, pinned to the
RFC 8439 vectors in tests/test_chacha_cpu.py), and the section 2.8.2 vector of
tests/golden/chacha_vectors.json runs through the batch as one of its records.

The hash shapes come from the kernel's own decomposition
(otc_chacha_batch_spans, in HASHED blocks: AAD blocks + data blocks + the
length block).  Data and AADs are slices of one seeded pool; the AADs start at
odd addresses on purpose."""
import json
import os
import time

import numpy as np
import pytest
import torch

from our_tree_amd import models, ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

CB = ops.chacha_batch_ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RFC = next(v for v in json.load(open(os.path.join(ROOT, "tests", "golden", "chacha_vectors.json")))["aead"]
           if v["name"] == "rfc8439-2.8.2")

MIB = 1 << 20
DATA = 3 * MIB                # the pool's data region: records are cut from its front, 16-byte aligned
AAD_AT = DATA + 1             # the AAD region starts at an odd address
POOL = DATA + 256 * 1024
KEYS = [bytes(range(3, 35)), bytes(range(60, 92)), bytes(range(201, 233))]
KEY = KEYS[0]
ONE_LENS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 8191, 8193]

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


# ---- the hash alone ---------------------------------------------------------------
def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def ref_hash(otk, data, aad):
    return cpu_ref.poly1305(otk, pad16(aad) + pad16(data) + len(aad).to_bytes(8, "little") + len(data).to_bytes(8, "little"))


def otks(n, seed):
    b = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
    return [r.tobytes() for r in b]


def check_hash(pool, lens, aad_lens=None, keys=None, lanes=(16, 64)):
    """Both forms of the kernel: 16 and 64 lanes per record; equal to each other and to the oracle."""
    xs, hx, ad, ha = cut(pool, lens, aad_lens)
    keys = keys or otks(len(lens), 7 + len(lens))
    want = [ref_hash(k, d, a) for k, d, a in zip(keys, hx, ha)]
    for ln in lanes:
        got = rows(CB.poly1305_batch(xs, keys, aads=ad if aad_lens else None, lanes=ln))
        for m, w in enumerate(want):
            assert got[m] == w, (ln, m, lens[m], len(ha[m]), got[m].hex(), w.hex())


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1007, 1008, 1009])
def test_hash_one_record(pool, n, lanes):
    """The narrowest case: one record, no AAD, then behind a 13-byte AAD."""
    check_hash(pool, [n], lanes=(lanes,))
    check_hash(pool, [n], [13], lanes=(lanes,))


def test_hash_around_every_span(pool):
    """Records whose HASHED block count is S-1, S, S+1, 2S+1 for every span,
    reached once by data alone (nb = data blocks + 1) and once behind a
    1-block AAD (nb = 1 + data blocks + 1); the last data block once full and
    once holding a single byte."""
    spans = CB.chacha_batch_spans()
    assert 16 in spans and 64 in spans and spans == sorted(set(spans))
    lens, aads = [], []
    for s in spans:
        for nb in (s - 1, s, s + 1, 2 * s + 1):
            for aad, nd in ((0, nb - 1), (13, nb - 2)):
                for n in (16 * nd, 16 * nd - 15):
                    lens.append(n)
                    aads.append(aad)
    check_hash(pool, lens, aads)


def test_hash_aad_lengths_and_gmac_shape(pool):
    """AADs of 16 and 17 bytes (one block exactly, one byte into the second), and a record of no data behind 64 KiB of AAD."""
    check_hash(pool, [100, 100, 0, 0, 33], [16, 17, 16, 65536, 0])


def test_hash_adversarial_key_and_data(gpu):
    """All-0xFF records under r all ones before clamping and s all ones: the largest limbs the carry bound allows."""
    key = b"\xff" * 32
    for n in (16, 1024, 4096, 65536 + 16):
        x = torch.full((n,), 0xFF, dtype=torch.uint8, device=gpu)
        want = ref_hash(key, b"\xff" * n, b"")
        for ln in (16, 64):
            assert rows(CB.poly1305_batch([x], [key], lanes=ln))[0] == want, (n, ln)


# ---- the AEAD -----------------------------------------------------------------------
def ref_seal(key, nonce, data, aad):
    return cpu_ref.chacha20_poly1305(key, nonce, data, aad)


def check_roundtrip(batch, outs_bytes, nv, hn, want, lens):
    """After ``encrypt``: ciphertexts and tags equal the oracle's; ``decrypt`` of them returns the plaintext."""
    _, tags = batch.encrypt(nv)
    got_t = rows(tags)
    cts = outs_bytes()
    for m, (ct, tag) in enumerate(want):
        assert cts[m] == ct, (m, lens[m], "ciphertext")
        assert got_t[m] == tag, (m, lens[m], "tag", got_t[m].hex(), tag.hex())
    return cts, tags.clone()


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("n", ONE_LENS)
def test_aead_one_record(pool, gpu, n, lanes):
    xs, hx, ad, ha = cut(pool, [n], [13])
    nv, hn = make_nonces(gpu, 1, n)
    ct, tag = ref_seal(KEY, hn[0], hx[0], ha[0])
    b = CB.ChaChaBatch(xs, KEY, aads=ad, lanes=lanes)
    outs, tags = b.encrypt(nv)
    assert host(outs[0]) == ct and host(tags) == tag
    d = CB.ChaChaBatch(outs, KEY, aads=ad, lanes=lanes)
    pts, ok = d.decrypt(nv, tags.clone())
    assert host(pts[0]) == hx[0] and ok.tolist() == [True]


def test_aead_one_mib_record(pool, gpu):
    """The cap: 256 tiles and 65538 hashed blocks in one record, in place."""
    x = pool["dev"][:MIB].clone()
    nv, hn = make_nonces(gpu, 1, 5)
    ct, tag = ref_seal(KEYS[1], hn[0], pool["host"][:MIB], b"")
    b = CB.ChaChaBatch([x], KEYS[1], outs=[x])
    _, tags = b.encrypt(nv)
    assert host(x) == ct and host(tags) == tag
    _, ok = b.decrypt(nv, tags.clone())
    assert host(x) == pool["host"][:MIB] and ok.tolist() == [True]


def test_rfc_8439_vector_as_a_record_of_a_batch(pool, gpu):
    """Section 2.8.2 in the middle of other records, under its own key."""
    key, nonce, aad, pt = (bytes.fromhex(RFC[k]) for k in ("key", "nonce", "aad", "pt"))
    xs, hx, _, _ = cut(pool, [100, 0, 5000])
    xs = [xs[0], torch.frombuffer(bytearray(pt), dtype=torch.uint8).to(gpu), xs[1], xs[2]]
    nv, hn = make_nonces(gpu, 4, 9)
    nv[1] = torch.frombuffer(bytearray(nonce), dtype=torch.uint8).to(gpu)
    outs, tags = CB.chacha20_poly1305_encrypt_batch(xs, [KEY, key], nv, aads=[b"", aad, b"x", None], key_index=[0, 1, 0, 0])
    assert host(outs[1]).hex() == RFC["ct"] and rows(tags)[1].hex() == RFC["tag"]
    assert host(outs[3]) == ref_seal(KEY, hn[3], hx[2], b"")[0]


def mixed(pool, gpu):
    lens, aads = [], []
    for i in range(300):
        lens.append(0 if i % 3 == 1 else ONE_LENS[(i // 3 * 7 + i) % len(ONE_LENS)])
        aads.append([0, 13, 16, 17, 1, 40][i % 6] if i % 4 else 0)
    kidx = [(i * 5 + i // 7) % 3 for i in range(300)]
    xs, hx, ad, ha = cut(pool, lens, aads)
    nv, hn = make_nonces(gpu, 300, 77)
    want = [ref_seal(KEYS[k], n, d, a) for k, n, d, a in zip(kidx, hn, hx, ha)]
    return lens, kidx, xs, hx, ad, ha, nv, hn, want


_mixed = {}


@pytest.fixture(scope="module")
def mix(pool, gpu):
    """About 300 records, lengths of ONE_LENS interleaved with empty ones, three keys, AADs on some; the oracle once."""
    if not _mixed:
        _mixed["v"] = mixed(pool, gpu)
    return _mixed["v"]


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_aead_mixed_batch_of_tensors(mix, gpu, inplace):
    lens, kidx, xs, hx, ad, ha, nv, hn, want = mix
    xs = [x.clone() for x in xs]  # the pool is never written
    b = CB.ChaChaBatch(xs, KEYS, outs=xs if inplace else None, aads=ad, key_index=kidx)
    assert b.ntiles == sum((n + 4095) // 4096 for n in lens)
    _, tags = check_roundtrip(b, lambda: [host(o) for o in b.outs], nv, hn, want, lens)
    d = b if inplace else CB.ChaChaBatch(b.outs, KEYS, outs=b.outs, aads=ad, key_index=kidx)
    pts, ok = d.decrypt(nv, tags)
    assert ok.dtype == torch.bool and bool(ok.all())
    for m, p in enumerate(pts):
        assert host(p) == hx[m], (m, lens[m])


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_aead_mixed_batch_packed(mix, pool, gpu, inplace):
    lens, kidx, xs, hx, ad, ha, nv, hn, want = mix
    total = sum((n + 15) // 16 * 16 for n in lens)
    buf = pool["dev"][:total].clone()
    # the packed form takes one AAD length for all: 13 bytes each, rows of a [n, 13] tensor at an odd address
    aad = pool["dev"][AAD_AT:AAD_AT + 13 * len(lens)].view(len(lens), 13)
    ha13 = [pool["host"][AAD_AT + 13 * m:AAD_AT + 13 * m + 13] for m in range(len(lens))]
    want13 = [ref_seal(KEYS[k], n, d, a) for k, n, d, a in zip(kidx, hn, hx, ha13)]
    b = CB.ChaChaBatch.packed(buf, lens, KEYS, out=buf if inplace else None, aad=aad, key_index=kidx)
    offs = np.concatenate([[0], np.cumsum([(n + 15) // 16 * 16 for n in lens])[:-1]])
    before = host(b.out) if not inplace else None

    def outs_bytes():
        o = host(b.out)
        return [o[at:at + n] for at, n in zip(offs, lens)]

    _, tags = check_roundtrip(b, outs_bytes, nv, hn, want13, lens)
    if not inplace:  # bytes of out outside the records are not written
        after = host(b.out)
        for at, n in zip(offs, lens):
            pad = (n + 15) // 16 * 16 - n
            assert after[at + n:at + n + pad] == before[at + n:at + n + pad]
    d = CB.ChaChaBatch.packed(b.out, lens, KEYS, out=b.out, aad=aad, key_index=kidx)
    _, ok = d.decrypt(nv, tags)
    assert bool(ok.all()) and outs_bytes() == hx


# ---- forgery --------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("what", ["ciphertext", "tag", "aad", "nonce"])
def test_a_forged_record_fails_alone(pool, gpu, what, inplace):
    lens = [4097, 0, 100, 5000, 64, 1, 8193]
    F = 3  # the forged record, in the middle
    xs, hx, ad, ha = cut(pool, lens, [13] * len(lens))
    nv, hn = make_nonces(gpu, len(lens), 31)
    kidx = [i % 3 for i in range(len(lens))]
    outs, tags = CB.chacha20_poly1305_encrypt_batch(xs, KEYS, nv, aads=ad, key_index=kidx)
    cts = [o.clone() for o in outs]
    tags, nv, ad = tags.clone(), nv.clone(), [a.clone() for a in ad]
    {"ciphertext": cts[F], "tag": tags[F], "aad": ad[F], "nonce": nv[F]}[what][5] ^= 0x10
    d = CB.ChaChaBatch(cts, KEYS, outs=cts if inplace else None, aads=ad, key_index=kidx)
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
    lens = [100, 4096, 0, 5000]
    xs, hx, ad, ha = cut(pool, lens, [13] * 4)
    b = CB.ChaChaBatch(xs, KEYS[:2], aads=ad, key_index=[0, 1, 0, 1])
    seen = []
    for seed in (1, 2):
        nv, hn = make_nonces(gpu, 4, seed)
        outs, tags = b.encrypt(nv)
        got = [host(o) for o in outs]
        for m in range(4):
            ct, tag = ref_seal(KEYS[m % 2], hn[m], hx[m], ha[m])
            assert got[m] == ct and rows(tags)[m] == tag
        seen.append(got)
    assert seen[0][0] != seen[1][0] and seen[0][3] != seen[1][3]


def test_one_nonce_under_two_keys(pool, gpu):
    """The keystream depends on the record's key: equal plaintexts and nonces, different ciphertexts."""
    x = pool["dev"][:4100]
    nv, hn = make_nonces(gpu, 1, 3)
    nv = nv.repeat(2, 1)
    outs, _ = CB.chacha20_poly1305_encrypt_batch([x, x], KEYS[:2], nv)
    a, b = host(outs[0]), host(outs[1])
    assert a != b and a == ref_seal(KEYS[0], hn[0], pool["host"][:4100], b"")[0] \
        and b == ref_seal(KEYS[1], hn[0], pool["host"][:4100], b"")[0]


# ---- graph ---------------------------------------------------------------------------
def test_encrypt_replays_in_a_graph(pool, gpu):
    """The chain is linear on one stream: captured once, replayed after nonces and inputs changed in place."""
    lens = [4097, 0, 100, 64]
    xs = [x.clone() for x in cut(pool, lens)[0]]
    nv, _ = make_nonces(gpu, 4, 11)
    b = CB.ChaChaBatch(xs, KEYS, key_index=[0, 1, 2, 0])
    b.encrypt(nv)  # warm: code objects are loaded outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.encrypt(nv)
    nv2, hn2 = make_nonces(gpu, 4, 12)
    nv.copy_(nv2)
    new = [pool["dev"][MIB + 16 * m:MIB + 16 * m + n] for m, n in enumerate(lens)]
    for x, y in zip(xs, new):
        x.copy_(y)
    g.replay()
    for m, n in enumerate(lens):
        ct, tag = ref_seal(KEYS[[0, 1, 2, 0][m]], hn2[m], pool["host"][MIB + 16 * m:MIB + 16 * m + n], b"")
        assert host(b.outs[m]) == ct and rows(b.tags)[m] == tag, m


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
    lens = [4097, 0, 100, 8193]
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
    b = CB.ChaChaBatch(xs, KEYS, aads=aad, key_index=[0, 1, 2, 1])
    want = [ref_seal(KEYS[k], n, d, a) for k, n, d, a in zip([0, 1, 2, 1], hn, hf, hfa)]

    def call(s):
        outs, tags = b.encrypt(nv, stream=s)
        return list(outs) + [tags]

    run_contract(gpu, xs + [aad, nv], fresh + [faad, fnv], b.outs + [b.tags], call,
                 [w[0] for w in want] + [b"".join(w[1] for w in want)])


def test_stream_contract_decrypt(pool, gpu):
    lens, xs, fresh, hf, aad, faad, hfa, nv, fnv, hn = contract_setup(pool, gpu)
    # the late inputs are ciphertexts with their tags: decrypt returns the plaintexts and all-true verdicts
    sealed = [ref_seal(KEYS[k], n, d, a) for k, n, d, a in zip([0, 1, 2, 1], hn, hf, hfa)]
    fresh = [torch.frombuffer(bytearray(c), dtype=torch.uint8).to(gpu) if c else f for (c, _), f in zip(sealed, fresh)]
    ftags = torch.frombuffer(bytearray(b"".join(t for _, t in sealed)), dtype=torch.uint8).to(gpu).view(4, 16)
    tags = torch.zeros_like(ftags)
    b = CB.ChaChaBatch(xs, KEYS, aads=aad, key_index=[0, 1, 2, 1])

    def call(s):
        outs, ok = b.decrypt(nv, tags, stream=s)
        return list(outs) + [ok.view(torch.uint8)]

    run_contract(gpu, xs + [aad, nv, tags], fresh + [faad, fnv, ftags], b.outs + [b.ok], call, hf + [b"\x01" * 4])


def test_stream_contract_poly1305(pool, gpu):
    lens, xs, fresh, hf, aad, faad, hfa, nv, fnv, hn = contract_setup(pool, gpu)
    keys = otks(4, 5)
    fkeys = otks(4, 6)
    otk = torch.frombuffer(bytearray(b"".join(keys)), dtype=torch.uint8).to(gpu).view(4, 32)
    fotk = torch.frombuffer(bytearray(b"".join(fkeys)), dtype=torch.uint8).to(gpu).view(4, 32)
    b = CB.ChaChaBatch(xs, KEY, outs=xs, aads=aad)
    want = b"".join(ref_hash(k, d, a) for k, d, a in zip(fkeys, hf, hfa))
    run_contract(gpu, xs + [aad, otk], fresh + [faad, fotk], [], lambda s: [b.poly1305(otk, stream=s)], [want])


# ---- the object interface ----------------------------------------------------------------
def test_model_batch_roundtrip_against_the_single_message_ops(pool, gpu):
    lens = [100, 0, 5000]
    xs, hx, _, _ = cut(pool, lens)
    aads = [b"header-0", b"", b"header-2 is longer"]
    nv, hn = make_nonces(gpu, 3, 15)
    m = models.chacha.ChaCha20Poly1305(KEY)
    outs, tags = m.encrypt_batch(xs, nv, aads=aads)
    for i in range(3):
        ct, tag = ops.chacha20_poly1305_encrypt(xs[i], KEY, hn[i], aads[i])
        assert host(outs[i]) == host(ct) and rows(tags)[i] == host(tag)
    pts, ok = m.decrypt_batch(outs, nv, tags.clone(), aads=aads)
    assert bool(ok.all())
    for i in range(3):
        assert host(pts[i]) == hx[i]
        assert host(ops.chacha20_poly1305_decrypt(outs[i], KEY, hn[i], rows(tags)[i], aads[i])) == hx[i]
