"""What a run of a batched AES-CCM plan may do (otc.h otc_aes_ccm_batch): one
linear chain of launches on the given stream, no allocation, no host wait.  So
it replays in a captured graph with nonces and inputs changed in place, and --
by the method of tests/test_gpu_ocb_batch.py -- it runs in stream order behind
pending work without the host waiting for it."""
import time

import numpy as np
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

CB = ops.ccm_batch_ops
KEY = bytes(range(3, 19))
NB, TB = 13, 8
LENS = [1040, 0, 100, 8193]
AAD = 13


def host(t: torch.Tensor) -> bytes:
    torch.cuda.synchronize()
    return t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def rows(t, width):
    b = host(t)
    return [b[i:i + width] for i in range(0, len(b), width)]


def dev_bytes(gpu, b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)


def material(gpu, seed, lens=LENS):
    """Records, AADs ([n, 13]) and nonces of one seed: device tensors and host bytes."""
    rng = np.random.default_rng(seed)
    hx = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    ha = [rng.integers(0, 256, AAD, dtype=np.uint8).tobytes() for _ in lens]
    hn = [rng.integers(0, 256, NB, dtype=np.uint8).tobytes() for _ in lens]
    xs = [dev_bytes(gpu, b) for b in hx]
    return xs, hx, dev_bytes(gpu, b"".join(ha)).view(len(lens), AAD), ha, dev_bytes(gpu, b"".join(hn)).view(len(lens), NB), hn


# ---- graph ---------------------------------------------------------------------------
def test_encrypt_and_decrypt_replay_in_a_graph(gpu):
    """Captured once, replayed after nonces, AADs and inputs changed in place."""
    lens = [1040, 0, 100, 64, 4113]
    n = len(lens)
    xs, _, aad, _, nv, _ = material(gpu, 11, lens)
    b = CB.CcmBatch(xs, KEY, aads=aad, nonce_bytes=NB, tag_bytes=TB)
    d = CB.CcmBatch(b.outs, KEY, aads=aad, nonce_bytes=NB, tag_bytes=TB)
    expect = torch.zeros((n, TB), dtype=torch.uint8, device=gpu)
    b.encrypt(nv)  # warm: code objects are loaded outside the capture
    d.decrypt(nv, expect)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.encrypt(nv)
        expect.copy_(b.tags)
        d.decrypt(nv, expect)
    for seed in (12, 13):
        new, hnew, aad2, ha2, nv2, hn2 = material(gpu, seed, lens)
        nv.copy_(nv2)
        aad.copy_(aad2)
        for x, y in zip(xs, new):
            x.copy_(y)
        g.replay()
        want = cpu_ref.ccm_batch(KEY, hn2, hnew, ha2, tag_bytes=TB)
        for m in range(n):
            assert host(b.outs[m]) == want[m][0] and rows(b.tags, TB)[m] == want[m][1], (seed, m)
            assert host(d.outs[m]) == hnew[m] and rows(d.tags, TB)[m] == want[m][1], (seed, m)
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
    """Behind a delay on a fresh independent stream go, with no host wait in
    between, the copies that PRODUCE the op's inputs (``fresh`` into
    ``inputs``), the op, and copies that CONSUME its results.  The event behind
    the delay has not fired when the enqueue returns, and the consumed bytes
    equal ``expect`` (the oracle over the fresh inputs)."""
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


def test_stream_contract_encrypt(gpu):
    xs, _, aad, _, nv, _ = material(gpu, 21)
    fresh, hf, faad, hfa, fnv, hn = material(gpu, 22)
    b = CB.CcmBatch(xs, KEY, aads=aad, nonce_bytes=NB, tag_bytes=TB)
    want = cpu_ref.ccm_batch(KEY, hn, hf, hfa, tag_bytes=TB)

    def call(s):
        outs, tags = b.encrypt(nv, stream=s)
        return list(outs) + [tags]

    run_contract(gpu, xs + [aad, nv], fresh + [faad, fnv], b.outs + [b.tags], call,
                 [w[0] for w in want] + [b"".join(w[1] for w in want)])


def test_stream_contract_decrypt(gpu):
    xs, _, aad, _, nv, _ = material(gpu, 23)
    _, hf, faad, hfa, fnv, hn = material(gpu, 24)
    # the late inputs are ciphertexts with their tags: decrypt returns the plaintexts and all-true verdicts
    sealed = cpu_ref.ccm_batch(KEY, hn, hf, hfa, tag_bytes=TB)
    fresh = [dev_bytes(gpu, c) for c, _ in sealed]
    ftags = dev_bytes(gpu, b"".join(t for _, t in sealed)).view(len(LENS), TB)
    tags = torch.zeros_like(ftags)
    b = CB.CcmBatch(xs, KEY, aads=aad, nonce_bytes=NB, tag_bytes=TB)

    def call(s):
        outs, ok = b.decrypt(nv, tags, stream=s)
        return list(outs) + [ok.view(torch.uint8)]

    run_contract(gpu, xs + [aad, nv, tags], fresh + [faad, fnv, ftags], b.outs + [b.ok], call,
                 hf + [b"\x01" * len(LENS)])
