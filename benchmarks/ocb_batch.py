#!/usr/bin/env python3
"""Serving-shaped AES-OCB3: many small records under one key, each with its
own 12-byte nonce, AAD and 16-byte tag, on one MI355X.  Per (shape, key size),
in ONE process, the arms alternated run by run:

  ocb_batch_encrypt / _decrypt    ops.ocb_batch_ops.OcbBatch (packed layout):
                                  one pass over the data -- the feature
  gcm_batch_encrypt / _decrypt    ops.GcmBatch under the same key: two passes
  chacha_batch_encrypt            ops.chacha_batch_ops.ChaChaBatch (one 32-byte
                                  key): two passes, no AES
  ctr_batch                       ops.CtrBatch under the same key: one pass,
                                  no authentication -- the one-pass ceiling
  per_record_loop                 ops.ocb_ops.ocb_encrypt per record over the
                                  first --loop-records records: the only way
                                  without the batch

Timed with device events: --warmup rounds, then --iters timed ones (the
per-record loop: 1 and --loop-iters).  Before anything is timed a seeded
sample of every arm's output is compared with the C oracle.  Prints one JSON
line per (shape, key size).

--prep-aad instead times the batch with --prep-aad-bytes of AAD per record
against the same batch without AAD: the difference is what the prep kernel
spends hashing long AADs with 16 lanes per record.

    python benchmarks/ocb_batch.py
    python benchmarks/ocb_batch.py --shapes 16384x4096 --keybits 128
    python benchmarks/ocb_batch.py --prep-aad
"""
import argparse
import json
import os
import random
import statistics

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # before torch / HIP: dmabuf IPC only on this host driver (as bench.py)
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from our_tree_amd import ops  # noqa: E402
from our_tree_amd.models import cpu_ref  # noqa: E402

OB = ops.ocb_batch_ops
CB = ops.chacha_batch_ops


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rate(ms_list, nbytes, nrec):
    med, best = statistics.median(ms_list), min(ms_list)
    return {"ms_median": round(med, 4), "ms_best": round(best, 4), "ms_worst": round(max(ms_list), 4),
            "gbps": round(nbytes / med / 1e6, 2), "records_per_s": round(nrec / med * 1e3)}


def alternate(arms, warmup, iters):
    """Every arm once per round, --warmup rounds dropped: {arm: [ms]}."""
    ms = {k: [] for k in arms}
    for it in range(warmup + iters):
        for k, fn in arms.items():
            t = once_ms(fn)
            if it >= warmup:
                ms[k].append(t)
    return ms


def make_inputs(dev, n, size, aad_len, keybits):
    key = bytes((11 * i + keybits + 1) & 0xFF for i in range(keybits // 8))
    src = torch.empty(n * size, dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=n + size)
    rng = np.random.default_rng(size + aad_len + keybits)
    nonce_host = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    aad_host = rng.integers(0, 256, (n, max(aad_len, 1)), dtype=np.uint8)[:, :aad_len]
    aad = torch.from_numpy(np.ascontiguousarray(aad_host)).to(dev) if aad_len else None
    return key, src, nonce_host, torch.from_numpy(nonce_host).to(dev), aad_host, aad


def piece(t, i, size):
    return t[i * size:(i + 1) * size].cpu().numpy().tobytes()


def run_shape(dev, n, size, keybits, args):
    total = n * size
    aad_len = args.aad
    key, src, nonce_host, nonces, aad_host, aad = make_inputs(dev, n, size, aad_len, keybits)
    key32 = (key * 2)[:32]
    o_ct, o_back, g_ct, g_back, c_ct, r_ct, l_ct = (torch.empty_like(src) for _ in range(7))
    lens = [size] * n
    counters = np.zeros((n, 16), dtype=np.uint8)
    counters[:, :12] = nonce_host
    counters[:, 15] = 1

    o_enc = OB.OcbBatch.packed(src, lens, key, out=o_ct, aad=aad)
    o_dec = OB.OcbBatch.packed(o_ct, lens, key, out=o_back, aad=aad)
    g_enc = ops.GcmBatch.packed(src, lens, key, out=g_ct, aad=aad)
    g_dec = ops.GcmBatch.packed(g_ct, lens, key, out=g_back, aad=aad)
    c_enc = CB.ChaChaBatch.packed(src, lens, key32, out=c_ct, aad=aad)
    ctr = ops.CtrBatch.packed(src, lens, [key], counters, out=r_ct, key_index=np.zeros(n, dtype=np.int64))
    nloop = min(args.loop_records, n)
    xs, outs = list(src[:nloop * size].split(size)), list(l_ct[:nloop * size].split(size))
    nb = [nonce_host[i].tobytes() for i in range(n)]
    aadb = [aad_host[i].tobytes() for i in range(n)]
    loop_tags = []

    def loop():
        loop_tags.clear()
        for i in range(nloop):
            loop_tags.append(ops.ocb_ops.ocb_encrypt(xs[i], key, nb[i], aadb[i], out=outs[i])[1])

    # every arm once, and a seeded sample of its output against the oracle, before anything is timed
    o_enc.encrypt(nonces)
    o_tags = o_enc.tags.clone()
    _, o_ok = o_dec.decrypt(nonces, o_tags)
    g_enc.encrypt(nonces)
    g_tags = g_enc.tags.clone()
    _, g_ok = g_dec.decrypt(nonces, g_tags)
    c_enc.encrypt(nonces)
    ctr.run()
    loop()
    torch.cuda.synchronize()
    good = {"ocb_batch": bool(o_ok.all()), "gcm_batch": bool(g_ok.all()), "chacha_batch": True, "ctr_batch": True,
            "per_record_loop": True}
    ot, gt, ct_ = o_tags.cpu().numpy(), g_tags.cpu().numpy(), c_enc.tags.cpu().numpy()
    sample = random.Random(5).sample(range(n), min(6, n))
    for i in sample + [j for j in (0, nloop - 1) if j not in sample]:
        pt = piece(src, i, size)
        w_ct, w_tag = cpu_ref.ocb(key, nb[i], pt, aadb[i])
        good["ocb_batch"] &= piece(o_ct, i, size) == w_ct and ot[i].tobytes() == w_tag and piece(o_back, i, size) == pt
        w_ct, w_tag = cpu_ref.gcm(key, nb[i], pt, aadb[i])
        good["gcm_batch"] &= piece(g_ct, i, size) == w_ct and gt[i].tobytes() == w_tag and piece(g_back, i, size) == pt
        w_ct, w_tag = cpu_ref.chacha20_poly1305(key32, nb[i], pt, aadb[i])
        good["chacha_batch"] &= piece(c_ct, i, size) == w_ct and ct_[i].tobytes() == w_tag
        good["ctr_batch"] &= piece(r_ct, i, size) == cpu_ref.ctr(key, counters[i].tobytes(), pt)
        if i < nloop:
            w_ct, w_tag = cpu_ref.ocb(key, nb[i], pt, aadb[i])
            good["per_record_loop"] &= piece(l_ct, i, size) == w_ct and loop_tags[i].cpu().numpy().tobytes() == w_tag

    arms = {
        "ocb_batch_encrypt": lambda: o_enc.encrypt(nonces),
        "ocb_batch_decrypt": lambda: o_dec.decrypt(nonces, o_tags),
        "gcm_batch_encrypt": lambda: g_enc.encrypt(nonces),
        "gcm_batch_decrypt": lambda: g_dec.decrypt(nonces, g_tags),
        "chacha_batch_encrypt": lambda: c_enc.encrypt(nonces),
        "ctr_batch": lambda: ctr.run(),
    }
    ms = alternate(arms, args.warmup, args.iters)
    loop_ms = []
    for it in range(1 + args.loop_iters):
        t = once_ms(loop)
        if it >= 1:
            loop_ms.append(t)

    res = {"metric": "AES-OCB3 many-record throughput", "keybits": keybits, "records": n, "record_bytes": size,
           "aad_bytes": aad_len, "total_bytes": total, "ocb_tiles": o_enc.ntiles, "gcm_hash_lanes": g_enc.lanes,
           "chacha_hash_lanes": c_enc.lanes, "warmup": args.warmup, "iters": args.iters,
           "data": "synthetic random records, random nonces"}
    for k in arms:
        res[k] = rate(ms[k], total, n)
    res["per_record_loop"] = dict(rate(loop_ms, nloop * size, nloop), records=nloop, iters=args.loop_iters)
    g = lambda k: res[k]["gbps"]  # noqa: E731
    res["ocb_over_gcm_batch"] = {"encrypt": round(g("ocb_batch_encrypt") / g("gcm_batch_encrypt"), 3),
                                 "decrypt": round(g("ocb_batch_decrypt") / g("gcm_batch_decrypt"), 3)}
    res["share_of_ctr_batch"] = {k: round(g(k) / g("ctr_batch"), 3) for k in arms if k != "ctr_batch"}
    res["ocb_over_chacha_batch_encrypt"] = round(g("ocb_batch_encrypt") / g("chacha_batch_encrypt"), 3)
    res["per_record_loop_over_ocb_batch"] = round(g("per_record_loop") / g("ocb_batch_encrypt"), 3)
    res["verified_sample"] = good
    print(json.dumps(res), flush=True)
    return all(good.values())


def run_prep_aad(dev, args):
    """The batch with a long AAD per record against the same batch without: what prep's 16-lane hash costs."""
    n, size, aad_len = args.prep_records, 1024, args.prep_aad_bytes
    key, src, nonce_host, nonces, aad_host, aad = make_inputs(dev, n, size, aad_len, 128)
    out = torch.empty_like(src)
    lens = [size] * n
    with_aad = OB.OcbBatch.packed(src, lens, key, out=out, aad=aad)
    without = OB.OcbBatch.packed(src, lens, key, out=out)
    with_aad.encrypt(nonces)
    torch.cuda.synchronize()
    tags = with_aad.tags.cpu().numpy()
    good = True
    for i in (0, n // 2, n - 1):
        w_ct, w_tag = cpu_ref.ocb(key, nonce_host[i].tobytes(), piece(src, i, size), aad_host[i].tobytes())
        good = good and piece(out, i, size) == w_ct and tags[i].tobytes() == w_tag
    ms = alternate({"with_aad": lambda: with_aad.encrypt(nonces), "without_aad": lambda: without.encrypt(nonces)},
                   args.warmup, args.iters)
    a, b = statistics.median(ms["with_aad"]), statistics.median(ms["without_aad"])
    res = {"metric": "batched OCB3 prep kernel: long AADs", "keybits": 128, "records": n, "record_bytes": size,
           "aad_bytes": aad_len, "ms_with_aad": round(a, 4), "ms_without_aad": round(b, 4),
           "prep_hash_ms": round(a - b, 4), "aad_gbps": round(n * aad_len / max(a - b, 1e-6) / 1e6, 2),
           "warmup": args.warmup, "iters": args.iters, "verified_sample": good}
    print(json.dumps(res), flush=True)
    return good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x4096,65536x1024,4096x16384", help="RECORDSxBYTES, comma separated")
    ap.add_argument("--keybits", default="128,256", help="AES key sizes, comma separated")
    ap.add_argument("--aad", type=int, default=13, help="AAD bytes per record")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-records", type=int, default=1024)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--prep-aad", action="store_true", help="time the prep kernel's AAD hash instead of the arms")
    ap.add_argument("--prep-aad-bytes", type=int, default=65536)
    ap.add_argument("--prep-records", type=int, default=1024)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    good = True
    if args.prep_aad:
        good = run_prep_aad(dev, args)
    else:
        for shape in args.shapes.split(","):
            n, size = (int(v) for v in shape.split("x"))
            if size % 16:
                raise SystemExit("record sizes must be multiples of 16 (the records are views of one buffer)")
            for keybits in (int(v) for v in args.keybits.split(",")):
                good = run_shape(dev, n, size, keybits, args) and good
    if not good:
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
