#!/usr/bin/env python3
"""Serving-shaped AES-CCM: many short records under one key, each with its own
nonce, AAD and tag, on one MI355X.  Per (shape, key size), in ONE process, the
arms alternated run by run:

  ccm_batch_encrypt / _decrypt    ops.ccm_batch_ops.CcmBatch (packed layout): one
                                  record per lane, MAC and counter mode as two
                                  blocks in flight, one pass -- the feature
  gcm_batch_encrypt / _decrypt    ops.GcmBatch under the same key: two passes
  ocb_batch_encrypt / _decrypt    ops.ocb_batch_ops.OcbBatch: one pass, one
                                  cipher call per block
  cbc_segments_encrypt            ops.cbc_encrypt_segments with the record length
                                  as the segment length: the same one chain per
                                  lane with ONE cipher call per block -- CCM makes
                                  two on the same LDS tables, so about half of
                                  this rate is what to expect at chip-filling
                                  batches
  per_record_loop                 ops.ccm_batch_ops.ccm_encrypt per record over
                                  the first --loop-records records: a plan, an
                                  upload and a launch each

Timed with device events: --warmup rounds, then --iters timed ones (the
per-record loop: 1 and --loop-iters).  Before anything is timed a seeded sample
of every arm's output is compared with the C oracle.  Prints one JSON line per
(shape, key size).

--order-ab instead times ONE mixed-length batch (--order-records records of
16 .. --order-max bytes, lengths drawn log-uniformly, in random order) with the
planner's order -- sorted by block count, longest first -- against the records
as given: the lanes of a wave run for as long as the longest record among them.

    python benchmarks/ccm_batch.py
    python benchmarks/ccm_batch.py --shapes 262144x256 --keybits 256
    python benchmarks/ccm_batch.py --order-ab
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

CB = ops.ccm_batch_ops
OB = ops.ocb_batch_ops


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rate(ms_list, nbytes, nrec, digits=2):
    med, best = statistics.median(ms_list), min(ms_list)
    return {"ms_median": round(med, 4), "ms_best": round(best, 4), "ms_worst": round(max(ms_list), 4),
            "gbps": round(nbytes / med / 1e6, digits), "records_per_s": round(nrec / med * 1e3)}


def alternate(arms, warmup, iters):
    """Every arm once per round, --warmup rounds dropped: {arm: [ms]}."""
    ms = {k: [] for k in arms}
    for it in range(warmup + iters):
        for k, fn in arms.items():
            t = once_ms(fn)
            if it >= warmup:
                ms[k].append(t)
    return ms


def make_key(keybits):
    return bytes((11 * i + keybits + 1) & 0xFF for i in range(keybits // 8))


def piece(t, i, size):
    return t[i * size:(i + 1) * size].cpu().numpy().tobytes()


def run_shape(dev, n, size, keybits, args):
    total = n * size
    aad_len = args.aad
    key = make_key(keybits)
    src = torch.empty(total, dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=n + size)
    rng = np.random.default_rng(size + aad_len + keybits)
    nonce_host = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    nonces = torch.from_numpy(nonce_host).to(dev)
    aad_host = rng.integers(0, 256, (n, max(aad_len, 1)), dtype=np.uint8)[:, :aad_len]
    aad = torch.from_numpy(np.ascontiguousarray(aad_host)).to(dev) if aad_len else None
    c_ct, c_back, g_ct, g_back, o_ct, o_back, s_ct, l_ct = (torch.empty_like(src) for _ in range(8))
    lens = [size] * n

    c_enc = CB.CcmBatch.packed(src, lens, key, out=c_ct, aad=aad, tag_bytes=args.tag)
    c_dec = CB.CcmBatch.packed(c_ct, lens, key, out=c_back, aad=aad, tag_bytes=args.tag)
    g_enc = ops.GcmBatch.packed(src, lens, key, out=g_ct, aad=aad)
    g_dec = ops.GcmBatch.packed(g_ct, lens, key, out=g_back, aad=aad)
    o_enc = OB.OcbBatch.packed(src, lens, key, out=o_ct, aad=aad)
    o_dec = OB.OcbBatch.packed(o_ct, lens, key, out=o_back, aad=aad)
    iv0 = bytes(range(16))
    nloop = min(args.loop_records, n)
    xs, outs = list(src[:nloop * size].split(size)), list(l_ct[:nloop * size].split(size))
    nb = [nonce_host[i].tobytes() for i in range(n)]
    aadb = [aad_host[i].tobytes() for i in range(n)]
    loop_tags = []

    def loop():
        loop_tags.clear()
        for i in range(nloop):
            loop_tags.append(CB.ccm_encrypt(xs[i], key, nb[i], aadb[i], out=outs[i], tag_bytes=args.tag)[1])

    # every arm once, and a seeded sample of its output against the oracle, before anything is timed
    c_enc.encrypt(nonces)
    c_tags = c_enc.tags.clone()
    _, c_ok = c_dec.decrypt(nonces, c_tags)
    g_enc.encrypt(nonces)
    g_tags = g_enc.tags.clone()
    _, g_ok = g_dec.decrypt(nonces, g_tags)
    o_enc.encrypt(nonces)
    o_tags = o_enc.tags.clone()
    _, o_ok = o_dec.decrypt(nonces, o_tags)
    ops.cbc_encrypt_segments(src, key, iv0, size, out=s_ct)
    loop()
    torch.cuda.synchronize()
    good = {"ccm_batch": bool(c_ok.all()), "gcm_batch": bool(g_ok.all()), "ocb_batch": bool(o_ok.all()),
            "cbc_segments": True, "per_record_loop": True}
    ct_, gt, ot = c_tags.cpu().numpy(), g_tags.cpu().numpy(), o_tags.cpu().numpy()
    sample = random.Random(5).sample(range(n), min(6, n))
    for i in sample + [j for j in (0, nloop - 1, n - 1) if j not in sample]:
        pt = piece(src, i, size)
        w_ct, w_tag = cpu_ref.ccm(key, nb[i], pt, aadb[i], tag_bytes=args.tag)
        good["ccm_batch"] &= piece(c_ct, i, size) == w_ct and ct_[i].tobytes() == w_tag and piece(c_back, i, size) == pt
        if i < nloop:
            good["per_record_loop"] &= piece(l_ct, i, size) == w_ct and loop_tags[i] == w_tag
        w_ct, w_tag = cpu_ref.gcm(key, nb[i], pt, aadb[i])
        good["gcm_batch"] &= piece(g_ct, i, size) == w_ct and gt[i].tobytes() == w_tag and piece(g_back, i, size) == pt
        w_ct, w_tag = cpu_ref.ocb(key, nb[i], pt, aadb[i])
        good["ocb_batch"] &= piece(o_ct, i, size) == w_ct and ot[i].tobytes() == w_tag and piece(o_back, i, size) == pt
        iv = (int.from_bytes(iv0, "big") + i).to_bytes(16, "big")
        good["cbc_segments"] &= piece(s_ct, i, size) == cpu_ref.cbc(key, iv, pt)

    arms = {
        "ccm_batch_encrypt": lambda: c_enc.encrypt(nonces),
        "ccm_batch_decrypt": lambda: c_dec.decrypt(nonces, c_tags),
        "gcm_batch_encrypt": lambda: g_enc.encrypt(nonces),
        "gcm_batch_decrypt": lambda: g_dec.decrypt(nonces, g_tags),
        "ocb_batch_encrypt": lambda: o_enc.encrypt(nonces),
        "ocb_batch_decrypt": lambda: o_dec.decrypt(nonces, o_tags),
        "cbc_segments_encrypt": lambda: ops.cbc_encrypt_segments(src, key, iv0, size, out=s_ct),
    }
    ms = alternate(arms, args.warmup, args.iters)
    loop_ms = []
    for it in range(1 + args.loop_iters):
        t = once_ms(loop)
        if it >= 1:
            loop_ms.append(t)

    res = {"metric": "AES-CCM many-record throughput", "keybits": keybits, "records": n, "record_bytes": size,
           "aad_bytes": aad_len, "tag_bytes": args.tag, "total_bytes": total, "lanes_of_the_chip": CB.CcmBatch.spans()[-1],
           "warmup": args.warmup, "iters": args.iters, "data": "synthetic random records, random nonces"}
    for k in arms:
        res[k] = rate(ms[k], total, n)
    res["per_record_loop"] = dict(rate(loop_ms, nloop * size, nloop, digits=5), records=nloop, iters=args.loop_iters)
    g = lambda k: res[k]["gbps"]  # noqa: E731
    res["ccm_over_cbc_segments"] = {"encrypt": round(g("ccm_batch_encrypt") / g("cbc_segments_encrypt"), 3),
                                    "decrypt": round(g("ccm_batch_decrypt") / g("cbc_segments_encrypt"), 3),
                                    "expected": 0.5}
    res["ccm_over_gcm_batch"] = {"encrypt": round(g("ccm_batch_encrypt") / g("gcm_batch_encrypt"), 3),
                                 "decrypt": round(g("ccm_batch_decrypt") / g("gcm_batch_decrypt"), 3)}
    res["ccm_over_ocb_batch"] = {"encrypt": round(g("ccm_batch_encrypt") / g("ocb_batch_encrypt"), 3),
                                 "decrypt": round(g("ccm_batch_decrypt") / g("ocb_batch_decrypt"), 3)}
    res["per_record_loop_over_ccm_batch"] = round(g("per_record_loop") / g("ccm_batch_encrypt"), 7)
    res["verified_sample"] = good
    print(json.dumps(res), flush=True)
    return all(good.values())


def run_order_ab(dev, keybits, args):
    """One mixed-length batch: the planner's order against the records as given."""
    n = args.order_records
    rng = np.random.default_rng(n + keybits)
    lens = np.exp(rng.uniform(np.log(16), np.log(args.order_max), n)).astype(np.int64)
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum((lens[:-1] + 15) // 16 * 16)
    total = int(offs[-1] + (lens[-1] + 15) // 16 * 16)
    key = make_key(keybits)
    src = torch.empty(total, dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=n)
    nonce_host = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    nonces = torch.from_numpy(nonce_host).to(dev)
    out_s, out_i = torch.empty_like(src), torch.empty_like(src)
    arms, batches = {}, {}
    for name, sort, out in (("sorted", True, out_s), ("identity", False, out_i)):
        e = CB.CcmBatch.packed(src, lens, key, out=out, offsets=offs, _sort=sort)
        d = CB.CcmBatch.packed(out, lens, key, out=torch.empty_like(src), offsets=offs, _sort=sort)
        e.encrypt(nonces)
        tags = e.tags.clone()
        _, ok = d.decrypt(nonces, tags)
        batches[name] = (e, d, tags, bool(ok.all()))
        arms[name + "_encrypt"] = (lambda e=e: e.encrypt(nonces))
        arms[name + "_decrypt"] = (lambda d=d, tags=tags: d.decrypt(nonces, tags))
    torch.cuda.synchronize()
    good = batches["sorted"][3] and batches["identity"][3] and torch.equal(out_s, out_i) and \
        torch.equal(batches["sorted"][2], batches["identity"][2])
    ts = batches["sorted"][2].cpu().numpy()
    for i in random.Random(7).sample(range(n), 8) + [int(np.argmax(lens)), int(np.argmin(lens))]:
        o, k = int(offs[i]), int(lens[i])
        w_ct, w_tag = cpu_ref.ccm(key, nonce_host[i].tobytes(), src[o:o + k].cpu().numpy().tobytes())
        good = good and out_s[o:o + k].cpu().numpy().tobytes() == w_ct and ts[i].tobytes() == w_tag
    ms = alternate(arms, args.warmup, args.iters)
    nbytes = int(lens.sum())
    res = {"metric": "batched AES-CCM: the planner's order against the records as given", "keybits": keybits,
           "records": n, "min_bytes": int(lens.min()), "max_bytes": int(lens.max()), "total_bytes": nbytes,
           "lengths": "log-uniform, random order", "warmup": args.warmup, "iters": args.iters}
    for k in arms:
        res[k] = rate(ms[k], nbytes, n)
    res["sorted_over_identity"] = {d: round(res["sorted_" + d]["gbps"] / res["identity_" + d]["gbps"], 3)
                                   for d in ("encrypt", "decrypt")}
    res["verified_sample"] = bool(good)
    print(json.dumps(res), flush=True)
    return bool(good)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x4096,65536x1024,4096x16384,262144x256,1048576x256",
                    help="RECORDSxBYTES, comma separated")
    ap.add_argument("--keybits", default="128,256", help="AES key sizes, comma separated")
    ap.add_argument("--aad", type=int, default=13, help="AAD bytes per record")
    ap.add_argument("--tag", type=int, default=16, help="CCM tag bytes")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-records", type=int, default=256)
    ap.add_argument("--loop-iters", type=int, default=2)
    ap.add_argument("--order-ab", action="store_true", help="time the planner's order against the identity order")
    ap.add_argument("--order-records", type=int, default=262144)
    ap.add_argument("--order-max", type=int, default=16384, help="the longest record of the mixed batch, bytes")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    good = True
    for keybits in (int(v) for v in args.keybits.split(",")):
        if args.order_ab:
            good = run_order_ab(dev, keybits, args) and good
            continue
        for shape in args.shapes.split(","):
            n, size = (int(v) for v in shape.split("x"))
            if size % 16:
                raise SystemExit("record sizes must be multiples of 16 (the records are views of one buffer)")
            good = run_shape(dev, n, size, keybits, args) and good
    if not good:
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
