#!/usr/bin/env python3
"""Serving-shaped AES-GCM: many small records under one key, each with its own
12-byte IV, AAD and tag, on one MI355X.  Per shape, in ONE process, the arms
alternated run by run:

  batch_encrypt / batch_decrypt   ops.GcmBatch (packed layout): one linear chain
                                  of launches for every record
  ctr_batch                       ops.CtrBatch over the same records: the cipher
                                  alone, the ceiling of the CTR half
  ghash_one_message               ops.ghash over the same total bytes as ONE
                                  message: the ceiling of the hash
  per_record_loop                 ops.gcm_encrypt per record over the first
                                  --loop-records records: the only way without
                                  the batch

Timed with device events: --warmup runs, then --iters timed ones (the
per-record loop: 1 and --loop-iters).  A seeded sample of records and tags is
verified against the C oracle.  Prints one JSON line per (shape, AAD, key).

    python benchmarks/gcm_batch.py
    python benchmarks/gcm_batch.py --shapes 16384x4096 --bits 128 --aad 13
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


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rate(ms_list, nbytes, nrec):
    med, best = statistics.median(ms_list), min(ms_list)
    return {"ms_median": round(med, 4), "ms_best": round(best, 4), "gbps": round(nbytes / med / 1e6, 2),
            "records_per_s": round(nrec / med * 1e3)}


def run_shape(dev, n, size, aad_len, bits, args):
    key = bytes((7 * i + bits) & 0xFF for i in range(bits // 8))
    total = n * size
    src = torch.empty(total, dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=n + size)
    ct, back, ctr_out = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
    rng = np.random.default_rng(bits + aad_len)
    iv_host = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    ivs = torch.from_numpy(iv_host).to(dev)
    aad_host = rng.integers(0, 256, (n, max(aad_len, 1)), dtype=np.uint8)[:, :aad_len]
    aad = torch.from_numpy(np.ascontiguousarray(aad_host)).to(dev) if aad_len else None
    lens = [size] * n

    enc = ops.GcmBatch.packed(src, lens, key, out=ct, aad=aad, lanes=args.lanes)
    dec = ops.GcmBatch.packed(ct, lens, key, out=back, aad=aad, lanes=args.lanes)
    ctrs = np.zeros((n, 16), dtype=np.uint8)
    ctrs[:, :12] = iv_host
    ctrs[:, 15] = 2
    cb = ops.CtrBatch.packed(src, lens, [key], ctrs, out=ctr_out, key_index=np.zeros(n, dtype=np.int64),
                             tile_blocks=enc.tile_blocks)
    h = cpu_ref.gcm_h(key)
    nloop = min(args.loop_records, n)
    xs, outs = list(src[:nloop * size].split(size)), list(ctr_out[:nloop * size].split(size))
    ivb = [iv_host[i].tobytes() for i in range(nloop)]
    aadb = [aad_host[i].tobytes() for i in range(nloop)]

    def loop():
        for i in range(nloop):
            ops.gcm_encrypt(xs[i], key, ivb[i], aadb[i], out=outs[i])

    enc.encrypt(ivs)
    tags = enc.tags.clone()
    arms = {
        "batch_encrypt": lambda: enc.encrypt(ivs),
        "batch_decrypt": lambda: dec.decrypt(ivs, tags),
        "ctr_batch": cb.run,
        "ghash_one_message": lambda: ops.ghash(src, h),
    }
    ms = {k: [] for k in arms}
    for it in range(args.warmup + args.iters):  # alternated: every arm once per round
        for k, fn in arms.items():
            t = once_ms(fn)
            if it >= args.warmup:
                ms[k].append(t)
    loop_ms = []
    for it in range(1 + args.loop_iters):
        t = once_ms(loop)
        if it >= 1:
            loop_ms.append(t)

    res = {"metric": "AES-GCM many-record throughput", "records": n, "record_bytes": size, "aad_bytes": aad_len,
           "key_bits": bits, "total_bytes": total, "tile_blocks": enc.tile_blocks, "tiles": enc.ntiles, "hash_lanes": enc.lanes,
           "warmup": args.warmup, "iters": args.iters, "data": "synthetic random records, random IVs"}
    for k in arms:
        res[k] = rate(ms[k], total, n)
    res["per_record_loop"] = dict(rate(loop_ms, nloop * size, nloop), records=nloop, iters=args.loop_iters)
    res["batch_vs_per_record_loop"] = round(res["batch_encrypt"]["gbps"] / res["per_record_loop"]["gbps"], 1)
    res["batch_vs_ctr_batch"] = round(res["batch_encrypt"]["gbps"] / res["ctr_batch"]["gbps"], 3)
    res["decrypt_vs_ctr_batch"] = round(res["batch_decrypt"]["gbps"] / res["ctr_batch"]["gbps"], 3)

    # a seeded sample of records against the oracle: ciphertext, tag, and the way back
    enc.encrypt(ivs)
    _, okv = dec.decrypt(ivs, tags)
    torch.cuda.synchronize()
    good = bool(okv.all())
    tags_h = enc.tags.cpu().numpy()
    for i in random.Random(5).sample(range(n), min(8, n)):
        pt = src[i * size:(i + 1) * size].cpu().numpy().tobytes()
        want_ct, want_tag = cpu_ref.gcm(key, iv_host[i].tobytes(), pt, aad_host[i].tobytes())
        good = good and ct[i * size:(i + 1) * size].cpu().numpy().tobytes() == want_ct
        good = good and tags_h[i].tobytes() == want_tag
        good = good and back[i * size:(i + 1) * size].cpu().numpy().tobytes() == pt
    res["verified_sample"] = good
    print(json.dumps(res), flush=True)
    return good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x4096,65536x1024,4096x16384", help="RECORDSxBYTES, comma separated")
    ap.add_argument("--aad", default="13,0", help="AAD bytes per record, comma separated")
    ap.add_argument("--bits", default="128,256")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-records", type=int, default=1024)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=None, help="lanes of the hash kernel per record (16/64; default: auto)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    good = True
    for shape in args.shapes.split(","):
        n, size = (int(v) for v in shape.split("x"))
        if size % 16:
            raise SystemExit("record sizes must be multiples of 16 (the records are views of one buffer)")
        for aad_len in (int(v) for v in args.aad.split(",")):
            for bits in (int(v) for v in args.bits.split(",")):
                good = run_shape(dev, n, size, aad_len, bits, args) and good
    if not good:
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
