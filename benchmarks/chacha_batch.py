#!/usr/bin/env python3
"""Serving-shaped ChaCha20-Poly1305: many small records, each with its own
key (one of --keys, dealt round robin), 12-byte nonce, AAD and tag, on one
MI355X.  Per shape, in ONE process, the arms alternated run by run:

  batch_encrypt / batch_decrypt   ops.chacha_batch_ops.ChaChaBatch (packed
                                  layout): one linear chain of launches for
                                  every record -- the feature
  chacha20_one_message            ops.chacha20 over the same total bytes as ONE
                                  message: the ceiling of the cipher
  poly1305_one_message            ops.poly1305 over the same total bytes as ONE
                                  message: the ceiling of the hash
  gcm_batch_aes128                ops.GcmBatch (AES-128) over the same records:
                                  the other AEAD
  per_record_loop                 ops.chacha20_poly1305_encrypt per record over
                                  the first --loop-records records: the only way
                                  without the batch

The two single-message arms are unfused ceilings: the batch reads the data
twice (cipher, then hash), so its share of either is a share of an unfused
ceiling, not of a peak.  Timed with device events: --warmup runs, then --iters
timed ones (the per-record loop: 1 and --loop-iters).  A seeded sample of
records and tags is verified against the C oracle.  Prints one JSON line per
(shape, AAD).

--lanes-table instead times the two forms of the batched hash kernel (16 and 64
lanes per record) against each other, alternated, on uniform batches of 256 B,
1, 4, 16 and 64 KiB records: the whole encryption and the hash alone; one JSON
line per record size.  otc_chacha_batch_lanes' rule comes from that table.

    python benchmarks/chacha_batch.py
    python benchmarks/chacha_batch.py --shapes 16384x4096 --aad 13
    python benchmarks/chacha_batch.py --lanes-table
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

from our_tree_amd import _native, ops  # noqa: E402
from our_tree_amd.models import cpu_ref  # noqa: E402

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


def make_inputs(dev, n, size, aad_len, nkeys):
    keys = [bytes((11 * i + 3 * k + 1) & 0xFF for i in range(32)) for k in range(nkeys)]
    src = torch.empty(n * size, dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=n + size)
    rng = np.random.default_rng(size + aad_len)
    nonce_host = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    aad_host = rng.integers(0, 256, (n, max(aad_len, 1)), dtype=np.uint8)[:, :aad_len]
    aad = torch.from_numpy(np.ascontiguousarray(aad_host)).to(dev) if aad_len else None
    kidx = np.arange(n, dtype=np.int64) % nkeys
    return keys, src, nonce_host, torch.from_numpy(nonce_host).to(dev), aad_host, aad, kidx


def run_shape(dev, n, size, aad_len, args):
    total = n * size
    keys, src, nonce_host, nonces, aad_host, aad, kidx = make_inputs(dev, n, size, aad_len, args.keys)
    ct, back, other = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
    lens = [size] * n

    enc = CB.ChaChaBatch.packed(src, lens, keys, out=ct, aad=aad, key_index=kidx, lanes=args.lanes)
    dec = CB.ChaChaBatch.packed(ct, lens, keys, out=back, aad=aad, key_index=kidx, lanes=args.lanes)
    gcm = ops.GcmBatch.packed(src, lens, keys[0][:16], out=other, aad=aad)
    nloop = min(args.loop_records, n)
    xs, outs = list(src[:nloop * size].split(size)), list(other[:nloop * size].split(size))
    nb = [nonce_host[i].tobytes() for i in range(nloop)]
    aadb = [aad_host[i].tobytes() for i in range(nloop)]

    def loop():
        for i in range(nloop):
            ops.chacha20_poly1305_encrypt(xs[i], keys[kidx[i]], nb[i], aadb[i], out=outs[i])

    enc.encrypt(nonces)
    tags = enc.tags.clone()
    arms = {
        "batch_encrypt": lambda: enc.encrypt(nonces),
        "batch_decrypt": lambda: dec.decrypt(nonces, tags),
        "chacha20_one_message": lambda: ops.chacha20(src, keys[0], nb[0], 1, out=other),
        "poly1305_one_message": lambda: ops.poly1305(src, keys[0]),
        "gcm_batch_aes128": lambda: gcm.encrypt(nonces),
    }
    ms = alternate(arms, args.warmup, args.iters)
    loop_ms = []
    for it in range(1 + args.loop_iters):
        t = once_ms(loop)
        if it >= 1:
            loop_ms.append(t)

    res = {"metric": "ChaCha20-Poly1305 many-record throughput", "records": n, "record_bytes": size,
           "aad_bytes": aad_len, "keys": len(keys), "total_bytes": total, "tiles": enc.ntiles, "hash_lanes": enc.lanes,
           "warmup": args.warmup, "iters": args.iters, "data": "synthetic random records, random nonces"}
    for k in arms:
        res[k] = rate(ms[k], total, n)
    res["per_record_loop"] = dict(rate(loop_ms, nloop * size, nloop), records=nloop, iters=args.loop_iters)
    lp = res["per_record_loop"]["gbps"]
    res["encrypt_vs_per_record_loop"] = round(res["batch_encrypt"]["gbps"] / lp, 1)
    res["decrypt_vs_per_record_loop"] = round(res["batch_decrypt"]["gbps"] / lp, 1)
    for arm in ("batch_encrypt", "batch_decrypt"):
        res[arm + "_share_of_unfused_ceiling"] = {
            "chacha20_one_message": round(res[arm]["gbps"] / res["chacha20_one_message"]["gbps"], 3),
            "poly1305_one_message": round(res[arm]["gbps"] / res["poly1305_one_message"]["gbps"], 3)}
    res["encrypt_vs_gcm_batch_aes128"] = round(res["batch_encrypt"]["gbps"] / res["gcm_batch_aes128"]["gbps"], 3)
    res["faster_than_loop"] = res["batch_encrypt"]["gbps"] > lp and res["batch_decrypt"]["gbps"] > lp

    # a seeded sample of records against the oracle: ciphertext, tag, and the way back
    enc.encrypt(nonces)
    _, okv = dec.decrypt(nonces, tags)
    torch.cuda.synchronize()
    good = bool(okv.all())
    tags_h = enc.tags.cpu().numpy()
    for i in random.Random(5).sample(range(n), min(8, n)):
        pt = src[i * size:(i + 1) * size].cpu().numpy().tobytes()
        want_ct, want_tag = cpu_ref.chacha20_poly1305(keys[kidx[i]], nonce_host[i].tobytes(), pt, aad_host[i].tobytes())
        good = good and ct[i * size:(i + 1) * size].cpu().numpy().tobytes() == want_ct
        good = good and tags_h[i].tobytes() == want_tag
        good = good and back[i * size:(i + 1) * size].cpu().numpy().tobytes() == pt
    res["verified_sample"] = good
    print(json.dumps(res), flush=True)
    return good and res["faster_than_loop"]


def lanes_row(dev, size, args):
    """Both forms of the hash kernel on one uniform batch of --table-bytes in all, alternated."""
    n = max(1, args.table_bytes // size)
    keys, src, nonce_host, nonces, aad_host, aad, kidx = make_inputs(dev, n, size, 13, args.keys)
    ct = torch.empty_like(src)
    lens = [size] * n
    b = {ln: CB.ChaChaBatch.packed(src, lens, keys, out=ct, aad=aad, key_index=kidx, lanes=ln) for ln in (16, 64)}
    otk = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    arms = {}
    for ln in (16, 64):
        arms[f"encrypt_{ln}"] = lambda ln=ln: b[ln].encrypt(nonces)
        arms[f"hash_{ln}"] = lambda ln=ln: b[ln].poly1305(otk)
    ms = alternate(arms, args.warmup, args.iters)
    t16, t64 = b[16].encrypt(nonces)[1].clone(), b[64].encrypt(nonces)[1].clone()
    res = {"metric": "batched Poly1305: 16 against 64 lanes per record", "records": n, "record_bytes": size,
           "aad_bytes": 13, "hashed_blocks": (size + 15) // 16 + 2, "total_bytes": n * size, "warmup": args.warmup,
           "iters": args.iters, "rule_picks": int(_native.require_gpu_lib().otc_chacha_batch_lanes(
               np.ascontiguousarray(np.array([[0, 0, size, 0, 13, 0]] * 2, dtype=np.uint64)).ctypes.data, 2)),
           "tags_equal": bool(torch.equal(t16, t64))}
    for k in arms:
        res[k] = rate(ms[k], n * size, n)
    res["encrypt_16_over_64"] = round(res["encrypt_16"]["gbps"] / res["encrypt_64"]["gbps"], 3)
    res["hash_16_over_64"] = round(res["hash_16"]["gbps"] / res["hash_64"]["gbps"], 3)
    print(json.dumps(res), flush=True)
    return res["tags_equal"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x4096,65536x1024,4096x16384", help="RECORDSxBYTES, comma separated")
    ap.add_argument("--aad", default="0,13", help="AAD bytes per record, comma separated")
    ap.add_argument("--keys", type=int, default=256, help="distinct keys, dealt to the records round robin")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-records", type=int, default=1024)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=None, help="lanes of the hash kernel per record (16/64; default: auto)")
    ap.add_argument("--lanes-table", action="store_true", help="time 16 against 64 lanes instead of the arms")
    ap.add_argument("--table-sizes", default="256,1024,4096,16384,65536")
    ap.add_argument("--table-bytes", type=int, default=64 << 20, help="bytes of every batch of the lanes table")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    good = True
    if args.lanes_table:
        for size in (int(v) for v in args.table_sizes.split(",")):
            good = lanes_row(dev, size, args) and good
    else:
        for shape in args.shapes.split(","):
            n, size = (int(v) for v in shape.split("x"))
            if size % 16:
                raise SystemExit("record sizes must be multiples of 16 (the records are views of one buffer)")
            for aad_len in (int(v) for v in args.aad.split(",")):
                good = run_shape(dev, n, size, aad_len, args) and good
    if not good:
        raise SystemExit("verification failed, or the batch was not faster than the per-record loop")


if __name__ == "__main__":
    main()
