#!/usr/bin/env python3
"""Serving-shaped AES-GCM-SIV: many small records under one key-generating
key, each with its own 12-byte nonce, AAD and 16-byte tag, on one MI355X.  Per
(shape, key size), in ONE process, the arms alternated run by run:

  siv_batch_encrypt / _decrypt    ops.gcm_siv_batch_ops.GcmSivBatch (packed
                                  layout): the feature
  polyval_batch_16 / _64          its hash kernel alone (otc_polyval_batch over
                                  the batch's own H_m rows), both lane forms
  ctr_le32_batch                  its counter kernel alone (otc_aes_ctr_le32_batch
                                  over the batch's own schedules and tags)
  gcm_batch_encrypt / _decrypt    ops.GcmBatch under the same key bytes: the
                                  yardstick, the same two passes over the data
  ghash_batch                     GcmBatch's hash alone: polyval_batch's peer
  ocb_batch_encrypt               ops.ocb_batch_ops.OcbBatch: one pass
  ctr_batch                       ops.CtrBatch: one pass, no authentication;
                                  ctr_le32_batch's peer
  per_record_loop                 ops.gcm_siv_ops.gcm_siv_encrypt per record over
                                  the first --loop-records records: the only way
                                  without the batch

Timed with device events: --warmup rounds, then --iters timed ones (the
per-record loop: 1 and --loop-iters).  Before anything is timed a seeded sample
of every arm's output is compared with the C oracle.  Prints one JSON line per
(shape, key size).

    python benchmarks/gcm_siv_batch.py
    python benchmarks/gcm_siv_batch.py --shapes 16384x4096 --keybits 128
"""
import argparse
import ctypes
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

SB = ops.gcm_siv_batch_ops
OB = ops.ocb_batch_ops


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


def piece(t, i, size):
    return t[i * size:(i + 1) * size].cpu().numpy().tobytes()


def hashed(aad: bytes, data: bytes) -> bytes:
    return (aad + bytes(-len(aad) % 16) + data + bytes(-len(data) % 16) + (8 * len(aad)).to_bytes(8, "little") +
            (8 * len(data)).to_bytes(8, "little"))


def run_shape(dev, n, size, keybits, args):
    total = n * size
    aad_len = args.aad
    key = bytes((11 * i + keybits + 1) & 0xFF for i in range(keybits // 8))
    src = torch.empty(total, dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=n + size)
    rng = np.random.default_rng(size + aad_len + keybits)
    nonce_host = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    nonces = torch.from_numpy(nonce_host).to(dev)
    aad_host = rng.integers(0, 256, (n, max(aad_len, 1)), dtype=np.uint8)[:, :aad_len]
    aad = torch.from_numpy(np.ascontiguousarray(aad_host)).to(dev) if aad_len else None
    s_ct, s_back, g_ct, g_back, o_ct, r_ct, l_ct, h_ct = (torch.empty_like(src) for _ in range(8))
    lens = [size] * n
    counters = np.zeros((n, 16), dtype=np.uint8)
    counters[:, :12] = nonce_host
    counters[:, 15] = 1

    s_enc = SB.GcmSivBatch.packed(src, lens, key, out=s_ct, aad=aad)
    s_dec = SB.GcmSivBatch.packed(s_ct, lens, key, out=s_back, aad=aad)
    s_half = SB.GcmSivBatch.packed(src, lens, key, out=h_ct, aad=aad)  # its plan and workspace serve the halves alone
    g_enc = ops.GcmBatch.packed(src, lens, key, out=g_ct, aad=aad)
    g_dec = ops.GcmBatch.packed(g_ct, lens, key, out=g_back, aad=aad)
    o_enc = OB.OcbBatch.packed(src, lens, key, out=o_ct, aad=aad)
    ctr = ops.CtrBatch.packed(src, lens, [key], counters, out=r_ct, key_index=np.zeros(n, dtype=np.int64))
    nloop = min(args.loop_records, n)
    xs, outs = list(src[:nloop * size].split(size)), list(l_ct[:nloop * size].split(size))
    nb = [nonce_host[i].tobytes() for i in range(n)]
    aadb = [aad_host[i].tobytes() for i in range(n)]
    loop_tags = []

    def loop():
        loop_tags.clear()
        for i in range(nloop):
            loop_tags.append(ops.gcm_siv_ops.gcm_siv_encrypt(xs[i], key, nb[i], aadb[i], out=outs[i])[1])

    # the halves alone, through the C calls, over what a run of s_half left in its workspace
    lib = _native.require_gpu_lib()
    base, ws = s_half._plan.data_ptr(), s_half._ws.data_ptr()
    s_rows = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    nr = 10 if keybits == 128 else 14

    def polyval_alone(lanes):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _native.check(lib.otc_polyval_batch(base + s_half._o_desc, n, ws, s_rows.data_ptr(), lanes, st), "otc_polyval_batch")

    def ctr_alone():
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _native.check(lib.otc_aes_ctr_le32_batch(base + s_half._o_desc, ws + 32 * n, s_half.tags.data_ptr(),
                                                 base + s_half._o_map, base + s_half._o_first, s_half.ntiles, n, nr, st),
                      "otc_aes_ctr_le32_batch")

    # every arm once, and a seeded sample of its output against the oracle, before anything is timed
    s_enc.encrypt(nonces)
    s_tags = s_enc.tags.clone()
    _, s_ok = s_dec.decrypt(nonces, s_tags)
    s_half.encrypt(nonces)
    h_ct.fill_(0)
    ctr_alone()
    half_rows = {}
    for lanes in (16, 64):
        polyval_alone(lanes)
        half_rows[lanes] = s_rows.cpu().numpy().copy()
    g_enc.encrypt(nonces)
    g_tags = g_enc.tags.clone()
    _, g_ok = g_dec.decrypt(nonces, g_tags)
    g_enc.ghash()
    o_enc.encrypt(nonces)
    ctr.run()
    loop()
    torch.cuda.synchronize()
    good = {"siv_batch": bool(s_ok.all()), "polyval_batch": True, "ctr_le32_batch": bool(torch.equal(h_ct, s_ct)),
            "gcm_batch": bool(g_ok.all()), "ocb_batch": True, "ctr_batch": True, "per_record_loop": True}
    st_, gt, ot = s_tags.cpu().numpy(), g_tags.cpu().numpy(), o_enc.tags.cpu().numpy()
    sample = random.Random(5).sample(range(n), min(6, n))
    for i in sample + [j for j in (0, nloop - 1) if j not in sample]:
        pt = piece(src, i, size)
        w_ct, w_tag = cpu_ref.gcm_siv(key, nb[i], pt, aadb[i])
        good["siv_batch"] &= piece(s_ct, i, size) == w_ct and st_[i].tobytes() == w_tag and piece(s_back, i, size) == pt
        w_s = cpu_ref.polyval(cpu_ref.gcm_siv_derive(key, nb[i])[0], hashed(aadb[i], pt))
        good["polyval_batch"] &= half_rows[16][i].tobytes() == w_s and half_rows[64][i].tobytes() == w_s
        w_ct, w_tag = cpu_ref.gcm(key, nb[i], pt, aadb[i])
        good["gcm_batch"] &= piece(g_ct, i, size) == w_ct and gt[i].tobytes() == w_tag and piece(g_back, i, size) == pt
        w_ct, w_tag = cpu_ref.ocb(key, nb[i], pt, aadb[i])
        good["ocb_batch"] &= piece(o_ct, i, size) == w_ct and ot[i].tobytes() == w_tag
        good["ctr_batch"] &= piece(r_ct, i, size) == cpu_ref.ctr(key, counters[i].tobytes(), pt)
        if i < nloop:
            w_ct, w_tag = cpu_ref.gcm_siv(key, nb[i], pt, aadb[i])
            good["per_record_loop"] &= piece(l_ct, i, size) == w_ct and loop_tags[i].cpu().numpy().tobytes() == w_tag

    arms = {
        "siv_batch_encrypt": lambda: s_enc.encrypt(nonces),
        "siv_batch_decrypt": lambda: s_dec.decrypt(nonces, s_tags),
        "polyval_batch_16": lambda: polyval_alone(16),
        "polyval_batch_64": lambda: polyval_alone(64),
        "ctr_le32_batch": ctr_alone,
        "gcm_batch_encrypt": lambda: g_enc.encrypt(nonces),
        "gcm_batch_decrypt": lambda: g_dec.decrypt(nonces, g_tags),
        "ghash_batch": lambda: g_enc.ghash(),
        "ocb_batch_encrypt": lambda: o_enc.encrypt(nonces),
        "ctr_batch": lambda: ctr.run(),
    }
    ms = alternate(arms, args.warmup, args.iters)
    loop_ms = []
    for it in range(1 + args.loop_iters):
        t = once_ms(loop)
        if it >= 1:
            loop_ms.append(t)

    res = {"metric": "AES-GCM-SIV many-record throughput", "keybits": keybits, "records": n, "record_bytes": size,
           "aad_bytes": aad_len, "total_bytes": total, "siv_tiles": s_enc.ntiles, "siv_hash_lanes": s_enc.lanes,
           "gcm_hash_lanes": g_enc.lanes, "warmup": args.warmup, "iters": args.iters,
           "data": "synthetic random records, random nonces"}
    for k in arms:
        res[k] = rate(ms[k], total, n)
    res["per_record_loop"] = dict(rate(loop_ms, nloop * size, nloop), records=nloop, iters=args.loop_iters)
    g = lambda k: res[k]["gbps"]  # noqa: E731
    res["siv_over_gcm_batch"] = {"encrypt": round(g("siv_batch_encrypt") / g("gcm_batch_encrypt"), 3),
                                 "decrypt": round(g("siv_batch_decrypt") / g("gcm_batch_decrypt"), 3)}
    res["halves_over_their_peers"] = {"polyval_16_over_ghash": round(g("polyval_batch_16") / g("ghash_batch"), 3),
                                      "polyval_64_over_ghash": round(g("polyval_batch_64") / g("ghash_batch"), 3),
                                      "ctr_le32_over_ctr_batch": round(g("ctr_le32_batch") / g("ctr_batch"), 3)}
    res["siv_over_ocb_batch_encrypt"] = round(g("siv_batch_encrypt") / g("ocb_batch_encrypt"), 3)
    res["per_record_loop_over_siv_batch"] = round(g("per_record_loop") / g("siv_batch_encrypt"), 4)
    res["verified_sample"] = good
    print(json.dumps(res), flush=True)
    return all(good.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x4096,65536x1024,4096x16384", help="RECORDSxBYTES, comma separated")
    ap.add_argument("--keybits", default="128,256", help="AES key sizes, comma separated")
    ap.add_argument("--aad", type=int, default=13, help="AAD bytes per record")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-records", type=int, default=1024)
    ap.add_argument("--loop-iters", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    good = True
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
