#!/usr/bin/env python3
"""Serving-shaped AES-GCM with a key per record: many small records, each with
its own key (out of 1, 256 or n), 12-byte IV, AAD and 16-byte tag, on one
MI355X.  Per (shape, key size), in ONE process, the arms alternated run by run:

  mk_encrypt_1 / _256 / _n        ops.gcm_mk_batch_ops.GcmMkBatch (packed layout)
  mk_decrypt_256                  with 1, 256 and n keys: the feature.  The n-keys
                                  arm shows what the table copies cost once they
                                  miss L2 (1792 B of tables and 256 B of schedule
                                  per record)
  mk_ghash_16 / _64 (256 keys),   its hash kernel alone (otc_ghash_mk_batch), both
  mk_ghash_n                      lane forms; with n keys in the planned form
  mk_tables_256 / _n              its table kernel alone (otc_gcm_mk_batch_tables)
  gcm_batch_encrypt               ops.GcmBatch, one key: the ceiling
  ghash_batch                     GcmBatch's hash alone (positional tables)
  siv_batch_encrypt               ops.gcm_siv_batch_ops.GcmSivBatch, whose hash
                                  rebuilds its tables per record
  polyval_batch                   its hash alone, in its planned lane form
  ctr_batch                       ops.CtrBatch with the 256 keys: one pass, no
                                  authentication
  per_record_loop                 ops.gcm_encrypt per record over the first
                                  --loop-records records, key by key: the only
                                  way without the batch

--lanes-table instead times the hash alone and the whole encryption with 16 and
with 64 lanes per record at 1, 4, 8 and 16 KiB records (256 keys): what
otc_gcm_mk_batch_lanes' rule rests on.

Timed with device events: --warmup rounds, then --iters timed ones (the
per-record loop: 1 and --loop-iters).  Before anything is timed a seeded sample
of every arm's output is compared with the C oracle.  Prints one JSON line per
(shape, key size).

    python benchmarks/gcm_mk_batch.py
    python benchmarks/gcm_mk_batch.py --shapes 16384x4096 --keybits 128
    python benchmarks/gcm_mk_batch.py --lanes-table
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

MK = ops.gcm_mk_batch_ops
SB = ops.gcm_siv_batch_ops


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
    return (aad + bytes(-len(aad) % 16) + data + bytes(-len(data) % 16) + (8 * len(aad)).to_bytes(8, "big") +
            (8 * len(data)).to_bytes(8, "big"))


def make_keys(nkeys, keybits, seed):
    rows = np.random.default_rng(seed).integers(0, 256, (nkeys, keybits // 8), dtype=np.uint8)
    return [r.tobytes() for r in rows]


def inputs(dev, n, size, keybits, aad_len):
    total = n * size
    src = torch.empty(total, dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=n + size)
    rng = np.random.default_rng(size + aad_len + keybits)
    iv_host = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    aad_host = rng.integers(0, 256, (n, max(aad_len, 1)), dtype=np.uint8)[:, :aad_len]
    aad = torch.from_numpy(np.ascontiguousarray(aad_host)).to(dev) if aad_len else None
    return src, iv_host, torch.from_numpy(iv_host).to(dev), aad_host, aad


def stream_ptr(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def ghash_alone(lib, b, rows, lanes, dev):
    _native.check(lib.otc_ghash_mk_batch(b._plan.data_ptr() + b._o_desc, b.n, b._tab.data_ptr(), rows.data_ptr(), lanes,
                                         stream_ptr(dev)), "otc_ghash_mk_batch")


def run_shape(dev, n, size, keybits, args):
    total = n * size
    aad_len = args.aad
    src, iv_host, ivs, aad_host, aad = inputs(dev, n, size, keybits, aad_len)
    lens = [size] * n
    nk_mid = min(256, n)
    keys_n = make_keys(n, keybits, 1000 + keybits)
    keys_mid, key1 = keys_n[:nk_mid], keys_n[0]
    kidx_mid = (np.arange(n, dtype=np.int64) * 7 + 3) % nk_mid
    kidx_1 = np.zeros(n, dtype=np.int64)
    m1_ct, mm_ct, mm_back, mn_ct, g_ct, s_ct, r_ct, l_ct = (torch.empty_like(src) for _ in range(8))
    counters = np.zeros((n, 16), dtype=np.uint8)
    counters[:, :12] = iv_host
    counters[:, 15] = 2

    m1 = MK.GcmMkBatch.packed(src, lens, [key1], key_index=kidx_1, out=m1_ct, aad=aad)
    mm = MK.GcmMkBatch.packed(src, lens, keys_mid, key_index=kidx_mid, out=mm_ct, aad=aad)
    mm_dec = MK.GcmMkBatch.packed(mm_ct, lens, keys_mid, key_index=kidx_mid, out=mm_back, aad=aad)
    mn = MK.GcmMkBatch.packed(src, lens, keys_n, out=mn_ct, aad=aad)
    g_enc = ops.GcmBatch.packed(src, lens, key1, out=g_ct, aad=aad)
    siv = None
    if keybits != 192:
        siv = SB.GcmSivBatch.packed(src, lens, key1, out=s_ct, aad=aad)
    ctr = ops.CtrBatch.packed(src, lens, keys_mid, counters, out=r_ct, key_index=kidx_mid)
    nloop = min(args.loop_records, n)
    xs, outs = list(src[:nloop * size].split(size)), list(l_ct[:nloop * size].split(size))
    ivb = [iv_host[i].tobytes() for i in range(n)]
    aadb = [aad_host[i].tobytes() for i in range(n)]
    loop_tags = []

    def loop():
        loop_tags.clear()
        for i in range(nloop):
            loop_tags.append(ops.gcm_encrypt(xs[i], keys_mid[kidx_mid[i]], ivb[i], aadb[i], out=outs[i])[1])

    lib = _native.require_gpu_lib()
    rows = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    s_rows = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    nr = {128: 10, 192: 12, 256: 14}[keybits]

    def tables_alone(b):
        _native.check(lib.otc_gcm_mk_batch_tables(b._keys.data_ptr(), b.nkeys, nr, b._tab.data_ptr(), stream_ptr(dev)),
                      "otc_gcm_mk_batch_tables")

    def polyval_alone():  # over the H_m rows a run of the GCM-SIV batch left in its workspace
        _native.check(lib.otc_polyval_batch(siv._plan.data_ptr() + siv._o_desc, n, siv._ws.data_ptr(), s_rows.data_ptr(),
                                            siv.lanes, stream_ptr(dev)), "otc_polyval_batch")

    # every arm once, and a seeded sample of its output against the oracle, before anything is timed
    m1.encrypt(ivs)
    mm.encrypt(ivs)
    mm_tags = mm.tags.clone()
    _, mm_ok = mm_dec.decrypt(ivs, mm_tags)
    mn.encrypt(ivs)
    hrows = {}
    for lanes in (16, 64):
        ghash_alone(lib, mm, rows, lanes, dev)
        hrows[lanes] = rows.cpu().numpy().copy()
    ghash_alone(lib, mn, rows, mn.lanes, dev)
    hrows["n"] = rows.cpu().numpy().copy()
    tables_alone(mm)
    tables_alone(mn)
    g_enc.encrypt(ivs)
    g_enc.ghash()
    if siv:
        siv.encrypt(ivs)
        polyval_alone()
    ctr.run()
    loop()
    torch.cuda.synchronize()
    good = {"mk_1": bool(torch.equal(m1_ct, g_ct)) and bool(torch.equal(m1.tags, g_enc.tags)), "mk_256": bool(mm_ok.all()),
            "mk_n": True, "mk_ghash": True, "gcm_batch": True, "ctr_batch": True, "per_record_loop": True}
    mt, nt, gt = mm_tags.cpu().numpy(), mn.tags.cpu().numpy(), g_enc.tags.cpu().numpy()
    sample = random.Random(5).sample(range(n), min(6, n))
    for i in sample + [j for j in (0, nloop - 1) if j not in sample]:
        pt = piece(src, i, size)
        k = keys_mid[kidx_mid[i]]
        w_ct, w_tag = cpu_ref.gcm(k, ivb[i], pt, aadb[i])
        good["mk_256"] &= piece(mm_ct, i, size) == w_ct and mt[i].tobytes() == w_tag and piece(mm_back, i, size) == pt
        w_h = cpu_ref.ghash(cpu_ref.gcm_h(k), hashed(aadb[i], pt))
        good["mk_ghash"] &= hrows[16][i].tobytes() == w_h and hrows[64][i].tobytes() == w_h
        good["mk_ghash"] &= hrows["n"][i].tobytes() == cpu_ref.ghash(cpu_ref.gcm_h(keys_n[i]), hashed(aadb[i], pt))
        good["ctr_batch"] &= piece(r_ct, i, size) == w_ct
        if i < nloop:
            good["per_record_loop"] &= piece(l_ct, i, size) == w_ct and loop_tags[i].cpu().numpy().tobytes() == w_tag
        w_ct, w_tag = cpu_ref.gcm(keys_n[i], ivb[i], pt, aadb[i])
        good["mk_n"] &= piece(mn_ct, i, size) == w_ct and nt[i].tobytes() == w_tag
        w_ct, w_tag = cpu_ref.gcm(key1, ivb[i], pt, aadb[i])
        good["gcm_batch"] &= piece(g_ct, i, size) == w_ct and gt[i].tobytes() == w_tag
        if siv:
            w_ct, w_tag = cpu_ref.gcm_siv(key1, ivb[i], pt, aadb[i])
            good["siv_batch"] = good.get("siv_batch", True) and piece(s_ct, i, size) == w_ct

    arms = {
        "mk_encrypt_1": lambda: m1.encrypt(ivs),
        "mk_encrypt_256": lambda: mm.encrypt(ivs),
        "mk_decrypt_256": lambda: mm_dec.decrypt(ivs, mm_tags),
        "mk_encrypt_n": lambda: mn.encrypt(ivs),
        "mk_ghash_16": lambda: ghash_alone(lib, mm, rows, 16, dev),
        "mk_ghash_64": lambda: ghash_alone(lib, mm, rows, 64, dev),
        "mk_ghash_n": lambda: ghash_alone(lib, mn, rows, mn.lanes, dev),
        "mk_tables_256": lambda: tables_alone(mm),
        "mk_tables_n": lambda: tables_alone(mn),
        "gcm_batch_encrypt": lambda: g_enc.encrypt(ivs),
        "ghash_batch": lambda: g_enc.ghash(),
        "ctr_batch": lambda: ctr.run(),
    }
    if siv:
        arms["siv_batch_encrypt"] = lambda: siv.encrypt(ivs)
        arms["polyval_batch"] = polyval_alone
    ms = alternate(arms, args.warmup, args.iters)
    loop_ms = []
    for it in range(1 + args.loop_iters):
        t = once_ms(loop)
        if it >= 1:
            loop_ms.append(t)

    res = {"metric": "AES-GCM many-record throughput, a key per record", "keybits": keybits, "records": n,
           "record_bytes": size, "aad_bytes": aad_len, "total_bytes": total, "keys_mid": nk_mid, "mk_hash_lanes": mm.lanes,
           "gcm_hash_lanes": g_enc.lanes, "siv_hash_lanes": siv.lanes if siv else None, "tile_blocks": mm.tile_blocks,
           "warmup": args.warmup, "iters": args.iters, "data": "synthetic random records, random keys and IVs"}
    for k in arms:
        res[k] = rate(ms[k], total, n)
    for k, nk in (("mk_tables_256", nk_mid), ("mk_tables_n", n)):  # a table launch's unit is the key
        res[k] = {"ms_median": res[k]["ms_median"], "ms_best": res[k]["ms_best"], "keys": nk,
                  "keys_per_s": round(nk / res[k]["ms_median"] * 1e3)}
    res["per_record_loop"] = dict(rate(loop_ms, nloop * size, nloop), records=nloop, iters=args.loop_iters)
    g = lambda k: res[k]["gbps"]  # noqa: E731
    res["mk_over_gcm_batch_encrypt"] = {k: round(g(f"mk_encrypt_{k}") / g("gcm_batch_encrypt"), 3) for k in ("1", "256", "n")}
    res["mk_n_over_mk_256"] = {"encrypt": round(g("mk_encrypt_n") / g("mk_encrypt_256"), 3),
                               "ghash": round(g("mk_ghash_n") / g(f"mk_ghash_{mm.lanes}"), 3)}
    res["mk_over_ctr_batch"] = round(g("mk_encrypt_256") / g("ctr_batch"), 3)
    res["hash_alone"] = {"mk_over_ghash_batch": round(g(f"mk_ghash_{mm.lanes}") / g("ghash_batch"), 3)}
    if siv:
        res["mk_over_siv_batch_encrypt"] = round(g("mk_encrypt_256") / g("siv_batch_encrypt"), 3)
        res["hash_alone"]["mk_over_polyval_batch"] = round(g(f"mk_ghash_{mm.lanes}") / g("polyval_batch"), 3)
        res["hash_alone"]["polyval_over_ghash_batch"] = round(g("polyval_batch") / g("ghash_batch"), 3)
    res["per_record_loop_over_mk_batch"] = round(g("per_record_loop") / g("mk_encrypt_256"), 4)
    res["verified_sample"] = good
    print(json.dumps(res), flush=True)
    return all(good.values())


def lanes_table(dev, keybits, args):
    """The hash alone and the whole encryption, 16 against 64 lanes per record, 64 MiB of uniform records."""
    lib = _native.require_gpu_lib()
    ok = True
    for size in (1024, 4096, 8192, 16384):
        n = (64 << 20) // size
        src, iv_host, ivs, aad_host, aad = inputs(dev, n, size, keybits, args.aad)
        keys = make_keys(256, keybits, 2000 + keybits)
        kidx = (np.arange(n, dtype=np.int64) * 7 + 3) % 256
        out = torch.empty_like(src)
        b = {ln: MK.GcmMkBatch.packed(src, [size] * n, keys, key_index=kidx, out=out, aad=aad, lanes=ln) for ln in (16, 64)}
        rows = torch.empty((n, 16), dtype=torch.uint8, device=dev)
        desc = np.zeros((n, 6), dtype=np.uint64)  # what the rule reads: the lengths
        desc[:, 2], desc[:, 4] = size, args.aad
        tags = {}
        for ln in (16, 64):
            b[ln].encrypt(ivs)
            tags[ln] = b[ln].tags.cpu().numpy().copy()
        i = n // 3
        w_tag = cpu_ref.gcm(keys[kidx[i]], iv_host[i].tobytes(), piece(src, i, size), aad_host[i].tobytes())[1]
        good = tags[16][i].tobytes() == w_tag and (tags[16] == tags[64]).all()
        arms = {"ghash_16": lambda: ghash_alone(lib, b[16], rows, 16, dev), "ghash_64": lambda: ghash_alone(lib, b[64], rows, 64, dev),
                "encrypt_16": lambda: b[16].encrypt(ivs), "encrypt_64": lambda: b[64].encrypt(ivs)}
        ms = alternate(arms, args.warmup, args.iters)
        res = {"metric": "GcmMkBatch lanes per record", "keybits": keybits, "records": n, "record_bytes": size,
               "hashed_blocks": (args.aad + 15) // 16 + size // 16 + 1, "aad_bytes": args.aad,
               "rule_picks": lib.otc_gcm_mk_batch_lanes(desc.ctypes.data, n)}
        for k in arms:
            res[k] = rate(ms[k], n * size, n)
        res["ghash_16_over_64"] = round(res["ghash_16"]["gbps"] / res["ghash_64"]["gbps"], 3)
        res["encrypt_16_over_64"] = round(res["encrypt_16"]["gbps"] / res["encrypt_64"]["gbps"], 3)
        res["verified_sample"] = bool(good)
        print(json.dumps(res), flush=True)
        ok = ok and bool(good)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x4096,65536x1024,4096x16384", help="RECORDSxBYTES, comma separated")
    ap.add_argument("--keybits", default="128,256", help="AES key sizes, comma separated")
    ap.add_argument("--aad", type=int, default=13, help="AAD bytes per record")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-records", type=int, default=1024)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--lanes-table", action="store_true", help="16 against 64 lanes at 1, 4, 8 and 16 KiB records")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    good = True
    if args.lanes_table:
        for keybits in (int(v) for v in args.keybits.split(",")):
            good = lanes_table(dev, keybits, args) and good
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
