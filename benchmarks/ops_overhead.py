#!/usr/bin/env python3
"""Host time of the Python op layer (``our_tree_amd/ops``) on one GPU: what a
call costs to enqueue and what a batch costs to plan.  No kernel is measured.

  enqueue   --calls back-to-back calls between one perf_counter pair, one
            synchronisation after the loop; microseconds per call, the median
            of --reps such loops after a warm-up loop
  plan      a batch constructor, milliseconds, the median of --plan-runs

The tree under test is the one this file lies in, so two checkouts compare by
running each its own copy, alternating.  One JSON line per measurement.

    python benchmarks/ops_overhead.py --tree new --round 0 >> ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from our_tree_amd import _native, ops  # noqa: E402

MIB, KIB4, NREC = 1 << 20, 4096, 256
K16, K32, XTS_KEY = bytes(range(16)), bytes(range(32)), bytes(range(64))
CTR0, NONCE12 = bytes(range(16, 32)), bytes(range(12))


def enqueue_us(fn, calls, reps):
    def loop():
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        return dt / calls * 1e6
    loop()  # warm-up: key schedules, allocator, kernel load
    return statistics.median(loop() for _ in range(reps))


def plan_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default="this", help="label of this checkout in the records")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plan-runs", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)

    def buf(n):
        return ops.fill_random_(torch.empty(n, dtype=torch.uint8, device=dev), seed=n)

    big, big_out, small, small_b = buf(MIB), torch.empty(MIB, dtype=torch.uint8, device=dev), buf(KIB4), buf(KIB4)
    recs, ivs = buf(NREC * KIB4), buf(NREC * 12).view(NREC, 12)
    ctr_batch = ops.CtrBatch.packed(recs, [KIB4] * NREC, [K16], [CTR0] * NREC, key_index=[0] * NREC)
    gcm_batch = ops.GcmBatch.packed(recs, [KIB4] * NREC, K16)
    enqueue = {
        "ctr 1MiB out=": lambda: ops.ctr(big, K16, CTR0, out=big_out),
        "ecb_encrypt 1MiB": lambda: ops.ecb_encrypt(big, K16),
        "cbc_decrypt_segments 1MiB/4KiB": lambda: ops.cbc_decrypt_segments(big, K16, CTR0, KIB4),
        "xts_encrypt 1MiB/4KiB": lambda: ops.xts_encrypt(big, XTS_KEY, 7, KIB4),
        "gcm_encrypt 4KiB": lambda: ops.gcm_encrypt(small, K16, NONCE12),
        "chacha20 4KiB": lambda: ops.chacha20(small, K32, NONCE12),
        "xor 4KiB": lambda: ops.xor(small, small_b),
        "CtrBatch.run 256x4KiB": ctr_batch.run,
        "GcmBatch.encrypt 256x4KiB": lambda: gcm_batch.encrypt(ivs),
    }
    n_packed, n_list = 16384, 4096
    packed, lens = buf(n_packed * KIB4), [KIB4] * n_packed
    counters = torch.zeros((n_packed, 16), dtype=torch.uint8).numpy()
    kidx = [0] * n_packed
    xs = list(packed[: n_list * KIB4].view(n_list, KIB4).unbind(0))
    plan = {
        "CtrBatch.packed 16384x4KiB": lambda: ops.CtrBatch.packed(packed, lens, [K16], counters, key_index=kidx),
        "GcmBatch.packed 16384x4KiB": lambda: ops.GcmBatch.packed(packed, lens, K16),
        "CtrBatch(list) 4096": lambda: ops.CtrBatch(xs, [K16], [CTR0] * n_list, key_index=kidx[:n_list]),
        "GcmBatch(list) 4096": lambda: ops.GcmBatch(xs, K16),
    }
    common = {"tree": args.tree, "round": args.round, "torch": torch.__version__, "runtime": _native.runtime_info()}
    for name, fn in enqueue.items():
        print(json.dumps({"line": name, "unit": "us/call", "value": round(enqueue_us(fn, args.calls, args.reps), 3),
                          "calls": args.calls, "reps": args.reps, **common}), flush=True)
    for name, fn in plan.items():
        print(json.dumps({"line": name, "unit": "ms", "value": round(plan_ms(fn, args.plan_runs), 4),
                          "runs": args.plan_runs, **common}), flush=True)


if __name__ == "__main__":
    main()
