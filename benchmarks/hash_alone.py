#!/usr/bin/env python3
"""The two device hashes by themselves, ops.ghash and ops.poly1305, over 1 GiB
and 4 GiB of random device data in one process: median / minimum / maximum
GB/s of 10 calls timed with stream events after 3 warm-up calls.  One JSON
line per (hash, size); profiles/chacha/hash_alone.jsonl was made with it.

    python benchmarks/hash_alone.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from our_tree_amd import ops  # noqa: E402

H = bytes.fromhex("66e94bd4ef8a2c3b884cfa59ca342b2e")
PKEY = bytes(range(32))


def main():
    for n in (1 << 30, 4 << 30):
        x = torch.empty(n, dtype=torch.uint8, device="cuda")
        ops.fill_random_(x, seed=5)
        for name, fn in (("ghash", lambda: ops.ghash(x, H)), ("poly1305", lambda: ops.poly1305(x, PKEY))):
            for _ in range(3):
                fn()
            ms = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            gb = [n / (m * 1e6) for m in ms]
            print(json.dumps({"op": name, "bytes": n, "gbps_median": round(statistics.median(gb), 1),
                              "gbps_min": round(min(gb), 1), "gbps_max": round(max(gb), 1)}), flush=True)
        del x


if __name__ == "__main__":
    main()
