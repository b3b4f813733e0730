#!/usr/bin/env python3
"""AES-OCB3 against the engine's other AES paths over ONE large message on one
MI355X.  Per (key size, direction, size), in ONE process, the arms alternated
run by run:

  ocb   ops.ocb_ops.ocb_encrypt / ocb_decrypt: the one-pass AEAD -- the feature
  xts   ops.xts_encrypt / xts_decrypt with 4 KiB units: the same shape of work
        (offset in, T-table rounds, offset out) without a checksum or a tag
  ecb   ops.ecb_encrypt / ecb_decrypt, impl="ttable": the bare block cipher on
        the grid T-table kernel
  gcm   ops.gcm_encrypt / gcm_decrypt: the two-pass AEAD (CTR32, then GHASH)

ocb_decrypt and gcm_decrypt include their 16-byte tag readback.  Timed with
device events: --warmup rounds, then --iters timed ones; the rate is that of
the median.  Verified per row: the tag of the decryption equals that of the
encryption and the way back gives the plaintext; seeded windows of the
ciphertext equal the C oracle's (through the block primitive, which starts
anywhere in a message); up to --verify-whole bytes the whole ciphertext and
the tag equal the oracle's.  Prints one JSON line per row and appends it to
--out (default profiles/ocb/ocb.jsonl).

    python benchmarks/ocb.py
    python benchmarks/ocb.py --sizes 64M --bits 128 --out profiles/ocb/run1.jsonl
"""
import argparse
import json
import os
import random
import statistics

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # before torch / HIP: dmabuf IPC only on this host driver (as bench.py)
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from our_tree_amd import _native, ops  # noqa: E402
from our_tree_amd.models import cpu_ref  # noqa: E402

OCB = ops.ocb_ops
NONCE = bytes(range(0x40, 0x4C))
AAD = bytes(range(13))
WINDOW = 256 * 16 + 48  # bytes of one verified window: a pass of a wave and a little more


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rate(ms_list, nbytes):
    med = statistics.median(ms_list)
    return {"ms_median": round(med, 4), "ms_best": round(min(ms_list), 4), "ms_worst": round(max(ms_list), 4),
            "gbps": round(nbytes / med / 1e6, 1)}


def alternate(arms, warmup, iters):
    """Every arm once per round, --warmup rounds dropped: {arm: [ms]}."""
    ms = {k: [] for k in arms}
    for it in range(warmup + iters):
        for k, fn in arms.items():
            t = once_ms(fn)
            if it >= warmup:
                ms[k].append(t)
    return ms


def host(t):
    return t.cpu().numpy().tobytes()


def verify(key, src, ct, tag, back, tag_dec, whole):
    """The round trip, sampled windows against the oracle, and below `whole` bytes everything."""
    n = src.numel()
    good = torch.equal(back, src) and host(tag_dec) == host(tag)
    off0 = cpu_ref.ocb_offset0(key, NONCE)
    blocks = n // 16
    starts = [0, max(blocks - WINDOW // 16, 0)] + [random.Random(n + i).randrange(0, max(blocks - WINDOW // 16, 1))
                                                  for i in range(6)]
    for b0 in starts:
        nb = min(WINDOW // 16, blocks - b0)
        want, _ = cpu_ref.ocb_blocks(key, off0, host(src[16 * b0:16 * (b0 + nb)]), b0)
        good = good and host(ct[16 * b0:16 * (b0 + nb)]) == want
    if n <= whole:
        good = good and (host(ct), host(tag)) == cpu_ref.ocb(key, NONCE, host(src), AAD)
    return bool(good)


def run_row(dev, bits, decrypt, n, args, src, dst, tmp):
    key = bytes((7 * i + bits) & 0xFF for i in range(bits // 8))
    xts_key = key + bytes((13 * i + 5) & 0xFF for i in range(bits // 8))
    iv = bytes(range(0x50, 0x5C))
    x, out, other = src[:n], dst[:n], tmp[:n]
    nblk = n - n % 16

    # the inputs of the decryption arms are real ciphertexts with their tags
    c_ocb, t_ocb = OCB.ocb_encrypt(x, key, NONCE, AAD, out=other)
    c_ocb, t_ocb = c_ocb.clone(), t_ocb.clone()
    if decrypt:
        c_gcm, t_gcm = ops.gcm_encrypt(x, key, iv, AAD)
        t_gcm = host(t_gcm)
        t_ocb_h = host(t_ocb)
        arms = {
            "ocb": lambda: OCB.ocb_decrypt(c_ocb, key, NONCE, t_ocb_h, AAD, out=out),
            "xts": lambda: ops.xts_decrypt(x[:nblk], xts_key, 0, 4096, out=out[:nblk]),
            "ecb": lambda: ops.ecb_decrypt(x[:nblk], key, out=out[:nblk], impl="ttable"),
            "gcm": lambda: ops.gcm_decrypt(c_gcm, key, iv, t_gcm, AAD, out=out),
        }
    else:
        arms = {
            "ocb": lambda: OCB.ocb_encrypt(x, key, NONCE, AAD, out=out),
            "xts": lambda: ops.xts_encrypt(x[:nblk], xts_key, 0, 4096, out=out[:nblk]),
            "ecb": lambda: ops.ecb_encrypt(x[:nblk], key, out=out[:nblk], impl="ttable"),
            "gcm": lambda: ops.gcm_encrypt(x, key, iv, AAD, out=out),
        }
    ms = alternate(arms, args.warmup, args.iters)

    res = {"metric": "AES-OCB3 one-message throughput", "key_bits": bits, "direction": "decrypt" if decrypt else "encrypt",
           "bytes": n, "aad_bytes": len(AAD), "xts_unit_bytes": 4096, "warmup": args.warmup, "iters": args.iters,
           "data": "synthetic random bytes", "runtime": _native.runtime_info()}
    for k in arms:
        res[k] = rate(ms[k], n)
    res["ocb_over_xts"] = round(res["ocb"]["gbps"] / res["xts"]["gbps"], 3)
    res["ocb_over_ecb"] = round(res["ocb"]["gbps"] / res["ecb"]["gbps"], 3)
    res["ocb_over_gcm"] = round(res["ocb"]["gbps"] / res["gcm"]["gbps"], 3)

    # the tag of the decryption is the computed one: through the C call's 16 bytes
    back = OCB.ocb_decrypt(c_ocb, key, NONCE, t_ocb, AAD, out=out)
    _, tag_dec = OCB._ocb(c_ocb, key, NONCE, AAD, other, 16, True)
    res["verified_sample"] = verify(key, x, c_ocb, t_ocb, back, tag_dec, args.verify_whole)
    del c_ocb
    return res


def size_of(s):
    mult = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}
    return int(s[:-1]) * mult[s[-1].upper()] if s[-1].upper() in mult else int(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64M,1G,4G", help="message bytes, comma separated (K / M / G suffixes)")
    ap.add_argument("--bits", default="128,256", help="AES key sizes, comma separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--verify-whole", type=size_of, default=64 << 20, help="up to this size the whole result is compared with the oracle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocb", "ocb.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sizes = [size_of(s) for s in args.sizes.split(",")]
    src = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=7253)
    dst, tmp = torch.empty_like(src), torch.empty_like(src)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    good = True
    with open(args.out, "a") as f:
        for n in sizes:
            for bits in (int(b) for b in args.bits.split(",")):
                for decrypt in (False, True):
                    res = run_row(dev, bits, decrypt, n, args, src, dst, tmp)
                    line = json.dumps(res)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                    good = good and res["verified_sample"]
    if not good:
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
