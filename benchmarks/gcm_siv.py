#!/usr/bin/env python3
"""AES-GCM-SIV against AES-GCM and its own two halves over ONE large message on
one MI355X.  Per (key size, size), in ONE process, the arms alternated run by
run:

  siv_enc    ops.gcm_siv_ops.gcm_siv_encrypt: POLYVAL, finisher, counter mode from the tag -- the feature
  siv_dec    ops.gcm_siv_ops.gcm_siv_decrypt (with its 16-byte tag readback)
  gcm_tt     ops.gcm_encrypt(impl="ttable"): the same two passes, counter by value from the host
  gcm_auto   ops.gcm_encrypt(impl="auto"): what a caller of GCM gets
  polyval    ops.gcm_siv_ops.polyval alone        ghash     ops.ghash alone
  ctr_le32   ops.gcm_siv_ops.ctr_le32 alone       ctr32_tt  ops.ctr32(impl="ttable") alone

Timed with device events: --warmup rounds, then --iters timed ones; the rate is
that of the median.  Verified per row, outside the timed region: the way back
gives the plaintext and the decryption computes the encryption's tag; seeded
windows of the ciphertext equal the C oracle's counter mode from that tag; the
two hashes alone and the two counter modes alone equal the oracle's on windows
or, up to --verify-whole bytes, everything does (ciphertext, tag, hashes).  Past
that size the hashes are checked against themselves cut in two and chained.
Prints one JSON line per row and appends it to --out (default
profiles/gcm_siv/gcm_siv.jsonl).

    python benchmarks/gcm_siv.py
    python benchmarks/gcm_siv.py --sizes 64M --bits 128 --out profiles/gcm_siv/run1.jsonl
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

SIV = ops.gcm_siv_ops
NONCE = bytes(range(0x40, 0x4C))
AAD = bytes(range(13))
H = bytes.fromhex("25629347589242761d31f826ba4b757b")
CTR_BE = bytes(range(0x10, 0x1C)) + (2).to_bytes(4, "big")
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


def windows(n):
    """Block numbers of the verified windows: the first, the last, six seeded ones."""
    blocks = n // 16
    last = max(blocks - WINDOW // 16, 0)
    return [(b0, min(WINDOW // 16, blocks - b0)) for b0 in [0, last] + [random.Random(n + i).randrange(0, max(last, 1))
                                                                      for i in range(6)]]


def le32_at(ctr: bytes, block: int) -> bytes:
    return ((int.from_bytes(ctr[:4], "little") + block) % (1 << 32)).to_bytes(4, "little") + ctr[4:15] + bytes([ctr[15] | 0x80])


def be32_at(ctr: bytes, block: int) -> bytes:
    return ctr[:12] + ((int.from_bytes(ctr[12:], "big") + block) % (1 << 32)).to_bytes(4, "big")


def verify(key, src, out, tmp, whole):
    """Everything the timed arms computed, again, against the oracle."""
    n = src.numel()
    ct, tag = SIV.gcm_siv_encrypt(src, key, NONCE, AAD, out=tmp)
    tag_h = host(tag)
    back, tag_dec = SIV._gcm_siv(ct, key, NONCE, AAD, out, tag)  # the decryption's launches: its computed tag
    good = torch.equal(back, src) and host(tag_dec) == tag_h
    good = good and torch.equal(SIV.gcm_siv_decrypt(ct, key, NONCE, tag_h, AAD, out=out), src)
    ek = cpu_ref.gcm_siv_derive(key, NONCE)[1]
    for b0, nb in windows(n):
        sl = slice(16 * b0, 16 * (b0 + nb))
        good = good and host(ct[sl]) == cpu_ref.ctr_le32(ek, le32_at(tag_h, b0), host(src[sl]))
    # the halves alone
    c_dev = torch.frombuffer(bytearray(tag_h), dtype=torch.uint8).to(src.device)
    SIV.ctr_le32(src, key, c_dev, out=out)
    for b0, nb in windows(n):
        sl = slice(16 * b0, 16 * (b0 + nb))
        good = good and host(out[sl]) == cpu_ref.ctr_le32(key, le32_at(tag_h, b0), host(src[sl]))
    ops.ctr32(src, key, CTR_BE, out=out, impl="ttable")
    for b0, nb in windows(n):
        sl = slice(16 * b0, 16 * (b0 + nb))
        good = good and host(out[sl]) == cpu_ref.ctr32(key, be32_at(CTR_BE, b0), host(src[sl]))
    pv, gh = host(SIV.polyval(src, H)), host(ops.ghash(src, H))
    if n <= whole:
        s = host(src)
        good = good and (host(ct), tag_h) == cpu_ref.gcm_siv(key, NONCE, s, AAD)
        good = good and pv == cpu_ref.polyval(H, s) and gh == cpu_ref.ghash(H, s)
    else:
        cut = (n // 3) // 16 * 16 + 16 * 5
        good = good and pv == host(SIV.polyval(src[cut:], H, host(SIV.polyval(src[:cut], H))))
        good = good and gh == host(ops.ghash(src[cut:], H, host(ops.ghash(src[:cut], H))))
    return bool(good)


def run_row(bits, n, args, src, dst, tmp):
    key = bytes((7 * i + bits) & 0xFF for i in range(bits // 8))
    iv = bytes(range(0x50, 0x5C))
    x, out, other = src[:n], dst[:n], tmp[:n]

    # the input of the decryption arm is a real ciphertext with its tag, on the device
    c_siv, t_siv = SIV.gcm_siv_encrypt(x, key, NONCE, AAD, out=other)
    t_siv = t_siv.clone()
    arms = {
        "siv_enc": lambda: SIV.gcm_siv_encrypt(x, key, NONCE, AAD, out=out),
        "siv_dec": lambda: SIV.gcm_siv_decrypt(c_siv, key, NONCE, t_siv, AAD, out=out),
        "gcm_tt": lambda: ops.gcm_encrypt(x, key, iv, AAD, out=out, impl="ttable"),
        "gcm_auto": lambda: ops.gcm_encrypt(x, key, iv, AAD, out=out, impl="auto"),
        "polyval": lambda: SIV.polyval(x, H),
        "ghash": lambda: ops.ghash(x, H),
        "ctr_le32": lambda: SIV.ctr_le32(x, key, t_siv, out=out),
        "ctr32_tt": lambda: ops.ctr32(x, key, CTR_BE, out=out, impl="ttable"),
    }
    ms = alternate(arms, args.warmup, args.iters)

    res = {"metric": "AES-GCM-SIV one-message throughput", "key_bits": bits, "bytes": n, "aad_bytes": len(AAD),
           "warmup": args.warmup, "iters": args.iters, "data": "synthetic random bytes", "runtime": _native.runtime_info()}
    for k in arms:
        res[k] = rate(ms[k], n)
    ratio = lambda a, b: round(res[a]["gbps"] / res[b]["gbps"], 3)
    res["siv_enc_over_gcm_tt"] = ratio("siv_enc", "gcm_tt")
    res["siv_dec_over_gcm_tt"] = ratio("siv_dec", "gcm_tt")
    res["siv_enc_over_gcm_auto"] = ratio("siv_enc", "gcm_auto")
    res["polyval_over_ghash"] = ratio("polyval", "ghash")
    res["ctr_le32_over_ctr32_tt"] = ratio("ctr_le32", "ctr32_tt")
    # the two passes by themselves, one behind the other: what the AEAD adds is the finisher and the tag's way between them
    halves = res["polyval"]["ms_median"] + res["ctr_le32"]["ms_median"]
    res["siv_enc_ms_over_halves_ms"] = round(res["siv_enc"]["ms_median"] / halves, 3)
    del c_siv
    res["verified_sample"] = verify(key, x, out, other, args.verify_whole)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcm_siv", "gcm_siv.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sizes = [size_of(s) for s in args.sizes.split(",")]
    src = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
    ops.fill_random_(src, seed=8452)
    dst, tmp = torch.empty_like(src), torch.empty_like(src)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    good = True
    with open(args.out, "a") as f:
        for n in sizes:
            for bits in (int(b) for b in args.bits.split(",")):
                res = run_row(bits, n, args, src, dst, tmp)
                line = json.dumps(res)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
                good = good and res["verified_sample"]
    if not good:
        raise SystemExit("verification failed")


if __name__ == "__main__":
    main()
