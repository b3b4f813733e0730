#!/usr/bin/env python3
"""How far ahead of their use the CTR bulk kernels issue their plaintext loads.

Disassembles a built aes_bs.o the way tools/isa_count.py does and, for every
CTR bulk kernel (k_aes_bs_t3, full tasks only: straight-line code), walks the
output phase -- everything after the last LDS-DMA load, which is issued once
rounds 1-2 are done -- with a model of the in-order vector-memory counter:
every global load / store is one outstanding operation, `s_waitcnt vmcnt(N)`
retires all but the youngest N.  For each such wait that retires a load it
prints

    the youngest load the wait covers, and the VALU instructions between that
    load's issue and the wait ("distance": the work that hides its latency),

and per kernel the minimum distance over those waits and, for the first
vmcnt(0) of the phase (hipcc's conservative wait in front of the first read of
LDS written by DMA), how many of the loads it covers were issued after the
byte stages of the output transposes (after the last v_perm_b32): loads that
wait a full round trip with next to nothing in between.

    tools/isa_load_distance.py [-v] build/obj/hip/aes_bs.o [other aes_bs.o ...]

One summary line per kernel:
    OBJ: CTR AES-128 waits 15 min_distance 222 min_after_first 222 late_under_first_vmcnt0 0
(min_after_first: the same minimum without the phase's first wait.)  -v adds
one line per wait.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_count  # noqa: E402

LLVM = isa_count.LLVM


def kernels(obj):
    """(mode, bits, [mnemonic + operands, ...]) of every CTR bulk kernel"""
    with tempfile.TemporaryDirectory() as tmp:
        co = isa_count.code_object(obj, tmp)
        asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    out = []
    for f in re.split(r"\n(?=[0-9a-f]+ <)", asm):
        m = re.match(r"[0-9a-f]+ <(.*?)>:", f)
        if not m or "k_aes_bs_t3" not in m.group(1):
            continue
        tm = re.search(r"t3ILi(\d+)ELi0ELi\d+ELb([01])ELb1EEE", m.group(1))  # MODE 0 = CTR, FO = true
        if not tm:
            continue
        ins = re.findall(r"^\s+([a-z_0-9]+[^/\n]*?)\s*(?://.*)?$", f, re.M)
        out.append(("CTR" if tm.group(2) == "1" else "CTR-nocache", isa_count.NAMES.get(f"Li{tm.group(1)}E", "?"), ins))
    return out


def analyse(ins):
    """-> (waits, late): waits = [(wait index, vmcnt N, youngest covered load's
    index, VALU between)], late = loads under the phase's first vmcnt(0) that
    were issued after the last v_perm_b32 (None: no vmcnt(0) in the phase)"""
    op = [i.split()[0] for i in ins]
    dma = [k for k, o in enumerate(op) if o.startswith("global_load_lds")]
    start = dma[-1] + 1 if dma else 0
    perms = [k for k, o in enumerate(op) if o == "v_perm_b32"]
    last_perm = perms[-1] if perms else -1
    valu_before = [0]
    for o in op:
        valu_before.append(valu_before[-1] + (1 if o.startswith("v_") else 0))
    pending = []  # (index, is_load) of outstanding vector-memory operations, oldest first
    waits, late = [], None
    for k, o in enumerate(op):
        if o.startswith(("global_", "buffer_", "flat_", "scratch_")):
            pending.append((k, "load" in o and k >= start))
        elif o == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", ins[k])
            if not m:
                continue
            n = int(m.group(1))
            done, pending = pending[:max(0, len(pending) - n)], pending[max(0, len(pending) - n):]
            loads = [i for i, is_load in done if is_load]
            if k < start or not loads:
                continue
            waits.append((k, n, loads[-1], valu_before[k] - valu_before[loads[-1]]))
            if n == 0 and late is None:
                late = sum(1 for i in loads if i > last_perm)
    return waits, late


def main():
    verbose = "-v" in sys.argv[1:]
    for obj in [a for a in sys.argv[1:] if a != "-v"]:
        for mode, bits, ins in kernels(obj):
            waits, late = analyse(ins)
            dist = min((w[3] for w in waits), default=-1)
            rest = min((w[3] for w in waits[1:]), default=-1)  # without the phase's first wait
            print(f"{obj}: {mode} {bits} waits {len(waits)} min_distance {dist} min_after_first {rest} "
                  f"late_under_first_vmcnt0 {0 if late is None else late}")
            if verbose:
                for k, n, ld, d in waits:
                    print(f"    instr {k}: vmcnt({n}) covers the load at instr {ld} ({k - ld} instructions, {d} VALU earlier)")


if __name__ == "__main__":
    main()
