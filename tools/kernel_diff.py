#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code in two hipcc objects.

For a refactor that must not change the device code: extracts both code
objects (as tools/isa_count.py does), disassembles them without addresses and
raw bytes, masks what only depends on where a kernel lands -- branch-target
labels and the pc-relative literal of the s_add_u32 after an s_getpc_b64 --
and compares, per kernel symbol, the instruction text and the resources:
.vgpr_count, .sgpr_count and the private segment size from the notes, the
allocated VGPRs and static LDS bytes from the kernel descriptor.  Kernel order
in the object does not count.

    tools/kernel_diff.py OLD.o NEW.o [NAME-PART]

prints one line per kernel,

    same|differs  OLD_INSNS NEW_INSNS  (vgpr, sgpr, scratch, alloc, lds) x 2  NAME

then a summary, and exits non-zero when the two kernel sets differ (1) -- not
when a kernel's code does: which differences are acceptable is the caller's
judgement.  With NAME-PART, also a unified diff of the masked instructions of
every differing kernel whose symbol contains it.
"""
import difflib
import re
import subprocess
import sys
import tempfile

import isa_count
from isa_count import LLVM


def resources(co):
    """kernel symbol -> (vgpr_count, sgpr_count, private segment, allocated VGPRs, static LDS)"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    sgpr = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        sg = re.search(r"\.sgpr_count:\s+(\d+)", blk)
        if name:
            sgpr[name.group(1)] = int(sg.group(1)) if sg else -1
    meta = isa_count.metadata(co)
    desc = isa_count.descriptor_vgprs(co, with_lds=True)
    out = {}
    for k, (alloc, lds) in desc.items():
        vg, scratch = meta.get(k + ".kd", meta.get(k, (-1, -1)))
        out[k] = (vg, sgpr.get(k + ".kd", sgpr.get(k, -1)), scratch, alloc, lds)
    return out


def kernels(obj):
    """kernel symbol -> (masked instruction lines, resources)"""
    with tempfile.TemporaryDirectory() as tmp:
        co = isa_count.code_object(obj, tmp)
        asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                             check=True, capture_output=True, text=True).stdout
        res = resources(co)
    out = {}
    for f in re.split(r"\n(?=<[^>]+>:)", asm):
        m = re.match(r"<([^>]+)>:", f)
        if not m or m.group(1) not in res:
            continue  # a branch-target label inside a kernel splits nothing: only kernel symbols open a block
        ins, getpc = [], False
        for line in f.splitlines()[1:]:
            line = re.sub(r"\s*//.*$", "", line).strip()
            if not line or line == "..." or re.match(r"<[^>]+>:$", line):
                continue  # "...": zero padding up to the next kernel, which depends on the order
            line = re.sub(r"<[^>]+>", "<L>", line)
            if re.match(r"s_(c?branch\w*|call\w*)\s", line):
                line = re.sub(r"(-?\d+|0x[0-9a-f]+)\s*(<L>)?$", "<L>", line)
            if getpc and line.startswith("s_add_u32"):
                line = re.sub(r"(,\s*)\S+$", r"\1<PCREL>", line)
            getpc = line.startswith("s_getpc_b64")
            ins.append(line)
        out[m.group(1)] = (ins, res[m.group(1)])
    return out


def main():
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    show = sys.argv[3] if len(sys.argv) == 4 else None
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = 0
    for k in sorted(set(old) & set(new)):
        (oi, orr), (ni, nr) = old[k], new[k]
        ok = oi == ni and orr == nr
        same += ok
        print(f"{'same' if ok else 'differs'} {len(oi)} {len(ni)} {orr} {nr} {k}")
        if show and show in k and not ok:
            print("\n".join(difflib.unified_diff(oi, ni, "old", "new", n=2, lineterm="")))
    for k in sorted(set(old) - set(new)):
        print(f"only-old {len(old[k][0])} - {old[k][1]} - {k}")
    for k in sorted(set(new) - set(old)):
        print(f"only-new - {len(new[k][0])} - {new[k][1]} {k}")
    both = len(set(old) & set(new))
    print(f"{both} kernels in both, {same} same, {both - same} differ, "
          f"{len(set(old) - set(new))} only in OLD, {len(set(new) - set(old))} only in NEW")
    return 1 if set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
