"""The bitsliced CTR kernel's output phase (csrc/hip/aes_bs.hip: depth-first
output transpose, stores per quad of slots, plaintext loads into the registers
a quad frees): every byte of ``ops.ctr(..., impl="bitslice")`` against the C
oracle, at the shapes where a slot, a quad or a task can go wrong.

Each case runs random plaintext out of place and in place (the loads of later
slots are issued behind the stores of earlier ones, to the same buffer), and
all-zero plaintext, where the output is the keystream itself and a permuted
slot shows as a wrong block whatever the data.  All shapes are <= 1.1 MiB."""
import hashlib

import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

TASK = 2048 * 16  # bytes of one wave's task: 32 slots x 64 lanes x 16 B


def det(tag, n):
    """n deterministic bytes"""
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha256(f"{tag}/{i}".encode()).digest()
        i += 1
    return out[:n]


def ctr_block(hi, lo):
    return hi.to_bytes(8, "big") + (lo & ((1 << 64) - 1)).to_bytes(8, "big")


HI = 0x0123456789ABCDEF
# name: (counter high half, counter low half, bytes)
CASES = {
    # bulk launch only, every slot of one wave
    "one_full_task": (HI, 0x5A5A5A5A5A5A5000, TASK),
    # more than one workgroup of 4 waves, the second with one live wave
    "five_tasks": (HI, 0x1122334455660800, 5 * TASK),
    # partial first task, partial last task, trailing partial block
    "unaligned_1": (HI, 0x00000000DEAD0001, 3 * TASK + 37 * 16 + 5),
    "unaligned_2047": (HI, 0x00000000DEAD07FF, 3 * TASK + 37 * 16 + 5),
    # the low 64 bits carry into the high half inside the buffer
    "carry": (HI, (1 << 64) - 2048 * 2 - 77, 5 * TASK),
    "carry_aligned": (HI, (1 << 64) - 2048 * 2, 5 * TASK),
    # a 65536-block group boundary of the counter-cache tables inside the buffer
    "group_boundary": (HI, 0x0000000700008005, (1 << 20) + (64 << 10)),
    "group_boundary_aligned": (HI, 0x0000000700008000, (1 << 20) + (64 << 10)),
}


def test_case_geometry():
    """the cases are what their names say (no GPU work)"""
    for name, (hi, lo, n) in CASES.items():
        assert n <= int(1.1 * (1 << 20)), name
    assert CASES["one_full_task"][1] % 2048 == 0 and CASES["five_tasks"][1] % 2048 == 0
    assert CASES["unaligned_1"][1] % 2048 == 1 and CASES["unaligned_2047"][1] % 2048 == 2047
    for name in ("carry", "carry_aligned"):
        hi, lo, n = CASES[name]
        assert lo + n // 16 > (1 << 64) > lo, name
    for name in ("group_boundary", "group_boundary_aligned"):
        hi, lo, n = CASES[name]
        assert lo // 65536 != (lo + n // 16 - 1) // 65536, name


@pytest.fixture(scope="module")
def oracle():
    """expected outputs, computed once per (case, key size, plaintext kind)"""
    memo = {}

    def get(name, bits, kind):
        k = (name, bits, kind)
        if k not in memo:
            hi, lo, n = CASES[name]
            key = det(f"key{bits}", bits // 8)
            src = bytes(n) if kind == "zero" else det(name, n)
            memo[k] = (key, ctr_block(hi, lo), src, cpu_ref.ctr(key, ctr_block(hi, lo), src))
        return memo[k]

    return get


def first_diff(a, b):
    if a == b:
        return None
    i = next(i for i in range(min(len(a), len(b))) if a[i] != b[i]) if len(a) == len(b) else -1
    return {"byte": i, "block": i // 16, "slot": (i // 16 % 2048) // 64, "lane": i // 16 % 64}


@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("name", list(CASES))
def test_ctr_output_phase(gpu, oracle, name, bits):
    key, ctr0, src, exp = oracle(name, bits, "random")
    x = torch.frombuffer(bytearray(src), dtype=torch.uint8).to(gpu)
    y = ops.ctr(x, key, ctr0, impl="bitslice")  # out of place
    torch.cuda.synchronize()
    assert x.cpu().numpy().tobytes() == src, "the input of an out-of-place call changed"
    assert first_diff(y.cpu().numpy().tobytes(), exp) is None
    ops.ctr(x, key, ctr0, out=x, impl="bitslice")  # in place
    torch.cuda.synchronize()
    assert first_diff(x.cpu().numpy().tobytes(), exp) is None
    key, ctr0, zsrc, zexp = oracle(name, bits, "zero")
    z = torch.zeros(len(zsrc), dtype=torch.uint8, device=gpu)
    ops.ctr(z, key, ctr0, out=z, impl="bitslice")  # the keystream itself
    torch.cuda.synchronize()
    assert first_diff(z.cpu().numpy().tobytes(), zexp) is None
