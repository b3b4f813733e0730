"""Guard bands around the buffers of the AES-OCB3 ops (csrc/hip/aes_ocb.hip),
by the arena method of tests/test_gpu_bounds.py (its ``run_guarded``: 0xA5
guards around the output, input arenas filled with 0x00 and then 0xFF, in
place): no kernel writes outside its output, changes its input, or lets bytes
outside its input reach the result or the tag.

The widest single store step of these kernels is one pass of the bulk
kernel's workgroup: 16 waves x 4 blocks per lane x 64 lanes x 16 bytes =
64 KiB (one store instruction of a wave covers 1 KiB; the finisher stores
single bytes into the output and four words into the tag; the checksum is 16
bytes of atomics).  The helper's guards are 64 KiB + 64 bytes, wider than
that, so a wrong range check shows as a changed guard byte and never as a
fault."""
import ctypes

import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref
from test_gpu_bounds import GUARD, host, run_guarded

ocb = ops.ocb_ops
pytestmark = pytest.mark.gpu

BLOCK = 16
PASS = 256 * 16            # aes_ocb.hip OCB_PASS blocks: one pass of a wave
RUN = 2048 * 16            # OCB_RUN: a wave's run
CHUNK = 16 * RUN           # OCB_CHUNK: a workgroup's chunk per grid step
STORE_STEP = 16 * PASS     # the 16 waves of a workgroup, one pass each
assert GUARD > STORE_STEP

KEY = bytes(range(0x21, 0x41))
KEY128 = bytes(range(0x51, 0x61))
NONCE = bytes(range(0x30, 0x3C))
AAD = bytes(range(13))
SHIFTS = [0, 3]
# around a lane's block, a pass, a wave's run and a workgroup's chunk
LENGTHS = [1, BLOCK - 1, BLOCK, BLOCK + 1, PASS - 1, PASS, PASS + 1, RUN - BLOCK, RUN + 1, STORE_STEP + BLOCK + 1,
           CHUNK - 1, CHUNK + BLOCK, CHUNK + RUN + PASS + 17]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_encrypt_guarded(gpu, n, shift):
    tags = []

    def op(x, out):
        tags.append(ocb.ocb_encrypt(x, KEY, NONCE, AAD, out=out)[1])

    ref = {}

    def expect(x):
        ref["ct"], ref["tag"] = cpu_ref.ocb(KEY, NONCE, host(x), AAD)
        return ref["ct"]

    run_guarded(op, gpu, n, ref=expect, seed=n % 1009, shift=shift, also_inplace=True,
                what=f"ocb_encrypt n={n}")
    assert {host(t) for t in tags} == {ref["tag"]}  # the same tag under both fills and in place


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_decrypt_guarded(gpu, n, shift):
    """The input is random bytes taken as a ciphertext; the tag it needs comes from the oracle."""
    def op(x, out):
        tag = cpu_ref.ocb(KEY128, NONCE, host(x), AAD, decrypt=True)[1]
        ocb.ocb_decrypt(x, KEY128, NONCE, tag, AAD, out=out)

    run_guarded(op, gpu, n, ref=lambda x: cpu_ref.ocb(KEY128, NONCE, host(x), AAD, decrypt=True)[0], seed=n % 1009,
                shift=shift, also_inplace=True, what=f"ocb_decrypt n={n}")


@pytest.mark.parametrize("decrypt", [False, True], ids=["enc", "dec"])
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("nb,first", [(1, 0), (1, 255), (255, 1), (256, 0), (257, 255), (2048, 254), (2049, (1 << 31) - 100),
                                      (32768 + 300, 77), (1000, (1 << 32) - 1000)])
def test_blocks_guarded(gpu, nb, first, shift, decrypt):
    """A call that starts in the middle of a pass of the message's numbering
    skips the lanes in front of its first block: they must not touch memory."""
    off0 = cpu_ref.ocb_offset0(KEY, NONCE)
    sums, ref = [], {}

    def op(x, out):
        sums.append(ocb.ocb_blocks(x, KEY, off0, first, out=out, decrypt=decrypt)[1])

    def expect(x):
        ref["out"], ref["cs"] = cpu_ref.ocb_blocks(KEY, off0, host(x), first, decrypt=decrypt)
        return ref["out"]

    run_guarded(op, gpu, 16 * nb, ref=expect, seed=nb % 1009, shift=shift, also_inplace=True,
                what=f"ocb_blocks nb={nb} first={first}")
    assert {host(s) for s in sums} == {ref["cs"]}


def test_the_tag_stays_inside_its_16_bytes(gpu):
    """The checksum's atomics and the finisher's stores through the C call, with
    tag_dev itself the guarded region (the ops allocate their own tag)."""
    lib = _native.require_gpu_lib()
    k = _native.OtcOcbKey()
    assert lib.otc_ocb_key_init(ctypes.byref(k), _native.as_u8p(KEY), 256) == 0
    n = CHUNK + RUN + 5

    def op(x, tag):
        sink = torch.empty_like(x)
        rc = lib.otc_aes_ocb(x.data_ptr(), sink.data_ptr(), n, ctypes.byref(k), 1, _native.as_u8p(NONCE), 12,
                             _native.as_u8p(AAD), 13, 12, tag.data_ptr(), None)
        assert rc == 0

    run_guarded(op, gpu, 16, n_in=(n,), ref=lambda x: cpu_ref.ocb(KEY, NONCE, host(x), AAD, tag_bytes=12)[1] + bytes(4),
                seed=3, what="ocb tag")
