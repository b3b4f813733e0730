"""Guard bands around the buffers of the AES-GCM-SIV ops
(csrc/hip/aes_gcm_siv.hip), by the arena method of tests/test_gpu_bounds.py (its
``run_guarded``: 0xA5 guards around the output, input arenas filled with 0x00
and then 0xFF, in place): no kernel writes outside its output, changes its
input, or lets bytes outside its input reach the result or the tag.

The widest single store step of these kernels is one pass of the counter
kernel's workgroup: 16 waves x 4 blocks per lane x 64 lanes x 16 bytes =
64 KiB (one store instruction of a wave covers 1 KiB; its partial last block
is stored byte by byte; the hash's level kernel stores 16 partials of 16
bytes per workgroup step, into its workspace; the finisher stores four words
into the tag).  The helper's guards are 64 KiB + 64 bytes, wider than that, so
a wrong range check shows as a changed guard byte and never as a fault."""
import ctypes

import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref
from test_gpu_bounds import GUARD, host, run_guarded

siv = ops.gcm_siv_ops
pytestmark = pytest.mark.gpu

BLOCK = 16
HASH_PASS = 64 * 16        # ghash_levels_dev.h: one load of a wave of the level kernel
PASS = 256 * 16            # aes_gcm_siv.hip SIV_PASS blocks: one pass of a wave
RUN = 2048 * 16            # SIV_RUN: a wave's run; also GH_SPAN, the hash's wave span
CHUNK = 16 * RUN           # SIV_CHUNK: a workgroup's chunk per grid step; also the hash's workgroup step
STORE_STEP = 16 * PASS     # the 16 waves of a workgroup, one pass each
assert GUARD > STORE_STEP

KEY = bytes(range(0x21, 0x41))
KEY128 = bytes(range(0x51, 0x61))
NONCE = bytes(range(0x30, 0x3C))
AAD = bytes(range(13))
H = bytes.fromhex("25629347589242761d31f826ba4b757b")
CTR = (0xFFFFFF00).to_bytes(4, "little") + bytes(range(0x70, 0x7B)) + b"\x85"  # wraps 256 blocks into a call
SHIFTS = [0, 3]
# around a lane's block, a pass, a wave's run and a workgroup's chunk
LENGTHS = [1, BLOCK - 1, BLOCK, BLOCK + 1, HASH_PASS + 1, PASS - 1, PASS, PASS + 1, RUN - BLOCK, RUN + 1,
           STORE_STEP + BLOCK + 1, CHUNK - 1, CHUNK + BLOCK, CHUNK + RUN + PASS + 17]


def test_the_lengths_are_the_kernels_boundaries():
    assert {BLOCK, HASH_PASS, PASS, RUN, CHUNK} <= set(siv.ctr_le32_spans())
    assert {HASH_PASS, RUN, CHUNK} <= set(siv.polyval_spans())


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_encrypt_guarded(gpu, n, shift):
    tags = []

    def op(x, out):
        tags.append(siv.gcm_siv_encrypt(x, KEY, NONCE, AAD, out=out)[1])

    ref = {}

    def expect(x):
        ref["ct"], ref["tag"] = cpu_ref.gcm_siv(KEY, NONCE, host(x), AAD)
        return ref["ct"]

    run_guarded(op, gpu, n, ref=expect, seed=n % 1009, shift=shift, also_inplace=True, what=f"gcm_siv_encrypt n={n}")
    assert {host(t) for t in tags} == {ref["tag"]}  # the same tag under both fills and in place


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_decrypt_guarded(gpu, n, shift):
    """The input is random bytes taken as a ciphertext under a fixed received
    tag.  In this mode the received tag starts the counter mode, so no tag makes
    arbitrary bytes authentic, and ``gcm_siv_decrypt`` would zero its output:
    the run is the op's own launch path without the comparison at its end
    (``_gcm_siv`` with the received tag on the device), and the computed tag is
    compared with the oracle's here."""
    received = bytes(range(0xB0, 0xC0))
    tag_in = torch.frombuffer(bytearray(received), dtype=torch.uint8).to(gpu)
    tags, ref = [], {}

    def op(x, out):
        tags.append(siv._gcm_siv(x, KEY128, NONCE, AAD, out, tag_in)[1])

    def expect(x):
        ref["pt"], ref["tag"] = cpu_ref.gcm_siv(KEY128, NONCE, host(x), AAD, decrypt=True, tag=received)
        return ref["pt"]

    run_guarded(op, gpu, n, ref=expect, seed=n % 1009, shift=shift, also_inplace=True, what=f"gcm_siv_decrypt n={n}")
    assert {host(t) for t in tags} == {ref["tag"]}
    assert host(tag_in) == received  # the counter kernel only reads the received tag


@pytest.mark.parametrize("bits", [128, 256])
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_ctr_le32_guarded(gpu, n, shift, bits):
    key = KEY[: bits // 8]
    c = torch.frombuffer(bytearray(CTR), dtype=torch.uint8).to(gpu)
    run_guarded(lambda x, out: siv.ctr_le32(x, key, c, out=out), gpu, n,
                ref=lambda x: cpu_ref.ctr_le32(key, CTR, host(x)), seed=n % 1009, shift=shift, also_inplace=True,
                what=f"ctr_le32 n={n}")
    assert host(c) == CTR  # the kernel only reads its counter block


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_polyval_guarded(gpu, n, shift):
    """The data is the guarded input, the 16-byte result the guarded output."""
    def op(x, y):
        y.copy_(siv.polyval(x, H))

    run_guarded(op, gpu, 16, n_in=(n,), ref=lambda x: cpu_ref.polyval(H, host(x)), seed=n % 1009, shift=shift,
                what=f"polyval n={n}")


def test_the_tag_stays_inside_its_16_bytes(gpu):
    """The finisher's stores and the counter kernel's read of the tag through
    the C call, with tag_dev itself the guarded region (the ops allocate their own tag)."""
    lib = _native.require_gpu_lib()
    k = _native.OtcGcmSivKey()
    assert lib.otc_gcm_siv_key_init(ctypes.byref(k), _native.as_u8p(KEY), 256) == 0
    n = CHUNK + RUN + 5

    def op(x, tag):
        sink = torch.empty_like(x)
        with torch.cuda.device(gpu):
            rc = lib.otc_aes_gcm_siv(x.data_ptr(), sink.data_ptr(), n, ctypes.byref(k), 1, _native.as_u8p(NONCE),
                                     _native.as_u8p(AAD), 13, None, tag.data_ptr(), None)
        assert rc == 0

    run_guarded(op, gpu, 16, n_in=(n,), ref=lambda x: cpu_ref.gcm_siv(KEY, NONCE, host(x), AAD)[1], seed=3,
                what="gcm_siv tag")
