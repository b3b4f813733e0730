"""Guard bands around the buffers of ops.chacha20, ops.poly1305 and the
ChaCha20-Poly1305 ops (csrc/hip/chacha.hip), by the arena method of
tests/test_gpu_bounds.py (its ``run_guarded``: 0xA5 guards around the output,
input arenas filled with 0x00 and then 0xFF, in place): no kernel writes
outside its output, changes its input, or lets bytes outside its input reach
the result.

The widest store step of the new kernels is one ChaCha20 bulk workgroup:
4 waves x 4 passes x 4 KiB = 64 KiB (one store instruction of a wave covers
at most 4 KiB; the edge kernel stores single bytes; Poly1305 stores 32-byte
partials into its own workspace and 4-byte words into the tag).  The helper's
guards are 64 KiB + 64 bytes, wider than that, so a wrong range check shows as
a changed guard byte and never as a fault."""
import pytest
import torch

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref
from test_gpu_bounds import GUARD, host, run_guarded

pytestmark = pytest.mark.gpu

STORE_STEP = 4 * 4 * 4096  # chacha.hip CC_WAVES * CC_RUN * CC_PASS
PASS = 4096                # one pass of a wave: the bulk / edge split falls on a multiple of it
assert GUARD > STORE_STEP

KEY = bytes(range(11, 43))
NONCE = bytes(range(0x30, 0x3C))
AAD = bytes(range(13))
SHIFTS = [0, 3]
# around a lane's block, a pass (the bulk / edge split) and the workgroup's store step
LENGTHS = [1, 63, 64, 65, PASS - 1, PASS, PASS + 1, STORE_STEP - 1, STORE_STEP, STORE_STEP + 1, 2 * STORE_STEP + PASS + 17]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_chacha20_guarded(gpu, n, shift):
    run_guarded(lambda x, out: ops.chacha20(x, KEY, NONCE, 7, out=out), gpu, n,
                ref=lambda x: cpu_ref.chacha20(KEY, NONCE, host(x), 7), seed=n % 1009, shift=shift, also_inplace=True,
                what=f"chacha20 n={n}")


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 1024, 1025, PASS - 1, PASS + 1, 32768 - 1, 32768, 32768 + 1, STORE_STEP + 1])
def test_poly1305_guarded(gpu, n, shift):
    """The output is the 16-byte tag, written into a guarded region; the input
    arena must come back unchanged and its fill must not reach the tag."""
    run_guarded(lambda x, out: out.copy_(ops.poly1305(x, KEY)), gpu, 16, n_in=(n,),
                ref=lambda x: cpu_ref.poly1305(KEY, host(x)), seed=n % 1009, shift=shift, what=f"poly1305 n={n}")


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [1, 63, 65, PASS - 1, PASS + 1, STORE_STEP - 1, STORE_STEP + 1])
def test_aead_encrypt_guarded(gpu, n, shift):
    tags = []

    def op(x, out):
        tags.append(ops.chacha20_poly1305_encrypt(x, KEY, NONCE, AAD, out=out)[1])

    def check(x, out):
        # out is the ciphertext by now (in place x is too)
        assert host(tags[-1]) == cpu_ref.chacha20_poly1305(KEY, NONCE, host(out), AAD, decrypt=True)[1]

    run_guarded(op, gpu, n, ref=lambda x: cpu_ref.chacha20_poly1305(KEY, NONCE, host(x), AAD)[0], check=check,
                seed=n % 1009, shift=shift, also_inplace=True, what=f"chacha20_poly1305_encrypt n={n}")
    assert len({host(t) for t in tags}) == 1  # the same tag under both fills and in place


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [1, 63, 65, PASS - 1, PASS + 1, STORE_STEP - 1, STORE_STEP + 1])
def test_aead_decrypt_guarded(gpu, n, shift):
    """The input is random bytes taken as a ciphertext; the tag it needs comes from the oracle."""
    def op(x, out):
        tag = cpu_ref.chacha20_poly1305(KEY, NONCE, host(x), AAD, decrypt=True)[1]
        ops.chacha20_poly1305_decrypt(x, KEY, NONCE, tag, AAD, out=out)

    run_guarded(op, gpu, n, ref=lambda x: cpu_ref.chacha20_poly1305(KEY, NONCE, host(x), AAD, decrypt=True)[0],
                seed=n % 1009, shift=shift, also_inplace=True, what=f"chacha20_poly1305_decrypt n={n}")
