"""The stream contract of the AES-GCM-SIV ops (ops.gcm_siv_ops), by
``run_contract`` of tests/test_gpu_async_contract.py: every launch of a call --
the table builder, the hash's levels, the finisher, the counter kernel that
reads the tag the finisher wrote, the staging copies of a misaligned view --
runs in the order of the caller's stream; ``polyval``, ``ctr_le32`` and
``gcm_siv_encrypt`` make the host wait for nothing, although the counter mode
starts at a value computed on the device; ``gcm_siv_decrypt`` waits only for
the 16 bytes of the tag it documents."""
import pytest

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref
from test_gpu_async_contract import A5, Case, _aead_dec_make, _view_make, dev, one, run_contract, std_make

siv = ops.gcm_siv_ops
pytestmark = pytest.mark.gpu

K128, K256 = bytes(range(0x10, 0x20)), bytes(range(0x60, 0x80))
NONCE = bytes(range(0x40, 0x4C))
AAD13 = bytes(range(0x80, 0x8D))
H = bytes.fromhex("25629347589242761d31f826ba4b757b")
Y0 = bytes(range(0xA0, 0xB0))
N = 3 * 32768 + 4096 + 16 * 37 + 5  # whole wave spans and runs, a pass, a partial pass and trailing bytes
N_HASH = 65541
CTR_WRAP = (0xFFFFFFF0).to_bytes(4, "little") + bytes(range(0x30, 0x3C))  # wraps 16 blocks into the call


def _forced(c: bytes) -> bytes:
    return c[:15] + bytes([c[15] | 0x80])


def _seal(key, aad=b""):
    return lambda st, x: list(cpu_ref.gcm_siv(key, NONCE, x, aad))


def _dec_tensor_make(gpu):
    """The received tag on the device: the counter kernel reads it there, nothing of it goes to the host first."""
    st = _aead_dec_make(N, lambda pt: cpu_ref.gcm_siv(K128, NONCE, pt))(gpu)
    st.tag_dev = dev(st.tag, gpu)
    return st


CASES = [
    one("polyval", "polyval", N_HASH, lambda x, o: siv.polyval(x, H, Y0), lambda x: cpu_ref.polyval(H, x, Y0), family="gcm siv"),
    Case("polyval misaligned view", ("polyval",), _view_make(N_HASH),
         lambda st: siv.polyval(st.inputs[0], H), lambda st, x: [cpu_ref.polyval(H, x)], family="gcm siv"),
    # the data and the counter block are both inputs: the block is produced on the stream, in front of the call
    Case("ctr_le32 counter on the device", ("ctr_le32",), std_make(N, 16),
         lambda st: siv.ctr_le32(st.inputs[0], K256, st.inputs[1], out=st.out),
         lambda st, x, c: [cpu_ref.ctr_le32(K256, _forced(c), x)], family="gcm siv", want_impl="ttable"),
    Case("ctr_le32 counter as bytes, across the wrap, in place", ("ctr_le32",), std_make(N, out=False),
         lambda st: siv.ctr_le32(st.inputs[0], K128, CTR_WRAP, out=st.inputs[0]),
         lambda st, x: [cpu_ref.ctr_le32(K128, _forced(CTR_WRAP), x)], family="gcm siv", inplace=(0,)),
    Case("gcm_siv_encrypt", ("gcm_siv_encrypt",), std_make(N),
         lambda st: siv.gcm_siv_encrypt(st.inputs[0], K256, NONCE, AAD13, out=st.out), _seal(K256, AAD13),
         family="gcm siv", want_impl="ttable"),
    Case("gcm_siv_encrypt aes128, in place", ("gcm_siv_encrypt",), std_make(N, out=False),
         lambda st: siv.gcm_siv_encrypt(st.inputs[0], K128, NONCE, out=st.inputs[0]), _seal(K128),
         family="gcm siv", inplace=(0,)),
    Case("gcm_siv_encrypt misaligned views", ("gcm_siv_encrypt",), _view_make(N),
         lambda st: (siv.gcm_siv_encrypt(st.inputs[0], K256, NONCE, AAD13, out=st.out)[1], st.buf2),
         lambda st, x: [cpu_ref.gcm_siv(K256, NONCE, x, AAD13)[1],
                        bytes([A5]) * 5 + cpu_ref.gcm_siv(K256, NONCE, x, AAD13)[0] + bytes([A5]) * 11], family="gcm siv"),
    Case("gcm_siv_encrypt below a block", ("gcm_siv_encrypt",), std_make(11),
         lambda st: siv.gcm_siv_encrypt(st.inputs[0], K256, NONCE, AAD13, out=st.out), _seal(K256, AAD13),
         family="gcm siv"),
    Case("gcm_siv_decrypt", ("gcm_siv_decrypt",), _aead_dec_make(N, lambda pt: cpu_ref.gcm_siv(K256, NONCE, pt, AAD13)),
         lambda st: siv.gcm_siv_decrypt(st.inputs[0], K256, NONCE, st.tag, AAD13, out=st.out),
         lambda st, x: [cpu_ref.gcm_siv(K256, NONCE, x, AAD13, decrypt=True, tag=st.tag)[0]], family="gcm siv",
         syncs=True),
    Case("gcm_siv_decrypt tag on the device", ("gcm_siv_decrypt",), _dec_tensor_make,
         lambda st: siv.gcm_siv_decrypt(st.inputs[0], K128, NONCE, st.tag_dev, out=st.out),
         lambda st, x: [cpu_ref.gcm_siv(K128, NONCE, x, decrypt=True, tag=st.tag)[0]], family="gcm siv", syncs=True),
]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stream_contract(gpu, case):
    run_contract(case, gpu)


def test_every_gcm_siv_op_has_a_row():
    """ops.gcm_siv_ops' device ops are not in ops.__all__ (whose rows the other file keeps): their rows are here."""
    covered = {o for c in CASES for o in c.ops}
    public = {n for n in vars(siv) if n.startswith(("polyval", "ctr_le32", "gcm_siv_"))}
    assert public - covered == {"polyval_spans", "ctr_le32_spans", "gcm_siv_check"}  # two queries and a host-side check
    assert not public & set(ops.__all__)
    assert [c.name for c in CASES if c.syncs] == [c.name for c in CASES if c.ops == ("gcm_siv_decrypt",)]
