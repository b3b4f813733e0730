"""The stream contract of the AES-OCB3 ops (ops.ocb_ops), by ``run_contract``
of tests/test_gpu_async_contract.py: every launch of a call -- the clearing of
the checksum, the bulk kernel, the finisher, the staging copies of a
misaligned view -- runs in the order of the caller's stream; ``ocb_encrypt``
and ``ocb_blocks`` make the host wait for nothing; ``ocb_decrypt`` waits only
for the 16 bytes of the tag it documents."""
import pytest

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref
from test_gpu_async_contract import A5, Case, _aead_dec_make, _view_make, run_contract, std_make

ocb = ops.ocb_ops
pytestmark = pytest.mark.gpu

K128, K256 = bytes(range(0x10, 0x20)), bytes(range(0x60, 0x80))
NONCE = bytes(range(0x40, 0x4C))
AAD13 = bytes(range(0x80, 0x8D))
N = 3 * 32768 + 4096 + 16 * 37 + 5  # whole runs, a pass, a partial pass and trailing bytes
NB = 2048 + 300                     # blocks: a run and a partial one
FIRST = (1 << 31) - 100
OFF0 = cpu_ref.ocb_offset0(K256, NONCE)


CASES = [
    Case("ocb_encrypt", ("ocb_encrypt",), std_make(N),
         lambda st: ocb.ocb_encrypt(st.inputs[0], K256, NONCE, AAD13, out=st.out),
         lambda st, x: list(cpu_ref.ocb(K256, NONCE, x, AAD13)), family="ocb", want_impl="ttable"),
    Case("ocb_encrypt short tag, in place", ("ocb_encrypt",), std_make(N, out=False),
         lambda st: ocb.ocb_encrypt(st.inputs[0], K128, NONCE, out=st.inputs[0], tag_bytes=12),
         lambda st, x: list(cpu_ref.ocb(K128, NONCE, x, tag_bytes=12)), family="ocb", inplace=(0,)),
    Case("ocb_encrypt misaligned views", ("ocb_encrypt",), _view_make(N),
         lambda st: (ocb.ocb_encrypt(st.inputs[0], K256, NONCE, AAD13, out=st.out)[1], st.buf2),
         lambda st, x: [cpu_ref.ocb(K256, NONCE, x, AAD13)[1],
                        bytes([A5]) * 5 + cpu_ref.ocb(K256, NONCE, x, AAD13)[0] + bytes([A5]) * 11], family="ocb"),
    Case("ocb_encrypt below a block", ("ocb_encrypt",), std_make(11),
         lambda st: ocb.ocb_encrypt(st.inputs[0], K256, NONCE, AAD13, out=st.out),
         lambda st, x: list(cpu_ref.ocb(K256, NONCE, x, AAD13)), family="ocb"),
    Case("ocb_decrypt", ("ocb_decrypt",), _aead_dec_make(N, lambda pt: cpu_ref.ocb(K256, NONCE, pt, AAD13)),
         lambda st: ocb.ocb_decrypt(st.inputs[0], K256, NONCE, st.tag, AAD13, out=st.out),
         lambda st, x: [cpu_ref.ocb(K256, NONCE, x, AAD13, decrypt=True)[0]], family="ocb", syncs=True),
    # the data and the running checksum are both inputs; the checksum is also a result
    Case("ocb_blocks", ("ocb_blocks",), std_make(16 * NB, 16),
         lambda st: ocb.ocb_blocks(st.inputs[0], K256, OFF0, FIRST, checksum=st.inputs[1], out=st.out),
         lambda st, x, cs: list(cpu_ref.ocb_blocks(K256, OFF0, x, FIRST, cs)), family="ocb", inplace=(1,)),
    Case("ocb_blocks decrypt, fresh checksum", ("ocb_blocks",), std_make(16 * NB),
         lambda st: ocb.ocb_blocks(st.inputs[0], K128, OFF0, 254, out=st.out, decrypt=True),
         lambda st, x: list(cpu_ref.ocb_blocks(K128, OFF0, x, 254, decrypt=True)), family="ocb"),
]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stream_contract(gpu, case):
    run_contract(case, gpu)


def test_every_ocb_op_has_a_row():
    """ops.ocb_ops' device ops are not in ops.__all__ (whose rows the other file keeps): their rows are here."""
    covered = {o for c in CASES for o in c.ops}
    public = {n for n in vars(ocb) if n.startswith("ocb_")}
    assert public - covered == {"ocb_spans", "ocb_check", "ocb_check_blocks"}  # a query and two host-side checks
    assert not public & set(ops.__all__)
