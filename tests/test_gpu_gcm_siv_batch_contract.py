"""The stream contract of the batched AES-GCM-SIV ops
(ops.gcm_siv_batch_ops), by ``run_contract`` of
tests/test_gpu_async_contract.py: every launch of a run -- derive, the batched
POLYVAL, the finisher, the counter kernel that reads the tags the finisher
wrote (or a decryption's received tags), the wipe -- runs in the order of the
caller's stream, also when the stream is handed over from another one, while
work on another stream goes on; the host waits for nothing although the
counter mode starts at values computed on the device and the verdicts are
formed there; the two halves by themselves keep the same contract.  The plan
is made before the delay; data, nonces and tags come late."""
import pytest

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref
from test_gpu_async_contract import A5, Case, _on_default, _slots, dev, hostb, rnd, run_contract, std_make

SB = ops.gcm_siv_batch_ops
pytestmark = pytest.mark.gpu

K128, K256 = bytes(range(0x10, 0x20)), bytes(range(0x60, 0x80))
SB_N = 37
SB_LENS = [1, 4096, 0] + [(i * 331 + 7) % 4200 + 1 for i in range(SB_N - 4)] + [3 * 4096 + 17]
SB_OFFS, SB_DATA = _slots(SB_LENS)
SB_AAD_LENS = [5 + m if m % 3 == 1 else 0 for m in range(SB_N)]  # device AADs, packed from an odd address
SB_AAD_OFFS = [SB_DATA + 1 + sum(SB_AAD_LENS[:m]) for m in range(SB_N)]
SB_POOL = SB_DATA + 1 + sum(SB_AAD_LENS)
SB_FORGED = 5  # decrypt: this record's received tag is wrong


def _aad(pool: bytes, m: int) -> bytes:
    """Record m's AAD: host bytes (m % 3 == 0), a device view of the pool (1) or none (2)."""
    if m % 3 == 0:
        return bytes((m + i) & 0xFF for i in range(13))
    return pool[SB_AAD_OFFS[m]:SB_AAD_OFFS[m] + SB_AAD_LENS[m]]


def _records(pool: bytes, nonces: bytes):
    for m, (o, n) in enumerate(zip(SB_OFFS, SB_LENS)):
        yield m, o, n, pool[o:o + n], nonces[12 * m:12 * m + 12], _aad(pool, m)


def _batch_make(decrypt, key, lanes):
    def make(gpu):
        st = std_make(SB_POOL, (SB_N, 12), (SB_N, 16))(gpu)
        if decrypt:  # the late inputs are valid ciphertexts and their tags, but for one forgery
            pool, nonces = bytearray(hostb(st.fresh[0])), hostb(st.fresh[1])
            tags = bytearray()
            for m, o, n, pt, nonce, aad in _records(bytes(pool), nonces):
                pool[o:o + n], t = cpu_ref.gcm_siv(key, nonce, pt, aad)
                tags += t
            tags[16 * SB_FORGED + 3] ^= 0x10
            st.fresh = [dev(bytes(pool), gpu), st.fresh[1], dev(bytes(tags), gpu, (SB_N, 16))]
        else:
            st.inputs, st.fresh = st.inputs[:2], st.fresh[:2]
        x = st.inputs[0]
        xs = [x[o:o + n] for o, n in zip(SB_OFFS, SB_LENS)]
        outs = [st.out[o:o + n] for o, n in zip(SB_OFFS, SB_LENS)]
        aads = [_aad(b"", m) if m % 3 == 0 else x[SB_AAD_OFFS[m]:SB_AAD_OFFS[m] + SB_AAD_LENS[m]] if m % 3 == 1
                else None for m in range(SB_N)]
        st.key = key
        st.batch = SB.GcmSivBatch(xs, key, outs=outs, aads=aads, lanes=lanes)
        st.outs = [st.out, st.batch.tags, st.batch.ok]
        return st
    return make


def _encrypt_ref(st, pool, nonces):
    exp, tags = bytearray([A5]) * SB_POOL, bytearray()
    for m, o, n, pt, nonce, aad in _records(pool, nonces):
        exp[o:o + n], t = cpu_ref.gcm_siv(st.key, nonce, pt, aad)
        tags += t
    return [bytes(exp), bytes(tags)]


def _decrypt_ref(st, pool, nonces, tags):
    exp, ok, computed = bytearray([A5]) * SB_POOL, bytearray(), bytearray()
    for m, o, n, ct, nonce, aad in _records(pool, nonces):
        received = tags[16 * m:16 * m + 16]
        pt, t = cpu_ref.gcm_siv(st.key, nonce, ct, aad, decrypt=True, tag=received)
        good = t == received
        exp[o:o + n] = pt if good else bytes(n)  # a failed record is zeroed, and so is its computed tag
        computed += t if good else bytes(16)
        ok.append(int(good))
    return [bytes(exp), bytes(ok), bytes(computed)]


def _encrypt(st, **kw):
    st.batch.encrypt(st.inputs[1], **kw)
    return st.out, st.batch.tags


def _decrypt(st, **kw):
    _, ok = st.batch.decrypt(st.inputs[1], st.inputs[2], **kw)
    return st.out, ok, st.batch.tags


# -- the halves: the data, the hash keys / counter rows come late; the plan is made inside the call --
HV_LENS = [1, 16, 4096, 1000, 255 * 16, 3 * 4096 + 17, 0, 17]
HV_OFFS, HV_DATA = _slots(HV_LENS)
HV_N = len(HV_LENS)


def _halves_make(gpu):
    return std_make(HV_DATA, (HV_N, 16))(gpu)


def _views(t):
    return [t[o:o + n] for o, n in zip(HV_OFFS, HV_LENS)]


def _polyval_ref(st, pool, hs):
    out = bytearray()
    for m, (o, n) in enumerate(zip(HV_OFFS, HV_LENS)):
        x = pool[o:o + n]
        out += cpu_ref.polyval(hs[16 * m:16 * m + 16], x + bytes(-n % 16) + bytes(8) + (8 * n).to_bytes(8, "little"))
    return [bytes(out)]


HV_KEYS = [rnd(32, 900 + m) for m in range(HV_N)]


def _ctr_call(st):
    SB.ctr_le32_batch(_views(st.inputs[0]), HV_KEYS, st.inputs[1], outs=_views(st.out))
    return st.out


def _ctr_ref(st, pool, ctrs):
    exp = bytearray([A5]) * HV_DATA
    for m, (o, n) in enumerate(zip(HV_OFFS, HV_LENS)):
        c = ctrs[16 * m:16 * m + 16]
        exp[o:o + n] = cpu_ref.ctr_le32(HV_KEYS[m], c[:15] + bytes([c[15] | 0x80]), pool[o:o + n])
    return [bytes(exp)]


CASES = [
    Case("GcmSivBatch.encrypt", ("GcmSivBatch",), _batch_make(False, K256, 16), _encrypt, _encrypt_ref,
         family="gcm siv batch", want_impl="ttable"),
    Case("GcmSivBatch.encrypt aes128, 64 lanes", ("GcmSivBatch",), _batch_make(False, K128, 64), _encrypt, _encrypt_ref,
         family="gcm siv batch", want_impl="ttable"),
    Case("GcmSivBatch.encrypt(stream=s) from the default stream", ("GcmSivBatch",), _batch_make(False, K256, 16),
         lambda st: _on_default(st, lambda stream: _encrypt(st, stream=stream)), _encrypt_ref, family="gcm siv batch"),
    Case("GcmSivBatch.decrypt", ("GcmSivBatch",), _batch_make(True, K256, 16), _decrypt, _decrypt_ref,
         family="gcm siv batch", want_impl="ttable"),
    Case("GcmSivBatch.decrypt(stream=s) from the default stream", ("GcmSivBatch",), _batch_make(True, K128, 64),
         lambda st: _on_default(st, lambda stream: _decrypt(st, stream=stream)), _decrypt_ref, family="gcm siv batch"),
    Case("polyval_batch", ("polyval_batch",), _halves_make,
         lambda st: SB.polyval_batch(_views(st.inputs[0]), st.inputs[1], lanes=16), _polyval_ref, family="gcm siv batch"),
    Case("polyval_batch, 64 lanes", ("polyval_batch",), _halves_make,
         lambda st: SB.polyval_batch(_views(st.inputs[0]), st.inputs[1], lanes=64), _polyval_ref, family="gcm siv batch"),
    Case("ctr_le32_batch", ("ctr_le32_batch",), _halves_make, _ctr_call, _ctr_ref, family="gcm siv batch",
         want_impl="ttable"),
]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stream_contract(gpu, case):
    run_contract(case, gpu)


def test_every_batched_gcm_siv_op_has_a_row():
    """ops.gcm_siv_batch_ops' device ops are not in ops.__all__ (whose rows the other file keeps): their rows are here."""
    covered = {o for c in CASES for o in c.ops}
    public = {"GcmSivBatch", "polyval_batch", "ctr_le32_batch"}
    assert public <= covered and all(hasattr(SB, n) for n in public)
    assert not public & set(ops.__all__)
    assert not [c.name for c in CASES if c.syncs]  # nothing here documents a readback
