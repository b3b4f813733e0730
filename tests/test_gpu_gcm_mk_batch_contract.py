"""The stream contract of the many-key batched AES-GCM ops
(ops.gcm_mk_batch_ops), by ``run_contract`` of
tests/test_gpu_async_contract.py: every launch of a run -- prep, the batched
CTR kernel with its key index per record, the batched hash on the keys' table
images, the finisher, the wipe -- runs in the order of the caller's stream, also
when the stream is handed over from another one, while work on another stream
goes on; the host waits for nothing although the verdicts are formed on the
device; the hash by itself keeps the same contract.  The plan, the schedules
and the table images are made before the delay; data, IVs and tags come late."""
import pytest

from our_tree_amd import ops
from our_tree_amd.models import cpu_ref
from test_gpu_async_contract import A5, Case, _on_default, _slots, dev, hostb, rnd, run_contract, std_make

MK = ops.gcm_mk_batch_ops
pytestmark = pytest.mark.gpu

MK_N = 37
MK_LENS = [1, 4096, 0] + [(i * 331 + 7) % 4200 + 1 for i in range(MK_N - 4)] + [3 * 4096 + 17]
MK_OFFS, MK_DATA = _slots(MK_LENS)
MK_AAD_LENS = [5 + m if m % 3 == 1 else 0 for m in range(MK_N)]  # device AADs, packed from an odd address
MK_AAD_OFFS = [MK_DATA + 1 + sum(MK_AAD_LENS[:m]) for m in range(MK_N)]
MK_POOL = MK_DATA + 1 + sum(MK_AAD_LENS)
MK_FORGED = 5  # decrypt: this record's received tag is wrong
MK_NKEYS = 7
MK_KIDX = [(5 * m + 3) % MK_NKEYS for m in range(MK_N)]


def _keys(bits):
    return [rnd(bits // 8, 700 + bits + k) for k in range(MK_NKEYS)]


def _aad(pool: bytes, m: int) -> bytes:
    """Record m's AAD: host bytes (m % 3 == 0), a device view of the pool (1) or none (2)."""
    if m % 3 == 0:
        return bytes((m + i) & 0xFF for i in range(13))
    return pool[MK_AAD_OFFS[m]:MK_AAD_OFFS[m] + MK_AAD_LENS[m]]


def _records(pool: bytes, ivs: bytes):
    for m, (o, n) in enumerate(zip(MK_OFFS, MK_LENS)):
        yield m, o, n, pool[o:o + n], ivs[12 * m:12 * m + 12], _aad(pool, m)


def _batch_make(decrypt, bits, lanes):
    keys = _keys(bits)

    def make(gpu):
        st = std_make(MK_POOL, (MK_N, 12), (MK_N, 16))(gpu)
        if decrypt:  # the late inputs are valid ciphertexts and their tags, but for one forgery
            pool, ivs = bytearray(hostb(st.fresh[0])), hostb(st.fresh[1])
            tags = bytearray()
            for m, o, n, pt, iv, aad in _records(bytes(pool), ivs):
                pool[o:o + n], t = cpu_ref.gcm(keys[MK_KIDX[m]], iv, pt, aad)
                tags += t
            tags[16 * MK_FORGED + 3] ^= 0x10
            st.fresh = [dev(bytes(pool), gpu), st.fresh[1], dev(bytes(tags), gpu, (MK_N, 16))]
        else:
            st.inputs, st.fresh = st.inputs[:2], st.fresh[:2]
        x = st.inputs[0]
        xs = [x[o:o + n] for o, n in zip(MK_OFFS, MK_LENS)]
        outs = [st.out[o:o + n] for o, n in zip(MK_OFFS, MK_LENS)]
        aads = [_aad(b"", m) if m % 3 == 0 else x[MK_AAD_OFFS[m]:MK_AAD_OFFS[m] + MK_AAD_LENS[m]] if m % 3 == 1
                else None for m in range(MK_N)]
        st.keys = keys
        st.batch = MK.GcmMkBatch(xs, keys, key_index=MK_KIDX, outs=outs, aads=aads, lanes=lanes)
        st.outs = [st.out, st.batch.tags, st.batch.ok]
        return st
    return make


def _encrypt_ref(st, pool, ivs):
    exp, tags = bytearray([A5]) * MK_POOL, bytearray()
    for m, o, n, pt, iv, aad in _records(pool, ivs):
        exp[o:o + n], t = cpu_ref.gcm(st.keys[MK_KIDX[m]], iv, pt, aad)
        tags += t
    return [bytes(exp), bytes(tags)]


def _decrypt_ref(st, pool, ivs, tags):
    exp, ok, computed = bytearray([A5]) * MK_POOL, bytearray(), bytearray()
    for m, o, n, ct, iv, aad in _records(pool, ivs):
        pt, t = cpu_ref.gcm(st.keys[MK_KIDX[m]], iv, ct, aad, decrypt=True)
        good = t == tags[16 * m:16 * m + 16]
        exp[o:o + n] = pt if good else bytes(n)  # a failed record is zeroed, and so is its computed tag
        computed += t if good else bytes(16)
        ok.append(int(good))
    return [bytes(exp), bytes(ok), bytes(computed)]


def _hash_ref(st, pool, ivs):
    out = bytearray()
    for m, o, n, x, iv, aad in _records(pool, ivs):
        out += cpu_ref.ghash(cpu_ref.gcm_h(st.keys[MK_KIDX[m]]), aad + bytes(-len(aad) % 16) + x + bytes(-n % 16) +
                             (8 * len(aad)).to_bytes(8, "big") + (8 * n).to_bytes(8, "big"))
    return [bytes(out)]


def _encrypt(st, **kw):
    st.batch.encrypt(st.inputs[1], **kw)
    return st.out, st.batch.tags


def _decrypt(st, **kw):
    _, ok = st.batch.decrypt(st.inputs[1], st.inputs[2], **kw)
    return st.out, ok, st.batch.tags


CASES = [
    Case("GcmMkBatch.encrypt", ("GcmMkBatch",), _batch_make(False, 256, 16), _encrypt, _encrypt_ref,
         family="gcm mk batch", want_impl="ttable"),
    Case("GcmMkBatch.encrypt aes128, 64 lanes", ("GcmMkBatch",), _batch_make(False, 128, 64), _encrypt, _encrypt_ref,
         family="gcm mk batch", want_impl="ttable"),
    Case("GcmMkBatch.encrypt(stream=s) from the default stream", ("GcmMkBatch",), _batch_make(False, 192, 16),
         lambda st: _on_default(st, lambda stream: _encrypt(st, stream=stream)), _encrypt_ref, family="gcm mk batch"),
    Case("GcmMkBatch.decrypt", ("GcmMkBatch",), _batch_make(True, 256, 16), _decrypt, _decrypt_ref,
         family="gcm mk batch", want_impl="ttable"),
    Case("GcmMkBatch.decrypt(stream=s) from the default stream", ("GcmMkBatch",), _batch_make(True, 128, 64),
         lambda st: _on_default(st, lambda stream: _decrypt(st, stream=stream)), _decrypt_ref, family="gcm mk batch"),
    Case("GcmMkBatch.ghash", ("GcmMkBatch",), _batch_make(False, 256, 16), lambda st: st.batch.ghash(), _hash_ref,
         family="gcm mk batch"),
    Case("GcmMkBatch.ghash(stream=s) from the default stream, 64 lanes", ("GcmMkBatch",), _batch_make(False, 128, 64),
         lambda st: _on_default(st, st.batch.ghash), _hash_ref, family="gcm mk batch"),
]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stream_contract(gpu, case):
    run_contract(case, gpu)


def test_every_op_of_the_module_has_a_row():
    """ops.gcm_mk_batch_ops' device ops are not in ops.__all__ (whose rows the other file keeps): their rows are
    here.  The plan-and-run-once functions plan (synchronising, as documented) and call the class, which has rows."""
    covered = {o for c in CASES for o in c.ops}
    assert {"GcmMkBatch"} <= covered and hasattr(MK, "GcmMkBatch")
    assert not {"GcmMkBatch", "ghash_mk_batch", "gcm_mk_encrypt_batch", "gcm_mk_decrypt_batch"} & set(ops.__all__)
    assert not [c.name for c in CASES if c.syncs]  # nothing here documents a readback
