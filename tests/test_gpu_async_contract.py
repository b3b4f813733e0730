"""The stream contract of every device op (docs/API.md section 2: "device
pointers, asynchronous on a caller-supplied ``hipStream_t``"): an op runs in
the order of the stream it is given, and enqueuing it makes the host wait for
nothing.

``run_contract`` puts pending work in front of an op -- one sleeping wave
(``ops.clock_probe``) that holds a fresh, non-default stream for ``DELAY``
seconds -- and enqueues behind it, without any host wait in between, the
copies that PRODUCE the op's device inputs, the op itself, and copies that
CONSUME every device result.  Then:

* order: the consumed bytes equal the CPU oracle over the late inputs.  An op
  (or one of its 2-6 launches, or a staging copy) on another stream runs while
  the delay still holds the producers back and shows the result of the stale
  inputs; a consumer that does not wait for the op's last launch shows the
  fill pattern;
* no host wait: right after the last enqueue the event recorded behind the
  delay has not fired.  A hidden ``hipStreamSynchronize``, a blocking
  ``hipMemcpy`` or a ``.cpu()`` anywhere in the call returns only after it.

``DELAY`` is a condition, not a measurement: it has to be long against the
host cost of enqueuing one case, and the helper checks that itself
(``t_enqueue < DELAY / 4``, else the case fails as inconclusive).

The helper's own tests come first; they run plain torch ops, never a kernel
of the project's, and touch nothing outside initialised buffers.  The table
``CASES`` has one row per op and launch chain; ``test_every_op_has_a_row``
(no GPU needed) keeps it complete.  ``test_two_calls_released_together``
releases two chains of calls of one family on two streams at the same instant:
calls that shared a table, a workspace or a claim word would corrupt each
other.  ``test_back_to_back_calls_do_not_wait`` enqueues three calls of one
family behind the delay: the row "ctr32 bitslice across the wrap" found that
the second of two bitsliced launches waited on the host for the first (the
runtime's hipFreeAsync, see otc_device.h ws_alloc), and so did every second
call of any family with a per-call workspace.
``test_a_call_does_not_wait_for_another_stream`` holds the other side of that
fix: a kept workspace never chains one stream behind another's pending work."""
import ctypes
import dataclasses
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from our_tree_amd import _native, ops
from our_tree_amd.models import cpu_ref
from our_tree_amd.parallel import jobs

DELAY = 0.3      # seconds the pending work in front of every case runs
WINDOW = 0.001   # clock_probe's measuring window behind the delay
A5, Z5 = 0xA5, 0x5A  # fill of the outputs / of the consumer's buffers before the run

TASK = 2048 * 16  # bytes of one bitsliced task (aes_bs.hip)
UNIT = 2048 * 16  # bytes of one claim unit (otc_device.h CLAIM_UNIT)
MIB = 1 << 20


def hostb(t: torch.Tensor) -> bytes:
    return t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def rnd(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def dev(b: bytes, gpu, shape=None) -> torch.Tensor:
    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if b else torch.empty(0, dtype=torch.uint8, device=gpu)
    return t if shape is None else t.view(shape)


def bxor(a: bytes, b: bytes) -> bytes:
    return (np.frombuffer(a, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes()


@dataclasses.dataclass
class Case:
    """One row.  ``make(gpu)`` -> a namespace with ``inputs`` (every device
    tensor the op reads, holding seeded stale bytes), ``fresh`` (equally
    shaped, other seeded bytes), ``outs`` (every tensor the op writes that is
    not an input: filled with 0xA5 before the run) and whatever the call
    needs besides (``out``, a planned batch); the helper adds ``stream``.
    ``call(st)`` -> the op's results, device tensors (consumed by a copy on
    the stream) or host ``bytes``.  ``ref(st, *fresh_host_bytes)`` -> the
    expected bytes of every result from the CPU oracle.  ``syncs``: the op
    documents a readback, so only its order is checked.  ``inplace``: indices
    of the inputs the op overwrites.  ``want_impl``: what ``last_impl()`` must
    report after the warm-up.  ``check(st)``: host-side state to compare."""
    name: str
    ops: tuple
    make: callable
    call: callable
    ref: callable
    family: str = ""
    syncs: bool = False
    inplace: tuple = ()
    want_impl: str = None
    check: callable = None


def _first_diff(got: bytes, exp: bytes) -> str:
    g, e = np.frombuffer(got, dtype=np.uint8), np.frombuffer(exp, dtype=np.uint8)
    idx = np.nonzero(g != e)[0]
    return f"{idx.size} of {g.size} bytes differ, from +{int(idx[0])} to +{int(idx[-1])}"


def independent_stream(gpu, other=None, tries=12):
    """A fresh stream that does not share its hardware queue with ``other``
    (default: the default, null stream).  A process's streams are dealt onto
    a few hardware queues; a launch that went to the null stream by mistake
    -- a forgotten ``stream`` argument -- simply waits behind the delay if the
    two share a queue, and every fourth case would miss it.  Probed with a
    5 ms delay on the candidate: work on the other stream finishes while it
    still runs."""
    default = torch.cuda.default_stream(gpu) if other is None else other
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    for _ in range(tries):
        s = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(s):  # the probe's result tensor is zeroed on the current stream
            probe = ops.clock_probe(0.005, WINDOW, stream=s)
        behind = torch.cuda.Event()
        behind.record(s)
        with torch.cuda.stream(default):
            flag.add_(1)
        done = torch.cuda.Event()
        done.record(default)
        done.synchronize()
        independent = not behind.query()
        s.synchronize()
        del probe
        if independent:
            return s
    raise AssertionError(f"none of {tries} fresh streams runs independently of the other stream: the order checks "
                         f"prove nothing on this machine")


def run_contract(case: Case, gpu, log=print) -> dict:
    """Steps 1-6 of the module docstring for one case; raises AssertionError."""
    st = case.make(gpu)
    stale = [t.clone() for t in st.inputs]
    fresh_host = [hostb(t) for t in st.fresh]
    expect = [bytes(e) for e in case.ref(st, *fresh_host)]  # before anything is enqueued
    zs = [torch.empty(len(e), dtype=torch.uint8, device=gpu) for e in expect]
    s = independent_stream(gpu)
    st.stream = s
    torch.cuda.synchronize()

    def enqueue(delay):
        """The delay, producers, the op, consumers on ``s`` with no host wait
        in between; -> (results, whether the delay was still running at the
        end, the probe's tensor to keep alive)."""
        with torch.cuda.stream(s):
            probe = ops.clock_probe(delay, WINDOW, stream=s)
            e_d = torch.cuda.Event()
            e_d.record(s)
            for inp, f in zip(st.inputs, st.fresh):
                inp.copy_(f)
            res = case.call(st)
            res = list(res) if isinstance(res, (list, tuple)) else [res]
            assert len(res) == len(expect), f"{case.name}: {len(res)} results, the reference has {len(expect)}"
            for r, z, e in zip(res, zs, expect):
                if isinstance(r, torch.Tensor):
                    assert r.numel() * r.element_size() == len(e), (case.name, tuple(r.shape), len(e))
                    z.copy_(r.reshape(-1).view(torch.uint8))
            waiting = not e_d.query()
        return res, waiting, probe

    try:
        # 1. warm-up, twice: the first run loads code objects, creates auxiliary
        # streams and fills the allocator caches of ``s``; the second is timed
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            enqueue(0.0)
            times.append(time.perf_counter() - t0)
            s.synchronize()
        t_enqueue = times[1]
        log(f"t_enqueue [{case.family}] {case.name}: {t_enqueue * 1e3:.3f} ms (first run {times[0] * 1e3:.3f} ms, "
            f"limit DELAY / 4 = {DELAY / 4 * 1e3:.0f} ms)")
        if times[0] >= DELAY:  # even cold, an enqueue must not come near the delay
            raise AssertionError(f"{case.name}: inconclusive: the first host enqueue took {times[0] * 1e3:.1f} ms, "
                                 f"as long as the {DELAY * 1e3:.0f} ms delay")
        if t_enqueue >= DELAY / 4:
            raise AssertionError(f"{case.name}: inconclusive: host enqueue took {t_enqueue * 1e3:.1f} ms, not short "
                                 f"against the {DELAY * 1e3:.0f} ms delay (limit {DELAY / 4 * 1e3:.0f} ms)")
        if case.want_impl is not None:
            assert ops.last_impl() == case.want_impl, (case.name, ops.last_impl(), ops.split_fallback_reason())
        if case.check is not None:
            case.check(st)

        # 2. reset
        for inp, o in zip(st.inputs, stale):
            inp.copy_(o)
        for o in st.outs:
            o.fill_(A5)
        for z in zs:
            z.fill_(Z5)
        # the blocks that the warm-up's temporaries (staging copies of misaligned views) left in the
        # allocator's cache of ``s`` still hold the fresh bytes: a mis-streamed kernel reading such a
        # block before its copy has run would find the right input there.  Overwrite them.
        with torch.cuda.stream(s):
            junk = [torch.empty_like(t).fill_(0x3C) for _ in range(2) for t in list(st.inputs) + zs]
            del junk
        torch.cuda.synchronize()

        # 3. + 4. enqueue behind the delay; is the delay still running?
        res, waiting, probe = enqueue(DELAY)
        s.synchronize()

        # 5. order
        stale_ref = None
        for i, (r, z, e) in enumerate(zip(res, zs, expect)):
            got = hostb(z) if isinstance(r, torch.Tensor) else bytes(r)
            if got == e:
                continue
            if stale_ref is None:
                stale_ref = [bytes(b) for b in case.ref(st, *[hostb(t) for t in stale])]
            if got == stale_ref[i]:
                why = "it is the result of the stale inputs: the op ran before its input was produced"
            elif any(got == fresh_host[k] for k in case.inplace):
                why = "it is what the producer wrote over the op's own result: the op ran before its input was produced"
            elif got and set(got) <= {Z5}:
                why = "the consumer's buffer still holds 0x5A: the consumer ran before the op finished (or never ran)"
            elif got and set(got) <= {A5}:
                why = "it still holds the 0xA5 fill: the consumer ran before the op finished"
            else:
                why = "neither the stale result nor a fill pattern: " + (_first_diff(got, e) if len(got) == len(e) else
                                                                         f"{len(got)} bytes for {len(e)}")
            raise AssertionError(f"{case.name}: order: result {i} differs from the reference; {why}")
        for i, (inp, f) in enumerate(zip(st.inputs, st.fresh)):
            if i not in case.inplace:
                assert torch.equal(inp, f), f"{case.name}: order: input {i} no longer holds what its producer wrote"
        if case.check is not None:
            case.check(st)

        # 6. no host wait
        if not case.syncs:
            assert waiting, (f"{case.name}: host wait: the pending work in front of the call had finished when the "
                             f"enqueue returned -- the call (or the copies around it) waited for the stream")
        return {"t_enqueue": t_enqueue, "waiting": waiting}
    finally:
        torch.cuda.synchronize()  # nothing is in flight when the buffers go


# ---- the helper's own tests: plain torch ops ------------------------------------

def std_make(*shapes, out=True, seed=0):
    """Inputs of these shapes (ints: flat byte counts), and an output of the first one's size."""
    def make(gpu):
        st = SimpleNamespace()
        size = [int(np.prod(sh)) for sh in shapes]
        st.inputs = [dev(rnd(n, 1000 + seed + i), gpu, sh) for i, (n, sh) in enumerate(zip(size, shapes))]
        st.fresh = [dev(rnd(n, 2000 + seed + i), gpu, sh) for i, (n, sh) in enumerate(zip(size, shapes))]
        st.out = torch.empty(size[0], dtype=torch.uint8, device=gpu) if out else None
        st.outs = [st.out] if out else []
        return st
    return make


def _torch_xor(st):
    st.out.copy_(st.inputs[0] ^ 0x5C)
    return st.out


def _torch_case(call=_torch_xor, name="torch xor"):
    return Case(name, ("torch",), std_make(4099), call, lambda st, x: [bxor(x, b"\x5c" * len(x))])


@pytest.mark.gpu
def test_helper_accepts_a_correct_op(gpu):
    r = run_contract(_torch_case(), gpu)
    assert r["waiting"] and r["t_enqueue"] < DELAY / 4


@pytest.mark.gpu
def test_helper_rejects_a_misstreamed_op(gpu):
    """The same op on a side stream that does not wait for ``s``.  Streams
    share a few hardware queues: a side stream that lands on the queue of ``s``
    simply waits behind the delay, so up to three fresh ones are tried."""
    rejected = 0
    for _ in range(3):
        side = torch.cuda.Stream(device=gpu)

        def call(st, side=side):
            with torch.cuda.stream(side):
                _torch_xor(st)
            return st.out

        try:
            run_contract(_torch_case(call, "mis-streamed torch xor"), gpu)
        except AssertionError as e:
            assert "order: result 0" in str(e) and "ran before its input was produced" in str(e), str(e)
            rejected += 1
            break
    assert rejected, ("no independent side stream ran ahead of the delayed stream in 3 attempts: the order checks of "
                      "this file prove nothing on this machine")


@pytest.mark.gpu
def test_helper_rejects_a_host_wait(gpu):
    def call(st):
        _torch_xor(st)
        torch.cuda.current_stream().synchronize()
        return st.out

    with pytest.raises(AssertionError, match="host wait: the pending work in front of the call had finished"):
        run_contract(_torch_case(call, "synchronising torch xor"), gpu)


@pytest.mark.gpu
def test_helper_rejects_a_slow_enqueue_as_inconclusive(gpu):
    def call(st):
        time.sleep(DELAY / 4)
        return _torch_xor(st)

    with pytest.raises(AssertionError, match="inconclusive: host enqueue took"):
        run_contract(_torch_case(call, "slow torch xor"), gpu)


# ---- the table ------------------------------------------------------------------

K128 = bytes(range(0x10, 0x20))
K256 = bytes(range(0x60, 0x80))
XTS_KEY = K256 + bytes(range(0x80, 0xA0))
IV = bytes(range(0xA0, 0xB0))
CTR_HI = bytes.fromhex("0123456789abcdef")
CTR0 = CTR_HI + (0x5A5A5A5A00000FFD).to_bytes(8, "big")
CTR_BS = CTR_HI + (0x5A5A5A5A00000801).to_bytes(8, "big")  # low half = 1 (mod 2048): a masked head, an edge task
CTR32_WRAP = bytes(range(0x30, 0x3C)) + (0xFFFFFFF0).to_bytes(4, "big")  # wraps 16 blocks into the call
NONCE4, IVEC8 = bytes.fromhex("c0c1c2c3"), bytes.fromhex("d0d1d2d3d4d5d6d7")
GCM_IV = bytes(range(0x40, 0x4C))
AAD13 = bytes(range(13))
GHASH_H = bytes.fromhex("66e94bd4ef8a2c3b884cfa59ca342b2e")
CC_KEY = bytes(range(101, 133))
CC_NONCE = bytes(range(0xC0, 0xCC))
POLY_KEY = bytes((i * 37 + 11) & 0xFF for i in range(32))
TWEAK0 = 0x0123456789ABCDEF


def one(name, op, n, f, ref, **kw):
    """An op of one data input and an ``out=`` buffer: ``f(x, out)``, ``ref(host bytes)``."""
    return Case(name, (op,), std_make(n), lambda st: f(st.inputs[0], st.out), lambda st, x: [ref(x)], **kw)


def _view_make(n):
    def make(gpu):
        st = SimpleNamespace()
        st.buf = dev(rnd(n + 16, 1100), gpu)
        st.buf2 = torch.empty(n + 16, dtype=torch.uint8, device=gpu)
        st.inputs, st.fresh = [st.buf[3:3 + n]], [dev(rnd(n, 2100), gpu)]
        st.out, st.outs = st.buf2[5:5 + n], [st.buf2]
        return st
    return make


def _aead_dec_make(n, seal):
    """A ciphertext produced late and its tag (host bytes, as received): ``seal(pt) -> (ct, tag)``."""
    def make(gpu):
        st = std_make(n)(gpu)
        ct, st.tag = seal(rnd(n, 2200))
        st.fresh = [dev(ct, gpu)]
        return st
    return make


N_TT = 4096 * 16 + 5
N_BS_CTR = 3 * TASK + 37 * 16 + 5
N_ECB_TT = 4097 * 16
N_ECB_BS = 5 * UNIT + 300 * 16  # claimed units, and a remainder for the T-table kernel
N_SPLIT = 16 * 2048 * 40 + 48  # the degenerate split of test_split_after_release_resources
SEG, NSEG = 512, 300
N_HASH = 65541

CASES = [
    one("ctr ttable aes128", "ctr", N_TT, lambda x, o: ops.ctr(x, K128, CTR0, out=o, impl="ttable"),
        lambda x: cpu_ref.ctr(K128, CTR0, x), want_impl="ttable"),
    one("ctr bitslice", "ctr", N_BS_CTR, lambda x, o: ops.ctr(x, K256, CTR_BS, out=o, impl="bitslice"),
        lambda x: cpu_ref.ctr(K256, CTR_BS, x), want_impl="bitslice"),
    Case("ctr misaligned views", ("ctr",), _view_make(N_TT),
         lambda st: (ops.ctr(st.inputs[0], K256, CTR0, out=st.out), st.buf2)[1],
         lambda st, x: [bytes([A5]) * 5 + cpu_ref.ctr(K256, CTR0, x) + bytes([A5]) * 11]),
    one("ctr_rfc3686", "ctr_rfc3686", 16 * 300 + 3, lambda x, o: ops.ctr_rfc3686(x, K256, NONCE4, IVEC8, out=o),
        lambda x: cpu_ref.ctr(K256, NONCE4 + IVEC8 + b"\x00\x00\x00\x01", x)),  # no 64-bit wrap: the 128-bit oracle
    one("ctr32 ttable across the wrap", "ctr32", 4096 + 3,
        lambda x, o: ops.ctr32(x, K256, CTR32_WRAP, out=o, impl="ttable"), lambda x: cpu_ref.ctr32(K256, CTR32_WRAP, x),
        want_impl="ttable"),
    one("ctr32 bitslice across the wrap", "ctr32", 4096 + 3,
        lambda x, o: ops.ctr32(x, K256, CTR32_WRAP, out=o, impl="bitslice"),
        lambda x: cpu_ref.ctr32(K256, CTR32_WRAP, x), want_impl="bitslice"),  # the call's second launch reports it
]

_BLOCK_MODES = [
    ("ecb_encrypt", lambda x, o, i: ops.ecb_encrypt(x, K256, out=o, impl=i), lambda x: cpu_ref.ecb(K256, x)),
    ("ecb_decrypt", lambda x, o, i: ops.ecb_decrypt(x, K256, out=o, impl=i),
     lambda x: cpu_ref.ecb(K256, x, decrypt=True)),
    ("cbc_decrypt", lambda x, o, i: ops.cbc_decrypt(x, K256, IV, out=o, impl=i),
     lambda x: cpu_ref.cbc(K256, IV, x, decrypt=True)),
    ("cfb128_decrypt", lambda x, o, i: ops.cfb128_decrypt(x, K256, IV, out=o, impl=i),
     lambda x: cpu_ref.cfb128(K256, IV, x, decrypt=True)),
]
for _impl, _n in (("ttable", N_ECB_TT), ("bitslice", N_ECB_BS)):
    for _op, _f, _ref in _BLOCK_MODES:
        CASES.append(one(f"{_op} {_impl}", _op, _n, lambda x, o, f=_f, i=_impl: f(x, o, i), _ref, want_impl=_impl))


def _split_check(st):
    assert ops.split_fallback_reason() == "", ops.split_fallback_reason()


CASES.append(one("ecb_encrypt split", "ecb_encrypt", N_SPLIT,
                 lambda x, o: ops.ecb_encrypt(x, K256, out=o, impl="split"), lambda x: cpu_ref.ecb(K256, x),
                 want_impl="split", check=_split_check))

CASES += [
    one("cbc_encrypt_segments", "cbc_encrypt_segments", SEG * NSEG,
        lambda x, o: ops.cbc_encrypt_segments(x, K256, IV, SEG, out=o), lambda x: cpu_ref.cbc_segments(K256, IV, x, SEG)),
    one("cfb128_encrypt_segments", "cfb128_encrypt_segments", SEG * NSEG,
        lambda x, o: ops.cfb128_encrypt_segments(x, K256, IV, SEG, out=o),
        lambda x: cpu_ref.cfb128_segments(K256, IV, x, SEG)),
    one("cbc_decrypt_segments", "cbc_decrypt_segments", SEG * NSEG,
        lambda x, o: ops.cbc_decrypt_segments(x, K256, IV, SEG, out=o),
        lambda x: cpu_ref.cbc_segments(K256, IV, x, SEG, decrypt=True)),
    one("cfb128_decrypt_segments", "cfb128_decrypt_segments", SEG * NSEG,
        lambda x, o: ops.cfb128_decrypt_segments(x, K256, IV, SEG, out=o),
        lambda x: cpu_ref.cfb128_segments(K256, IV, x, SEG, decrypt=True)),
    one("xts_encrypt 17 units", "xts_encrypt", 17 * 4096, lambda x, o: ops.xts_encrypt(x, XTS_KEY, TWEAK0, 4096, out=o),
        lambda x: cpu_ref.xts(XTS_KEY, TWEAK0, x, 4096)),
    one("xts_decrypt 17 units", "xts_decrypt", 17 * 4096, lambda x, o: ops.xts_decrypt(x, XTS_KEY, TWEAK0, 4096, out=o),
        lambda x: cpu_ref.xts(XTS_KEY, TWEAK0, x, 4096, decrypt=True)),
    one("xts_encrypt one unit, stealing", "xts_encrypt", 4096 + 15,
        lambda x, o: ops.xts_encrypt(x, XTS_KEY, TWEAK0, None, out=o), lambda x: cpu_ref.xts(XTS_KEY, TWEAK0, x)),
    Case("ghash", ("ghash",), std_make(N_HASH, out=False), lambda st: ops.ghash(st.inputs[0], GHASH_H),
         lambda st, x: [cpu_ref.ghash(GHASH_H, x)]),
    Case("gcm_encrypt", ("gcm_encrypt",), std_make(N_HASH),
         lambda st: ops.gcm_encrypt(st.inputs[0], K256, GCM_IV, AAD13, out=st.out),
         lambda st, x: list(cpu_ref.gcm(K256, GCM_IV, x, AAD13))),
    Case("gcm_decrypt", ("gcm_decrypt",), _aead_dec_make(N_HASH, lambda pt: cpu_ref.gcm(K256, GCM_IV, pt, AAD13)),
         lambda st: ops.gcm_decrypt(st.inputs[0], K256, GCM_IV, st.tag, AAD13, out=st.out),
         lambda st, x: [cpu_ref.gcm(K256, GCM_IV, x, AAD13, decrypt=True)[0]], syncs=True),
    one("chacha20", "chacha20", 65536 + 77, lambda x, o: ops.chacha20(x, CC_KEY, CC_NONCE, 3, out=o),
        lambda x: cpu_ref.chacha20(CC_KEY, CC_NONCE, x, 3)),
    Case("poly1305", ("poly1305",), std_make(N_HASH, out=False), lambda st: ops.poly1305(st.inputs[0], POLY_KEY),
         lambda st, x: [cpu_ref.poly1305(POLY_KEY, x)]),
    Case("chacha20_poly1305_encrypt", ("chacha20_poly1305_encrypt",), std_make(N_HASH),
         lambda st: ops.chacha20_poly1305_encrypt(st.inputs[0], CC_KEY, CC_NONCE, AAD13, out=st.out),
         lambda st, x: list(cpu_ref.chacha20_poly1305(CC_KEY, CC_NONCE, x, AAD13))),
    Case("chacha20_poly1305_decrypt", ("chacha20_poly1305_decrypt",),
         _aead_dec_make(N_HASH, lambda pt: cpu_ref.chacha20_poly1305(CC_KEY, CC_NONCE, pt, AAD13)),
         lambda st: ops.chacha20_poly1305_decrypt(st.inputs[0], CC_KEY, CC_NONCE, st.tag, AAD13, out=st.out),
         lambda st, x: [cpu_ref.chacha20_poly1305(CC_KEY, CC_NONCE, x, AAD13, decrypt=True)[0]], syncs=True),
]


# -- planned batches: the plan is made before the delay, the data comes late --

def _slots(lens):
    """Back-to-back 16-byte aligned slots: (offsets, total)."""
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += (n + 15) // 16 * 16
    return offs, at


def _on_default(st, f):
    """Call ``f(stream=s)`` with the DEFAULT stream current, as a caller that hands a stream over would."""
    with torch.cuda.stream(torch.cuda.default_stream(st.stream.device)):
        return f(stream=st.stream)


CB_LENS = [4096, 777, 12288]
CB_KEYS, CB_KIDX = [K128, K256], [0, 1, 0]
CB_CTRS = [CTR0, CTR_BS, CTR_HI + (2**64 - 3).to_bytes(8, "big")]  # the last one carries into the high half
CB_OFFS, CB_TOTAL = _slots(CB_LENS)


def _ctr_batch_make(gpu):
    st = std_make(CB_TOTAL)(gpu)  # the messages are views of one pool, the outputs of st.out: gaps stay 0xA5
    xs = [st.inputs[0][o:o + n] for o, n in zip(CB_OFFS, CB_LENS)]
    outs = [st.out[o:o + n] for o, n in zip(CB_OFFS, CB_LENS)]
    st.batch = ops.CtrBatch(xs, CB_KEYS, CB_CTRS, outs=outs, key_index=CB_KIDX)
    return st


def _ctr_batch_ref(st, pool):
    exp = bytearray([A5]) * CB_TOTAL
    for o, n, c, k in zip(CB_OFFS, CB_LENS, CB_CTRS, CB_KIDX):
        exp[o:o + n] = cpu_ref.ctr(CB_KEYS[k], c, pool[o:o + n])
    return [bytes(exp)]


CASES += [
    Case("CtrBatch.run()", ("CtrBatch",), _ctr_batch_make, lambda st: (st.batch.run(), st.out)[1], _ctr_batch_ref),
    Case("CtrBatch.run(stream=s) from the default stream", ("CtrBatch",), _ctr_batch_make,
         lambda st: (_on_default(st, st.batch.run), st.out)[1], _ctr_batch_ref),
]

GB_N = 37
GB_LENS = [1, 4096] + [(i * 331 + 7) % 4096 + 1 for i in range(GB_N - 2)]
GB_OFFS, GB_DATA = _slots(GB_LENS)
GB_AAD_LENS = [5 + m if m % 3 == 1 else 0 for m in range(GB_N)]  # device AADs, packed from an odd address
GB_AAD_OFFS = [GB_DATA + 1 + sum(GB_AAD_LENS[:m]) for m in range(GB_N)]
GB_POOL = GB_DATA + 1 + sum(GB_AAD_LENS)
GB_FORGED = 5  # decrypt: this record's received tag is wrong


def _gb_aad(pool: bytes, m: int) -> bytes:
    """Record m's AAD: host bytes (m % 3 == 0), a device view of the pool (1) or none (2)."""
    if m % 3 == 0:
        return bytes((m + i) & 0xFF for i in range(13))
    return pool[GB_AAD_OFFS[m]:GB_AAD_OFFS[m] + GB_AAD_LENS[m]]


def _gb_records(pool: bytes, ivs: bytes):
    for m, (o, n) in enumerate(zip(GB_OFFS, GB_LENS)):
        yield m, o, n, pool[o:o + n], ivs[12 * m:12 * m + 12], _gb_aad(pool, m)


def _gcm_batch_make(decrypt):
    def make(gpu):
        st = std_make(GB_POOL, (GB_N, 12), (GB_N, 16))(gpu)
        if decrypt:  # the late inputs are valid ciphertexts and their tags, but for one forgery
            pool, ivs = bytearray(hostb(st.fresh[0])), hostb(st.fresh[1])
            tags = bytearray()
            for m, o, n, pt, iv, aad in _gb_records(bytes(pool), ivs):
                pool[o:o + n], t = cpu_ref.gcm(K256, iv, pt, aad)
                tags += t
            tags[16 * GB_FORGED + 3] ^= 0x10
            st.fresh = [dev(bytes(pool), gpu), st.fresh[1], dev(bytes(tags), gpu, (GB_N, 16))]
        else:
            st.inputs, st.fresh = st.inputs[:2], st.fresh[:2]
        x = st.inputs[0]
        xs = [x[o:o + n] for o, n in zip(GB_OFFS, GB_LENS)]
        outs = [st.out[o:o + n] for o, n in zip(GB_OFFS, GB_LENS)]
        aads = [_gb_aad(b"", m) if m % 3 == 0 else x[GB_AAD_OFFS[m]:GB_AAD_OFFS[m] + GB_AAD_LENS[m]] if m % 3 == 1
                else None for m in range(GB_N)]
        st.batch = ops.GcmBatch(xs, K256, outs=outs, aads=aads)
        st.outs = [st.out, st.batch.tags, st.batch.ok]
        return st
    return make


def _gb_encrypt_ref(st, pool, ivs):
    exp, tags = bytearray([A5]) * GB_POOL, bytearray()
    for m, o, n, pt, iv, aad in _gb_records(pool, ivs):
        exp[o:o + n], t = cpu_ref.gcm(K256, iv, pt, aad)
        tags += t
    return [bytes(exp), bytes(tags)]


def _gb_decrypt_ref(st, pool, ivs, tags):
    exp, ok, computed = bytearray([A5]) * GB_POOL, bytearray(), bytearray()
    for m, o, n, ct, iv, aad in _gb_records(pool, ivs):
        pt, t = cpu_ref.gcm(K256, iv, ct, aad, decrypt=True)
        good = t == tags[16 * m:16 * m + 16]
        exp[o:o + n] = pt if good else bytes(n)  # a failed record is zeroed, and so is its computed tag
        computed += t if good else bytes(16)
        ok.append(int(good))
    return [bytes(exp), bytes(ok), bytes(computed)]


def _gb_hash_ref(st, pool, ivs):
    h, out = cpu_ref.gcm_h(K256), bytearray()
    for m, o, n, x, iv, aad in _gb_records(pool, ivs):
        out += cpu_ref.ghash(h, aad + bytes(-len(aad) % 16) + x + bytes(-n % 16) + (8 * len(aad)).to_bytes(8, "big") +
                             (8 * n).to_bytes(8, "big"))
    return [bytes(out)]


def _gb_encrypt(st, **kw):
    st.batch.encrypt(st.inputs[1], **kw)
    return st.out, st.batch.tags


def _gb_decrypt(st, **kw):
    _, ok = st.batch.decrypt(st.inputs[1], st.inputs[2], **kw)
    return st.out, ok, st.batch.tags


CASES += [
    Case("GcmBatch.encrypt", ("GcmBatch",), _gcm_batch_make(False), _gb_encrypt, _gb_encrypt_ref),
    Case("GcmBatch.encrypt(stream=s) from the default stream", ("GcmBatch",), _gcm_batch_make(False),
         lambda st: _on_default(st, lambda stream: _gb_encrypt(st, stream=stream)), _gb_encrypt_ref),
    Case("GcmBatch.decrypt", ("GcmBatch",), _gcm_batch_make(True), _gb_decrypt, _gb_decrypt_ref),
    Case("GcmBatch.decrypt(stream=s) from the default stream", ("GcmBatch",), _gcm_batch_make(True),
         lambda st: _on_default(st, lambda stream: _gb_decrypt(st, stream=stream)), _gb_decrypt_ref),
    Case("GcmBatch.ghash", ("GcmBatch",), _gcm_batch_make(False), lambda st: st.batch.ghash(), _gb_hash_ref),
    Case("GcmBatch.ghash(stream=s) from the default stream", ("GcmBatch",), _gcm_batch_make(False),
         lambda st: _on_default(st, st.batch.ghash), _gb_hash_ref),
]


# -- the resumable stream: 5 bytes before the delay, 4099 behind it (head from the kept block, body, tail) --

CS_FIRST, CS_N = 5, 4099


def _ctr_stream_make(gpu):
    st = std_make(CS_N)(gpu)
    first = rnd(CS_FIRST, 1300)
    s0 = ops.CtrStream(K256, CTR0)
    s0.update(dev(first, gpu))
    st.state0 = s0.state()
    nc, sb, off = bytearray(CTR0), bytearray(16), [0]
    cpu_ref.ctr_stream(K256, nc, sb, off, first)
    assert (st.state0["nonce_counter"], st.state0["stream_block"], st.state0["nc_off"]) == (bytes(nc), bytes(sb), off[0])
    st.oracle0 = (bytes(nc), bytes(sb), off[0])
    cpu_ref.ctr_stream(K256, nc, sb, off, hostb(st.fresh[0]))
    st.ctx_expect = (bytes(nc), bytes(sb), off[0])
    return st


def _ctr_stream_call(st):
    st.cs = ops.CtrStream.from_state(K256, st.state0)  # the context is host state: every run resumes the same one
    return st.cs.update(st.inputs[0], out=st.out)


def _ctr_stream_ref(st, x):
    nc, sb, off = bytearray(st.oracle0[0]), bytearray(st.oracle0[1]), [st.oracle0[2]]
    return [cpu_ref.ctr_stream(K256, nc, sb, off, x)]


def _ctr_stream_check(st):
    assert (st.cs.nonce_counter, st.cs.stream_block, st.cs.nc_off) == st.ctx_expect


# -- byte streams --

RC4_NS, RC4_LEN, RC4_DROP = 200, 35, 3


def _rc4_multi_ref(st, keys, x):
    ks = b"".join(cpu_ref.arc4_keystream(keys[16 * r:16 * r + 16], RC4_LEN, drop=RC4_DROP) for r in range(RC4_NS))
    return [bxor(x, ks)]


def _rc4_batch_make(gpu):
    st = std_make((RC4_NS, ops.stream_ops.RC4_STATE_BYTES), (RC4_NS, RC4_LEN))(gpu)
    keys = [[bytes((7 * r + 13 * i + seed) & 0xFF for i in range(1 + r % 32)) for r in range(RC4_NS)] for seed in (1, 2)]
    st.inputs[0], st.fresh[0] = ops.rc4_states(keys[0]).to(gpu), ops.rc4_states(keys[1]).to(gpu)
    st.out = torch.empty(RC4_NS * RC4_LEN, dtype=torch.uint8, device=gpu)
    st.outs = [st.out]
    return st


def _rc4_batch_ref(st, states, x):
    """rc4_crypt (rc4.h) from every state image: the outputs and the advanced states."""
    lib, nb = _native.cpu_lib(), ops.stream_ops.RC4_STATE_BYTES
    out, after = bytearray(), bytearray()
    for r in range(RC4_NS):
        s = _native.Rc4State.from_buffer_copy(states[nb * r:nb * r + nb])
        o = ctypes.create_string_buffer(RC4_LEN)
        lib.rc4_crypt(ctypes.byref(s), x[RC4_LEN * r:RC4_LEN * r + RC4_LEN], o, RC4_LEN)
        out += o.raw
        after += bytes(s)
    return [bytes(out), bytes(after)]


def _fill_make(gpu):
    st = std_make(4096 + 5)(gpu)
    # the op reads nothing, so the late producer overwrites the buffer it fills: a fill that ran early is lost
    st.inputs, st.fresh, st.outs = [st.out], [torch.full_like(st.out, 0x33)], []
    st.expect = hostb(ops.fill_random_(torch.empty_like(st.out), seed=77))  # the same fill, beforehand, default stream
    return st


def _checksum_ref(st, x):
    return [jobs.checksum(torch.frombuffer(bytearray(x), dtype=torch.uint8)).to_bytes(8, "little")]


CASES += [
    Case("CtrStream.update", ("CtrStream",), _ctr_stream_make, _ctr_stream_call, _ctr_stream_ref, check=_ctr_stream_check),
    Case("xor", ("xor",), std_make(MIB + 13, MIB + 13), lambda st: ops.xor(st.inputs[0], st.inputs[1], out=st.out),
         lambda st, a, b: [bxor(a, b)]),
    Case("rc4_multi", ("rc4_multi",), std_make((RC4_NS, RC4_LEN), (RC4_NS, 16)),
         lambda st: ops.rc4_multi(st.inputs[1], RC4_LEN, x=st.inputs[0], drop=RC4_DROP, out=st.out.view(RC4_NS, RC4_LEN)),
         lambda st, x, keys: _rc4_multi_ref(st, keys, x)),
    Case("rc4_crypt_batch", ("rc4_crypt_batch",), _rc4_batch_make,
         lambda st: (ops.rc4_crypt_batch(st.inputs[0], st.inputs[1], out=st.out.view(RC4_NS, RC4_LEN)), st.inputs[0]),
         _rc4_batch_ref, inplace=(0,)),
    Case("fill_random_", ("fill_random_",), _fill_make, lambda st: ops.fill_random_(st.out, seed=77),
         lambda st, x: [st.expect], inplace=(0,)),
    Case("checksum", ("checksum",), std_make(MIB, out=False),
         lambda st: ops.checksum(st.inputs[0]).to_bytes(8, "little"), _checksum_ref, syncs=True),
]

FAMILIES = {"ctr": "ctr", "ctr_rfc3686": "ctr", "ctr32": "ctr", "CtrStream": "ctr", "CtrBatch": "ctr batch",
            "ecb_encrypt": "ecb / cbc / cfb", "ecb_decrypt": "ecb / cbc / cfb", "cbc_decrypt": "ecb / cbc / cfb",
            "cfb128_decrypt": "ecb / cbc / cfb", "cbc_encrypt_segments": "segments", "cbc_decrypt_segments": "segments",
            "cfb128_encrypt_segments": "segments", "cfb128_decrypt_segments": "segments", "xts_encrypt": "xts",
            "xts_decrypt": "xts", "ghash": "gcm", "gcm_encrypt": "gcm", "gcm_decrypt": "gcm", "GcmBatch": "gcm batch",
            "chacha20": "chacha", "poly1305": "chacha", "chacha20_poly1305_encrypt": "chacha",
            "chacha20_poly1305_decrypt": "chacha", "xor": "stream ops", "rc4_multi": "stream ops",
            "rc4_crypt_batch": "stream ops", "fill_random_": "stream ops", "checksum": "stream ops"}
for _c in CASES:
    _c.family = FAMILIES[_c.ops[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name.replace(" ", "_") for c in CASES])
def test_stream_contract(gpu, case):
    run_contract(case, gpu)


# ---- completeness ---------------------------------------------------------------

EXEMPT = {
    "IMPLS": "a constant",
    "pick_impl": "a host-side query, launches nothing",
    "last_impl": "a host-side query, launches nothing",
    "split_fallback_reason": "a host-side query, launches nothing",
    "ghash_spans": "a host-side query, launches nothing",
    "gcm_batch_spans": "a host-side query, launches nothing",
    "poly1305_spans": "a host-side query, launches nothing",
    "expand_key": "host-side key schedule",
    "rc4_states": "host-side rc4_init into a CPU tensor",
    "clock_probe": "the delay itself: every case runs behind it",
    "clock_ghz": "reads a probe's result back by definition",
    "GcmTagError": "an exception class",
    "ChaChaTagError": "an exception class",
    "ctr_batch": "plans (host work, an upload) and calls CtrBatch.run, which has rows",
    "gcm_encrypt_batch": "plans (synchronising, as documented) and calls GcmBatch.encrypt, which has rows",
    "gcm_decrypt_batch": "plans (synchronising, as documented) and calls GcmBatch.decrypt, which has rows",
    "ghash_batch": "plans (synchronising, as documented) and calls GcmBatch.ghash, which has rows",
}


def test_every_op_has_a_row():
    """A name added to ``ops.__all__`` needs a row in CASES, or a reason here."""
    covered = {o for c in CASES for o in c.ops}
    names = set(ops.__all__)
    missing = sorted(n for n in names if n not in covered and n not in EXEMPT)
    assert not missing, f"no stream-contract row (and no EXEMPT reason) for: {missing}"
    assert not covered & set(EXEMPT), sorted(covered & set(EXEMPT))
    assert (covered | set(EXEMPT)) <= names, sorted((covered | set(EXEMPT)) - names)
    assert all(EXEMPT.values())
    assert len({c.name for c in CASES}) == len(CASES)


# ---- overlap: two chains of calls released at the same instant ------------------

OV_DELAY = 0.05
OV_CALLS = 4
OV_N = 4 * MIB
OV_KEYS = [K256, bytes(range(0xC0, 0xE0))]
OV_CTRS = [CTR_BS, CTR_HI + (0x1111111100000FFD).to_bytes(8, "big")]
OV_REC = 64 * 1024


_REFS = {}


def _once(key, f):
    """The oracle's answer for ``key``, computed once for the tests that share it."""
    if key not in _REFS:
        _REFS[key] = f()
    return _REFS[key]


def _ov_single(tag, n, f, ref, check=None):
    """A family of one data input: ``f(x, out, i)`` on stream i, ``ref(host bytes, i)`` -> the expected results."""
    def build(i, gpu):
        xh = rnd(n, 3000 + i)
        x = dev(xh, gpu)
        outs = [torch.full((n,), A5, dtype=torch.uint8, device=gpu) for _ in range(OV_CALLS + 1)]

        def call(j):
            r = f(x, outs[j], i)
            if check is not None:
                check()
            return list(r) if isinstance(r, (list, tuple)) else [r]

        exp = _once((tag, i), lambda: ref(xh, i))
        return SimpleNamespace(call=call, expect=list(exp) if isinstance(exp, (list, tuple)) else [exp], keep=(x, outs))
    return build


def _ov_split_check():
    assert ops.last_impl() == "split" and ops.split_fallback_reason() == "", (ops.last_impl(), ops.split_fallback_reason())


def _ov_ctr_batch(i, gpu):
    lens = [OV_REC] * (OV_N // OV_REC) + [777]
    offs, total = _slots(lens)
    xh = rnd(total, 3100 + i)
    x, out = dev(xh, gpu), torch.full((total,), A5, dtype=torch.uint8, device=gpu)
    ctrs = [cpu_ref.ctr128_add(OV_CTRS[i], 5000 * m) for m in range(len(lens))]
    keys = [OV_KEYS[i], K128]
    kidx = [m % 2 for m in range(len(lens))]
    b = ops.CtrBatch([x[o:o + n] for o, n in zip(offs, lens)], keys, ctrs, outs=[out[o:o + n] for o, n in zip(offs, lens)],
                     key_index=kidx)

    def ref():
        exp = bytearray([A5]) * total
        for o, n, c, k in zip(offs, lens, ctrs, kidx):
            exp[o:o + n] = cpu_ref.ctr(keys[k], c, xh[o:o + n])
        return [bytes(exp)]

    return SimpleNamespace(call=lambda j: (b.run(), [out])[1], expect=_once(("ctr batch", i), ref), wipe=[out], keep=(x, b))


def _ov_gcm_batch(i, gpu):
    lens = [OV_REC] * (OV_N // OV_REC) + [777]
    offs, total = _slots(lens)
    xh, ivh = rnd(total, 3200 + i), rnd(12 * len(lens), 3300 + i)
    x, out = dev(xh, gpu), torch.full((total,), A5, dtype=torch.uint8, device=gpu)
    ivs = dev(ivh, gpu, (len(lens), 12))
    aads = [bytes((m + k) & 0xFF for k in range(13)) if m % 2 else None for m in range(len(lens))]
    b = ops.GcmBatch([x[o:o + n] for o, n in zip(offs, lens)], OV_KEYS[i], outs=[out[o:o + n] for o, n in zip(offs, lens)],
                     aads=aads)

    def ref():
        exp, tags = bytearray([A5]) * total, bytearray()
        for m, (o, n) in enumerate(zip(offs, lens)):
            exp[o:o + n], t = cpu_ref.gcm(OV_KEYS[i], ivh[12 * m:12 * m + 12], xh[o:o + n], aads[m] or b"")
            tags += t
        return [bytes(exp), bytes(tags)]

    return SimpleNamespace(call=lambda j: (b.encrypt(ivs), [out, b.tags])[1], expect=_once(("gcm batch", i), ref),
                           wipe=[out, b.tags], keep=(x, ivs, b))


OVERLAP = {
    "ctr bitslice": _ov_single("ctr bitslice", OV_N + 37 * 16 + 5, lambda x, o, i: ops.ctr(x, OV_KEYS[i], OV_CTRS[i], out=o, impl="bitslice"),
                               lambda x, i: cpu_ref.ctr(OV_KEYS[i], OV_CTRS[i], x)),
    "ecb_encrypt bitslice": _ov_single("ecb_encrypt bitslice", OV_N + 300 * 16, lambda x, o, i: ops.ecb_encrypt(x, OV_KEYS[i], out=o, impl="bitslice"),
                                       lambda x, i: cpu_ref.ecb(OV_KEYS[i], x)),
    "ecb_encrypt split": _ov_single("ecb_encrypt split", N_SPLIT, lambda x, o, i: ops.ecb_encrypt(x, OV_KEYS[i], out=o, impl="split"),
                                    lambda x, i: cpu_ref.ecb(OV_KEYS[i], x), check=_ov_split_check),
    "ghash": _ov_single("ghash", OV_N + 5, lambda x, o, i: ops.ghash(x, OV_KEYS[i][:16]), lambda x, i: cpu_ref.ghash(OV_KEYS[i][:16], x)),
    "gcm_encrypt": _ov_single("gcm_encrypt", OV_N + 5, lambda x, o, i: ops.gcm_encrypt(x, OV_KEYS[i], GCM_IV, AAD13, out=o),
                              lambda x, i: cpu_ref.gcm(OV_KEYS[i], GCM_IV, x, AAD13)),
    "poly1305": _ov_single("poly1305", OV_N + 5, lambda x, o, i: ops.poly1305(x, OV_KEYS[i]), lambda x, i: cpu_ref.poly1305(OV_KEYS[i], x)),
    "chacha20_poly1305_encrypt": _ov_single(
        "chacha20_poly1305_encrypt", OV_N + 5, lambda x, o, i: ops.chacha20_poly1305_encrypt(x, OV_KEYS[i], CC_NONCE, AAD13, out=o),
        lambda x, i: cpu_ref.chacha20_poly1305(OV_KEYS[i], CC_NONCE, x, AAD13)),
    "two CtrBatches": _ov_ctr_batch,
    "two GcmBatches": _ov_gcm_batch,
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(OVERLAP), ids=[f.replace(" ", "_") for f in OVERLAP])
def test_two_calls_released_together(gpu, family):
    """Two streams wait for one event behind a short delay; each carries four
    calls of the family with its own key and data.  Both chains start when the
    delay ends, so the calls of the two streams very likely run on the chip
    together (not asserted: the test cannot fail falsely); every output must
    equal its oracle."""
    fams = [OVERLAP[family](i, gpu) for i in range(2)]
    streams = [torch.cuda.Stream(device=gpu) for _ in range(3)]
    torch.cuda.synchronize()
    try:
        for f, s in zip(fams, streams[1:]):  # warm-up into the spare output: code objects, pools, auxiliary streams
            with torch.cuda.stream(s):
                f.call(OV_CALLS)
        torch.cuda.synchronize()
        for f in fams:
            for t in getattr(f, "wipe", []):
                t.fill_(A5)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):  # the probe's result tensor is zeroed on the current stream
            probe = ops.clock_probe(OV_DELAY, WINDOW, stream=streams[0])
        go = torch.cuda.Event()
        go.record(streams[0])
        results = []
        for f, s in zip(fams, streams[1:]):
            s.wait_event(go)
            with torch.cuda.stream(s):
                results.append([f.call(j) for j in range(OV_CALLS)])
        torch.cuda.synchronize()
        del probe
        for i, (f, res) in enumerate(zip(fams, results)):
            for j, rs in enumerate(res):
                assert len(rs) == len(f.expect)
                for k, (r, e) in enumerate(zip(rs, f.expect)):
                    got = hostb(r)
                    assert len(got) == len(e), (family, i, j, k, len(got), len(e))
                    assert got == e, f"{family}: stream {i}, call {j}, result {k}: {_first_diff(got, e)}"
    finally:
        torch.cuda.synchronize()


# ---- calls enqueued back to back ------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("family", list(OVERLAP), ids=[f.replace(" ", "_") for f in OVERLAP])
def test_back_to_back_calls_do_not_wait(gpu, family):
    """Three calls of one family on one stream behind the delay.  The second
    call finds the first one's per-call workspace returned but still in use on
    the device: hipFreeAsync of a block that hipMallocAsync had handed out
    again while its earlier free was pending waited on the host for that
    earlier free, so every second call blocked until the first had run
    (otc_device.h ws_alloc).  Every output equals its oracle, and the delay
    is still running when the third call has returned."""
    f = OVERLAP[family](0, gpu)
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(s):
            for k in range(2):  # code objects, pools, auxiliary streams; then the timed run
                t0 = time.perf_counter()
                for _ in range(3):
                    f.call(OV_CALLS)
                t_enqueue = time.perf_counter() - t0
                s.synchronize()
        print(f"t_enqueue [back to back] {family}: {t_enqueue * 1e3:.3f} ms (limit DELAY / 4 = {DELAY / 4 * 1e3:.0f} ms)")
        assert t_enqueue < DELAY / 4, f"{family}: inconclusive: host enqueue took {t_enqueue * 1e3:.1f} ms"
        for t in getattr(f, "wipe", []):
            t.fill_(A5)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            probe = ops.clock_probe(DELAY, WINDOW, stream=s)
            e_d = torch.cuda.Event()
            e_d.record(s)
            res = [f.call(j) for j in range(3)]
            waiting = not e_d.query()
        s.synchronize()
        del probe
        for j, rs in enumerate(res):
            for k, (r, e) in enumerate(zip(rs, f.expect)):
                got = hostb(r)
                assert got == e, f"{family}: call {j}, result {k}: " + (_first_diff(got, e) if len(got) == len(e) else
                                                                       f"{len(got)} bytes for {len(e)}")
        assert waiting, f"{family}: host wait: one of three calls enqueued back to back waited for the stream"
    finally:
        torch.cuda.synchronize()


# ---- calls on two streams ---------------------------------------------------------

# The claimed forms of ECB (the split, and impl "bitslice") run on pooled auxiliary streams, and a
# pair goes back to the pool as soon as its work is enqueued (split.cpp aux_give): the next such
# call, from whatever stream, queues behind it by design.  They are not in this test.
OWN_STREAM = [f for f in OVERLAP if not f.startswith("ecb_encrypt")]


@pytest.mark.gpu
@pytest.mark.parametrize("family", OWN_STREAM, ids=[f.replace(" ", "_") for f in OWN_STREAM])
def test_a_call_does_not_wait_for_another_stream(gpu, family):
    """Stream A holds two calls of the family behind the delay, so whatever
    workspaces the library keeps between calls were last used by work that has
    not run yet.  A call of the same family on stream B (a hardware queue of
    its own) must finish while A's delay is still running: a workspace handed
    from one stream to another with a device-side wait would chain B behind
    everything queued on A."""
    fa, fb = (OVERLAP[family](i, gpu) for i in range(2))
    sa = independent_stream(gpu)
    sb = independent_stream(gpu, other=sa)
    torch.cuda.synchronize()
    try:
        for f, s in ((fa, sa), (fb, sb)):  # code objects, pools, auxiliary streams, kept workspaces
            with torch.cuda.stream(s):
                f.call(OV_CALLS)
        torch.cuda.synchronize()
        for t in getattr(fb, "wipe", []):
            t.fill_(A5)
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            probe = ops.clock_probe(DELAY, WINDOW, stream=sa)
            e_a = torch.cuda.Event()
            e_a.record(sa)
            for j in range(2):
                fa.call(j)
        with torch.cuda.stream(sb):
            res = fb.call(0)
            e_b = torch.cuda.Event()
            e_b.record(sb)
        e_b.synchronize()
        independent = not e_a.query()
        torch.cuda.synchronize()
        del probe
        for k, (r, e) in enumerate(zip(res, fb.expect)):
            got = hostb(r)
            assert got == e, f"{family}: result {k}: " + (_first_diff(got, e) if len(got) == len(e) else "wrong size")
        assert independent, f"{family}: the call on stream B finished only after the pending work on stream A"
    finally:
        torch.cuda.synchronize()
