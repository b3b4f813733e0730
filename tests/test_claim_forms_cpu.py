"""The plan of tests/claim_forms_child.py, checked without a GPU: every case's
shape is recomputed here from its byte count alone with the host formulas of
split.cpp (claim_alone, preassigned_back), engine.cpp (ctr_common,
seg_enc_run) and aes_tt.hip (tt_ctr_claim_units) --

    nunits = blocks / 2048            (CTR: ceil((blocks + ctr_lo % 4096) / 2048);
                                       segment encryption: segments / 64)
    pb      = min(nunits, 16 CUs)     units handed to the waves without a claim
    claimed = nunits - pb             units taken from the claim word
    past    = blocks - nunits * 2048  run by workgroup 0 (CTR: none)

-- and must reach what the case says it is there for, at 256, 304, 64 and 1
CUs.  The child's fast segment oracle is compared with cpu_ref's."""
import pytest

import claim_forms_child as child

CUS = (256, 304, 64, 1)
U = 2048 * 16
M64 = (1 << 64) - 1


def ctr_lo(c):
    """The low half of the first block's counter, as the engine computes it."""
    if c["kind"] == "ctr":
        return (int.from_bytes(child.COUNTER[8:], "big") + child.CTR_BLOCK_OFFSET) & M64
    assert child.RFC_IVEC[4:] == b"\xff" * 4
    return ((int.from_bytes(child.RFC_IVEC[4:], "big") << 32 | 1) + child.RFC_BLOCK_OFFSET) & M64  # engine.cpp otc_aes_ctr_rfc3686


def host_shape(c, cus):
    """(nunits, minimum, pb, claimed, past) of case c's call by the host formulas."""
    n = c["nbytes"]
    if c["kind"] == "segenc":
        assert n % c["seg"] == 0 and c["seg"] % 16 == 0
        total, unit, minimum = n // c["seg"], 64, 16
        nunits = total // unit
    elif c["kind"] in ("ctr", "rfc3686"):
        blocks = n // 16 + (1 if n % 16 else 0)
        total, unit, minimum = blocks + (ctr_lo(c) & 4095), 2048, 2
        nunits = (total + unit - 1) // unit
        total = nunits * unit  # rounded up: nothing past the last unit
    else:
        assert n % 16 == 0 and (not c["seg"] or n % c["seg"] == 0)
        total, unit, minimum = n // 16, 2048, 2
        nunits = total // unit
    pb = min(nunits, 16 * cus)
    return nunits, minimum, pb, nunits - pb, total - nunits * unit


@pytest.mark.parametrize("which", child.SETS)
@pytest.mark.parametrize("cus", CUS)
def test_plan_reaches_what_it_names(cus, which):
    cases = child.plan(cus, which)
    assert [c["name"] for c in cases] == [c["name"] for c in child.plan(256, which)], "case names depend on the CU count"
    assert len({c["name"] for c in cases}) == len(cases)
    w = 16 * cus
    for c in cases:
        nunits, minimum, pb, claimed, past = host_shape(c, cus)
        tags, form, ctx = set(c["reaches"]), c["form"], (cus, c["name"])
        assert tags, ctx
        assert c["units"] == nunits and c["set"] == which, ctx
        assert nunits <= 0x7FFFFFFF, ctx
        if which == "thresholds":  # every call claims if it can
            assert form == ("claim" if nunits >= minimum else "grid"), ctx
        else:                      # the defaults hold: no persistent T-table kernel below 512 MiB
            assert form != "claim" and c["nbytes"] < 512 << 20 and c["kind"] == "whole", ctx
        if form == "claim":
            assert (c["pf"], c["pb"], c["claimed"], c["past"], c["idle"]) == (0, pb, claimed, past, w - pb), ctx
        if form == "grid":
            assert tags <= {"fallback", "default-threshold"}, ctx
        for t in tags:
            if t == "fallback":
                assert form == "grid" and nunits < minimum and which == "thresholds", ctx
            elif t == "default-threshold":
                assert form == "grid" and nunits >= minimum and which != "thresholds", ctx
            elif t == "claimed":
                assert form == "claim" and claimed > 0, ctx
            elif t == "no-claimed":
                assert form == "claim" and claimed == 0, ctx
            elif t == "past":
                assert past > 0 and c["past"] == past, ctx
            elif t == "no-past":
                assert past == 0, ctx
            elif t == "idle-waves":
                assert form == "claim" and w - pb > 0, ctx
            elif t == "one-idle-wave":
                assert form == "claim" and w - pb == 1, ctx
            elif t == "no-idle-waves":
                assert form == "claim" and pb == w, ctx
            elif t == "masked-head":
                assert ctr_lo(c) % 4096 != 0 and c["head"] == ctr_lo(c) % 4096, ctx
            elif t == "partial-block":
                assert c["nbytes"] % 16 == 11, ctx
            elif t == "carry-in-claimed-unit":
                k = (1 << 64) - ctr_lo(c)        # the block whose counter's low half is 0
                v = (ctr_lo(c) & 4095) + k       # ... in the virtual range
                assert 0 < k < c["nbytes"] // 16, ctx
                # the last block before the wrap and the first after it both lie in claimed units
                assert 0 <= (v - 1) // 2048 < v // 2048 < claimed, ctx
            elif t == "segment-spans-units":
                assert c["seg"] // 16 == 2 * 2048, ctx
            elif t == "front-only":
                assert form == "bitslice" and (c["pb"], c["pf"] + c["claimed"]) == (0, nunits) and nunits >= 1, ctx
            elif t == "back-only":
                assert form == "split" and nunits >= 2 and (c["pf"], c["pb"], c["claimed"]) == (0, nunits, 0), ctx
            elif t == "split-front-middle-back":
                pf = min(nunits - pb, 4 * cus)   # split.cpp split_run
                assert form == "split" and c["nbytes"] == (22 * cus + 5) * U + 48, ctx  # test_gpu_kernels.claimed_split
                assert (c["pf"], c["pb"], c["claimed"]) == (pf, pb, nunits - pf - pb) and min(pf, pb, nunits - pf - pb) > 0, ctx
            else:
                raise AssertionError(f"unknown tag {t!r} in {ctx}")
        if c["kind"] == "segdec":  # IV_s carries into the high half inside the buffer
            assert int.from_bytes(child.IV0_SEG[8:], "big") == 2**64 - 3 and c["nbytes"] // c["seg"] > 3, ctx
        if c["kind"] in ("ctr", "rfc3686"):
            assert child.CTR_BLOCK_OFFSET % 2 == 1 and ctr_lo(c) == 2**64 - child.CTR_K, ctx
        assert c["inplace"] == (c["mode"] in ("ecb-enc", "ecb-dec", "ctr", "rfc3686", "cbc-enc-seg", "cfb-enc-seg")), ctx
    # a call that runs the grid kernel leaves the claim accounting as the call before it left it:
    # decidable only if that call did not report the same unit count
    for a, b in zip(cases, cases[1:]):
        assert a["units"] != b["units"], (cus, a["name"], b["name"])
    if cus == 256:
        for c in cases:
            # 160 MiB, but for the split's shape, which tests/test_gpu_kernels.py claimed_split() sets (176 MiB)
            assert c["nbytes"] <= 160 << 20 or "split-front-middle-back" in c["reaches"], c["name"]


def test_plan_covers_the_table():
    cases = child.plan(256, "thresholds")
    names = {c["name"] for c in cases}
    for mode in child.WHOLE_MODES:
        for bits in (128, 192, 256):
            assert f"{mode}-{bits}/two-units/claim" in names and f"{mode}-{bits}/one-unit/grid" in names
        assert f"{mode}-{child.CLAIMED_BITS[mode]}/claimed/claim" in names
    assert [child.CLAIMED_BITS[m] for m in child.WHOLE_MODES] == [128, 192, 256, 128]
    for mode in ("ecb-enc", "cbc-dec"):
        for shape in ("waves-minus-1", "all-preassigned"):
            assert f"{mode}-{child.CLAIMED_BITS[mode]}/{shape}/claim" in names
    for c in cases:
        if c["kind"] == "whole" or c["kind"] == "segdec":
            assert c["impls"] == ["ttable", "auto"], c["name"]
    segdec = {(c["mode"], c["seg"]) for c in cases if c["kind"] == "segdec"}
    assert segdec == {(m, s) for m in ("cbc-dec-seg", "cfb-dec-seg") for s in (16, 4096, 65536)}
    ctr = {(c["kind"], c["bits"], c["name"].split("/")[1]) for c in cases if c["kind"] in ("ctr", "rfc3686")}
    assert ctr == {("ctr", b, s) for b in (128, 192, 256) for s in ("two-units", "one-unit")} | {
        ("ctr", 128, "claimed"), ("ctr", 256, "claimed"), ("rfc3686", 256, "two-units"), ("rfc3686", 128, "claimed")}
    for mode in ("cbc-enc-seg", "cfb-enc-seg"):
        got = sorted((c["bits"], c["seg"], c["nbytes"] // c["seg"]) for c in cases if c["mode"] == mode)
        w = 4096
        assert got == sorted([(256, 16, (w + 5) * 64 + 37), (128, 16, (w + 5) * 64 + 37), (256, 48, (w + 5) * 64 + 37),
                              (256, 512, 16 * 64 + 37), (256, 4096, 16 * 64 + 37), (256, 512, w * 64),
                              (256, 512, 15 * 64 + 63)])
    forms = child.plan(256, "forms")
    for mode in child.WHOLE_MODES:
        got = {(c["form"], c["name"].split("/")[1]) for c in forms if c["mode"] == mode}
        assert got == {("bitslice", "two-units"), ("bitslice", "claimed"), ("split", "two-units"),
                       ("split", "claimed-split"), ("grid", "two-units"), ("grid", "claimed")}
    assert [c["name"] for c in child.plan(256, "envcheck")] == ["ecb-enc-256/two-units/grid"]


def test_plan_prints_without_a_gpu(capsys):
    assert child.main(["--plan", "--cus", "256"]) == 0
    out = capsys.readouterr().out
    for c in child.plan(256):
        assert f"{c['name']} " in out and f" {c['nbytes']} " in out
    with pytest.raises(ValueError):
        child.plan(0)


@pytest.mark.parametrize("decrypt", [False, True])
@pytest.mark.parametrize("mode", ["cbc", "cfb"])
def test_segment_oracle_equals_cpu_ref(mode, decrypt):
    """The child's segment oracle (one C call per segment, no copies, threads)
    is cpu_ref's, IV_s carry included, for every segment size of the plan."""
    import numpy as np

    from our_tree_amd.models import cpu_ref

    ref = cpu_ref.cbc_segments if mode == "cbc" else cpu_ref.cfb128_segments
    for bits, seg, nseg in ((256, 16, 70), (128, 48, 9), (192, 512, 7), (256, 4096, 5)):
        data = np.random.default_rng(seg).integers(0, 256, size=seg * nseg, dtype=np.uint8)
        key = child.key_of(bits)
        for threads in (1, 3):
            got = child.seg_oracle(mode, key, child.IV0_SEG, data, seg, decrypt, threads=threads)
            assert got.tobytes() == ref(key, child.IV0_SEG, data.tobytes(), seg, decrypt), (bits, seg, threads)
