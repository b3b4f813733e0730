"""Every persistent claim kernel against the C oracle, byte for byte.

The persistent kernels -- T-table CTR (k_aes_ctr_tt_persist), the whole-buffer
T-table claim kernels of ECB / CBC-dec / CFB-dec and their segment forms
(tt_claim, claim_walk) and persistent segment encryption
(k_aes_seg_enc_tt_claim) -- are routed to from 512 MiB / 1 GiB, where the rest
of the suite can only sample windows or compare them with another claim kernel
that shares their host plan.  A process started with
OTC_TT_PERSISTENT_MIN_MIB, OTC_TT_CTR_PERSISTENT_MIN_MIB and
OTC_SEGENC_PERSISTENT_MIN_MIB at 0 reaches them at 64 KiB .. ~130 MiB, where
the C oracle checks every byte: tests/claim_forms_child.py runs there, once per
set, and each test here asserts one of its records (output equal to the oracle
out of place and in place, and the claim accounting of the planned kernel).

Three child processes, one at a time, each under its own time limit; after a
child that ended like a fault (or did not run to its end) no further child is
started and every test of the module fails with that status."""
import json
import os
import subprocess
import sys
import time

import pytest

import claim_forms_child as child

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "claim_forms_child.py")
# Time limits: three times a clean run of each child on an MI355X (a shared
# machine; the oracle is CPU-bound), rounded up to the next 10 s.  A child's
# time is mostly its start (torch, the library) and the oracle; the device
# part of all cases together is 0.03 s.
LIMIT_S = {
    "thresholds": 30,  # measured 7.5 s (62 cases; oracle 5.0 s)
    "forms": 20,       # measured 3.9 s (24 cases; oracle 1.6 s)
    "envcheck": 10,    # measured 2.0 s (1 case)
}
THRESHOLD_VARS = ("OTC_TT_PERSISTENT_MIN_MIB", "OTC_TT_CTR_PERSISTENT_MIN_MIB", "OTC_SEGENC_PERSISTENT_MIN_MIB")
FAULT_STATUS = (134, 139, 124, 137)
_stopped = []  # why no further child may start: the first child that did not end clean


def run_child(which, tmp_path_factory, env_changes):
    """One child process of set ``which``: dict(status, fault, records, stdout,
    stderr); status None: not started, because an earlier child did not end clean."""
    if _stopped:
        return dict(status=None, fault=False, records={}, stdout="", stderr=f"not started: {_stopped[0]}", seconds=0.0)
    out = tmp_path_factory.mktemp(f"claim_forms_{which}") / "records.jsonl"
    env = dict(os.environ)
    for v in THRESHOLD_VARS:  # whatever the caller's shell holds, the child starts from the defaults
        env.pop(v, None)
    env.update(env_changes)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, CHILD, "--set", which, "--out", str(out)], env=env, capture_output=True,
                           text=True, timeout=LIMIT_S[which])
        status, stdout, stderr = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as e:  # the child has been killed
        as_text = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
        status, stdout, stderr = 124, as_text(e.stdout), as_text(e.stderr) + f"\n[time limit of {LIMIT_S[which]} s]"
    records = {}
    if out.exists():
        for line in out.read_text().splitlines():
            r = json.loads(line)
            records[r["name"]] = r
    fault = status in FAULT_STATUS or status < 0 or "illegal memory access" in (stdout + stderr)
    if status != 0 or fault:
        _stopped.append(f"the {which!r} child ended with status {status}" + (" (fault-like)" if fault else "") +
                        f"; stderr ends: {stderr[-600:]!r}")
    return dict(status=status, fault=fault, records=records, stdout=stdout, stderr=stderr,
                seconds=round(time.perf_counter() - t0, 1))


def check_ended_clean(run, which):
    if run["status"] != 0 or run["fault"]:
        pytest.fail(f"the {which!r} child ended with status {run['status']}: {run['stderr'][-1500:]}", pytrace=False)


def check_record(run, which, name):
    check_ended_clean(run, which)
    r = run["records"].get(name)
    assert r is not None, f"{name}: the child wrote no record"
    if r["skipped"]:
        assert name.startswith("rfc3686-"), f"{name}: skipped ({r['skipped']}); only the AES-NI oracle's cases may be"
        pytest.skip(r["skipped"])
    print(f"{name}: {r['ran']} units {r['units']} planned {r['planned']} device {r['device_s']} s oracle {r['oracle_s']} s")
    assert r["passed"], (f"{name}: first differing byte {r['first_diff']} (unit {r['diff_unit']} of "
                         f"{r['planned']['units']}), ran {r['ran']}, accounting {r['units']}, planned {r['planned']}: " +
                         "; ".join(r["problems"]))
    assert r["calls"] and all(c["equal"] for c in r["calls"]), name
    assert r["ran"].split("/")[1] == r["planned"]["form"], name


@pytest.fixture(scope="module")
def thresholds_run(gpu, tmp_path_factory):
    """The child with every threshold at 0: every claim path, small."""
    return run_child("thresholds", tmp_path_factory, {v: "0" for v in THRESHOLD_VARS})


@pytest.fixture(scope="module")
def forms_run(gpu, tmp_path_factory, thresholds_run):
    """The child with the environment's thresholds unset: the forms that need none.  After the first child."""
    return run_child("forms", tmp_path_factory, {})


@pytest.fixture(scope="module")
def envcheck_run(gpu, tmp_path_factory, forms_run):
    """The child started with an unparsable threshold.  After the other two."""
    return run_child("envcheck", tmp_path_factory, {"OTC_TT_PERSISTENT_MIN_MIB": "abc"})


@pytest.mark.parametrize("name", [c["name"] for c in child.plan(256, "thresholds")])
def test_persistent_kernel_equals_oracle(thresholds_run, name):
    """Thresholds at 0: the persistent T-table kernels (and, below their
    minimum unit counts, the grid kernels) over whole buffers."""
    check_record(thresholds_run, "thresholds", name)


@pytest.mark.parametrize("name", [c["name"] for c in child.plan(256, "forms")])
def test_other_forms_equal_oracle(forms_run, name):
    """The same shapes through the bitsliced claim kernel alone, the
    co-resident split and the grid T-table kernel, against the same oracle."""
    check_record(forms_run, "forms", name)


def test_every_planned_case_ran(thresholds_run, forms_run):
    for which, run in (("thresholds", thresholds_run), ("forms", forms_run)):
        check_ended_clean(run, which)
        cus = next(iter(run["records"].values()))["cus"]
        assert list(run["records"]) == [c["name"] for c in child.plan(cus, which)], which
        skipped = [n for n, r in run["records"].items() if r["skipped"]]
        assert all(n.startswith("rfc3686-") for n in skipped), skipped
        slow = sorted(run["records"].values(), key=lambda r: -(r["device_s"] + r["oracle_s"]))[:3]
        print(which, "child:", run["seconds"], "s of", LIMIT_S[which], "s; slowest cases (device s, oracle s):", [(r["name"], r["device_s"], r["oracle_s"]) for r in slow])


def test_unparsable_threshold_keeps_the_default(envcheck_run):
    """OTC_TT_PERSISTENT_MIN_MIB=abc: not "0 MiB, every call persistent" but
    the default, said once on stderr; the two-unit ECB call is correct and
    runs the grid kernel."""
    (name,) = [c["name"] for c in child.plan(256, "envcheck")]
    check_record(envcheck_run, "envcheck", name)
    print("envcheck child:", envcheck_run["seconds"], "s of", LIMIT_S["envcheck"], "s")
    r = envcheck_run["records"][name]
    assert r["planned"]["form"] == "grid" and r["units"] == dict(front=0, back=0, nunits=0), r
    warnings = [ln for ln in envcheck_run["stderr"].splitlines() if "OTC_TT_PERSISTENT_MIN_MIB=abc" in ln]
    assert len(warnings) == 1 and "ignoring" in warnings[0], envcheck_run["stderr"][-1500:]
