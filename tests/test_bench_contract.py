"""bench.py driver contract: one JSON line with the fields the round driver
reads (metric/value/unit/n_gpus/steps/warmup/ms_per_step/...), the metric and
config BASELINE.json names, and value consistent with ms_per_step.

The GPU test runs the real headline step on a small shard (0.25 GiB instead of
64 GiB, so it finishes in seconds); the CPU test only checks the CLI surface.
The extras are read from ``--full`` runs; a plain run carries the headline
alone and, with ``--dump-outputs``, writes the last step's output."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
            "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def test_bench_cli_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in r.stdout


def test_baseline_ratios_are_labelled():
    """vs_baseline divides AES-128-CTR bytes by the AES-256 CPU headline and
    says so; the AES-128-equivalent ratio uses the 14/10 round ratio
    """
    sys.path.insert(0, ROOT)
    import bench

    r = bench.baseline_ratios(1519.0)
    assert bench.BASELINE_GBPS == 0.519
    assert r["vs_baseline"] == pytest.approx(1519.0 / 0.519, rel=1e-3)
    assert "AES-128" in r["vs_baseline_what"] and "CTR-256" in r["vs_baseline_what"]
    assert "results.frankchn.aesni:32" in r["vs_baseline_what"]
    assert r["vs_baseline_aes128_equiv"] == pytest.approx(1519.0 / (0.519 * 1.4), rel=1e-3)


def _cpu_bench(*extra, timeout=300):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--gib", "0.0005",
                           "--steps", "2", "--warmup", "1", "--scatter-rounds", "2", "--full", *extra],
                          capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_bench_cpu_rehearsal_per_rank(n):
    """The whole multi-rank flow on the host (self-spawned ranks, gloo, C
    oracle): one JSON line with a per-rank row for every rank, the preflight
    verdict and the node energy keys (None off the GPU)."""
    r = _cpu_bench("--gpus", str(n))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == n and d["config"]["parallelism"] == f"dp{n}" and d["config"]["device"] == "cpu"
    pr = d["per_rank"]
    assert [x["rank"] for x in pr] == list(range(n))
    for x in pr:
        assert set(bench_keys()) <= set(x)
        assert x["verified"] is True and x["gbps"] > 0
    assert d["verified_sample"] is True
    assert d["per_rank_gbps_min"] == min(x["gbps"] for x in pr)
    assert d["preflight"]["ok"] is True and d["preflight"]["backend"] == "gloo"
    assert "joules_per_gb" in d and "ppt_residency_max" in d and "avg_socket_w_per_gpu" in d
    assert d["rccl_ranks"] == n and d["rccl_ranks_verified"] == n


def bench_keys():
    sys.path.insert(0, ROOT)
    import bench

    return bench.RANK_KEYS


def test_bench_cpu_preflight_fault_rank5():
    r = _cpu_bench("--gpus", "8", "--preflight-fault-rank", "5")
    assert r.returncode != 0
    d = json.loads(r.stdout.splitlines()[0])
    assert d["error"] == "preflight verification failed"
    assert d["preflight"]["per_rank_ok"] == [g != 5 for g in range(8)]


def test_bench_cpu_preflight_hang_is_bounded():
    r = _cpu_bench("--gpus", "4", "--preflight-hang-rank", "2", "--preflight-timeout", "5", timeout=120)
    assert r.returncode == 3
    d = json.loads(r.stdout.splitlines()[0])
    assert "did not finish within 5 s" in d["error"]


def test_node_energy_and_table():
    sys.path.insert(0, ROOT)
    import bench

    nan = float("nan")
    rows = [[100.0, 1.9, 1.0, 50.0, 100.0, 1300.0, 0.5, 0.9, 1800.0, 10.0, 20.0],
            [90.0, nan, 1.0, 60.0, 120.0, 1350.0, 0.5, 0.95, 1790.0, nan, nan]]
    t = bench.per_rank_table(rows)
    assert t[0]["verified"] is True and t[1]["held_clock_ghz"] is None and t[1]["xgmi_read_kb"] is None
    e = bench.node_energy(t)
    assert e["joules_per_gb"] == pytest.approx(110.0 / 220.0)  # all joules over all window bytes
    assert e["avg_socket_w_per_gpu"] == pytest.approx(1325.0) and e["ppt_residency_max"] == 0.95
    t[1]["joules"] = None
    assert bench.node_energy(t)["joules_per_gb"] is None  # one rank unmeasured: no whole-node J/GB


@pytest.mark.gpu
def test_bench_json_line(gpu):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                        "--gib", "0.25", "--no-clock", "--full",
                        "--scatter-mib", "64", "--scatter-rounds", "2", "--stream-gib", "0.25",
                        "--stream-passes", "2"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    # stdout is the one JSON line and nothing else (RCCL's banner goes to stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    d = json.loads(lines[0])
    for k in REQUIRED:
        assert k in d, k
    assert d["metric"] == "GB/s AES-128-CTR (whole node)"
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["config"]["model"] == "AES-128-CTR" and d["config"]["parallelism"] == "dp1"
    assert d["verified_sample"] is True
    assert d["config"]["impl_resolved"] == "ttable"  # 0.25 GiB: below the bitsliced threshold
    assert d["bitsliced_ctr_verified"] is True and d["aes256_ctr_verified"] is True  # the extras, checked
    assert d["aes256_ecb_verified"] is True and d["aes256_ecb_gbps_whole_node"] > 0
    assert d["aes256_ecb_impl"] in ("split", "ttable")  # the reference's workload: AES-256 ECB
    nbytes = d["config"]["per_gpu_bytes"]
    assert nbytes == int(0.25 * (1 << 30))
    # value (GB/s) and ms_per_step describe the same timed region
    assert d["value"] == pytest.approx(nbytes / (d["ms_per_step"] * 1e-3) / 1e9, rel=0.01)
    assert d["value"] > 100.0  # the HIP kernel ran (an eager fallback would be far slower)
    # the communication pass ran through a (1-rank) RCCL group and verified
    assert d["rccl_ranks"] == 1 and d["rccl_backend"] == "nccl"
    assert d["rccl_scatter_verified"] is True and d["rccl_cbc256_scatter_gbps"] > 0
    assert d["rccl_ranks_verified"] == 1
    assert d["rccl_xgmi_bytes_verified"] == 0 and d["rccl_xgmi_bytes_timed"] == 0  # 1 rank: nothing crosses
    assert "vs_baseline_what" in d and d["vs_baseline_aes128_equiv"] < d["vs_baseline"]
    # host-streamed pass: verified, every rank's NUMA node and PCIe rates
    assert d["stream_ctr_verified"] is True and d["stream_ctr_gbps_whole_node"] > 5
    assert d["stream_ctr_bytes_per_rank"] == 2 * int(0.25 * (1 << 30))
    pr = d["stream_ctr_per_rank"]
    assert len(pr) == 1 and pr[0]["rank"] == 0 and pr[0]["h2d_gbps"] > 0 and pr[0]["d2h_gbps"] > 0
    # per-rank table: this rank's own rate, clock, verification and energy
    assert [x["rank"] for x in d["per_rank"]] == [0]
    x = d["per_rank"][0]
    assert x["verified"] is True and x["gbps"] > 100
    assert x["joules"] is not None and x["joules"] > 0, d.get("energy_unavailable")
    assert 100 < x["avg_socket_w"] < 2000 and 0.0 <= x["ppt_residency"] <= 1.0
    assert x["energy_gb"] >= 3 * nbytes / 1e9  # the timed steps, extended to >= 2 s by untimed ones
    assert d["joules_per_gb"] == pytest.approx(x["joules"] / x["energy_gb"], rel=1e-3)
    assert d["energy_window_s"] >= 2.0
    assert d["preflight"]["ok"] is True and d["preflight"]["backend"] == "nccl"
    # the reference's own GPU methodology beside pinned and kernel-only, verified
    assert d["refmethod_verified"] is True
    assert d["refmethod_ecb256_1000mib_gbps"] > 2.41
    assert d["kernel_only_ecb256_1000mib_gbps"] > d["pinned_e2e_ecb256_1000mib_gbps"] > 0


FULL_ONLY = ("rccl_ranks", "stream_ctr_verified", "refmethod_verified", "aes256_ctr_verified",
             "bitsliced_ctr_verified", "ttable_ctr_verified", "aes256_ecb_verified", "energy_window_s")


def _bench_inputs(n):
    """key, counter and (on the host) plaintext as bench.py draws them"""
    import torch

    gen = torch.Generator().manual_seed(1337)
    key = bytes(torch.randint(0, 256, (16,), generator=gen, dtype=torch.uint8).tolist())
    torch.randint(0, 256, (32,), generator=gen, dtype=torch.uint8)  # the AES-256 key
    counter = bytes(torch.randint(0, 256, (16,), generator=gen, dtype=torch.uint8).tolist())
    plain = torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(1000), dtype=torch.uint8)
    return key, counter, plain.numpy().tobytes()


def _plain_cpu_bench(gib, out):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--gib", gib,
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_whole_small_shard(tmp_path):
    """Without --full: the headline keys and nothing that takes a run of its
    own; --dump-outputs writes the whole of a small shard as float32, equal to
    the oracle's CTR of the seeded input (3 in-place steps = one encryption)."""
    import numpy as np

    from our_tree_amd.models import cpu_ref

    d = _plain_cpu_bench("0.0005", tmp_path)
    for k in REQUIRED:
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    n = d["config"]["per_gpu_bytes"]
    # value is rounded to 3 decimals, and small on the host
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3) / 1e9, abs=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    assert d["verified_sample"] is None and d["per_rank"][0]["verified"] is None
    assert os.listdir(tmp_path) == ["ctr_out_rank0.npy"]
    a = np.load(tmp_path / "ctr_out_rank0.npy")
    assert a.dtype == np.float32 and a.shape == (n,)
    key, counter, plain = _bench_inputs(n)
    assert a.astype(np.uint8).tobytes() == cpu_ref.ctr(key, counter, plain)


def test_dump_outputs_sample_is_reproducible(tmp_path):
    """A shard above the dump budget: head, seeded 4 KiB chunks, tail -- 12 MiB
    as float32 (48 MB <= 64 MB), identical from run to run, head and tail equal
    to the oracle's."""
    import numpy as np

    from our_tree_amd.models import cpu_ref

    d = _plain_cpu_bench("0.02", tmp_path / "a")
    _plain_cpu_bench("0.02", tmp_path / "b")
    a = np.load(tmp_path / "a" / "ctr_out_rank0.npy")
    b = np.load(tmp_path / "b" / "ctr_out_rank0.npy")
    assert a.dtype == np.float32 and a.shape == (12 << 20,) and a.nbytes <= 64e6
    assert np.array_equal(a, b)
    n = d["config"]["per_gpu_bytes"]
    assert n > a.size
    key, counter, plain = _bench_inputs(n)
    S = 1 << 16
    assert a[:S].astype(np.uint8).tobytes() == cpu_ref.ctr(key, counter, plain[:S])
    assert a[-S:].astype(np.uint8).tobytes() == cpu_ref.ctr(key, counter, plain[n - S:], (n - S) // 16)
    # every sampled 4 KiB chunk is a chunk of the oracle's output
    want = np.frombuffer(cpu_ref.ctr(key, counter, plain), dtype=np.uint8)
    rows = {want[i:i + 4096].tobytes() for i in range(0, n - 4095, 4096)}
    edge = (12 << 20) // 8
    mid = a[edge:-edge].astype(np.uint8).reshape(-1, 4096)
    assert all(r.tobytes() in rows for r in mid)


@pytest.mark.gpu
def test_plain_bench_dump_on_gpu(gpu, tmp_path):
    """The plain run on the GPU: lean line, and the dumped sample's head and
    tail are the oracle's CTR of the shard fill_random_ made (3 in-place steps)."""
    import numpy as np
    import torch

    from our_tree_amd import ops
    from our_tree_amd.models import cpu_ref

    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--gib", "0.25", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    d = json.loads(lines[0])
    for k in REQUIRED:
        assert k in d, k
    assert d["metric"] == "GB/s AES-128-CTR (whole node)" and d["unit"] == "GB/s" and d["dtype"] == "uint8"
    assert d["steps"] == 2 and d["higher_is_better"] is True
    n = d["config"]["per_gpu_bytes"]
    assert n == int(0.25 * (1 << 30))
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3) / 1e9, rel=0.01)
    assert d["value"] > 100.0  # the HIP kernel ran
    assert not [k for k in FULL_ONLY if k in d]
    a = np.load(tmp_path / "ctr_out_rank0.npy")
    assert a.dtype == np.float32 and a.shape == (12 << 20,)
    key, counter, _ = _bench_inputs(16)
    plain = ops.fill_random_(torch.empty(n, dtype=torch.uint8, device=gpu), seed=1000)
    S = 1 << 16
    head, tail = plain[:S].cpu().numpy().tobytes(), plain[n - S:].cpu().numpy().tobytes()
    assert a[:S].astype(np.uint8).tobytes() == cpu_ref.ctr(key, counter, head)
    assert a[-S:].astype(np.uint8).tobytes() == cpu_ref.ctr(key, counter, tail, (n - S) // 16)


@pytest.mark.parametrize("script", ["bench.py", "benchmarks/cbc_scatter.py", "benchmarks/stream_ctr.py",
                                    "benchmarks/batch_ctr.py", "benchmarks/pcie_bw.py"])
def test_ipc_env_set_before_torch(script):
    """HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf IPC: the only kind this host
    driver supports) must be in the environment before torch / HIP load, for
    every way a script starts -- torchrun too, not only the self-spawned ranks
    (round-3 review, weak #3)."""
    import ast

    tree = ast.parse(open(os.path.join(ROOT, script)).read())
    set_at = torch_at = None
    for node in tree.body:
        src = ast.dump(node)
        if set_at is None and "HSA_ENABLE_IPC_MODE_LEGACY" in src and "setdefault" in src:
            set_at = node.lineno
        if torch_at is None and isinstance(node, (ast.Import, ast.ImportFrom)) and "torch" in src:
            torch_at = node.lineno
    assert set_at is not None and (torch_at is None or set_at < torch_at), (script, set_at, torch_at)
