"""-m gpu: bench.py honours the driver's contract - ONE JSON line from rank 0 with the named fields - on one rank, and its
sharded code path (row-balanced partition, fp64 [G | R] all-reduce, deferred diagnostics, bit-identity check of the
replicated factor) runs end to end with two ranks sharing this box's GPU over gloo (RCCL needs one device per rank)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]


def _last_json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, stdout[-2000:]
    return json.loads(lines[-1])


def _check_per_kernel(d, most_of_the_step=True):
    """roofline.per_kernel: every hot launch site of the step with its share; the block's kernel is the arg-max of
    launches_per_step x avg_us; the kernels of a step cannot take longer than the step"""
    r = d["roofline"]
    pk = r["per_kernel"]
    assert pk and all(k in e for e in pk for k in ("role", "kernel", "launches_per_step", "avg_us", "algorithmic_bytes", "traffic", "frac"))
    shares = [e["launches_per_step"] * e["avg_us"] for e in pk]
    with_bytes = [e for e in pk if e["algorithmic_bytes"]]
    top = max(with_bytes, key=lambda e: e["launches_per_step"] * e["avg_us"])
    assert r["kernel"] == top["kernel"] and r["kernel_role"] == top["role"], (r["kernel"], top["kernel"])
    assert abs(r["avg_us"] - top["avg_us"]) < 1e-6 and r["frac"] == top["frac"]
    # (10 %: a sampled launch carries its event pair; the calibrated overhead is subtracted, the perturbation of a 3-9 us kernel
    # by the markers around it is not)
    assert sum(shares) <= 1e3 * d["ms_per_step"] * 1.10, (sum(shares), d["ms_per_step"], [(e["role"], e["launches_per_step"], e["avg_us"]) for e in pk])
    if most_of_the_step:  # ... and the timed sites are most of the step (not asserted on regions of a few hundred microseconds,
        assert sum(shares) >= 0.5 * 1e3 * d["ms_per_step"]  # where the synchronisation of the region is most of its time)
    assert 0 < r["step_frac"] < 1 and abs(r["step_frac"] - d["algorithmic_bytes_per_iter"] / (d["ms_per_step"] * 1e-3) / 8e12) < 2e-3


def test_roofline_names_the_dominant_kernel_of_config_4():
    """on the PARAFAC2 + L2-ball stack the dominant site is the chained row pass (six launches per iteration), not the
    X passes (two)"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "c4", "--steps", "5",
                          "--warmup", "2", "--regions", "3", "--no-api", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = _last_json(out.stdout)
    _check_per_kernel(d)
    assert d["roofline"]["kernel_role"] == "chained B row pass" and d["roofline"]["launches_per_step"] == 6.0, d["roofline"]["kernel_role"]
    roles = {e["role"]: e for e in d["roofline"]["per_kernel"]}
    assert roles["X C pass"]["launches_per_step"] == 1.0 and roles["PARAFAC2 per-slab algebra"]["launches_per_step"] == 5.0


def test_single_rank_line():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "6",
                          "--warmup", "2", "--regions", "3", "--cpu-budget", "2", "--full"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = _last_json(out.stdout)
    assert all(k in d for k in REQUIRED), sorted(set(REQUIRED) - set(d))
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["higher_is_better"] is True and d["vs_baseline"] is None and "workload" in d["config"]
    assert len(d["region_ms"]) == 3 and abs(d["ms_per_step"] * d["steps"] - sorted(d["region_ms"])[1]) < 1e-3
    assert d["region_ms_stats"]["min"] <= d["region_ms_stats"]["median"] <= d["region_ms_stats"]["max"]
    assert d["settling"]["probes"] >= 2 and d["settling"]["ms"] >= 100.0
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None or str(r["traffic_source"]).startswith("static: profiles/")
    # ... and against what the box's memory system delivers to a pure streaming read, measured in the same process
    # (mcl_read_bandwidth): between 4 and 8 TB/s on an MI355X, the fraction against it above the one against the spec
    assert 4000.0 < r["peak_achievable"] <= 8000.0, r["peak_achievable"]
    assert abs(r["frac_achievable"] - r["achieved"] / r["peak_achievable"]) < 2e-3 and r["frac_achievable"] >= r["frac"]
    _check_per_kernel(d, most_of_the_step=False)
    m = r["mfma"]
    assert m["unit"] == "TFLOP/s" and m["peak"] == 157.3 and 0 < m["frac"] < 1 and abs(m["frac"] - m["achieved"] / m["peak"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    # every leg of the command accounts for its wall time (the driver's run took 521 s and nothing said where),
    # on stderr as it goes and in the line; the whole command stays far inside the driver's timeout
    w = d["wall_s"]
    for name in ("import_torch", "device_init", "data_synthesis", "engine_setup", "warmup", "settling", "timed_regions",
                 "api_block", "cpu_baseline", "total_until_print"):
        assert name in w, sorted(w)
        assert f"[bench] {name}:" in out.stderr or name == "total_until_print"
    legs = sum(v for k, v in w.items() if "." not in k and k != "total_until_print")
    assert abs(legs - w["total_until_print"]) < 1.0 and w["total_until_print"] < 90.0, w
    # a --gpus value that does not match an EXISTING launch is refused instead of silently re-labelled
    bad = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         env=dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "WORLD_SIZE" in (bad.stderr + bad.stdout)


def test_plain_run_times_its_steps_and_dumps_what_they_computed(tmp_path):
    """without --full: ONE timed region of exactly --steps steps, the headline fields and none of the --full legs; with the
    same arguments two runs start from the same seeded state, so what --dump-outputs writes agrees between them"""
    dumps = []
    for run in range(2):
        out_dir = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "7",
                              "--warmup", "2", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        d = _last_json(out.stdout)
        assert d["metric"] == "AO-ADMM outer-iters/sec" and d["unit"] == "outer-iters/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["steps"] == 7 and d["warmup"] == 2
        assert d["timed_regions"] == 1 and len(d["region_ms"]) == 1 and abs(d["ms_per_step"] * 7 - d["region_ms"][0]) < 1e-3
        assert abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
        assert not {"roofline", "api", "cpu_baseline", "replicated_C_bit_identical"} & set(d), sorted(d)
        assert not {"roofline+checks", "api_block", "cpu_baseline"} & set(d["wall_s"]) and "dump_outputs" in d["wall_s"]
        files = sorted(out_dir.glob("*.npy"))
        assert [f.stem for f in files] == ["A", "B", "C", "diagnostics"] and sum(f.stat().st_size for f in files) <= 64e6
        dumped = {f.stem: np.load(f) for f in files}
        assert dumped["A"].shape == (256, 8) and dumped["B"].shape == (256 * 256, 8) and dumped["C"].shape == (128, 8)
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in dumped.values())
        dumps.append(dumped)
    for name, a in dumps[0].items():
        np.testing.assert_allclose(dumps[1][name], a, rtol=1e-5, atol=1e-7, err_msg=name)


@pytest.mark.parametrize("n", [2, 4])
def test_gpus_2_without_a_launcher_spawns_its_own_ranks(n):
    """the driver's command form: `python bench.py --gpus N ...` with no torch.distributed.run around it;
    N ranks share this box's one GPU over gloo (N = 8 cannot be rehearsed on the card: a GPU box admits at most 6 processes
    on it - the 8-rank collectives are covered on the CPU by tests/test_dist_gloo.py)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MCL_BENCH_SHARE_GPU="1", MCL_BENCH_BACKEND="gloo")
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(n), "--config", "c3_4th", "--steps", "4",
                          "--warmup", "2", "--regions", "2", "--settle-ms", "20", "--full"], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]  # ONE JSON line on stdout, nothing else
    d = json.loads(lines[0])
    assert all(k in d for k in REQUIRED), sorted(set(REQUIRED) - set(d))
    assert d["n_gpus"] == n and d["scaling"] == "strong" and d["replicated_C_bit_identical"] is True
    assert d["collectives_per_step"] == 1.0 and d["config"]["sum_J"] == 256 * 512  # the WHOLE problem, split n ways
    assert d["cpu_baseline"]["value"] is None and "N = 1" in d["cpu_baseline"]["sample"]
    assert d["wall_s"]["total_until_print"] < 120.0, d["wall_s"]
    if n != 2:
        return
    # a failing rank turns into a non-zero exit code of the launcher (here: an unknown process-group backend)
    bad = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--config", "c3_8th"], env=dict(env, MCL_BENCH_BACKEND="no_such_backend"),
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0


@pytest.mark.parametrize("config,n", [("c3_8th", 2), ("c4", 2), ("c4", 4)])
def test_two_ranks_sharing_the_gpu(config, n, tmp_path):
    env = dict(os.environ, MCL_BENCH_SHARE_GPU="1", MCL_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    port = str(29400 + (os.getpid() + len(config) + 7 * n) % 200)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(REPO, "bench.py"), "--gpus", str(n), "--config", config, "--steps", "4",
           "--warmup", "2", "--regions", "2", "--settle-ms", "20", "--full", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = _last_json(out.stdout)
    assert d["n_gpus"] == n and d["scaling"] == "strong" and d["cpu_baseline"]["value"] is None
    assert d["replicated_C_bit_identical"] is True
    assert d["collectives_per_step"] == (6.0 if config == "c4" else 1.0)  # [G | R] (+ PARAFAC2 per inner iteration)
    assert 0 < d["final_rel_rec_error"] < 1
    # --dump-outputs gathers the sharded factors of every rank in row order
    dumped = {name: np.load(tmp_path / f"{name}.npy") for name in ("A", "B", "C", "diagnostics")}
    r = d["config"]["rank"]
    assert dumped["A"].shape == (d["config"]["I"], r) and dumped["B"].shape == (d["config"]["sum_J"], r)
    assert dumped["C"].shape == (d["config"]["K"], r) and all(np.isfinite(a).all() for a in dumped.values())
