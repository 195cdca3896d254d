"""The driver's bench contract (bench.py): ``--gpus N`` without torchrun must start N ranks itself
(one process per GPU; here gloo on CPU), report ``n_gpus == N`` and the process-group size, and print
exactly one JSON line with the required keys."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_spawns_ranks(gpus):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--sf", "0.002",
                        "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=540, env=env,
                       cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert KEYS <= set(out)
    assert out["n_gpus"] == gpus and out["config"]["world"]["size"] == gpus
    assert out["steps"] == 1 and out["warmup"] == 0 and out["value"] > 0


def _bench(tmp_path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--sf", "0.002",
                        "--steps", "2", "--warmup", "1", *extra], capture_output=True, text=True, timeout=540,
                       env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    [line] = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return json.loads(line)


@pytest.mark.timeout(600)
def test_bench_plain_full_and_dump_outputs(tmp_path):
    """A plain run times its steps only (the untimed passes report None); ``--full`` adds them;
    ``--dump-outputs`` writes the last step's result columns as float arrays, the same from run to run."""
    import numpy as np

    plain = _bench(tmp_path, "--dump-outputs", str(tmp_path / "a"))
    assert KEYS <= set(plain) and plain["steps"] == 2 and plain["ms_per_step"] > 0
    assert plain["collect_ms"] is None and plain["collect_geomean_ms"] is None
    assert plain["kernels"]["shape_shared_geomean_ms"] is None
    full = _bench(tmp_path, "--full", "--dump-outputs", str(tmp_path / "b"))
    assert set(full) == set(plain) and full["metric"] == plain["metric"]
    assert full["collect_geomean_ms"] > 0 and set(full["collect_ms"]) == set(full["per_query_ms"])
    assert full["kernels"]["shape_shared_geomean_ms"] > 0
    a, b = (sorted(os.listdir(tmp_path / d)) for d in ("a", "b"))
    assert a == b and all(f.endswith(".npy") for f in a)
    assert {f[:2] for f in a} == {f"{i:02d}" for i in range(plain["config"]["queries"])}  # every query
    size = 0
    for f in a:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and x.ndim == 1
        assert np.array_equal(x, y, equal_nan=True), f
        size += x.nbytes
    assert 0 < size <= 64_000_000
    counts = np.load(tmp_path / "a" / next(f for f in a if f.startswith("00_") and "__02_" in f))
    assert counts.sum() == plain["rows_per_gpu"]  # Basic Aggregation's count(*) over every row


@pytest.mark.timeout(600)
def test_bench_total_sf_strong_scaling():
    """``--total-sf``: the fixed-total-SF (strong scaling) curve -- 2 ranks each hold half of SF 0.02
    and the JSON line says so (scaling "strong", the total and per-GPU scale factors in config)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--total-sf", "0.02",
                        "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=540, env=env,
                       cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["scaling"] == "strong" and out["n_gpus"] == 2
    assert out["config"]["scale_factor_total"] == pytest.approx(0.02)
    assert out["config"]["scale_factor_per_gpu"] == pytest.approx(0.01)
    assert "SF0.02 total" in out["config"]["model"]
