"""bench.py's command line: --dump-outputs writes what the last timed tick
returned, a plain run measures the headline only, --full adds the rest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_and_names(tmp_path):
    """float64 stays float64, everything else (the uint8 safe set too) is
    written as float32, one <name>.npy each; values unchanged."""
    rng = np.random.default_rng(1)
    arrays = {"mu": rng.normal(size=1000).astype(np.float32), "lo": rng.normal(size=1000),
              "safe": (rng.uniform(size=1000) > 0.5).astype(np.uint8), "argmax": np.array([1.5, 7.0])}
    bench.dump_outputs(str(tmp_path / "d"), arrays, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["argmax.npy", "lo.npy", "mu.npy", "safe.npy"]
    for k, v in arrays.items():
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype == (np.float64 if v.dtype == np.float64 else np.float32)
        assert np.array_equal(got, v)
    bench.dump_outputs(str(tmp_path / "r"), {"mu": arrays["mu"]}, 3, 8)
    assert os.listdir(tmp_path / "r") == ["mu_rank3.npy"]


def test_dump_outputs_samples_past_the_cap(tmp_path, monkeypatch):
    """Past the byte cap every array is cut to the same fixed sample (the same
    elements on every call, in grid order); small arrays stay whole."""
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    n = 20000
    arrays = {"mu": np.arange(n, dtype=np.float32), "hi": np.arange(n, dtype=np.float64) * 2,
              "argmax": np.array([0.25, 11.0])}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, 0, 1)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in arrays}
    assert sum(v.nbytes for v in a.values()) <= 64 << 10
    assert all(np.array_equal(a[k], b[k]) for k in arrays)
    assert 0 < a["mu"].size < n and np.all(np.diff(a["mu"]) > 0)
    assert np.array_equal(a["hi"], 2.0 * a["mu"])          # the same elements of every array
    assert np.array_equal(a["argmax"], arrays["argmax"])


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """C2, plain: --steps is the number of timed ticks, ms_per_step and value
    agree, nothing that takes a run of its own is measured, and the dump is
    the tick's five arrays plus the argmax key, identical from run to run in
    its inputs (the safe set and the key are decided in f64 from mu/sd)."""
    line = _bench("--gpus", "1", "--config", "C2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    m = line["config"]["M"]
    assert line["steps"] == 3 and line["full"] is False and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["unit"] == "grid-points/s"
    assert line["value"] == pytest.approx(m / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None and line["regimes"] is None and line["subgoal"] is None
    assert line["fill_roofline"]["achieved"] is None and line["roofline"]["achieved"] > 0
    out = {k: np.load(tmp_path / f"{k}.npy") for k in ("mu", "sd", "lo", "hi", "safe", "argmax")}
    assert out["mu"].dtype == out["sd"].dtype == out["safe"].dtype == np.float32
    assert out["lo"].dtype == out["hi"].dtype == out["argmax"].dtype == np.float64
    assert all(out[k].shape == (m,) for k in ("mu", "sd", "lo", "hi", "safe"))
    assert all(np.isfinite(v).all() for v in out.values())
    assert np.all(out["hi"] >= out["lo"]) and set(np.unique(out["safe"])) <= {0.0, 1.0}
    score, idx = out["argmax"]
    assert idx == line["argmax"]["index"] and score == line["argmax"]["score"]
    assert idx >= 0 and out["safe"][int(idx)] == 1.0
    assert score == pytest.approx((out["hi"] - out["lo"])[int(idx)], rel=1e-12)


@pytest.mark.gpu
def test_full_run_measures_the_rest():
    """--full (here without the CPU baseline and the regimes, which have
    options of their own) adds the fill roofline and the subgoal timing."""
    line = _bench("--gpus", "1", "--config", "C2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu",
                  "--no-regimes")
    assert line["full"] is True and line["steps"] == 2
    assert line["fill_roofline"]["achieved"] > 0 and line["subgoal"]["ms"] > 0
