"""bench.py's contract with whoever runs it: a plain run prints the headline line alone (everything else is behind --full), and
--dump-outputs writes what the timed path computed as float64 DIR/<name>.npy files of at most 64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from solve_keyframe_pose_graph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cost_per_iteration", "final_cost", "quaternions", "switches", "translations"]
FULL_ONLY = ["roofline", "roofline_pcg", "roofline_mg", "roofline_k1_out_of_cache", "other_kernels", "cpu_baseline", "converged", "value_ceres_decision_rule",
             "lm_iters_per_s_including_transfers", "c5_strong"]


def _summary(costs, final):
    s = capi.Summary()
    s.num_logged = len(costs)
    for k, c in enumerate(costs):
        s.iterations[k].cost = c
    s.final_cost = final
    return s


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_outputs_writes_float64_arrays_and_a_fixed_sample_above_the_cap(tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    n, m = 5000, 4000
    q, t, s = rng.random(4 * n), rng.random(3 * n), rng.random(m)
    summ = _summary([9.0, 7.5, 7.0], 7.0)
    bench.dump_outputs(str(tmp_path / "all"), q, t, s, summ)
    a = _load(tmp_path / "all")
    assert sorted(os.listdir(tmp_path / "all")) == [n_ + ".npy" for n_ in NAMES]
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["quaternions"], q.reshape(n, 4)) and np.array_equal(a["translations"], t.reshape(n, 3)) and np.array_equal(a["switches"], s)
    assert np.array_equal(a["cost_per_iteration"], [9.0, 7.5, 7.0]) and np.array_equal(a["final_cost"], [7.0])

    cap = 100000      # below what the arrays need: a sample of keyframes and switches, the same one every time
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", cap)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), q, t, s, summ)
        assert sum(os.path.getsize(os.path.join(tmp_path, d, f)) for f in os.listdir(tmp_path / d)) <= cap
    s1, s2 = _load(tmp_path / "s1"), _load(tmp_path / "s2")
    assert all(np.array_equal(s1[k], s2[k]) for k in NAMES)
    assert 0 < len(s1["quaternions"]) < n and len(s1["quaternions"]) == len(s1["translations"]) and 0 < len(s1["switches"]) < m
    rows = [int(np.flatnonzero((q.reshape(n, 4) == r).all(axis=1))[0]) for r in s1["quaternions"]]      # real rows of the state, in order, kept together
    assert rows == sorted(rows) and np.array_equal(s1["translations"], t.reshape(n, 3)[rows])
    assert np.array_equal(s1["cost_per_iteration"], a["cost_per_iteration"])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps_the_timed_result(tmp_path):
    steps, poses = 3, 20000
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--poses-per-gpu", str(poses),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["unit"] == "LM iters/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["metric"].startswith("LM iters/sec")
    assert d["steps"] == steps and d["value"] > 0 and d["ms_per_step"] == pytest.approx(1e3 / d["value"], rel=1e-12)
    assert not [k for k in FULL_ONLY if k in d]
    a = _load(out)
    assert all(v.dtype == np.float64 for v in a.values())
    loops = int(round(bench.C3_LOOPS * poses / bench.C3_POSES))      # (bench.py's graph for --poses-per-gpu on one GPU)
    assert a["quaternions"].shape == (poses, 4) and a["translations"].shape == (poses, 3) and a["switches"].shape == (loops,)
    assert np.abs(np.linalg.norm(a["quaternions"], axis=1) - 1.0).max() < 1e-9
    assert a["cost_per_iteration"].shape == (steps + 1,)
    assert 2.0 * a["final_cost"][0] == d["chi2_final"] and 2.0 * a["cost_per_iteration"][0] == pytest.approx(d["chi2_initial"], rel=1e-12)
