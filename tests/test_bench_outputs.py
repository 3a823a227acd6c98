"""bench.py's result line and --dump-outputs: a plain run times exactly --steps steps, reports ms_per_step, and writes what its last
timed step computed as float64 .npy files, within the size limit and the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_write_outputs_one_array_per_variable_type_in_key_order(tmp_path):
    import bench
    from gtsam_personal_amd.graph import CAM_BUNDLER, POINT3
    from gtsam_personal_amd.synthetic import make_bal
    _, initial, _, _ = make_bal(n_cam=6, n_pt=50, obs_per_point=4, seed=3)
    bench.write_outputs(str(tmp_path), initial, {"error": 2.5, "lambda": 1e-5})
    out = _load_dir(tmp_path)
    assert sorted(out) == ["error", "lambda", "values_camera", "values_point3"]
    assert all(a.dtype == np.float64 for a in out.values())
    cams = [k for k in initial.keys() if initial.type(k) == CAM_BUNDLER]
    pts = [k for k in initial.keys() if initial.type(k) == POINT3]
    assert out["values_camera"].shape == (6, 17) and out["values_point3"].shape == (50, 3)
    assert np.array_equal(out["values_camera"], np.stack([initial.at(k) for k in cams]))
    assert np.array_equal(out["values_point3"], np.stack([initial.at(k) for k in pts]))
    assert out["error"].tolist() == [2.5] and out["lambda"].tolist() == [1e-5]


def test_write_outputs_samples_a_fixed_subset_above_the_limit(tmp_path, monkeypatch):
    import bench
    from gtsam_personal_amd.synthetic import make_bal
    _, initial, _, _ = make_bal(n_cam=20, n_pt=400, obs_per_point=4, seed=5)
    full = tmp_path / "full"
    bench.write_outputs(str(full), initial, {"error": 1.0})
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    runs = []
    for name in ("a", "b"):
        bench.write_outputs(str(tmp_path / name), initial, {"error": 1.0})
        runs.append(_load_dir(tmp_path / name))
    assert sorted(runs[0]) == sorted(runs[1]) and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
    assert sum(a.nbytes for a in runs[0].values()) <= 4096
    ref = _load_dir(full)
    for name in ("values_camera", "values_point3"):
        rows = runs[0][name + "_rows"].astype(np.int64)
        assert 0 < len(rows) < len(ref[name]) and (np.diff(rows) > 0).all()
        assert np.array_equal(runs[0][name], ref[name][rows])


@pytest.mark.gpu
def test_plain_bench_run_times_the_given_steps_and_dumps_its_last_step(tmp_path):
    """the 100-camera / 10 000-point BAL graph (it has a METIS fixture) through the benchmark's own command line"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--cams", "100", "--points", "10000",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=dict(os.environ, BENCH_PRETOUCH_GB="0"))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-4000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "LM iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-9 * 1e3
    assert not {"cpu_baseline", "roofline", "kernel_ms_per_step", "measured_hbm_copy_gbps"} & set(d)  # those are --full's
    out = _load_dir(tmp_path)
    assert out["values_camera"].shape == (100, 17) and out["values_point3"].shape == (10000, 3)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in out.values())
    assert out["error"][0] == d["error_after_one_iteration"] < d["error_initial"]
