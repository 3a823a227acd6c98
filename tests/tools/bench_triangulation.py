#!/usr/bin/env python3
"""Side measurement (not the bench.py metric, not a test): lmgpu_triangulate_landmarks on the synthetic BAL graph of bench.py's default
size (1000 cameras, 100 000 points, 10 observations each), finalized under PCG so that no symbolic analysis is paid for.  One JSON line:
  dlt_device_ms / epi_device_ms     device time of the launches from lmgpu_get_triangulation_stats (HIP events), median of --reps calls
  dlt_wall_ms / epi_wall_ms         host wall-clock of the whole call (launches + the download of points and statuses), median
  dlt_statuses / epi_statuses, epi_max_iterations / epi_sum_iterations
  degree_histogram                  observations per landmark -> landmarks
  floor_bytes                       measurements + CSR (camera index, measurement reference, row pointer, order, value index) read once,
                                    point + status + iteration count written once; the cameras are L2 hits and not counted
  hbm_copy_gbps                     lmgpu_peak_hbm_copy on this device; *_fraction_of_floor = (floor_bytes / hbm_copy_gbps) / device time
  restatement_ms_per_point_*        the numpy restatement of tests/ on the first --restatement-points landmarks of the same input
    python tests/tools/bench_triangulation.py [--reps N] [--cams C --points P --obs K] [--restatement-points M]"""
import argparse
import collections
import ctypes as ct
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import triangulation_cases as c  # noqa: E402
import triangulation_restatement as r  # noqa: E402
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, LevenbergMarquardtOptimizer, LevenbergMarquardtParams,  # noqa: E402
                                PCGSolverParameters, TriangulationParameters)
from gtsam_personal_amd.synthetic import make_bal  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cams", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--obs", type=int, default=10)
    ap.add_argument("--restatement-points", type=int, default=2000)
    args = ap.parse_args()
    graph, initial, _, ordering = make_bal(n_cam=args.cams, n_pt=args.points, obs_per_point=args.obs, seed=42)
    params = LevenbergMarquardtParams()
    params.linearSolverType = "ITERATIVE"
    params.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    opt = LevenbergMarquardtOptimizer(graph, initial, ordering, params, device=0)
    case, _ = c.graph_batch("bench", graph, initial, ordering, r.Params())
    deg = np.diff(case["offsets"])
    n, n_obs = len(deg), int(deg.sum())
    out = dict(cameras=args.cams, points=n, observations=n_obs, degree_histogram=dict(sorted(collections.Counter(deg.tolist()).items())))
    out["floor_bytes"] = n_obs * (16 + 4 + 8) + n * (4 + 4 + 4) + n * (24 + 4 + 4)
    gbps = ct.c_double()
    if opt.lib.lmgpu_peak_hbm_copy(0, 1 << 30, 5, ct.byref(gbps)) == 0:
        out["hbm_copy_gbps"] = gbps.value
    for tag, epi in (("dlt", False), ("epi", True)):
        tp = TriangulationParameters(enableEPI=epi)
        opt.triangulate_landmarks(tp, write=False)  # builds the index / warms up
        wall, dev = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            res = opt.triangulate_landmarks(tp, write=False)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(res.stats.device_ms)
        out[f"{tag}_device_ms"], out[f"{tag}_wall_ms"] = statistics.median(dev), statistics.median(wall)
        out[f"{tag}_statuses"] = res.stats.n_status
        if epi:
            out["epi_max_iterations"], out["epi_sum_iterations"] = res.stats.max_iterations, res.stats.sum_iterations
        if "hbm_copy_gbps" in out:
            out[f"{tag}_fraction_of_floor"] = (out["floor_bytes"] / (out["hbm_copy_gbps"] * 1e9) * 1e3) / out[f"{tag}_device_ms"]
        m = min(args.restatement_points, n)
        sub = c.prefix(case, m)
        t = time.perf_counter()
        r.batch(sub["cams"], sub["model"], sub["offsets"], sub["obs_cam"], sub["obs_z"], r.Params(enableEPI=epi))
        out[f"restatement_ms_per_point_{tag}"] = (time.perf_counter() - t) * 1e3 / max(1, m)
    opt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
