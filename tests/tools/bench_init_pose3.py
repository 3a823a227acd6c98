#!/usr/bin/env python3
"""Side measurement (not the bench.py metric, not a test): InitializePose3 on full sphere2500 (2500 poses, 4949 between factors, a
prior on pose 0, the committed COLAMD ordering + the anchor last).  One JSON line of host wall-clock times, each the median of --reps
calls on a finalized object, the first call left out as a warm-up:
  chordal_ms              lmgpu_init_pose3_orientations_chordal (linearize + lambda = 0 solve + projection, rotations copied to the host)
  projection_ms           the projection kernel on its own through lmgpu_init_pose3_closest_rotations (upload + kernel + download)
  compute_poses_ms        lmgpu_init_pose3_compute_poses, singleIter (rotations from the device buffer)
  gradient_total_ms / gradient_iterations / gradient_per_iteration_us   gradient mode from the odometry chain, --grad-iters iterations
  initialize_ms           lmgpu_init_pose3_initialize (chordal), end to end
  session_build_s         building the object (two symbolic analyses, uploads)
  restatement_*_s         the numpy / scipy.sparse restatement of tests/ on the host, for scale
    python tests/tools/bench_init_pose3.py [--reps N] [--grad-iters K]"""
import argparse
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

import init_pose3_cases as c  # noqa: E402
import init_pose3_restatement as r  # noqa: E402
from gtsam_personal_amd import InitializePose3, _lib  # noqa: E402
from gtsam_personal_amd.datasets import chain_initial_pose3, load3D  # noqa: E402
from gtsam_personal_amd.init_pose3 import _Session  # noqa: E402


def med_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--grad-iters", type=int, default=1000)
    args = ap.parse_args()
    g = c.with_prior(load3D(os.path.join(c.GOLD, "sphere2500.txt"))[0])
    order = [int(k) for k in np.load(os.path.join(c.GOLD, "slam_orderings.npz"))["sphere2500_colamd"]] + [r.ANCHOR]
    pg = InitializePose3.buildPose3graph(g)
    t = time.perf_counter()
    s = _Session(pg, order)
    out = dict(poses=len(s.keys), factors=pg.size(), session_build_s=time.perf_counter() - t)
    out["chordal_ms"] = med_ms(s.chordal, args.reps)
    relaxed = np.ascontiguousarray(np.random.default_rng(0).standard_normal((len(s.keys), 9)))
    R = np.empty_like(relaxed)
    dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))
    out["projection_ms"] = med_ms(lambda: s.lib.lmgpu_init_pose3_closest_rotations(0, len(s.keys), dp(relaxed), dp(R)), args.reps)
    s.chordal()
    out["compute_poses_ms"] = med_ms(lambda: s.poses(None, True), args.reps)
    out["initialize_ms"] = med_ms(lambda: s.initialize(None, False), args.reps)
    guess = c.rots_of(chain_initial_pose3(g))
    s.gradient(guess, 10, True)
    t = time.perf_counter()
    _, it, mg = s.gradient(guess, args.grad_iters, True)
    gt = time.perf_counter() - t
    out.update(gradient_total_ms=gt * 1e3, gradient_iterations=it, gradient_per_iteration_us=gt * 1e6 / max(1, it), gradient_last_max_grad=mg)
    s.close()
    edges = r.extract(g)
    t = time.perf_counter()
    rots = r.orientations_chordal(edges)
    out["restatement_chordal_s"] = time.perf_counter() - t
    t = time.perf_counter()
    r.compute_poses(rots, edges, True, order)
    out["restatement_compute_poses_s"] = time.perf_counter() - t
    t = time.perf_counter()
    r.orientations_gradient(edges, guess, 3, True)
    out["restatement_gradient_per_iteration_s"] = (time.perf_counter() - t) / 3
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
