#!/usr/bin/env python3
"""Side measurement (not the bench.py metric, not a test): Levenberg-Marquardt on a synthetic visual-SLAM scene, once with one
SmartProjectionPoseFactor per landmark (poses only) and once in the explicit formulation the engine had before (a POINT3 variable per
landmark + one GenericProjectionFactor per observation, points eliminated first).  Poses on a ring looking at a box of landmarks, every
landmark seen by 2 .. --max-obs poses, odometry between neighbouring poses, a prior on the first pose; pixel noise on the measurements,
the poses start off the truth.  One JSON line: per formulation the wall-clock and device time of every LM iteration, for the smart graph
the device time of its triangulation and smart linearize launches (HIP events, lmgpu_get_smart_stats) and their share.
    python tests/tools/bench_smart.py [--poses N] [--landmarks N] [--max-obs K] [--iterations K]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import gtsam_personal_amd as gpa  # noqa: E402
from gtsam_personal_amd import graph as G  # noqa: E402
from gtsam_personal_amd import smart as S  # noqa: E402
import smart_restatement as sr  # noqa: E402
import triangulation_cases as tc  # noqa: E402

K5 = np.array([500.0, 480.0, 0.0, 320.0, 240.0])


def scene(n_poses, n_lm, max_obs, seed):
    rng = np.random.default_rng(seed)
    truth = []
    for i in range(n_poses):
        a = 2 * np.pi * i / n_poses
        R, t = tc.lookat(np.array([30 * np.cos(a), 30 * np.sin(a), rng.uniform(-3, 3)]), np.zeros(3))
        truth.append(sr.pose(R, t))
    lms = rng.uniform(-4, 4, (n_lm, 3))
    obs = []
    for p in lms:
        sel = np.sort(rng.choice(n_poses, int(rng.integers(2, max_obs + 1)), replace=False))
        obs.append((sel, [sr.project_jac(truth[i], K5, p)[0] + rng.normal(0, 0.5, 2) for i in sel]))
    start = [sr.retract(p, 2e-3 * rng.normal(0, 1, 6)) for p in truth]
    return truth, lms, obs, start


def common(graph, values, truth, start):
    keys = [G.X(i) for i in range(len(truth))]
    for k, p in zip(keys, start):
        values.insert(k, G.POSE3, p)
    odo = G.noiseModel.Isotropic.Sigma(6, 0.02, smart=False)
    for i in range(len(truth)):
        j = (i + 1) % len(truth)
        R, t = sr.Rt(sr.between(truth[i], truth[j]))
        graph.add_BetweenFactorPose3(keys[i], keys[j], R, t, odo)
    R, t = sr.Rt(truth[0])
    graph.add_PriorFactorPose3(keys[0], R, t, G.noiseModel.Isotropic.Sigma(6, 0.01, smart=False))
    return keys


def run(opt, iterations):
    """per lmgpu_iterate call: wall-clock ms, device ms (lmgpu_get_timings), tryLambda calls; the first call carries one-off setup"""
    wall, dev, inner = [], [], []
    e0 = opt.error()
    for _ in range(iterations):
        t = time.perf_counter()
        opt.iterate()
        wall.append(1e3 * (time.perf_counter() - t))
        tm = opt.timings()
        dev.append(tm["total_ms"])
        inner.append(tm["inner_iterations"])
    return dict(error0=e0, error=opt.error(), iterations=opt.iterations(), wall_ms=wall, device_ms=dev, inner_iterations=inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--landmarks", type=int, default=20000)
    ap.add_argument("--max-obs", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    truth, lms, obs, start = scene(args.poses, args.landmarks, args.max_obs, args.seed)
    pix = G.noiseModel.Isotropic.Sigma(2, 1.0, smart=False)

    g, v = gpa.NonlinearFactorGraph(), gpa.Values()
    keys = common(g, v, truth, start)
    prm = gpa.SmartProjectionParams(S.HESSIAN, S.ZERO_ON_DEGENERACY)
    for sel, zs in obs:
        f = gpa.SmartProjectionPoseFactor(pix, K5, prm)
        f.add(zs, [keys[i] for i in sel])
        g.add_SmartProjectionPoseFactor(f)
    t = time.perf_counter()
    opt = gpa.LevenbergMarquardtOptimizer(g, v, gpa.Ordering(keys))
    out = dict(poses=args.poses, landmarks=args.landmarks, observations=int(sum(len(s) for s, _ in obs)),
               smart=dict(build_s=time.perf_counter() - t))
    out["smart"].update(run(opt, args.iterations))
    st = opt.smart_stats()
    # one triangulation per linearize and one per trial lambda: its share of the last call's device time
    calls = 1 + out["smart"]["inner_iterations"][-1]
    out["smart"].update(triangulate_ms=st["triangulate_ms"], smart_linearize_ms=st["linearize_ms"], n_status=st["n_status"],
                        smart_share_of_last_call=(st["triangulate_ms"] * calls + st["linearize_ms"]) / max(out["smart"]["device_ms"][-1], 1e-9))
    pts, status = opt.smart_points()
    opt.close()

    g, v = gpa.NonlinearFactorGraph(), gpa.Values()
    keys = common(g, v, truth, start)
    lkeys = [G.L(i) for i in range(len(lms))]
    for k, p, q, s in zip(lkeys, lms, pts, status):
        v.insert(k, G.POINT3, q if s == 0 else p)  # start the points where the smart factors triangulated them
    pk = np.array([[keys[i], lkeys[j]] for j, (sel, _) in enumerate(obs) for i in sel], dtype=np.uint64)
    zk = np.array([np.concatenate([z, K5]) for _, zs in obs for z in zs])
    g._add(G.F_PROJECTION, pk, zk, pix)
    t = time.perf_counter()
    opt = gpa.LevenbergMarquardtOptimizer(g, v, gpa.Ordering(lkeys + keys))
    out["explicit"] = dict(build_s=time.perf_counter() - t)
    out["explicit"].update(run(opt, args.iterations))
    opt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
