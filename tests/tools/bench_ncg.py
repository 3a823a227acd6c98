#!/usr/bin/env python3
"""Side measurement (not the bench.py metric): NonlinearConjugateGradientOptimizer on the device (lmgpu_ncg_optimize).
One JSON line per case: milliseconds per NCG iteration (host wall clock around optimize(), divided by the line searches it ran,
the uncounted gradient-descent step included), trials per line search and host waits per line search.
Cases: the 5-pose Pose2 graph of the reference's test, tests/golden/sphere2500.txt (odometry-chained initial estimate, a prior on
pose 0) and a synthetic BAL graph.  --host-loop: the same iteration with the line search driven from Python through lmgpu_retract /
lmgpu_error / lmgpu_restore_values (one launch sequence, one blocking readback and one branch per trial), for comparison; it follows
Polak-Ribiere with the device's gradient (lmgpu_gradient).
    python tests/tools/bench_ncg.py [--iterations K] [--host-loop] [--case five_pose|sphere2500|bal|all] [--cameras N --points M]"""
import argparse
import ctypes as ct
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, GaussNewtonParams, NonlinearConjugateGradientOptimizer,  # noqa: E402
                                NonlinearFactorGraph, PCGSolverParameters, Values, noiseModel)
from gtsam_personal_amd.datasets import chain_initial_pose3, load3D  # noqa: E402
from gtsam_personal_amd.synthetic import make_bal  # noqa: E402


def five_pose():
    g = NonlinearFactorGraph()
    g.add_PriorFactorPose2(1, [0.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    odo = noiseModel.Diagonal.Sigmas([0.2, 0.2, 0.1])
    for a, b, th in ((1, 2, 0.0), (2, 3, math.pi / 2), (3, 4, math.pi / 2), (4, 5, math.pi / 2), (5, 2, math.pi / 2)):
        g.add_BetweenFactorPose2(a, b, [2.0, 0.0, th], odo)
    v = Values()
    for k, p in ((1, (0.5, 0.0, 0.2)), (2, (2.3, 0.1, -0.2)), (3, (4.1, 0.1, math.pi / 2)), (4, (4.0, 2.0, math.pi)), (5, (2.1, 2.1, -math.pi / 2))):
        v.insert_pose2(k, *p)
    return g, v


def sphere2500():
    graph, _ = load3D(os.path.join(ROOT, "tests", "golden", "sphere2500.txt"))
    initial = chain_initial_pose3(graph)
    graph.add_PriorFactorPose3(0, np.eye(3), np.zeros(3), noiseModel.Diagonal.Sigmas([0.1, 0.1, 0.1, 0.3, 0.3, 0.3]))
    return graph, initial


def host_loop(opt, iterations):
    """nonlinearConjugateGradient with lineSearch on the host: every trial is lmgpu_restore_values + lmgpu_retract + lmgpu_error"""
    phi = 0.5 * (1.0 + math.sqrt(5.0))
    resphi, tau = 2.0 - phi, 1e-5
    trials = readbacks = searches = 0

    def err_at(step, d):
        nonlocal trials, readbacks
        opt.restore_values()
        opt.retract(step * d)
        trials += 1
        readbacks += 1
        return opt.graph_error()

    def search(d):
        nonlocal searches
        searches += 1
        g = float(np.linalg.norm(d))
        lo, hi = -1.0 / g, 0.0
        new = lo + (hi - lo) / (phi + 1.0)
        new_e = err_at(new, d)
        while True:
            flag = hi - new > new - lo
            test = new + resphi * (hi - new) if flag else new - resphi * (new - lo)
            if (hi - lo) < tau * (abs(test) + abs(new)):
                return 0.5 * (lo + hi)
            te = err_at(test, d)
            if te >= new_e:
                if flag:
                    hi = test
                else:
                    lo = test
            else:
                if flag:
                    lo = new
                else:
                    hi = new
                new, new_e = test, te

    def advance(alpha, d):
        opt.restore_values()
        opt.retract(alpha * d)
        opt.save_values()

    opt.save_values()
    g = opt.gradient()
    readbacks += 1
    d = g.copy()
    advance(search(d), d)
    for _ in range(iterations):
        gp, g = g, opt.gradient()
        readbacks += 1
        beta = max(0.0, float(g @ (g - gp)) / float(gp @ gp))
        d = g + beta * d
        advance(search(d), d)
    readbacks += 1
    return opt.graph_error(), searches, trials, readbacks


def run(tag, graph, initial, iterations, host, no_fronts):
    p = GaussNewtonParams()
    p.maxIterations = iterations
    p.relativeErrorTol = p.absoluteErrorTol = 0.0  # run all the iterations asked for
    if no_fronts:
        p.linearSolverType = "ITERATIVE"
        p.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    opt = NonlinearConjugateGradientOptimizer(graph, initial, p, device=0)
    e0 = opt.error()
    opt.save_values()
    opt.line_search()  # warm-up: module load, first launches
    t = time.perf_counter()
    if host:
        err, searches, trials, waits = host_loop(opt, iterations)
    else:
        cp = opt._ncg_c()  # the C call alone: optimize() would add the download of the values into a Python Values
        opt._check(opt.lib.lmgpu_ncg_optimize(opt._h, ct.byref(cp), ct.byref(opt.state)))
        wall_device = time.perf_counter() - t
        tr = opt.trace()
        err, searches, trials, waits = opt.error(), len(tr), int(tr[:, 3].sum()), opt.host_waits()
    wall = wall_device if not host else time.perf_counter() - t
    print(json.dumps(dict(case=tag, mode="host-loop" if host else "device", factors=graph.size(), scalars=int(opt._ntot), line_searches=searches,
                          ms_per_iteration=1e3 * wall / searches, trials_per_line_search=trials / searches,
                          host_readbacks_per_iteration=waits / searches, initial_error=e0, final_error=err)), flush=True)
    opt.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--host-loop", action="store_true")
    ap.add_argument("--case", choices=("five_pose", "sphere2500", "bal", "all"), default="all")
    ap.add_argument("--cameras", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    a = ap.parse_args()
    if a.case in ("five_pose", "all"):
        run("five_pose", *five_pose(), a.iterations, a.host_loop, False)
    if a.case in ("sphere2500", "all"):
        run("sphere2500", *sphere2500(), a.iterations, a.host_loop, True)
    if a.case in ("bal", "all"):
        graph, initial, _, _ = make_bal(n_cam=a.cameras, n_pt=a.points, obs_per_point=10, seed=42)
        run(f"bal_{a.cameras}x{a.points}", graph, initial, a.iterations, a.host_loop, True)
