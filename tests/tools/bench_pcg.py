#!/usr/bin/env python3
"""Side measurement (not the bench.py metric): the PCG linear solver (linearSolverType = ITERATIVE, BlockJacobi, default
PCGSolverParameters) on C4 (1000 cameras, 100 000 points, 1 M factors) and on the 20 000-camera graph the direct path cannot hold.
One JSON line per case: LM iterations/s, CG iterations per solve, microseconds per CG iteration, block-Jacobi build time, and the
HBM fraction of one CG iteration against the model (two streaming passes over the Jacobian pool at 6.3 TB/s).
--fused: the A/B form with the forward product recomputed inside the transpose gather (liblmgpu_test.so, LMGPU_PCG_FUSED=1).
    python tests/tools/bench_pcg.py [--steps K] [--fused] [--case c4|cam20000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gtsam_personal_amd import _lib  # noqa: E402
from gtsam_personal_amd import BlockJacobiPreconditionerParameters, LevenbergMarquardtOptimizer, LevenbergMarquardtParams, PCGSolverParameters  # noqa: E402
from gtsam_personal_amd.synthetic import make_bal  # noqa: E402

HBM_TBPS = 6.3


def run(tag, n_cam, n_pt, steps, fused=False):
    graph, initial, _, _ = make_bal(n_cam=n_cam, n_pt=n_pt, obs_per_point=10, seed=42)
    params = LevenbergMarquardtParams()
    params.linearSolverType = "ITERATIVE"
    params.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    opt = LevenbergMarquardtOptimizer(graph, initial, None, params, device=0)
    opt.save_values()
    s0 = opt.copy_state()
    opt.iterate()  # warm-up
    opt.restore_values(s0)
    cg, pre, it_ms, n_solves, wall = 0, 0.0, 0.0, 0, 0.0
    for _ in range(steps):
        opt.restore_values(s0)
        t = time.perf_counter()
        opt.iterate()
        wall += time.perf_counter() - t
        st = opt.pcg_stats()  # the last solve of the iteration
        cg += st["iterations"]
        pre += st["precond_ms"]
        it_ms += st["iterate_ms"]
        n_solves += 1
    pool_bytes = 2 * 13 * 8 * graph.size()  # one SFM factor: 2 x 13 whitened doubles
    us_per_cg = 1e3 * it_ms / max(1, cg)
    model_us = 2 * pool_bytes / (HBM_TBPS * 1e12) * 1e6
    out = dict(case=tag, cameras=n_cam, points=n_pt, factors=graph.size(), lm_iters_per_s=steps / wall,
               cg_iters_per_solve=cg / n_solves, us_per_cg_iter=us_per_cg, block_jacobi_build_ms=pre / n_solves,
               hbm_fraction=model_us / us_per_cg if us_per_cg > 0 else 0.0, fused=fused, model_us_per_cg_iter=model_us, final_error=opt.error())
    print(json.dumps(out), flush=True)
    opt.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--case", choices=("c4", "cam20000", "both"), default="both")
    a = ap.parse_args()
    if a.fused:
        os.environ["LMGPU_PCG_FUSED"] = "1"
        _lib.use_test_library(True)
    if a.case in ("c4", "both"):
        run("c4", 1000, 100000, a.steps, a.fused)
    if a.case in ("cam20000", "both"):
        run("cam20000", 20000, 100000, a.steps, a.fused)
