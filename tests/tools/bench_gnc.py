#!/usr/bin/env python3
"""Side measurement (not the bench.py metric, not a test): GNC with an LM base and TLS on the C4-sized synthetic BAL graph (1000
cameras, 100 000 points, 1 M factors) with a share of displaced measurements.  One JSON line: per outer iteration the device time of
the weight update (unweighted error kernels + weights + reduction) next to the base optimizer's time, and the construction time of the handle for the same graph -- what every outer
iteration would pay through the interface without GNC (a new weighted graph = a new handle: ordering, plan, uploads).
base_optimizer_ms is host wall-clock time from the moment the weight update is queued (no wait in between), so it contains the weight
update's device time; base_minus_weight_ms subtracts it.  Host synchronisations are not counted here: that the loop adds none beyond the
base optimizer's own is a property of the code (include/lmgpu.h, lmgpu_gnc_optimize), not a measurement.
    python tests/tools/bench_gnc.py [--cams N] [--points N] [--share S] [--pixels P] [--max-outer K]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from gtsam_personal_amd import GncLMParams, GncOptimizer  # noqa: E402
import gnc_cases as gc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--obs", type=int, default=10)
    ap.add_argument("--share", type=float, default=0.05)
    ap.add_argument("--pixels", type=float, default=40.0)
    ap.add_argument("--max-outer", type=int, default=100)
    args = ap.parse_args()
    graph, initial, ordering, displaced = gc.bal_with_outliers(args.cams, args.points, args.obs, seed=42, share=args.share, pixels=args.pixels)
    p = GncLMParams()
    p.setMaxIterations(args.max_outer)
    t = time.perf_counter()
    gnc = GncOptimizer(graph, initial, p, ordering)
    build_s = time.perf_counter() - t
    t = time.perf_counter()
    gnc.optimize()
    wall_s = time.perf_counter() - t
    tr, w = gnc.trace(), gnc.getWeights()
    out = dict(factors=graph.size(), displaced=int(displaced.sum()), misclassified=int(((w < 0.5) != displaced).sum()),
               outer_iterations=int(gnc.result.iterations), stop=int(gnc.result.stop), base_iterations_total=int(gnc.result.base_iterations_total),
               handle_build_s=build_s, optimize_wall_s=wall_s,
               weight_update_ms=[round(float(x), 4) for x in tr[:, 3]], base_optimizer_ms=[round(float(x), 2) for x in tr[:, 4]],
               base_iterations=[int(x) for x in tr[:, 5]], base_minus_weight_ms=[round(float(x), 2) for x in tr[:, 4] - tr[:, 3]], weight_update_ms_mean=float(np.mean(tr[:, 3])) if len(tr) else None,
               base_optimizer_ms_mean=float(np.mean(tr[:, 4])) if len(tr) else None)
    print(json.dumps(out), flush=True)
    gnc.close()


if __name__ == "__main__":
    main()
