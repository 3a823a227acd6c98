#!/usr/bin/env python3
"""Side measurement (not the bench.py metric): marginal covariances by the path route (lmgpu_marginal_covariances: one factorization, one
walk per variable) against the existing route (lmgpu_marginal_covariance: one elimination + back-substitution per
column).

On sphere2500, city10000 and victoria_park (tests/golden/, COLAMD orderings as the full-size tests obtain them): the path route for ALL
variables, factorization and queries timed separately; the existing route on a fixed sample of 16 variables spread over the ordering, as
time per variable.  On the headline BAL graph (1000 cameras, 100 000 points): 8 cameras both ways.

Method: wall clock around calls that end with a host wait (every call here downloads its result), one untimed warm-up of each route,
then the median of --repeat timed runs; the factorization is made stale between runs by lmgpu_set_values of the same values.

    python tests/tools/bench_marginals.py [--repeat 5] [--skip-bal] [--out profiles/r09/marginals.json]"""
import argparse
import ctypes as ct
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_harness as oh  # noqa: E402
from gtsam_personal_amd import Marginals, noiseModel  # noqa: E402
from gtsam_personal_amd.datasets import chain_initial_pose3, load2D, load3D, readG2o  # noqa: E402
from gtsam_personal_amd.synthetic import make_bal  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _median_ms(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def measure(name, graph, values, ordering, path_keys, sample, repeat):
    """path_keys: what the path route is asked for (None: all variables); sample: the keys the existing route is timed on"""
    m = Marginals(graph, values, ordering)
    h = m._opt
    vals = h.values()
    n_path = len(ordering) if path_keys is None else len(path_keys)

    def factor():
        h.set_values(vals)  # stale
        h._check(h.lib.lmgpu_marginals_factor(h._h))

    factor()
    got = m.marginalCovariances(path_keys)  # warm-up: allocations, first launch
    factor_ms, factor_all = _median_ms(factor, repeat)
    query_ms, query_all = _median_ms(lambda: m.marginalCovariances(path_keys), repeat)
    st = m.marginalsStats()
    old = Marginals(graph, values, ordering)
    old.marginalCovariance(sample[0])  # warm-up
    worst = 0.0

    def old_all():
        for k in sample:
            old.marginalCovariance(k)

    old_ms, old_runs = _median_ms(old_all, max(1, min(repeat, 3)))
    for k in sample:
        if k in got:
            ref = old.marginalCovariance(k)
            worst = max(worst, float(np.linalg.norm(got[k] - ref) / np.linalg.norm(ref)))
    rec = {
        "workload": name, "variables": len(ordering), "scalars": int(h._ntot), "fronts": int(h.num_fronts()),
        "path_route": {"variables": n_path, "factor_ms": round(factor_ms, 4), "queries_ms": round(query_ms, 4),
                       "ms_per_variable": round((factor_ms + query_ms) / n_path, 6), "factor_runs_ms": factor_all, "query_runs_ms": query_all,
                       "longest_path": st["longest_path"], "stats": st},
        "column_route": {"variables": len(sample), "total_ms": round(old_ms, 4), "ms_per_variable": round(old_ms / len(sample), 6),
                         "runs_ms": old_runs},
        "worst_relative_difference_on_sample": worst,
    }
    rec["path_route_faster_per_variable"] = rec["path_route"]["ms_per_variable"] < rec["column_route"]["ms_per_variable"]
    m.close()
    old.close()
    print(f"{name}: path route {n_path} variables: factor {factor_ms:.3f} ms + queries {query_ms:.3f} ms = "
          f"{rec['path_route']['ms_per_variable'] * 1e3:.2f} us per variable; column route {rec['column_route']['ms_per_variable']:.3f} ms per "
          f"variable over {len(sample)}; worst relative difference {worst:.2e}", flush=True)
    return rec


def spread(ordering, n=16):
    keys = list(ordering)
    return [int(keys[i]) for i in np.linspace(0, len(keys) - 1, n).astype(int)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-bal", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    g, _ = load3D(os.path.join(GOLD, "sphere2500.txt"))
    init = chain_initial_pose3(g)
    g.add_PriorFactorPose3(0, np.eye(3), np.zeros(3), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]))
    o = oh.colamd(g)
    out.append(measure("sphere2500 / COLAMD", g, init, o, None, spread(o), a.repeat))
    g, init = readG2o(os.path.join(GOLD, "city10000.g2o"))
    g.add_PriorFactorPose2(0, init.at(0), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-8]))
    o = oh.colamd(g)
    out.append(measure("city10000 / COLAMD", g, init, o, None, spread(o), a.repeat))
    g, init = load2D(os.path.join(GOLD, "victoria_park.txt"))
    g.add_PriorFactorPose2(0, init.at(0), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-8]))
    o = oh.colamd(g)
    out.append(measure("victoria_park / COLAMD", g, init, o, None, spread(o), a.repeat))
    if not a.skip_bal:
        g, init, _, o = make_bal(n_cam=1000, n_pt=100000, obs_per_point=10, seed=42)
        cams = [int(k) for k in list(o)[100000:]]
        eight = [cams[i] for i in np.linspace(0, len(cams) - 1, 8).astype(int)]
        out.append(measure("BAL 1000 cameras / 100000 points, 8 cameras", g, init, o, eight, eight, max(1, min(a.repeat, 3))))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, text=True).stdout.strip()
    except OSError:
        commit = ""
    doc = {"date": time.strftime("%Y-%m-%d"), "parent_commit": commit, "repeat": a.repeat, "results": out}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
