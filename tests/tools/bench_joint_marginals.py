#!/usr/bin/env python3
"""Side measurement (not the bench.py metric): joint marginals and cross-covariances from the one factorization
(lmgpu_joint_marginal_covariances / lmgpu_marginal_cross_covariances: the source's path, then each target's branch)
against the existing route (lmgpu_joint_marginal_covariance: one elimination + back-substitution per column of the joint), which this
change does not touch.

Workloads (tests/golden/, COLAMD orderings as the full-size tests obtain them):
  1. victoria_park: the last pose with every landmark (one source, many targets) and 1000 pose-landmark joints read from the graph's own
     bearing-range factors; the first also under several values of the targets-per-workgroup cap (lmgpu_set_marginals_cross_cap);
  2. city10000: the last pose with every pose under several caps (a request large enough for the cap to matter), and 1000 pose-pose joints at loop-closure distances, read from the graph's own non-consecutive between factors;
  3. sphere2500: 1000 such joints;
  4. the headline BAL graph (1000 cameras, 100 000 points): 4 camera-camera joints.
The existing route is timed on a sample of 8 to 16 of the same pairs.

Method: wall clock around calls that end with a host wait (every call here downloads its result), one untimed warm-up of each route,
then the median of --repeat timed runs; the factorization is timed apart, made stale between runs by lmgpu_set_values of the same values.

    python tests/tools/bench_joint_marginals.py [--repeat 5] [--skip-bal] [--commit HASH] [--out profiles/r10/joint_marginals.json]"""
import argparse
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
CAPS = (1, 2, 4, 8, 16, 32, 64, 256, 0)


def _median_ms(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def _stats_delta(after, before):
    return {k: after[k] - before[k] for k in ("cross_launches", "cross_chunks", "cross_walks", "cross_targets", "cross_lds", "cross_scratch")}


def binary_factor_pairs(graph, keep):
    """(key, key) of every two-variable factor of the graph, in the graph's order, for which keep(a, b)"""
    rows = []
    for _, _, gi, keys, _, _, _ in graph.buckets():
        if keys.shape[1] == 2:
            rows += [(int(i), int(a), int(b)) for i, (a, b) in zip(gi.tolist(), keys.tolist()) if keep(int(a), int(b))]
    return [(a, b) for _, a, b in sorted(rows)]


def spread(items, n):
    items = list(items)
    return [items[i] for i in np.unique(np.linspace(0, len(items) - 1, min(n, len(items))).astype(int))]


def distinct(pairs):
    return list(dict.fromkeys((min(a, b), max(a, b)) for a, b in pairs))


def factor_time(m, repeat):
    h = m._opt
    vals = h.values()

    def factor():
        h.set_values(vals)  # stale
        h._check(h.lib.lmgpu_marginals_factor(h._h))

    factor()
    return _median_ms(factor, repeat)


def measure_joints(name, graph, values, ordering, joints, sample_n, repeat):
    """joints: the two-key sets of the new route; the old route runs on a sample of them"""
    m = Marginals(graph, values, ordering)
    factor_ms, factor_all = factor_time(m, repeat)
    got = m.jointMarginalCovariances(joints)  # warm-up: allocations, first launch
    before = m.marginalsStats()
    query_ms, query_all = _median_ms(lambda: m.jointMarginalCovariances(joints), repeat)
    after = m.marginalsStats()
    sample = spread(range(len(joints)), sample_n)
    old = Marginals(graph, values, ordering)
    old.jointMarginalCovariance(joints[sample[0]])  # warm-up

    def old_all():
        return [old.jointMarginalCovariance(joints[q]).fullMatrix() for q in sample]

    old_ms, old_runs = _median_ms(old_all, max(1, min(repeat, 3)))
    worst = 0.0
    for q, ref in zip(sample, old_all()):
        worst = max(worst, float(np.linalg.norm(got[q].fullMatrix() - ref) / np.linalg.norm(ref)))
    n = len(joints)
    per_run = {k: v // repeat for k, v in _stats_delta(after, before).items()}
    rec = {
        "workload": name, "variables": len(ordering), "scalars": int(m._opt._ntot), "fronts": int(m._opt.num_fronts()), "joints": n,
        "cross_route": {"factor_ms": round(factor_ms, 4), "queries_ms": round(query_ms, 4), "ms_per_joint_queries_only": round(query_ms / n, 6),
                        "ms_per_joint_with_factor": round((factor_ms + query_ms) / n, 6), "factor_runs_ms": factor_all, "query_runs_ms": query_all,
                        "per_request": per_run, "longest_union": after["longest_union"], "cross_cap": after["cross_cap"]},
        "column_route": {"joints": len(sample), "total_ms": round(old_ms, 4), "ms_per_joint": round(old_ms / len(sample), 6), "runs_ms": old_runs},
        "worst_relative_difference_on_sample": worst,
    }
    rec["column_over_cross_per_joint"] = round(rec["column_route"]["ms_per_joint"] / rec["cross_route"]["ms_per_joint_with_factor"], 2)
    rec["cross_route_faster_for_one_joint"] = factor_ms + query_ms / n < rec["column_route"]["ms_per_joint"]
    m.close()
    old.close()
    print(f"{name}: cross route {n} joints: factor {factor_ms:.3f} ms + queries {query_ms:.3f} ms = "
          f"{rec['cross_route']['ms_per_joint_with_factor'] * 1e3:.2f} us per joint; column route {rec['column_route']['ms_per_joint']:.3f} ms per "
          f"joint over {len(sample)}; ratio {rec['column_over_cross_per_joint']}; worst relative difference {worst:.2e}", flush=True)
    return rec


def measure_one_source(name, graph, values, ordering, source, targets, sample_n, repeat, sweep=None):
    """Sigma[target, source] for every target: one source walk per workgroup, the targets split by the cap; every cap of CAPS is timed"""
    m = Marginals(graph, values, ordering)
    h = m._opt
    factor_ms, _ = factor_time(m, repeat)
    pairs = [(t, source) for t in targets]
    caps = []
    base = None
    for cap in sweep or CAPS:  # (0: the built-in rule)
        assert h.lib.lmgpu_set_marginals_cross_cap(h._h, cap) == 0
        got = m.crossCovariances(pairs)  # warm-up
        before = m.marginalsStats()
        ms, runs = _median_ms(lambda: m.crossCovariances(pairs), repeat)
        after = m.marginalsStats()
        same = base is None or all(np.array_equal(got[p], base[p]) for p in pairs)
        base = base or got
        caps.append({"cap": cap, "queries_ms": round(ms, 4), "runs_ms": runs, "walks": _stats_delta(after, before)["cross_walks"] // repeat,
                     "same_bits_as_first_cap": bool(same)})
        print(f"{name}: cap {cap}: {ms:.3f} ms for {len(pairs)} targets ({caps[-1]['walks']} workgroups)", flush=True)
    h.lib.lmgpu_set_marginals_cross_cap(h._h, 0)
    st = m.marginalsStats()
    old = Marginals(graph, values, ordering)
    sample = spread(targets, sample_n)
    old.jointMarginalCovariance([source, sample[0]])

    def old_all():
        return [old.jointMarginalCovariance([source, t]).at(t, source) for t in sample]

    old_ms, old_runs = _median_ms(old_all, max(1, min(repeat, 3)))
    scale = float(np.linalg.norm(old.jointMarginalCovariance([source]).fullMatrix()))
    worst = max(float(np.linalg.norm(base[(t, source)] - ref) / scale) for t, ref in zip(sample, old_all()))
    best = min(caps, key=lambda c: c["queries_ms"])
    rec = {"workload": name, "variables": len(ordering), "targets": len(pairs), "factor_ms": round(factor_ms, 4), "caps": caps,
           "fastest_cap": best["cap"], "default_cap": st["cross_cap"], "longest_union": st["longest_union"],
           "cross_route_ms_per_pair_fastest": round(best["queries_ms"] / len(pairs), 6),
           "column_route": {"pairs": len(sample), "total_ms": round(old_ms, 4), "ms_per_pair": round(old_ms / len(sample), 6), "runs_ms": old_runs},
           "worst_difference_on_sample_relative_to_source_block": worst}
    m.close()
    old.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-bal", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the parent commit to record (default: git rev-parse of the tree)")
    a = ap.parse_args()
    out = []
    g, init = load2D(os.path.join(GOLD, "victoria_park.txt"))
    g.add_PriorFactorPose2(0, init.at(0), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-8]))
    o = oh.colamd(g)
    landmarks = sorted(int(k) for k in o if len(init.at(k)) == 2)
    last_pose = max(int(k) for k in o if len(init.at(k)) == 3)
    out.append(measure_one_source("victoria_park / COLAMD, last pose with every landmark", g, init, o, last_pose, landmarks, 12, a.repeat))
    lm = set(landmarks)
    pl = distinct(binary_factor_pairs(g, lambda x, y: (x in lm) != (y in lm)))
    out.append(measure_joints("victoria_park / COLAMD, pose-landmark joints", g, init, o, [list(p) for p in spread(pl, 1000)], 12, a.repeat))
    g, init = readG2o(os.path.join(GOLD, "city10000.g2o"))
    g.add_PriorFactorPose2(0, init.at(0), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-8]))
    o = oh.colamd(g)
    poses = sorted(int(k) for k in o)
    out.append(measure_one_source("city10000 / COLAMD, last pose with every pose", g, init, o, poses[-1], poses[:-1], 8, a.repeat, sweep=(1, 4, 8, 16, 64, 0)))
    loops = distinct(binary_factor_pairs(g, lambda x, y: abs(x - y) > 1))
    out.append(measure_joints("city10000 / COLAMD, loop-closure pose pairs", g, init, o, [list(p) for p in spread(loops, 1000)], 12, a.repeat))
    g, _ = load3D(os.path.join(GOLD, "sphere2500.txt"))
    init = chain_initial_pose3(g)
    g.add_PriorFactorPose3(0, np.eye(3), np.zeros(3), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]))
    o = oh.colamd(g)
    loops = distinct(binary_factor_pairs(g, lambda x, y: abs(x - y) > 1))
    out.append(measure_joints("sphere2500 / COLAMD, loop-closure pose pairs", g, init, o, [list(p) for p in spread(loops, 1000)], 12, a.repeat))
    if not a.skip_bal:
        g, init, _, o = make_bal(n_cam=1000, n_pt=100000, obs_per_point=10, seed=42)
        cams = [int(k) for k in list(o)[100000:]]
        joints = [[cams[i], cams[j]] for i, j in ((0, 999), (123, 124), (500, 17), (998, 250))]
        out.append(measure_joints("BAL 1000 cameras / 100000 points, 4 camera-camera joints", g, init, o, joints, 4, max(1, min(a.repeat, 3))))
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, text=True).stdout.strip()
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
