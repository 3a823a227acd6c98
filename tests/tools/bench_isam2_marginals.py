#!/usr/bin/env python3
"""Side measurement (not the bench.py metric, not a test): what ISAM2's covariances cost INSIDE the incremental loop, by the single-key
entry (lmgpu_isam2_marginal_covariance, which this change does not touch: the baseline, measured in the same process) and by the
many-marginals / cross-covariance route (lmgpu_isam2_marginal_covariances, lmgpu_isam2_cross_covariances).

Workload: timing/timeIncremental.cpp on tests/golden/city10000.g2o, one pose per update, every new pose initialised from the device's own
calculateEstimate(previous pose), default ISAM2Params; the constrained COLAMD orderings are replayed from
tests/golden/isam2_orderings_city10000.bin (the recording bench.py --workload isam2 replays), so oracle/_ref is not needed.  Every
--every-th step, between two updates:
  (a) the current pose alone                       old entry | new entry with n = 1
  (b) the last 64 poses                            64 calls of the old entry | ONE call of the new one
  (c) the current pose with each of 16 earlier poses (spread over the trajectory): ONE cross_covariances call, the current pose as keys_j
  (d) beside (c), the own marginals of those 16 earlier poses (walks as deep as the branches (c) descends): 16 old calls | ONE new call
Method: the C entry points through ctypes (every one ends with a host wait and a download), host clock around the call; per step one
untimed call of each route, then --repeat timed calls, old and new alternating; a step's figure is the median of its calls, the reported
figure the median over the steps (and the last step's, where the paths are longest).  The new blocks are compared with the old entry's at
every measured step.

    python tests/tools/bench_isam2_marginals.py [--poses 10000] [--every 100] [--repeat 7] [--commit HASH] [--out profiles/r12/isam2_marginals.json]"""
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
from gtsam_personal_amd import ISAM2, ISAM2Params, _lib  # noqa: E402
from gtsam_personal_amd._lib import LmgpuError  # noqa: E402
from gtsam_personal_amd.incremental_workloads import incremental_pose2_steps  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
U64 = ct.POINTER(ct.c_uint64)


class Replay:
    """the recorded orderings as the ccolamd callback: int32 n_cols, then the permutation, call after call"""

    def __init__(self, path):
        self.rec, self.at, self.calls = np.fromfile(path, dtype=np.int32), 0, 0

    def __call__(self, n_rows, n_cols, col_ptr, row_idx, cmember):
        if self.at + 1 + n_cols > len(self.rec) or self.rec[self.at] != n_cols:
            raise RuntimeError(f"recorded ordering {self.calls} does not fit this call ({n_cols} columns)")
        perm = self.rec[self.at + 1:self.at + 1 + n_cols]
        self.at += 1 + n_cols
        self.calls += 1
        return perm


def us(fn):
    t0 = time.perf_counter()
    fn()
    return 1e6 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit to record (default: git rev-parse of the tree)")
    a = ap.parse_args()
    isam = ISAM2(ISAM2Params(), ccolamd=Replay(os.path.join(GOLD, "isam2_orderings_city10000.bin")), device=0)
    lib, h = isam.lib, isam._h
    D = lambda x: x.ctypes.data_as(_lib._D)
    K = lambda x: x.ctypes.data_as(U64)
    one, many, cross = np.zeros(9), np.zeros(64 * 9), np.zeros(16 * 9)
    old64, deep16 = np.zeros((64, 3, 3)), np.zeros((16, 3, 3))
    rows, stopped = [], None
    t_loop = time.perf_counter()
    step = 0
    try:
        for g, v in incremental_pose2_steps(os.path.join(GOLD, "city10000.g2o"), a.poses, lambda k: isam.calculateEstimate(k)):
            isam.update(g, v)
            step += 1
            if step % a.every or step < 64:
                continue
            cur = np.array([step], dtype=np.uint64)
            last = np.arange(step - 63, step + 1, dtype=np.uint64)
            earlier = np.unique(np.linspace(0, step - 1, 16).astype(np.uint64))
            src = np.full(len(earlier), step, dtype=np.uint64)

            def old_one():
                assert lib.lmgpu_isam2_marginal_covariance(h, int(cur[0]), D(one)) == 0

            def new_one():
                assert lib.lmgpu_isam2_marginal_covariances(h, 1, K(cur), D(one)) == 0

            def old_many():
                for q, k in enumerate(last.tolist()):
                    assert lib.lmgpu_isam2_marginal_covariance(h, k, D(old64[q])) == 0

            def new_many():
                assert lib.lmgpu_isam2_marginal_covariances(h, 64, K(last), D(many)) == 0

            def new_cross():
                assert lib.lmgpu_isam2_cross_covariances(h, len(earlier), K(earlier), K(src), D(cross)) == 0

            def old_deep():  # (the 16 earlier poses' OWN marginals: walks of the depth (c) descends, by both entries)
                for q, k in enumerate(earlier.tolist()):
                    assert lib.lmgpu_isam2_marginal_covariance(h, k, D(deep16[q])) == 0

            def new_deep():
                assert lib.lmgpu_isam2_marginal_covariances(h, len(earlier), K(earlier), D(cross)) == 0

            routes = dict(a_old=old_one, a_new=new_one, b_old=old_many, b_new=new_many, c_new=new_cross, d_old=old_deep, d_new=new_deep)
            for fn in routes.values():  # untimed: first launches of a shape, allocations
                fn()
            worst = float(np.max(np.abs(many.reshape(64, 3, 3) - old64)) / np.max(np.abs(old64)))
            before = isam.marginals_stats()
            t = {name: [] for name in routes}
            for _ in range(a.repeat):
                for name, fn in routes.items():
                    t[name].append(us(fn))
            after = isam.marginals_stats()
            rows.append(dict(step=step, path_cliques=len(isam.marginals_path(step)), path_cliques_64th=len(isam.marginals_path(step - 63)),
                             path_cliques_earliest=len(isam.marginals_path(0)),
                             **{name: round(float(np.median(ts)), 2) for name, ts in t.items()}, new_vs_old_max_rel_diff=worst,
                             launches_per_marginals_call=(after["launches"] - before["launches"]) / (3 * a.repeat),
                             launches_per_c_call=(after["cross_launches"] - before["cross_launches"]) / a.repeat))
            print(json.dumps(rows[-1]), flush=True)
    except LmgpuError as e:  # (the recorded orderings no longer fit: report what was measured up to here)
        stopped = f"update {step + 1}: {e}"
    loop_s = time.perf_counter() - t_loop
    st = isam.marginals_stats()
    isam.close()
    if not rows:
        raise SystemExit(f"nothing measured ({stopped})")
    med = lambda name: round(float(np.median([r[name] for r in rows])), 2)
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    except OSError:
        commit = ""
    doc = {"date": time.strftime("%Y-%m-%d"), "commit": commit, "workload": f"city10000 incremental loop, {step} updates, measured every {a.every}th step",
           "unit": "us per call (host clock around a C call that ends with a wait and a download; median of the per-step medians)", "repeat": a.repeat,
           "a_current_pose": {"old_entry": med("a_old"), "new_entry_n1": med("a_new")},
           "b_last_64_poses": {"old_entry_64_calls": med("b_old"), "new_entry_one_call": med("b_new")},
           "c_current_pose_with_16_earlier": {"cross_covariances_one_call": med("c_new")},
           "d_marginals_of_those_16_earlier": {"old_entry_16_calls": med("d_old"), "new_entry_one_call": med("d_new")},
           "last_measured_step": rows[-1], "worst_new_vs_old_max_rel_diff": max(r["new_vs_old_max_rel_diff"] for r in rows),
           "stats": st, "loop_seconds_including_measurements": round(loop_s, 1), "stopped_early": stopped, "steps": rows}
    print(json.dumps({k: v for k, v in doc.items() if k != "steps"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
