"""Digests of what a solve of the batch path launches and writes, one line per case and launch form:

    <family>/<case> [<switches>] delta=<fnv1a>,<fnv1a>,<fnv1a>,<fnv1a> lin=<fnv1a> rsd=<fnv1a> launches=<category>:<count>,...

Cases: every case of dense_front_cases, lds_front_cases, leaf_group_cases, schur_cases, schur_var_cases and backsolve_wide_cases in its
default form (product library, or the test library where the case itself names a switch), then -- on the test library -- in every form
the case modules and their GPU tests list (SWITCH_RUNS, FORM_RUNS, GRAPH_RUNS, SWITCH_CASES, the leaf-group and Schur switch sets, the
64-row hops), and sphere2500 under the METIS ordering of tests/golden/slam_orderings.npz once.

Per line: linearize(), then four solves at lambda = 1e-5, 1e-2, 1e-5 and 1 (a graph-replay case makes its eager solve, its capture and
two replays).  delta: an FNV-1a over the bit patterns of each solve's delta; lin: one over the two linear errors of the four solves;
rsd: one over every front's [R S d] after the last solve; launches: the per-category launch counts of kernel_times() for one further
solve (FNV-1a taken over 64-bit words: xor the word, multiply by the prime).

Equal lines mean the same launches on the same tables wrote the same bits.  That is how a change to the solve's host path is held
against its parent: run this file in both, the parent twice (a line the parent does not reproduce against itself proves nothing),
compare the outputs.  Split (multi-rank) fronts are not here: tests/test_gpu_sharded_local.py and tests/test_sharding_gloo.py hold
them.  The incremental path has tests/tools/isam2_digest.py.  Needs a GPU.

    python tests/tools/solve_digest.py [--device N] [--cases SUBSTRING] > solve.txt
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import backsolve_wide_cases as wc  # noqa: E402
import dense_front_cases as dc  # noqa: E402
import lds_front_cases as lc  # noqa: E402
import leaf_group_cases as lg  # noqa: E402
import schur_cases as sc  # noqa: E402
import schur_var_cases as svc  # noqa: E402
from gtsam_personal_amd import LevenbergMarquardtOptimizer, LevenbergMarquardtParams, _lib, noiseModel  # noqa: E402
from gtsam_personal_amd.datasets import chain_initial_pose3, load3D  # noqa: E402

MASK = (1 << 64) - 1
LAMBDAS = (1e-5, 1e-2, 1e-5, 1.0)
UNMASKED, ADD, SPLIT = "LMGPU_SCHUR_UNMASKED", "LMGPU_NO_GATHER_WRITE", "LMGPU_SCHUR_SPLIT_DIAG"
NO_GROUPS, NO_BACKSUB_GROUPS = "LMGPU_NO_LEAF_GROUPS", "LMGPU_NO_BACKSUB_GROUPS"
GRAPH_ON, GRAPH_OFF = ("LMGPU_GRAPH", "1"), ("LMGPU_GRAPH", "0")


def fnv1a(words, h=0xcbf29ce484222325):
    for w in words:
        h = ((h ^ w) * 0x100000001b3) & MASK
    return h


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64).tolist()


def on(*names):
    return tuple((n, "1") for n in names)


def runs():
    """(family, case name, builder of the case dict, ((switch, value), ...)); no switches and none in the case: the product library"""
    out = []
    for name in dc.CASES:
        out.append(("dense", name, dc.case, ()))
    for sw, names in dc.SWITCH_RUNS:
        out += [("dense", name, dc.case, (sw,)) for name in names]
    for name in lc.CASES:
        out.append(("lds", name, lc.case, ()))
    for sw, names in lc.FORM_RUNS:
        out += [("lds", name, lc.case, (sw,)) for name in names]
    out += [("lds", name, lc.case, (GRAPH_ON,)) for name in lc.GRAPH_RUNS] + [("lds", "deep_chain", lc.case, (GRAPH_OFF,))]
    for name in lg.CASES:
        for form in ((), on(NO_GROUPS), on(NO_BACKSUB_GROUPS), on(NO_GROUPS, NO_BACKSUB_GROUPS)):
            out.append(("leaf_group", name, lg.case, form))
    for name in ("sfm_counts", "sfm_n5", "planar_pose"):
        for form in ((), on(NO_GROUPS), on(NO_BACKSUB_GROUPS), on(NO_GROUPS, NO_BACKSUB_GROUPS)):
            out.append(("leaf_group", name, lg.case, form + (GRAPH_ON,)))
    for name in ("sfm_counts", "planar_pose"):
        out.append(("leaf_group", name, lg.case, (("LMGPU_LEAF_GROUP_THREADS", "64"),)))
    for name in sc.CASES:
        out.append(("schur", name, sc.case, ()))
        forms = (on(UNMASKED), on(ADD), on(UNMASKED, ADD), on(SPLIT), on(SPLIT, ADD)) if name in sc.SWITCH_CASES else (on(SPLIT),)
        out += [("schur", name, sc.case, form) for form in forms]
    for form in ((), on(ADD), on(SPLIT), on(SPLIT, ADD)):
        out.append(("schur_var", svc.NAME, lambda _n: svc.case(), form))
    for name in wc.CASES:
        out.append(("backsolve_wide", name, wc.case, ()))
        out.append(("backsolve_wide", name, wc.case, on(wc.SWITCH_HOP64)))
    out.append(("slam", "sphere2500_metis", lambda _n: sphere2500(), ()))
    return out


def sphere2500():
    gold = os.path.join(ROOT, "tests", "golden")
    graph, _ = load3D(os.path.join(gold, "sphere2500.txt"))
    initial = chain_initial_pose3(graph)
    graph.add_PriorFactorPose3(0, np.eye(3), np.zeros(3), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]))
    keys = np.array(sorted(graph.keys()), dtype=np.uint64)
    ordering = [int(k) for k in keys[np.load(os.path.join(gold, "slam_orderings.npz"))["sphere2500_metis"]]]
    return dict(graph=graph, initial=initial, ordering=ordering)


def digest(c, device):
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], LevenbergMarquardtParams(), device=device)
    opt.linearize()
    deltas, lin = [], 0xcbf29ce484222325
    for lam in LAMBDAS:
        _, d, e0, e1 = opt.solve(lam)
        deltas.append(fnv1a(bits(d)))
        lin = fnv1a(bits([e0, e1]), lin)
    rsd = 0xcbf29ce484222325
    for i in range(opt.num_fronts()):
        rsd = fnv1a(bits(opt.front(i)[1]), rsd)
    opt.set_kernel_timing(True)
    opt.solve(LAMBDAS[-1])
    kt = opt.kernel_times()
    opt.set_kernel_timing(False)
    opt.close()
    return (f"delta={','.join(f'{h:016x}' for h in deltas)} lin={lin:016x} rsd={rsd:016x} launches="
            + ",".join(f"{k}:{v['launches']}" for k, v in kt.items()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cases", default="", help="only the lines whose <family>/<case> contains this")
    args = ap.parse_args()
    for family, name, build, form in runs():
        if args.cases not in f"{family}/{name}":
            continue
        c = build(name)
        env = tuple((s, "1") for s in c.get("switches", ())) + tuple(form)
        for sw, value in env:  # (read when the optimizer is built)
            os.environ[sw] = value
        # (LMGPU_GRAPH is read by both libraries: a case that sets nothing else stays on the product library)
        _lib.use_test_library(any(sw != "LMGPU_GRAPH" for sw, _ in env))
        label = " ".join(f"{sw}={value}" for sw, value in env) or "default"
        print(f"{family}/{name} [{label}] {digest(c, args.device)}", flush=True)
        for sw, _ in env:
            del os.environ[sw]


if __name__ == "__main__":
    main()
