"""Digests of what the device ISAM2 holds after every update / marginalizeLeaves call of a handful of short sequences, two lines per call:

    <sequence> <call> S <counters> vars=<n> facs=<n> unused=<keys> marg=<indices> del=<indices> fixed=<keys> tree=<fnv1a>
    <sequence> <call> N rsd=<fnv1a> delta=<fnv1a>

S (structure): the five ISAM2Result counters (- for marginalizeLeaves), the variable and factor counts, ISAM2Result::unusedKeys, the
marginal and deleted factor indices of marginalizeLeaves, getFixedVariables, and an FNV-1a over every clique's info (key count, frontal
keys, nf, n, parent) and key list, depth-first from the roots.  N (numbers): an FNV-1a over the bit patterns of every clique's [R S d]
and one over delta's (FNV-1a taken over 64-bit words: xor the word, multiply by the prime).

Two trees whose S lines are equal do the same bookkeeping; equal N lines mean the same launches on the same tables in the same order.
That is how a change to the update / marginalizeLeaves host path is held against its parent: run this file in both, the parent twice (an N
line the parent does not reproduce against itself proves nothing), compare the outputs.  Needs a GPU and oracle/_ref (the constrained
COLAMD); each sequence is the smallest that reaches a branch.

    python tests/tools/isam2_digest.py [--device N] [--sequences SUBSTRING] > isam2.txt
"""
import argparse
import ctypes as ct
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import oracle_harness as oh  # noqa: E402
from gtsam_personal_amd import ISAM2, ISAM2DoglegParams, ISAM2GaussNewtonParams, ISAM2Params, NonlinearFactorGraph, Values, _lib, noiseModel  # noqa: E402
from gtsam_personal_amd.incremental_workloads import (fixed_lag_pose2_steps, fixed_lag_update_params, incremental_pose2_steps,  # noqa: E402
                                                      visual_steps)

CITY = os.path.join(ROOT, "tests", "golden", "city10000.g2o")
MASK = (1 << 64) - 1


def fnv1a(words, h=0xcbf29ce484222325):
    for w in words:
        h = ((h ^ w) * 0x100000001b3) & MASK
    return h


class Digest:
    """an ISAM2 handle whose every call prints its two lines"""

    def __init__(self, name, params, device):
        self.name, self.calls = name, 0
        self.isam = ISAM2(params, ccolamd=oh.ccolamd_csc, device=device)

    def _lines(self, what, counters, marg=(), deleted=()):
        isam, lib = self.isam, self.isam.lib
        tree, rsd_h = 0xcbf29ce484222325, 0xcbf29ce484222325
        for i in range(lib.lmgpu_isam2_num_cliques(isam._h)):
            info = np.zeros(5, dtype=np.int32)
            isam._check(lib.lmgpu_isam2_clique_info(isam._h, i, info.ctypes.data_as(_lib._I)))
            keys, rsd = np.zeros(info[0], dtype=np.uint64), np.empty(int(info[2]) * int(info[3]))
            isam._check(lib.lmgpu_isam2_get_clique(isam._h, i, keys.ctypes.data_as(ct.POINTER(ct.c_uint64)), rsd.ctypes.data_as(_lib._D)))
            tree = fnv1a(keys.tolist(), fnv1a([int(x) & MASK for x in info.tolist()], tree))
            rsd_h = fnv1a(rsd.view(np.uint64).tolist(), rsd_h)
        delta = isam.getDelta()
        delta_h = fnv1a(np.concatenate([delta[k] for k in delta] + [np.zeros(0)]).view(np.uint64).tolist())
        head = f"{self.name} {self.calls:03d}:{what}"
        ids = lambda xs: ",".join(str(int(x)) for x in xs) or "-"  # noqa: E731
        print(f"{head} S {counters} vars={isam.size()} facs={isam.num_factors()} unused={ids(isam.unusedKeys())} marg={ids(marg)} "
              f"del={ids(deleted)} fixed={ids(isam.getFixedVariables())} tree={tree:016x}")
        print(f"{head} N rsd={rsd_h:016x} delta={delta_h:016x}", flush=True)
        self.calls += 1

    def update(self, *args, **kw):
        r = self.isam.update(*args, **kw).as_dict()
        self._lines("update", "/".join(str(r[k]) for k in ("variablesRelinearized", "variablesReeliminated", "factorsRecalculated", "cliques", "batch")))

    def marginalize(self, keys):
        marg, deleted = self.isam.marginalizeLeaves(keys)
        self._lines("marginalizeLeaves", "-", marg, deleted)

    def pose2(self, key):
        return np.asarray(self.isam.calculateEstimate(key), dtype=float)[:3]


def seq_visual(d):
    for g, v in visual_steps():
        d.update(g, v)


def seq_city(d):
    for g, v in incremental_pose2_steps(CITY, 300, d.pose2):
        d.update(g, v)


def seq_fixed_lag(d):
    for g, v, leaving in fixed_lag_pose2_steps(CITY, 300, 25, d.pose2):
        constrained, marked = fixed_lag_update_params(d.isam.cliques() if leaving else [], list(d.isam.getDelta().keys()), list(v.keys()), leaving)
        d.update(g, v, constrainedKeys=constrained, extraReelimKeys=marked)
        if leaving:
            d.marginalize(leaving)


def seq_wide(d):
    from test_gpu_isam2 import dense_pose2_steps
    for g, v in dense_pose2_steps():
        d.update(g, v)
    d.update(force_relinearize=True)


def seq_batch_threshold(d):
    odo = noiseModel.Diagonal.Sigmas([0.1, 0.1, 0.05])
    g, v = NonlinearFactorGraph(), Values()
    g.add_PriorFactorPose2(0, [0.0, 0.0, 0.0], odo)
    g.add_BetweenFactorPose2(0, 1, [1.0, 0.0, 0.0], odo)
    v.insert_pose2(0, 0.01, 0.01, 0.01)
    v.insert_pose2(1, 1.1, -0.1, 0.01)
    v.insert_pose2(2, 2.1, 0.1, 0.0)  # no factor yet
    d.update(g, v)
    g, v = NonlinearFactorGraph(), Values()
    g.add_BetweenFactorPose2(1, 2, [1.0, 0.0, 0.0], odo)
    d.update(g, v)  # two of three variables affected: recalculateBatch
    g, v = NonlinearFactorGraph(), Values()
    g.add_BetweenFactorPose2(2, 3, [1.0, 0.0, 0.0], odo)
    v.insert_pose2(3, 3.0, 0.0, 0.0)
    d.update(g, v)


def seq_removals(d):
    from isam2_examples import slamlike_steps
    for g, v in slamlike_steps():
        d.update(g, v)
    d.update(removeFactorIndices=[7, 14])  # the two measurements of landmark 100: it leaves the system
    d.update()
    br = noiseModel.Diagonal.Sigmas([np.pi / 100.0, 0.1])
    g, v = NonlinearFactorGraph(), Values()
    g.add_BearingRangeFactor2D(10, 100, np.pi / 4.0 + np.pi / 16.0, 4.5, br)
    g.add_BearingRangeFactor2D(5, 100, np.pi / 4.0, 5.0, br)
    v.insert_point2(100, [5.0 / np.sqrt(2.0), 5.0 / np.sqrt(2.0)])
    d.update(g, v)


EAGER = dict(relinearizeThreshold=0.01, relinearizeSkip=1)
SEQUENCES = {
    "visual": (seq_visual, ISAM2Params(**EAGER)),
    "city300": (seq_city, ISAM2Params()),
    "city300_partial": (seq_city, ISAM2Params(enablePartialRelinearizationCheck=True, **EAGER)),
    "fixed_lag300": (seq_fixed_lag, ISAM2Params(findUnusedFactorSlots=True)),
    "wide": (seq_wide, ISAM2Params(relinearizeThreshold=0.05, relinearizeSkip=2)),
    "dogleg": (seq_visual, ISAM2Params(ISAM2DoglegParams(1.0, 1e-5, 0), **EAGER)),
    "batch_threshold": (seq_batch_threshold, ISAM2Params(ISAM2GaussNewtonParams(0.001), 0.01, 1, True)),
    "removals": (seq_removals, ISAM2Params(**EAGER)),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sequences", default="", help="only the sequences whose name contains this")
    args = ap.parse_args()
    for name, (run, params) in SEQUENCES.items():
        if args.sequences not in name:
            continue
        d = Digest(name, params, args.device)
        run(d)
        d.isam.close()


if __name__ == "__main__":
    main()
