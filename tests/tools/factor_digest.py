"""Digests of what the batch path's factor kernels write, one line per case of the `whiten` and `interleaved` families of
tests/factor_bucket_cases.py (every factor type under both noise kinds at 1, 127, 128 and 129 factors; all types interleaved in graph
order, plain and under GNC weights):

    <case> J=<fnv1a> error=<fnv1a>

J: an FNV-1a over the bit patterns of every factor's whitened [A b], jacobian(g) in graph order, after linearize(); error: one over the
bits of graph_error() (FNV-1a taken over 64-bit words: xor the word, multiply by the prime).

Equal lines mean the same kernels wrote the same bits.  That is how a change to how the factor kernels are instantiated or launched is
held against its parent: run this file in both, the parent twice (a line the parent does not reproduce against itself proves nothing),
compare the outputs.  The incremental path has tests/tools/isam2_digest.py.  Needs a GPU.

    python tests/tools/factor_digest.py [--device N] [--cases SUBSTRING] > factors.txt
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import factor_bucket_cases as fb  # noqa: E402
from gtsam_personal_amd import LevenbergMarquardtOptimizer  # noqa: E402
from gtsam_personal_amd.optimizer import GncLMParams, GncOptimizer  # noqa: E402

MASK = (1 << 64) - 1


def fnv1a(words, h=0xcbf29ce484222325):
    for w in words:
        h = ((h ^ w) * 0x100000001b3) & MASK
    return h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cases", default="", help="only the cases whose name contains this")
    args = ap.parse_args()
    fx = fb.load()
    for name in fb.names("whiten") + fb.names("interleaved"):
        if args.cases not in name:
            continue
        c = fb.build(fx, name)
        if c.weights is None:
            opt = LevenbergMarquardtOptimizer(c.graph, c.values, c.ordering, device=args.device)
        else:
            gnc = GncOptimizer(c.graph, c.values, GncLMParams(), c.ordering, device=args.device)
            gnc.setWeights(c.weights)
            opt = gnc.base()
        opt.linearize()
        h = 0xcbf29ce484222325
        for g in range(len(c.factors)):
            h = fnv1a(np.ascontiguousarray(opt.jacobian(g), dtype=np.float64).reshape(-1).view(np.uint64).tolist(), h)
        e = fnv1a(np.array([opt.graph_error()], dtype=np.float64).view(np.uint64).tolist())
        print(f"{name} J={h:016x} error={e:016x}", flush=True)


if __name__ == "__main__":
    main()
