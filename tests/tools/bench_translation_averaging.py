#!/usr/bin/env python3
"""Side measurement (not the bench.py metric, not a test): 1dSfM translation averaging on a synthetic ring of cameras -- MFAS outlier
weights over --directions projection directions, then TranslationRecovery on the edges MFAS keeps.  Camera i sees its --band nearest
neighbours on either side (2 x band edges per camera), --outliers of the measured directions are replaced by random unit vectors, the
others carry a small angular noise.  One JSON line per --cameras value:
  mfas_kernel_ms / mfas_kernel_ms_per_direction   device time of one lmgpu_mfas_outlier_weights launch pair over all directions (median of
                                                  --reps), and that time divided by the number of directions (they run side by side)
  mfas_one_direction_ms                           the same launch pair with ONE direction: the length of the dependent chain of V steps
  mfas_call_ms                                    host wall clock of the whole call (checks, CSR, uploads, launches, downloads)
  mfas_outliers_found / mfas_inliers_dropped      planted outliers among the dropped edges (the planted fraction, largest sums first), inliers among them
  finalize_ms                                     lmgpu_translation_recovery_finalize (host logic, symbolic analysis, uploads)
  lm_iterations / lm_ms / lm_iterations_per_s     lmgpu_translation_recovery_run from ground truth perturbed by --init-noise
  position_error                                  largest distance to the ground truth after a similarity alignment, over the ring's radius
    python tests/tools/bench_translation_averaging.py [--cameras 1000 5000] [--band 10] [--directions 48] [--reps 5] [--solve-up-to 1000]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from gtsam_personal_amd import MFAS, BinaryMeasurement, LevenbergMarquardtParams, Values, noiseModel  # noqa: E402
from gtsam_personal_amd.translation_recovery import TranslationRecoverySession  # noqa: E402


def ring(V, band, outliers, seed):
    rng = np.random.RandomState(seed)
    R = V / (2 * np.pi)  # unit spacing along the ring
    a = 2 * np.pi * np.arange(V) / V
    pos = np.stack([R * np.cos(a), R * np.sin(a), rng.uniform(-1, 1, V)], axis=1)
    keys = np.array([(i, (i + k) % V) for k in range(1, band + 1) for i in range(V)], dtype=np.uint64)
    d = pos[keys[:, 1].astype(int)] - pos[keys[:, 0].astype(int)]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d += 0.01 * rng.normal(size=d.shape)
    bad = rng.rand(len(keys)) < outliers
    d[bad] = rng.normal(size=(int(bad.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pos, keys, d, bad


def dissection_order(V, band):
    """a nested-dissection elimination order of the banded ring: the last `band` nodes cut the ring open and go last, then intervals are
    halved by separators of `band` consecutive nodes"""
    order = []

    def interval(lo, hi):  # [lo, hi)
        if hi - lo <= 4 * band:
            order.extend(range(lo, hi))
            return
        mid = (lo + hi) // 2
        interval(lo, mid - band // 2)
        interval(mid - band // 2 + band, hi)
        order.extend(range(mid - band // 2, mid - band // 2 + band))

    interval(0, V - band)
    order.extend(range(V - band, V))
    return order


def align_error(got, want):
    """largest residual after the least-squares similarity (Umeyama) of got onto want"""
    mg, mw = got.mean(0), want.mean(0)
    G, W = got - mg, want - mw
    U, S, Vt = np.linalg.svd(W.T @ G)
    D = np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))])
    Rm = U @ D @ Vt
    s = (S * np.diag(D)).sum() / (G ** 2).sum()
    return float(np.linalg.norm(s * G @ Rm.T - W, axis=1).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, nargs="+", default=[1000, 5000])
    ap.add_argument("--band", type=int, default=10)
    ap.add_argument("--directions", type=int, default=48)
    ap.add_argument("--outliers", type=float, default=0.1)
    ap.add_argument("--init-noise", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve-up-to", type=int, default=1000,
                    help="largest ring on which TranslationRecovery is also SOLVED; above it MFAS and finalize only (DESIGN section 20: the "
                         "solve of the 5 000-camera ring ends in the engine's hand-off timeout)")
    args = ap.parse_args()
    for V in args.cameras:
        pos, keys, meas, bad = ring(V, args.band, args.outliers, seed=V)
        rng = np.random.RandomState(1)
        dirs = rng.normal(size=(args.directions, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        out = dict(cameras=V, edges=len(keys), directions=args.directions, planted_outliers=int(bad.sum()))
        MFAS.outlier_weights(keys, meas, dirs)  # warm-up
        kms, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            _, _, total, st = MFAS.outlier_weights(keys, meas, dirs)
            wall.append((time.perf_counter() - t) * 1e3)
            kms.append(st["kernel_ms"])
        one = [MFAS.outlier_weights(keys, meas, dirs[:1])[3]["kernel_ms"] for _ in range(args.reps)]
        out.update(mfas_kernel_ms=statistics.median(kms), mfas_kernel_ms_per_direction=statistics.median(kms) / args.directions,
                   mfas_one_direction_ms=statistics.median(one), mfas_call_ms=statistics.median(wall), mfas_global_state=st["global_state"])
        keep = np.ones(len(keys), dtype=bool)  # drop the planted fraction of the edges, those of the largest sums: never all of them
        keep[np.argsort(-total, kind="stable")[:int(round(args.outliers * len(keys)))]] = False
        out.update(mfas_outliers_found=int((~keep & bad).sum()), mfas_inliers_dropped=int((~keep & ~bad).sum()))
        model = noiseModel.Robust.Create(noiseModel.mEstimator.Huber.Create(1.345), noiseModel.Isotropic.Sigma(3, 0.02))
        rel = [BinaryMeasurement(int(a), int(b), z, model) for (a, b), z in zip(keys[keep].tolist(), meas[keep])]
        init = Values()
        irng = np.random.RandomState(2)
        for i in range(V):
            init.insert_point3(i, pos[i] + args.init_noise * irng.uniform(-1, 1, 3))
        s = TranslationRecoverySession(device=0)
        s.add_directions(rel)
        t = time.perf_counter()
        s.finalize(float(np.linalg.norm(pos[int(rel[0].key2())] - pos[int(rel[0].key1())])), init, dissection_order(V, args.band))
        out["finalize_ms"] = (time.perf_counter() - t) * 1e3
        out["recovery_edges"] = len(rel)
        if V > args.solve_up_to:  # MFAS and finalize only
            s.close()
            print(json.dumps(out), flush=True)
            continue
        p = LevenbergMarquardtParams()
        s.run(p)  # warm-up: run() starts from the initial values every time
        t = time.perf_counter()
        state = s.run(p)
        ms = (time.perf_counter() - t) * 1e3
        got = s.get()
        have = [i for i in range(V) if got.exists(i)]
        out.update(lm_iterations=state.iterations, lm_inner_iterations=state.totalNumberInnerIterations, lm_ms=ms,
                   lm_iterations_per_s=state.iterations / (ms * 1e-3), lm_final_error=state.error,
                   cameras_recovered=len(have),  # a camera all of whose edges were dropped has no position
                   position_error=align_error(np.stack([got.at(i) for i in have]), pos[have]) / (V / (2 * np.pi)))
        s.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
