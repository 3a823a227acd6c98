"""TEST INFRASTRUCTURE: the numpy-only half of the geometry edge-case tests.  It reads tests/golden/geometry_edges.npz (inputs and
50-digit expected values rounded to FP64, written by tests/tools/make_geometry_edges.py from tests/geometry_reference.py), builds the
graphs and measures how far a computed [H1 H2 (H3) b] / retracted value is from the expected one.  The same measure gives the floors
(the CPU oracle's deviation, stored in the fixture) and checks the device (tests/test_gpu_geometry_edges.py), so neither mpmath nor
the reference tree is needed where the GPU test runs.

Deviations are max-abs differences relative to max(1, |expected|) of that case and quantity.  MODE_EXP3 compares Exp(sgn * b[:6])
with the fixture's pose instead of b itself; MODE_ANGLE compares the angle row as (cos, sin)."""
from __future__ import annotations

import os

import numpy as np

from gtsam_personal_amd.graph import (CAM_BUNDLER, F_BEARING_RANGE_2D, F_PRIOR_POINT3, FACTOR_ROWS, FACTOR_VARS, POSE2, POSE3, VAR_DIM,
                                      VAR_STORE, NonlinearFactorGraph, Values, noiseModel)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_edges.npz")
MODE_DIRECT, MODE_EXP3, MODE_ANGLE = 0, 1, 2
EPS = 2.0 ** -52
GPU_MARGIN = 16.0      # device sin / cos / acos / atan2 / tan are a couple of ulp looser than glibc's, and hipcc contracts multiply-adds
PROJECT_TOL = 1e-9     # the project's tolerance for Jacobians and errors (tests/test_gpu_parity.py): the margin may never pass it
ORTHO_TOL = 32 * EPS   # R^T R - I of a retracted pose: stored base (~2 eps) times Exp (~4 eps) and the 3-term products' rounding
BUCKET_SIZES = (1, 64, 65, 129)


def load():
    return dict(np.load(FIXTURE, allow_pickle=False))


def factor_types(fx):
    return sorted(int(k[1:-5]) for k in fx if k.startswith("f") and k.endswith("_vals"))


def split_vals(ft, flat):
    out, o = [], 0
    for t in FACTOR_VARS[ft]:
        out.append(flat[o:o + VAR_STORE[t]])
        o += VAR_STORE[t]
    return out


def build_factor_graph(fx, ftypes, n, robust=None):
    """the first n rows of every factor type in `ftypes`, each factor on variables of its own, Unit noise; returns (graph, values,
    [(ftype, row)] in graph order)"""
    graph, values, order, key = NonlinearFactorGraph(), Values(), [], 0
    for ft in ftypes:
        for i in range(n):
            keys = []
            for t, v in zip(FACTOR_VARS[ft], split_vals(ft, fx["f%d_vals" % ft][i])):
                values.insert(key, t, v)
                keys.append(key)
                key += 1
            graph._add(ft, [keys], fx["f%d_meas" % ft][i], noiseModel.Unit.Create(FACTOR_ROWS[ft]))
            order.append((ft, i))
    return graph, values, order


def build_robust_graph(fx, kind):
    graph, values, rows = NonlinearFactorGraph(), Values(), np.nonzero(fx["b_kind"] == kind)[0]
    for key, i in enumerate(rows):
        values.insert_point3(key, [fx["b_d"][i], 0.0, 0.0])
        m = noiseModel.Unit.Create(3)
        m.robust_kind, m.robust_k = int(kind), float(fx["b_k"][i])
        graph._add(F_PRIOR_POINT3, [[key]], [0.0, 0.0, 0.0], m)
    return graph, values, rows


def build_retract_graph(fx, vt):
    """every retract case of variable type vt as a variable with a prior on its own value; returns (graph, values, packed delta)"""
    from gtsam_personal_amd.graph import F_PRIOR_CAM, F_PRIOR_POSE2, F_PRIOR_POSE3
    ft = {POSE2: F_PRIOR_POSE2, POSE3: F_PRIOR_POSE3, CAM_BUNDLER: F_PRIOR_CAM}[vt]
    graph, values = NonlinearFactorGraph(), Values()
    for key, v in enumerate(fx["r%d_val" % vt]):
        values.insert(key, vt, v)
        graph._add(ft, [[key]], v, noiseModel.Unit.Create(VAR_DIM[vt]))
    return graph, values, {k: d for k, d in enumerate(fx["r%d_delta" % vt])}


def exp_se3(xi):
    """FP64 SE(3) exponential (Rodrigues; the half-angle form of 1 - cos), smooth through every angle the cases use"""
    w, v = np.asarray(xi[:3], dtype=float), np.asarray(xi[3:6], dtype=float)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-4:
        A, B, C = 1 - th2 / 6, 0.5 - th2 / 24, 1.0 / 6 - th2 / 120
    else:
        A, B = np.sin(th) / th, 2 * np.sin(th / 2) ** 2 / th2
        C = (1 - A) / th2
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.concatenate([(np.eye(3) + A * W + B * W @ W).reshape(-1), v + B * (W @ v) + C * (W @ (W @ v))])


def _dev(got, exp):
    got, exp = np.asarray(got, dtype=float).reshape(-1), np.asarray(exp, dtype=float).reshape(-1)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float(np.abs(got - exp).max() / max(1.0, np.abs(exp).max()))


def factor_deviation(fx, ft, i, J):
    """(deviation of e, of H, of the factor's error 0.5 |b|^2) of a computed (rows, cols) [H | b] from row i of type ft"""
    rows = FACTOR_ROWS[ft]
    Je = fx["f%d_J" % ft][i].reshape(rows, -1)
    assert J.shape == Je.shape, (ft, i, J.shape)
    mode, b, be = int(fx["f%d_mode" % ft][i]), J[:, -1], Je[:, -1]
    dH = _dev(J[:, :-1], Je[:, :-1])
    if mode == MODE_DIRECT:
        de = _dev(b, be)
    elif mode == MODE_EXP3:
        de = max(_dev(exp_se3(fx["f%d_sgn" % ft][i] * b[:6]), fx["f%d_aux" % ft][i]), _dev(b[6:], be[6:]) if rows > 6 else 0.0)
    else:
        a = 0 if ft == F_BEARING_RANGE_2D else 2
        rest = [r for r in range(rows) if r != a]
        de = max(_dev([np.cos(b[a]), np.sin(b[a])], [np.cos(be[a]), np.sin(be[a])]), _dev(b[rest], be[rest]))
    return de, dH, _dev(0.5 * float(b @ b), fx["f%d_err" % ft][i])


def retract_deviation(vt, got, exp):
    """(deviation of the retracted stored value, max |R^T R - I| of it)"""
    got, exp = np.asarray(got, dtype=float), np.asarray(exp, dtype=float)
    if vt == POSE2:
        return max(_dev(got[:2], exp[:2]), _dev([np.cos(got[2]), np.sin(got[2])], [np.cos(exp[2]), np.sin(exp[2])])), 0.0
    R = got[:9].reshape(3, 3)
    return max(_dev(got[:9], exp[:9]), _dev(got[9:12], exp[9:12]), _dev(got[12:], exp[12:]) if vt == CAM_BUNDLER else 0.0), \
        float(np.abs(R.T @ R - np.eye(3)).max())


def tolerance(floor):
    """the device tolerance of a quantity whose oracle deviation is `floor`"""
    tol = GPU_MARGIN * max(float(floor), EPS)
    assert tol <= PROJECT_TOL, "an ill-conditioned case inflates the floor: replace the case"
    return tol
