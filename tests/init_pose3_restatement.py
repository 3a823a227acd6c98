"""TEST INFRASTRUCTURE: numpy restatement of the reference's InitializePose3, the checker of the device implementation.  It shares no
numerics with the library: dense / scipy.sparse linear algebra, numpy.linalg.svd, and the frozen CPU oracle for the Gauss-Newton step.

Which reference lines each function restates (gtsam/slam/InitializePose3.cpp unless stated otherwise):
  extract                  initialize::buildPoseGraph<Pose3>, InitializePose.h:36-52
  rotation_precision       :48-51 (first entry of noiseModel->whitenInPlace(e1)), per noise kind
  linear_orientation_rows  buildLinearOrientationGraph :37-71 (whitened [A1 A2 b] per factor + the anchor's prior)
  relaxed_orientations     GaussianFactorGraph::optimize of it (normal equations; scipy.sparse when importable, else dense)
  closest_to               SO3::ClosestTo, gtsam/geometry/SO3.cpp:202-208
  normalize_relaxed        normalizeRelaxedRotations :75-92
  orientations_chordal     computeOrientationsChordal :102-114
  symbolic_graph           createSymbolicGraph :221-253
  logmap / expmap          SO3::Logmap gtsam/geometry/SO3.cpp:299-375, so3::ExpmapFunctor :61-95
  gradient_tron            gradientTron :256-275
  orientations_gradient    computeOrientationsGradient :117-218 (returns the per-iteration maxGrad trace as well)
  compute_poses            initialize::computePoses<Pose3>, InitializePose.h:57-97 (Gauss-Newton = the CPU oracle)
  initialize               initialize :296-319
An edge is (k0, k1, R 3x3, t 3, NoiseModel), in graph order."""
from __future__ import annotations

import math

import numpy as np

from gtsam_personal_amd.graph import (F_BETWEEN_POSE3, F_PRIOR_POSE3, N_DIAG, N_GAUSS, N_ISO, N_UNIT, POSE3, NoiseModel, NonlinearFactorGraph,
                                      Ordering, Values)

ANCHOR = 99999999


def extract(graph: NonlinearFactorGraph):
    rec = []
    for ftype, _, gi, keys, meas, _, models in graph.buckets():
        for i, g in enumerate(gi.tolist()):
            rec.append((g, ftype, keys[i], meas[i], models[i]))
    rec.sort(key=lambda r: r[0])
    edges = []
    for _, ftype, keys, meas, model in rec:
        R, t = meas[:9].reshape(3, 3).copy(), meas[9:12].copy()
        if ftype == F_BETWEEN_POSE3:
            edges.append((int(keys[0]), int(keys[1]), R, t, model))
        elif ftype == F_PRIOR_POSE3:
            edges.append((ANCHOR, int(keys[0]), R, t, model))
    return edges


def rotation_precision(model: NoiseModel):
    e1 = np.zeros(6)
    e1[0] = 1.0
    if model.kind == N_UNIT:
        return 1.0
    if model.kind == N_ISO:
        return float((e1 / float(model.data))[0])
    if model.kind == N_DIAG:
        return float((e1 / model.data)[0])
    assert model.kind == N_GAUSS
    return float((model.data @ e1)[0])


def linear_orientation_rows(edges):
    """[(keys, whitened A blocks, whitened b)] like the reference's JacobianFactors"""
    out = []
    for k0, k1, R, _, model in edges:
        s = math.sqrt(rotation_precision(model))  # Isotropic::Precision(9, p): sigma = 1 / sqrt(p)
        M9 = np.zeros((9, 9))
        for b in range(3):
            M9[3 * b:3 * b + 3, 3 * b:3 * b + 3] = R
        out.append(((k0, k1), (-s * np.eye(9), s * M9), np.zeros(9)))
    out.append(((ANCHOR,), (np.eye(9),), np.eye(3).reshape(9)))
    return out


def relaxed_orientations(edges):
    rows = linear_orientation_rows(edges)
    keys = sorted({k for ks, _, _ in rows for k in ks})
    col = {k: 9 * i for i, k in enumerate(keys)}
    n = 9 * len(keys)
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        ri, ci, vv, bb = [], [], [], []
        r0 = 0
        for ks, As, b in rows:
            for k, A in zip(ks, As):
                nz = np.nonzero(A)
                ri.extend((r0 + nz[0]).tolist())
                ci.extend((col[k] + nz[1]).tolist())
                vv.extend(A[nz].tolist())
            bb.extend(b.tolist())
            r0 += 9
        A = sp.csr_matrix((vv, (ri, ci)), shape=(r0, n))
        x = spl.spsolve((A.T @ A).tocsc(), A.T @ np.array(bb))
    except ImportError:
        H, g = np.zeros((n, n)), np.zeros(n)
        for ks, As, b in rows:
            for k, A in zip(ks, As):
                g[col[k]:col[k] + 9] += A.T @ b
                for k2, A2 in zip(ks, As):
                    H[col[k]:col[k] + 9, col[k2]:col[k2] + 9] += A.T @ A2
        x = np.linalg.solve(H, g)
    return {k: x[col[k]:col[k] + 9].copy() for k in keys}


def closest_to(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def normalize_relaxed(relaxed):
    out = {}
    for k, v in relaxed.items():
        if k != ANCHOR:
            M = np.asarray(v).reshape(3, 3).T  # Eigen::Map<const Matrix3>: column-major
            out[k] = closest_to(M.T)
    return out


def orientations_chordal(edges):
    return normalize_relaxed(relaxed_orientations(edges))


def symbolic_graph(edges):
    adj = {}
    for i, (k0, k1, _, _, _) in enumerate(edges):
        adj.setdefault(k0, []).append(i)
        adj.setdefault(k1, []).append(i)
    return adj


def expmap(w):
    w = np.asarray(w, dtype=np.float64)
    theta2 = float(w @ w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if theta2 <= np.finfo(np.float64).eps:
        A, B = 1.0 - theta2 / 6.0, 0.5 - theta2 / 24.0
    else:
        theta = math.sqrt(theta2)
        A = math.sin(theta) / theta
        s2 = math.sin(theta / 2.0)
        B = 2.0 * s2 * s2 / theta2
    return np.eye(3) + A * W + B * (W @ W)


def logmap(R):
    R11, R12, R13 = R[0]
    R21, R22, R23 = R[1]
    R31, R32, R33 = R[2]
    tr = R11 + R22 + R33
    if tr + 1.0 < 1e-3:
        if R33 > R22 and R33 > R11:
            W, Q1, Q2, Q3 = R21 - R12, 2.0 + 2.0 * R33, R31 + R13, R23 + R32
            order = lambda s: np.array([s * Q2, s * Q3, s * Q1])
        elif R22 > R11:
            W, Q1, Q2, Q3 = R13 - R31, 2.0 + 2.0 * R22, R23 + R32, R12 + R21
            order = lambda s: np.array([s * Q3, s * Q1, s * Q2])
        else:
            W, Q1, Q2, Q3 = R32 - R23, 2.0 + 2.0 * R11, R12 + R21, R31 + R13
            order = lambda s: np.array([s * Q1, s * Q2, s * Q3])
        r = math.sqrt(Q1)
        norm = math.sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W)
        sgn = -1.0 if W < 0 else 1.0
        mag = math.pi - (2 * sgn * W) / norm
        return order(sgn * 0.5 / r * mag)
    tr_3 = tr - 3.0
    if tr_3 < -1e-6:
        c = (tr - 1.0) / 2.0
        theta = math.acos(c) if -1.0 <= c <= 1.0 else float("nan")
        magnitude = theta / (2.0 * math.sin(theta))
    else:
        magnitude = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0
    return magnitude * np.array([R32 - R23, R13 - R31, R21 - R12])


def gradient_tron(R1, R2, a, b):
    l = logmap(R1.T @ R2)
    th = float(np.linalg.norm(l))
    if th != th:
        R1pert = R1 @ expmap([0.01, 0.01, 0.01])
        l = logmap(R1pert.T @ R2)
        th = float(np.linalg.norm(l))
    if th > 1e-5 and th == th:
        l = l / th
    else:
        l = np.zeros(3)
        th = 0.0
    return a * b * th * math.exp(-b * th) * l


def gradient_constants(max_deg):
    b = 1.0
    f0 = 1 / b - (1 / b + math.pi) * math.exp(-b * math.pi)
    a = (math.pi * math.pi) / (2 * f0)
    rho = 2 * a * b
    return a, b, 2 / (max_deg * rho)


def orientations_gradient(edges, guess_rots, max_iter=10000, set_ref_frame=True):
    """guess_rots {key: R}; returns ({key: R}, iterations run, [maxGrad per iteration])"""
    inv = {ANCHOR: np.eye(3)}
    for k, R in guess_rots.items():
        inv.setdefault(k, np.asarray(R, dtype=np.float64).T.copy())
    adj = symbolic_graph(edges)
    a, b, stepsize = gradient_constants(max(len(adj[k]) for k in inv))
    trace = []
    it = 0
    while it < max_iter:
        grad, max_grad = {}, 0.0
        for key, Ri in inv.items():
            g = np.zeros(3)
            for fid in adj[key]:
                k0, k1, Rij = edges[fid][0], edges[fid][1], edges[fid][2]
                if key == k0:
                    g = g + gradient_tron(Ri, Rij @ inv[k1], a, b)
                elif key == k1:
                    g = g + gradient_tron(Ri, Rij.T @ inv[k0], a, b)
            grad[key] = stepsize * g
            n = float(np.linalg.norm(g))
            if n > max_grad:
                max_grad = n
        for key in inv:
            inv[key] = inv[key] @ expmap(grad[key])
        trace.append(max_grad)
        if it > 20 and max_grad < 5e-3:
            it += 1
            break
        it += 1
    ref = inv[ANCHOR]
    out = {k: (ref @ R.T if set_ref_frame else R.T.copy()) for k, R in inv.items() if k != ANCHOR}
    return out, it, trace


def pose_problem(rots, edges):
    """the graph and start of computePoses: poses (R, 0), the anchor at the identity with a Unit(6) prior"""
    g, v = NonlinearFactorGraph(), Values()
    for k0, k1, R, t, model in edges:
        g.add_BetweenFactorPose3(k0, k1, R, t, model)
    g.add_PriorFactorPose3(ANCHOR, np.eye(3), np.zeros(3), NoiseModel(6, N_UNIT))
    for k, R in rots.items():
        v.insert_pose3(k, R, np.zeros(3))
    v.insert_pose3(ANCHOR, np.eye(3), np.zeros(3))
    return g, v


def compute_poses(rots, edges, single_iter=True, ordering=None):
    import oracle_harness as oh
    from gtsam_personal_amd.optimizer import GaussNewtonParams
    g, v = pose_problem(rots, edges)
    prob = oh.OracleProblem(g, v, ordering if ordering is not None else Ordering.Natural(g))
    p = GaussNewtonParams()
    if single_iter:
        p.maxIterations = 1
    prob.lm_init(p)
    prob.gn_optimize(p)
    res = prob.values()  # {key: packed value}
    out = Values()
    for k in sorted(res):
        if k != ANCHOR:
            out.insert(k, POSE3, res[k])
    return out


def initialize(graph, given_guess_rots=None, use_gradient=False, ordering=None):
    edges = extract(graph)
    if use_gradient:
        rots, _, _ = orientations_gradient(edges, given_guess_rots)
    else:
        rots = orientations_chordal(edges)
    return compute_poses(rots, edges, True, ordering)


def graph_error(graph, values, ordering=None):
    import oracle_harness as oh
    return oh.OracleProblem(graph, values, ordering if ordering is not None else Ordering.Natural(graph)).error()
