"""Writes tests/golden/factor_bucket_edges.npz for tests/factor_bucket_cases.py:
  * 37 seeded, well-conditioned cases for every factor type: stored FP64 values and measurement, and the UNWHITENED [H1 H2 (H3) | b]
    (b = -e) evaluated in 50 digits by tests/geometry_reference.py (the four linear types -- prior Point3, prior Cal3_S2, chordal
    between, prior Vec9 -- are stated here) and rounded to FP64.  Benign inputs: rotation angles in [0.2, 2.5] rad (of the stored
    rotations and of every pose error), depths in [2, 20], ranges above 1, nothing behind a camera; the singular branches stay with
    tests/golden/geometry_edges.npz.  The cases are chained so that graphs can share variables (see factor_bucket_cases.py);
  * 37 retract cases (value, delta, 50-digit retracted value) per variable type, on the same chained values;
  * the floors: the CPU oracle's largest deviation from the reference chain per quantity and noise kind, over the whole case table.

    python tests/tools/make_factor_bucket_edges.py          (after __graft_entry__.build(): the floors need oracle/liblm_oracle.so)

tests/test_factor_bucket_reference.py regenerates all of it in memory and compares it with the committed file."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import factor_bucket_cases as fb  # noqa: E402
import geometry_reference as gr  # noqa: E402
from gtsam_personal_amd.graph import (CAL3_S2, CAM_BUNDLER, F_BEARING_RANGE_2D, F_BETWEEN_POSE2, F_BETWEEN_POSE3, F_CHORDAL_BETWEEN,  # noqa: E402
                                      F_PRIOR_CAL3_S2, F_PRIOR_CAM, F_PRIOR_POINT3, F_PRIOR_POSE2, F_PRIOR_POSE3, F_PRIOR_VEC9,
                                      F_PROJECTION, F_PROJECTION_BPS, F_SFM, F_SFM2, FACTOR_ROWS, FACTOR_VARS, POINT2, POINT3, POSE2,
                                      POSE3, VAR_DIM, VEC9)

N = fb.NCASE
M = gr.M
K0 = np.array([520.0, 480.0, 1.75, 320.0, 240.0])


# ---------------------------------------------------------------- FP64 input generation (the stored numbers are the cases)
def _rot(rng, lo=0.2, hi=2.5):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(lo, hi)
    W = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * W + (1 - np.cos(th)) * W @ W


def _pose3(rng, tscale=5.0):
    return np.concatenate([_rot(rng).reshape(-1), rng.uniform(-tscale, tscale, 3)])


def _compose3(a, b):
    Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    return np.concatenate([(Ra @ Rb).reshape(-1), a[9:] + Ra @ b[9:]])


def _inverse3(a):
    R = a[:9].reshape(3, 3)
    return np.concatenate([R.T.reshape(-1), -R.T @ a[9:]])


def _compose2(a, b):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], a[2] + b[2]])


def _inverse2(a):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), -a[2]])


def _in_front(rng, pose):
    """a world point at depth [2, 20] in front of `pose`, within half a unit of the axis at unit depth"""
    z = rng.uniform(2.0, 20.0)
    return pose[9:] + pose[:9].reshape(3, 3) @ np.array([rng.uniform(-0.5, 0.5) * z, rng.uniform(-0.5, 0.5) * z, z])


def _pixel(x):
    """pixels on a 2^-10 grid: the host's subtraction of Cal3Bundler's principal point from them is exact"""
    return np.round(np.asarray(x) * 1024.0) / 1024.0


def inputs():
    """{ftype: [(vals list, meas)]}, chained as factor_bucket_cases.py describes"""
    rng = np.random.default_rng(20261018)
    P2 = [np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-3, 3)]) for _ in range(N)]
    P3 = [_pose3(rng) for _ in range(N)]
    V9 = [rng.uniform(-1, 1, 9) for _ in range(N)]
    PT = [_in_front(rng, P3[0]) for _ in range(N)]
    T = {ft: [] for ft in fb.FACTOR_TYPES}
    sign = lambda: 1.0 if rng.random() < 0.5 else -1.0  # noqa: E731
    for i in range(N):
        j = (i + 1) % N
        # Pose2: the error is between(z, between(a, b)); z = h o e^-1 leaves the error e, angle in +-[0.2, 1]
        e2 = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), sign() * rng.uniform(0.2, 1.0)])
        h2 = _compose2(_inverse2(P2[i]), P2[j])
        T[F_BETWEEN_POSE2].append(([P2[i], P2[j]], _compose2(h2, _inverse2(e2))))
        T[F_PRIOR_POSE2].append(([P2[i]], _compose2(P2[i], np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), sign() * rng.uniform(0.2, 1.0)]))))
        r, a = rng.uniform(1.5, 10.0), rng.uniform(-3, 3)
        lm = P2[i][:2] + r * np.array([np.cos(a), np.sin(a)])
        T[F_BEARING_RANGE_2D].append(([P2[i], lm], np.array([a - P2[i][2] + sign() * rng.uniform(0.1, 0.5), r + rng.uniform(-0.5, 0.5)])))
        # Pose3: a relative pose whose rotation angle lies in [0.2, 2.5]
        e3 = np.concatenate([_rot(rng).reshape(-1), rng.uniform(-1, 1, 3)])
        h3 = _compose3(_inverse3(P3[i]), P3[j])
        T[F_BETWEEN_POSE3].append(([P3[i], P3[j]], _compose3(h3, _inverse3(e3))))
        T[F_PRIOR_POSE3].append(([P3[i]], _compose3(P3[i], np.concatenate([_rot(rng).reshape(-1), rng.uniform(-1, 1, 3)]))))
        cal = np.array([rng.uniform(400, 600), rng.uniform(-0.05, 0.05), rng.uniform(-0.01, 0.01), 3.0, -2.0])
        cam = np.concatenate([P3[i], cal])
        T[F_PRIOR_CAM].append(([cam], np.concatenate([_compose3(P3[i], np.concatenate([_rot(rng).reshape(-1), rng.uniform(-1, 1, 3)])),
                                                      cal[:3] + np.array([rng.uniform(-5, 5), rng.uniform(-0.01, 0.01), rng.uniform(-0.002, 0.002)]),
                                                      cal[3:]])))
        # projections: measured pixel = the FP64 projection moved by up to 2 px
        pt = _in_front(rng, P3[i])
        px = [float(x) for x in gr.project_bundler(gr.pose3(P3[i]), gr.V(pt), *gr.V(cal))]
        T[F_SFM].append(([cam, pt], _pixel(np.array(px) + rng.uniform(-2, 2, 2))))
        pt = _in_front(rng, P3[i])
        px = [float(x) for x in gr.project_cal3_s2(gr.pose3(P3[i]), gr.V(pt), gr.V(K0))]
        T[F_PROJECTION].append(([P3[i], pt], np.concatenate([_pixel(np.array(px) + rng.uniform(-2, 2, 2)), K0])))
        sensor = np.concatenate([_rot(rng, 0.2, 0.6).reshape(-1), rng.uniform(-0.2, 0.2, 3)])
        pt = _in_front(rng, _compose3(P3[i], sensor))
        px = [float(x) for x in gr.project_cal3_s2(gr.pose3(P3[i]), gr.V(pt), gr.V(K0), gr.pose3(sensor))]
        T[F_PROJECTION_BPS].append(([P3[i], pt], np.concatenate([_pixel(np.array(px) + rng.uniform(-2, 2, 2)), K0, sensor])))
        px = [float(x) for x in gr.project_cal3_s2(gr.pose3(P3[0]), gr.V(PT[i]), gr.V(K0))]
        T[F_SFM2].append(([P3[0], PT[i], K0], _pixel(np.array(px) + rng.uniform(-2, 2, 2))))
        # the linear types
        T[F_PRIOR_POINT3].append(([PT[i]], PT[i] + rng.uniform(-1, 1, 3)))
        T[F_PRIOR_CAL3_S2].append(([K0], K0 + rng.uniform(-3, 3, 5)))
        T[F_CHORDAL_BETWEEN].append(([V9[i], V9[j]], _rot(rng).reshape(-1)))
        T[F_PRIOR_VEC9].append(([V9[i]], rng.uniform(-1, 1, 9)))
    return T


def retract_inputs(T):
    """{vtype: [(value, delta)]} on the chained values"""
    rng = np.random.default_rng(37)
    src = {POSE2: F_PRIOR_POSE2, POSE3: F_PRIOR_POSE3, POINT3: F_PRIOR_POINT3, CAM_BUNDLER: F_PRIOR_CAM, CAL3_S2: F_PRIOR_CAL3_S2,
           VEC9: F_PRIOR_VEC9}
    out = {}
    for vt in fb.VAR_TYPES:
        rows = []
        for i in range(N):
            val = T[F_BEARING_RANGE_2D][i][0][1] if vt == POINT2 else T[src[vt]][i][0][0]
            d = rng.uniform(-1, 1, VAR_DIM[vt])
            if vt in (POSE3, CAM_BUNDLER):
                w = rng.normal(size=3)
                d[:3] = w / np.linalg.norm(w) * rng.uniform(0.2, 2.5)
            if vt == CAM_BUNDLER:
                d[6:] *= [5.0, 0.01, 0.002]
            rows.append((val, d))
        out[vt] = rows
    return out


# ---------------------------------------------------------------- 50-digit evaluation
def linear_factor(ft, vals, meas):
    """(e, [H...]) of the four linear types, exact in the stored numbers"""
    v0 = gr.V(vals[0])
    m = gr.V(meas)
    if ft in (F_PRIOR_POINT3, F_PRIOR_CAL3_S2, F_PRIOR_VEC9):
        return gr.sub(v0, m), [gr._ident(len(v0))]
    assert ft == F_CHORDAL_BETWEEN      # e = blockdiag(Rij, Rij, Rij) v1 - v0 with Rij = meas row-major
    v1 = gr.V(vals[1])
    e = [sum(m[3 * i + c] * v1[3 * k + c] for c in range(3)) - v0[3 * k + i] for k in range(3) for i in range(3)]
    H2 = gr.zeros(9, 9)
    for k in range(3):
        for i in range(3):
            for c in range(3):
                H2[3 * k + i][3 * k + c] = m[3 * i + c]
    return e, [[gr.sc(-1, r) for r in gr._ident(9)], H2]


def retract_value(vt, val, delta):
    if vt in (POSE2, POSE3, CAM_BUNDLER):
        return gr.retract_value(vt, val, delta)
    return gr.add(gr.V(val), gr.V(delta))


def expected():
    """every array of the fixture that comes from the 50-digit reference alone"""
    fx, T = {}, inputs()
    for ft, rows in T.items():
        J = []
        for vals, meas in rows:
            if ft in (F_PRIOR_POINT3, F_PRIOR_CAL3_S2, F_CHORDAL_BETWEEN, F_PRIOR_VEC9):
                e, H = linear_factor(ft, vals, meas)
            else:
                e, H, info = gr.evaluate_factor(ft, vals, meas)
                assert all(x in ("acos", "fullw", "front", "bfull", "rfull") for x in info), (ft, info)
            J.append([float(x) for i in range(FACTOR_ROWS[ft]) for x in sum((list(h[i]) for h in H), []) + [-e[i]]])
        fx["f%d_vals" % ft] = np.array([np.concatenate(v) for v, _ in rows])
        fx["f%d_meas" % ft] = np.array([m for _, m in rows])
        fx["f%d_J" % ft] = np.array(J)
        assert fx["f%d_J" % ft].shape == (N, fb.factor_size(ft)) and np.all(np.isfinite(fx["f%d_J" % ft]))
    for vt, rows in retract_inputs(T).items():
        fx["r%d_val" % vt] = np.array([r[0] for r in rows])
        fx["r%d_delta" % vt] = np.array([r[1] for r in rows])
        fx["r%d_exp" % vt] = np.array([[float(x) for x in retract_value(vt, r[0], r[1])] for r in rows])
    return fx


# ---------------------------------------------------------------- floors: the CPU oracle against the reference chain
FLOOR_KEYS = ("floor_J", "floor_err", "floor_hdiag", "floor_lin")


def oracle_deviations(fx):
    """the CPU oracle over every case of the classes it has a counterpart for (it has no GNC weights; reduce is exact and retract has
    a one-ulp floor by decree).  Returns (floors as fixture arrays, per-case deviations, per solved case (e0, e1, reduction) of the
    reference at the oracle's own delta).
      floor_J, floor_err   [factor type][unit, diagonal, gaussian][m-estimator id, 0 = none]: the factor's [A b]; its error -- without
                           Robust 0.5 |b|^2 of the oracle's b, factor by factor; with it the oracle's graph error over the (homogeneous) case
      floor_hdiag          [m-estimator id]: the Hessian diagonal, per variable
      floor_lin            (e0, e1) of solve() against the reference at the returned delta"""
    import oracle_harness as oh
    fl = dict(floor_J=np.zeros((14, 3, 9)), floor_err=np.zeros((14, 3, 9)), floor_hdiag=np.zeros(9), floor_lin=np.zeros(2))
    per_case, solved = {}, {}
    for name, (cls, _) in fb.CASES.items():
        if cls == "retract" or name == "interleaved_gnc":
            continue
        c = fb.build(fx, name)
        orc = oh.OracleProblem(c.graph, c.values, c.ordering)
        orc.linearize()
        blocks = c.reference_blocks()
        dJ = de = 0.0
        total = fb.fsum(b[1] for b in blocks)
        dtot = fb.dev(orc.error(), total)
        for g, (f, (Ab, err, _)) in enumerate(zip(c.factors, blocks)):
            s, J = fb.floor_index(f), orc.jacobian(g)
            a = fb.dev(J, fb.to_f64(Ab))
            b = dtot if s[2] else fb.dev(0.5 * float(J[:, -1] @ J[:, -1]), float(err))
            fl["floor_J"][s], fl["floor_err"][s] = max(fl["floor_J"][s], a), max(fl["floor_err"][s], b)
            dJ, de = max(dJ, a), max(de, b)
        hd, ref = orc.hessian_diagonal(), c.hessian_diagonal(blocks)
        dh = max(fb.dev(hd[k], fb.to_f64(ref[k])) for k in ref)
        rk = max(f["model"].robust_kind for f in c.factors)
        fl["floor_hdiag"][rk] = max(fl["floor_hdiag"][rk], dh)
        per_case[name] = (dJ, de, dh, dtot)
        if cls in ("linear_error", "interleaved"):
            rc, delta, e0, e1 = orc.solve(fb.LAMBDA)
            assert rc == 0, name
            r0, r1 = c.linear_errors(blocks, delta)
            fl["floor_lin"][0] = max(fl["floor_lin"][0], fb.dev(e0, r0))
            fl["floor_lin"][1] = max(fl["floor_lin"][1], fb.dev(e1, r1))
            solved[name] = (r0, r1, (r0 - r1) / r0)
            per_case[name] += (fb.dev(e0, r0), fb.dev(e1, r1))
    return fl, per_case, solved


def generate():
    fx = expected()
    fx.update(oracle_deviations(fx)[0])
    return fx


if __name__ == "__main__":
    out = generate()
    np.savez_compressed(fb.FIXTURE, **out)
    print("wrote %s: %d arrays, %d bytes" % (fb.FIXTURE, len(out), os.path.getsize(fb.FIXTURE)))
    for k in FLOOR_KEYS:
        print(k, "max %.3g" % out[k].max(), out[k] if out[k].size < 10 else "")
