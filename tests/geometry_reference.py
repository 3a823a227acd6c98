"""TEST INFRASTRUCTURE: the 50-digit reference of the geometry the factor and retract kernels evaluate, and the table of edge cases
that drives both the CPU oracle (tests/test_geometry_reference.py) and, through tests/golden/geometry_edges.npz, the HIP kernels
(tests/test_gpu_geometry_edges.py).  It shares no code with the library or with oracle/: everything is mpmath at mp.dps = 50 on the
stored FP64 inputs taken as exact numbers.

EXACT LAYER -- mathematical definitions, no series, no thresholds:
  se3_exp / se2_exp            matrix exponential of the twist (mp.expm)
  se3_log / se2_log            their inverses: angle = atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2), axis = vee(R - R^T) normalised, the
                               translation by solving V(w) u = t.  The only special points are the ones where that expression is 0 / 0:
                               R = I (log 0) and an exact half-turn (R symmetric: the axis is the eigenvector of R + I)
  compose3 / inverse3 / between3 / adjoint3, compose2 / inverse2 / between2 / adjoint2
  project_cal3_s2, project_bundler, bearing2, range2
  numerical_jacobian           central difference, step 1e-20 (exact to ~1e-30 at 50 digits; the logs work at 120 digits inside)

DOCUMENTED-FORMULA LAYER -- only where the library's contract (include/lmgpu.h, the comments of csrc/geometry_dev.hpp and
csrc/kernels_factors.hpp) is not exact mathematics, every branch evaluated in 50 digits:
  so3_logmap_formula           three regimes: tr + 1 < 1e-3 (first order about pi, sub-branch by the largest diagonal entry, sgn_w),
                               tr - 3 < -1e-6 (acos), else the Taylor magnitude 0.5 - (tr-3)/12 + (tr-3)^2/60
  pose3_logmap_formula         |w| < 1e-10: u = t, else u = t - (|w|/2) a x t + (1 - |w| / (2 tan(|w|/2))) a x (a x t)
  expmap_coefficients          theta^2 <= 1e-5: A = 1 - th2/6, B = 1/2 - th2/24, C = 1/6 - th2/120
  pose2 chart                  retract = compose(Pose2(d)), local = (x, y, theta) of the relative pose, theta = atan2(s, c)
  cheirality                   qz <= 0: projection factors give (2 fx, 2 fx) and zero Jacobians, the SFM factors a zero error
  bearing / range guards       |q| <= 1e-5: bearing (1, 0) with zero Jacobian; r <= 1e-10: range Jacobian (1, 1)
  robust_weight / robust_loss  the eight m-estimators
The Jacobian contract of BETWEEN_POSE3 / BETWEEN_POSE2 is H1 = -Ad(h^-1), H2 = I (the derivative of between, not of Local) and the
priors have H = I; between_jacobian_numeric() is the branch-free derivative they are checked against.

THE CASE TABLE -- factor_cases(), retract_cases(), robust_cases().  Every thresholded quantity stays at least 1 % away from its
threshold except where a case is named "exact".  Cases whose relative rotation is within 1e-6 of a half-turn, or on the tie axis
(0, 1, 1) / sqrt 2, are compared through Exp(e) (MODE_EXP3): the sign of w is ambiguous at pi and either permutation is valid on a tie.
Pose2 / bearing cases whose relative angle is exactly +-pi are compared as (cos, sin) (MODE_ANGLE): atan2(+-0, -1) may take either sign.
The renormalisation inside compose2 cannot be reached through the ABI (c and s always come from cos / sin of a stored angle), so there
is no case for it."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from gtsam_personal_amd.graph import (CAL3_S2, CAM_BUNDLER, F_BEARING_RANGE_2D, F_BETWEEN_POSE2, F_BETWEEN_POSE3, F_PRIOR_CAM,
                                      F_PRIOR_POSE2, F_PRIOR_POSE3, F_PROJECTION, F_PROJECTION_BPS, F_SFM, F_SFM2, FACTOR_VARS, POINT2, POINT3,
                                      POSE2, POSE3)

mp.mp.dps = 50
M = mp.mpf
MODE_DIRECT, MODE_EXP3, MODE_ANGLE = 0, 1, 2
ROWS_PER_TYPE = 129  # the largest bucket of the GPU test (one block of 128 lanes and one lane of the next)


# ---------------------------------------------------------------- small linear algebra on lists of mpf
def V(a):
    return [M(float(x)) for x in a]


def M3(v9):
    return [[M(float(v9[3 * i + j])) for j in range(3)] for i in range(3)]


def eye3():
    return [[M(int(i == j)) for j in range(3)] for i in range(3)]


def mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def mv(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def tp(A):
    return [[A[j][i] for j in range(len(A))] for i in range(len(A[0]))]


def add(a, b):
    return [x + y for x, y in zip(a, b)]


def sub(a, b):
    return [x - y for x, y in zip(a, b)]


def sc(s, a):
    return [s * x for x in a]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def norm(a):
    return mp.sqrt(dot(a, a))


def skew(w):
    return [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]


def pose3(v12):
    return M3(v12[:9]), V(v12[9:12])


def flat3(p):
    return [float(p[0][i][j]) for i in range(3) for j in range(3)] + [float(x) for x in p[1]]


# ---------------------------------------------------------------- exact layer
def se3_exp(xi):
    X = mp.zeros(4)
    W = skew(xi[:3])
    for i in range(3):
        for j in range(3):
            X[i, j] = W[i][j]
        X[i, 3] = xi[3 + i]
    E = mp.expm(X)
    return [[E[i, j] for j in range(3)] for i in range(3)], [E[i, 3] for i in range(3)]


def so3_log(R):
    with mp.workdps(120):
        a = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
        s, c = norm(a) / 2, (R[0][0] + R[1][1] + R[2][2] - 1) / 2
        if s == 0:
            if c > 0:
                return [M(0)] * 3
            cols = [[R[i][j] + int(i == j) for i in range(3)] for j in range(3)]  # R + I = 2 a a^T
            ax = max(cols, key=norm)
            return sc(mp.pi / norm(ax), ax)
        return sc(mp.atan2(s, c) / (2 * s), a)


def _left_jacobian(w):
    th = norm(w)
    W = skew(w)
    WW = mm(W, W)
    B, C = (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3
    return [[int(i == j) + B * W[i][j] + C * WW[i][j] for j in range(3)] for i in range(3)]


def se3_log(p):
    w = so3_log(p[0])
    with mp.workdps(120):
        if norm(w) == 0:
            return w + list(p[1])
        u = mp.lu_solve(mp.matrix(_left_jacobian(w)), mp.matrix(p[1]))
        return w + [u[i] for i in range(3)]


def compose3(a, b):
    return mm(a[0], b[0]), add(a[1], mv(a[0], b[1]))


def inverse3(a):
    Rt = tp(a[0])
    return Rt, sc(-1, mv(Rt, a[1]))


def between3(a, b):
    return compose3(inverse3(a), b)


def adjoint3(p):
    R, tR = p[0], mm(skew(p[1]), p[0])
    return [R[i] + [M(0)] * 3 for i in range(3)] + [tR[i] + R[i] for i in range(3)]


# Pose2 = (x, y, theta)
def se2_exp(xi):
    X = mp.matrix([[0, -xi[2], xi[0]], [xi[2], 0, xi[1]], [0, 0, 0]])
    E = mp.expm(X)
    return [E[0, 2], E[1, 2], xi[2]]


def se2_log(p):
    with mp.workdps(120):
        th = p[2]
        if th == 0:
            return [p[0], p[1], th]
        A, B = mp.sin(th) / th, (1 - mp.cos(th)) / th
        u = mp.lu_solve(mp.matrix([[A, -B], [B, A]]), mp.matrix([p[0], p[1]]))
        return [u[0], u[1], th]


def compose2(a, b):
    c, s = mp.cos(a[2]), mp.sin(a[2])
    return [a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], a[2] + b[2]]


def inverse2(a):
    c, s = mp.cos(a[2]), mp.sin(a[2])
    return [-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), -a[2]]


def between2(a, b):
    return compose2(inverse2(a), b)


def adjoint2(p):
    c, s = mp.cos(p[2]), mp.sin(p[2])
    return [[c, -s, p[1]], [s, c, -p[0]], [M(0), M(0), M(1)]]


def transform_to(p, point):
    return mv(tp(p[0]), sub(point, p[1]))


def project_cal3_s2(p, point, K, sensor=None):
    """pixel of `point` seen from pose p (o sensor) with K = (fx, fy, s, u0, v0); the point must be in front"""
    q = transform_to(p if sensor is None else compose3(p, sensor), point)
    u, v = q[0] / q[2], q[1] / q[2]
    return [K[0] * u + K[2] * v + K[3], K[1] * v + K[4]]


def project_bundler(p, point, f, k1, k2, u0=0, v0=0):
    q = transform_to(p, point)
    u, v = q[0] / q[2], q[1] / q[2]
    r2 = u * u + v * v
    g = 1 + k1 * r2 + k2 * r2 * r2
    return [u0 + f * g * u, v0 + f * g * v]


def bearing2(p, l):
    c, s = mp.cos(p[2]), mp.sin(p[2])
    dx, dy = l[0] - p[0], l[1] - p[1]
    return mp.atan2(-s * dx + c * dy, c * dx + s * dy)


def range2(p, l):
    return mp.sqrt((l[0] - p[0]) ** 2 + (l[1] - p[1]) ** 2)


def numerical_jacobian(f, dim, h=M("1e-20")):
    """rows x dim central difference of f: R^dim -> list"""
    cols = []
    for j in range(dim):
        d = [M(0)] * dim
        d[j] = h
        fp, fm = f(d), f(sc(-1, d))
        cols.append([(a - b) / (2 * h) for a, b in zip(fp, fm)])
    return tp(cols)


def between_jacobian_numeric(p1, p2, which):
    """d/d delta of Logmap(h0^-1 between(p1 Exp(d1), p2 Exp(d2))) at 0, h0 = between(p1, p2): the argument stays at the identity"""
    h0i = inverse3(between3(p1, p2))

    def f(d):
        a = compose3(p1, se3_exp(d)) if which == 0 else p1
        b = compose3(p2, se3_exp(d)) if which == 1 else p2
        return se3_log(compose3(h0i, between3(a, b)))
    return numerical_jacobian(f, 6)


def between2_jacobian_numeric(p1, p2, which):
    h0i = inverse2(between2(p1, p2))

    def f(d):
        a = compose2(p1, se2_exp(d)) if which == 0 else p1
        b = compose2(p2, se2_exp(d)) if which == 1 else p2
        return se2_log(compose2(h0i, between2(a, b)))
    return numerical_jacobian(f, 3)


# ---------------------------------------------------------------- documented-formula layer
def so3_logmap_formula(R):
    """returns (w, branch): branch = 'pi0' / 'pi1' / 'pi2' (largest diagonal entry R33 / R22 / R11), 'acos' or 'taylor'"""
    (R11, R12, R13), (R21, R22, R23), (R31, R32, R33) = R
    tr = R11 + R22 + R33
    if tr + 1 < M(1e-3):
        if R33 > R22 and R33 > R11:
            W, Q1, Q2, Q3, perm = R21 - R12, 2 + 2 * R33, R31 + R13, R23 + R32, 0
        elif R22 > R11:
            W, Q1, Q2, Q3, perm = R13 - R31, 2 + 2 * R22, R23 + R32, R12 + R21, 1
        else:
            W, Q1, Q2, Q3, perm = R32 - R23, 2 + 2 * R11, R12 + R21, R31 + R13, 2
        nrm = mp.sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W)
        sgn = -1 if W < 0 else 1
        s = sgn * (mp.pi - 2 * sgn * W / nrm) / (2 * mp.sqrt(Q1))
        return sc(s, [[Q2, Q3, Q1], [Q3, Q1, Q2], [Q1, Q2, Q3]][perm]), "pi%d" % perm
    t3 = tr - 3
    if t3 < M(-1e-6):
        th = mp.acos((tr - 1) / 2)
        mag, br = th / (2 * mp.sin(th)), "acos"
    else:
        mag, br = M(1) / 2 - t3 / 12 + t3 * t3 / 60, "taylor"
    return sc(mag, [R32 - R23, R13 - R31, R21 - R12]), br


def pose3_logmap_formula(p):
    """returns (xi, so3 branch, 'smallw' | 'fullw')"""
    w, br = so3_logmap_formula(p[0])
    T, t = p[1], norm(w)
    if t < M(1e-10):
        return w + list(T), br, "smallw"
    a = sc(1 / t, w)
    WT = cross(a, T)
    u = add(sub(T, sc(t / 2, WT)), sc(1 - t / (2 * mp.tan(t / 2)), cross(a, WT)))
    return w + u, br, "fullw"


def expmap_coefficients(th2):
    if th2 <= M(1e-5):
        return 1 - th2 / 6, M(1) / 2 - th2 / 24, M(1) / 6 - th2 / 120, "taylor"
    th = mp.sqrt(th2)
    A = mp.sin(th) / th
    return A, 2 * mp.sin(th / 2) ** 2 / th2, (1 - A) / th2, "full"


def pose3_expmap_formula(xi):
    w, v = xi[:3], xi[3:]
    A, B, C, _ = expmap_coefficients(dot(w, w))
    W = skew(w)
    WW = mm(W, W)
    R = [[int(i == j) + A * W[i][j] + B * WW[i][j] for j in range(3)] for i in range(3)]
    Wv = cross(w, v)
    return R, add(add(v, sc(B, Wv)), sc(C, cross(w, Wv)))


def wrap(th):
    return mp.atan2(mp.sin(th), mp.cos(th))


def robust_weight(kind, k, d):
    k, d = M(float(k)), M(float(d))
    if kind == 1:
        return 1 / (1 + d / k)
    if kind == 2:
        return M(1) if d <= k else k / d
    if kind == 3:
        return k * k / (k * k + d * d)
    if kind == 4:
        return (1 - d * d / (k * k)) ** 2 if d <= k else M(0)
    if kind == 5:
        return mp.exp(-d * d / (k * k))
    if kind == 6:
        return (k * k / (k * k + d * d)) ** 2
    if kind == 7:
        return (2 * k / (k + d * d)) ** 2 if d * d > k else M(1)
    if kind == 8:
        return M(0) if d <= k else (d - k) / d
    raise ValueError(kind)


def robust_loss(kind, k, d):
    k, d = M(float(k)), M(float(d))
    if kind == 1:
        return k * k * (d / k - mp.log(1 + d / k))
    if kind == 2:
        return d * d / 2 if d <= k else k * (d - k / 2)
    if kind == 3:
        return k * k * mp.log(1 + d * d / (k * k)) / 2
    if kind == 4:
        return k * k * (1 - (1 - d * d / (k * k)) ** 3) / 6 if d <= k else k * k / 6
    if kind == 5:
        return k * k * (1 - mp.exp(-d * d / (k * k))) / 2
    if kind == 6:
        return k * k * d * d / (k * k + d * d) / 2
    if kind == 7:
        e2 = d * d
        return (k * k * e2 + k * e2 * e2) / (e2 + k) ** 2
    if kind == 8:
        return M(0) if d < k else (k - d) ** 2 / 2
    raise ValueError(kind)


def _pinhole(p, point):
    """(ok, u, v, Dpose 2x6, Dpoint 2x3) of the normalised projection; ok = qz > 0"""
    Rt = tp(p[0])
    q = mv(Rt, sub(point, p[1]))
    if q[2] <= 0:
        return False, None, None, None, None
    d = 1 / q[2]
    u, v = q[0] * d, q[1] * d
    Dpose = [[u * v, -1 - u * u, v, -d, M(0), d * u], [1 + v * v, -u * v, -u, M(0), -d, d * v]]
    Dpoint = [[d * (Rt[0][j] - u * Rt[2][j]) for j in range(3)], [d * (Rt[1][j] - v * Rt[2][j]) for j in range(3)]]
    return True, u, v, Dpose, Dpoint


def zeros(r, c):
    return [[M(0)] * c for _ in range(r)]


def evaluate_factor(ftype, vals, meas):
    """(e, [H1, H2, (H3)], info) of one factor by the documented contract; vals = stored FP64 arrays (camera: 17), meas as the host
    passes it.  info names the branches taken."""
    if ftype in (F_BETWEEN_POSE3, F_PRIOR_POSE3, F_PRIOR_CAM):
        if ftype == F_BETWEEN_POSE3:
            h = between3(pose3(vals[0]), pose3(vals[1]))
            xi, br, sw = pose3_logmap_formula(between3(pose3(meas), h))
            return xi, [[sc(-1, r) for r in adjoint3(inverse3(h))], _ident(6)], (br, sw)
        xi, br, sw = pose3_logmap_formula(between3(pose3(vals[0]), pose3(meas)))
        e = sc(-1, xi)
        if ftype == F_PRIOR_CAM:
            e = e + [M(float(vals[0][12 + i])) - M(float(meas[12 + i])) for i in range(3)]
        return e, [_ident(len(e))], (br, sw)
    if ftype in (F_BETWEEN_POSE2, F_PRIOR_POSE2):
        if ftype == F_BETWEEN_POSE2:
            h = between2(V(vals[0]), V(vals[1]))
            d = between2(V(meas), h)
            return [d[0], d[1], wrap(d[2])], [[sc(-1, r) for r in adjoint2(inverse2(h))], _ident(3)], ()
        d = between2(V(vals[0]), V(meas))
        return [-d[0], -d[1], -wrap(d[2])], [_ident(3)], ()
    if ftype == F_BEARING_RANGE_2D:
        x, l = V(vals[0]), V(vals[1])
        c, s = mp.cos(x[2]), mp.sin(x[2])
        dx, dy = l[0] - x[0], l[1] - x[1]
        qx, qy = c * dx + s * dy, -s * dx + c * dy
        d2 = qx * qx + qy * qy
        n = mp.sqrt(d2)
        hb, cb, sb, gb = [M(0), M(0)], M(1), M(0), "bguard"
        if n > M(1e-5):
            hb, cb, sb, gb = [-qy / d2, qx / d2], qx / n, qy / n, "bfull"
        r = mp.sqrt(dx * dx + dy * dy)
        hr, gr = [M(1), M(1)], "rguard"
        if r > M(1e-10):
            hr, gr = [dx / r, dy / r], "rfull"
        H1 = [[-hb[0], -hb[1], hb[0] * qy - hb[1] * qx], [-hr[0] * c - hr[1] * s, hr[0] * s - hr[1] * c, M(0)]]
        H2 = [[hb[0] * c - hb[1] * s, hb[0] * s + hb[1] * c], [hr[0], hr[1]]]
        bm = M(float(meas[0]))
        cm, sm = mp.cos(bm), mp.sin(bm)
        return [-mp.atan2(cb * sm - sb * cm, cb * cm + sb * sm), r - M(float(meas[1]))], [H1, H2], (gb, gr)
    if ftype in (F_PROJECTION, F_PROJECTION_BPS, F_SFM2):
        K = V(vals[2]) if ftype == F_SFM2 else V(meas[2:7])
        p = pose3(vals[0])
        if ftype == F_PROJECTION_BPS:
            sensor = pose3(meas[7:19])
            p = compose3(p, sensor)
        ok, u, v, Dpose, Dpoint = _pinhole(p, V(vals[1]))
        if not ok:
            e = [M(0), M(0)] if ftype == F_SFM2 else [2 * K[0], 2 * K[0]]
            return e, [zeros(2, 6), zeros(2, 3)] + ([zeros(2, 5)] if ftype == F_SFM2 else []), ("behind",)
        Dp = [[K[0], K[2]], [M(0), K[1]]]
        H1, H2 = mm(Dp, Dpose), mm(Dp, Dpoint)
        if ftype == F_PROJECTION_BPS:
            H1 = mm(H1, adjoint3(inverse3(sensor)))
        e = [K[0] * u + K[2] * v + K[3] - M(float(meas[0])), K[1] * v + K[4] - M(float(meas[1]))]
        H = [H1, H2] + ([[[u, M(0), v, M(1), M(0)], [M(0), v, M(0), M(0), M(1)]]] if ftype == F_SFM2 else [])
        return e, H, ("front",)
    if ftype == F_SFM:
        cam = vals[0]
        ok, u, v, Dpose, Dpoint = _pinhole(pose3(cam), V(vals[1]))
        if not ok:
            return [M(0), M(0)], [zeros(2, 9), zeros(2, 3)], ("behind",)
        f, k1, k2, u0, v0 = V(cam[12:17])
        r2 = u * u + v * v
        g = 1 + (k1 + k2 * r2) * r2
        a = 2 * (k1 + 2 * k2 * r2)
        Dp = [[f * (g + a * u * u), f * a * u * v], [f * a * u * v, f * (g + a * v * v)]]
        Dcal = [[g * u, f * r2 * u, f * r2 * r2 * u], [g * v, f * r2 * v, f * r2 * r2 * v]]
        H1 = [x + y for x, y in zip(mm(Dp, Dpose), Dcal)]
        e = [u0 + f * g * u - M(float(meas[0])), v0 + f * g * v - M(float(meas[1]))]
        return e, [H1, mm(Dp, Dpoint)], ("front",)
    raise ValueError(ftype)


def _ident(n):
    return [[M(int(i == j)) for j in range(n)] for i in range(n)]


def retract_value(vtype, val, delta):
    """the retracted stored value from the EXACT layer: Pose3 / camera = p o exp(delta^), Pose2 = the chart compose(Pose2(delta));
    Pose2's angle is returned unwrapped (it is compared as cos / sin)"""
    if vtype == POSE2:
        return compose2(V(val), V(delta))
    r = compose3(pose3(val), se3_exp(V(delta[:6])))
    out = [r[0][i][j] for i in range(3) for j in range(3)] + list(r[1])
    if vtype == CAM_BUNDLER:
        out += [M(float(val[12 + i])) + M(float(delta[6 + i])) for i in range(3)] + V(val[15:17])
    return out


# ---------------------------------------------------------------- the case table
def _rot(axis, angle):
    ax = sc(1 / norm(axis), axis)
    return se3_exp(sc(angle, ax) + [M(0)] * 3)[0]


def _f64(p):
    return np.array(flat3(p))


PI = mp.pi
ANGLES = [("0", M(0)), ("1e-11", M("1e-11")), ("1e-9", M("1e-9")), ("9e-4", M("9e-4")), ("1.1e-3", M("1.1e-3")), ("1", M(1)),
          ("pi-0.033", PI - M("0.033")), ("pi-0.030", PI - M("0.030")), ("pi-1e-6", PI - M("1e-6")), ("pi-1e-9", PI - M("1e-9")), ("pi", PI)]
AXES = [("x", [1, .2, .1]), ("y", [.1, 1, .2]), ("z", [.2, .1, 1])]
TIE = [0, 1, 1]
# the so3 branch each angle must land in ('pi' = any of pi0 / pi1 / pi2 by the axis)
ANGLE_BRANCH = {"0": "taylor", "1e-11": "taylor", "1e-9": "taylor", "9e-4": "taylor", "1.1e-3": "acos", "1": "acos", "pi-0.033": "acos",
                "pi-0.030": "pi", "pi-1e-6": "pi", "pi-1e-9": "pi", "pi": "pi"}
BASES = [([.3, -.5, .8], M("0.9"), [1, -2, .5]), ([-.6, .2, .4], M("2.1"), [-3, .5, 2]), ([.1, .9, -.3], M("1.4"), [.25, 4, -1])]
CAL = [500., -0.05, 0.01, 3., -2.]  # f, k1, k2, u0, v0 of the camera cases


def _base(i):
    ax, ang, t = BASES[i % len(BASES)]
    return _rot(V(ax), ang), V(t)


def _pose3_cases():
    """(name, rel so that the error's pose is `rel`, intended so3 branch, mode, translation size)"""
    out, n = [], 0
    for aname, ang in ANGLES:
        for xname, ax in AXES:
            for sg in (1, -1):
                size = 1 if n % 2 == 0 else 1000
                n += 1
                d = PI - ang
                mode = MODE_EXP3 if d <= M("1e-6") else MODE_DIRECT
                br = ANGLE_BRANCH[aname]
                if br == "pi":
                    br = {"x": "pi2", "y": "pi1", "z": "pi0"}[xname]
                out.append(("%s_%s%s_t%g" % (aname, "+" if sg > 0 else "-", xname, size), V(ax), sg * ang, br, mode, size))
    for aname, ang in ANGLES[-3:]:
        for size in (1, 1000):
            out.append(("%s_tie_t%g" % (aname, size), V(TIE), ang, "pi", MODE_EXP3, size))
    return out


def _shift3(j):
    return np.array([0.5 * j, -0.25 * j, 0.125 * j])


def factor_cases():
    """{ftype: [case]}: ROWS_PER_TYPE cases per factor type, the base cases first, then repeats of them with all translations shifted
    (only of the cases that do not rely on an exactly representable difference).  case = dict(name, ftype, vals [stored arrays], meas,
    mode, sgn (MODE_EXP3: Exp(sgn * b[:6]) is the compared pose), branch (the branches the case must take, or None), base)"""
    T = {}

    def put(ft, name, vals, meas, mode=MODE_DIRECT, sgn=0, branch=None, shift=True):
        T.setdefault(ft, []).append(dict(name=name, ftype=ft, vals=[np.array(v, dtype=np.float64) for v in vals],
                                         meas=np.array(meas, dtype=np.float64), mode=mode, sgn=sgn, branch=branch, shift=shift, base=True))

    # ---- Pose3 relative rotation
    for i, (name, ax, ang, br, mode, size) in enumerate(_pose3_cases()):
        xi = sc(ang / norm(ax), ax) + sc(size / norm([.3, -.5, .8]), V([.3, -.5, .8]))
        rel = se3_exp(xi)
        p1 = _base(i)
        z = (_rot(V([.5, .4, -.7]), M("0.7")), sc(size, V([.2, -.1, .3])))
        bw = "smallw" if name.startswith(("0_", "1e-11_")) else "fullw"
        put(F_BETWEEN_POSE3, name, [_f64(p1), _f64(compose3(compose3(p1, z), rel))], _f64(z), mode, -1, (br, bw))
        put(F_PRIOR_POSE3, name, [_f64(p1)], _f64(compose3(p1, rel)), mode, 1, (br, bw))
        cam = np.concatenate([_f64(p1), CAL])
        zc = np.concatenate([_f64(compose3(p1, rel)), [CAL[0] + 1.5, CAL[1] - 0.01, CAL[2] + 0.002, CAL[3], CAL[4]]])
        put(F_PRIOR_CAM, name, [cam], zc, mode, 1, (br, bw))
    # exactly representable: signed-permutation bases, half-turns about the coordinate axes (W = 0, Q2 = Q3 = 0) and the identity
    Pz = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1.])
    Px = np.array([1, 0, 0, 0, 0, -1, 0, 1, 0.])
    for k, (nm, D) in enumerate([("x", [1, -1, -1]), ("y", [-1, 1, -1]), ("z", [-1, -1, 1]), ("identity", [1, 1, 1])]):
        R1 = Pz.reshape(3, 3)
        Rz = Px.reshape(3, 3)
        rel = np.diag(D).astype(float)
        p1 = np.concatenate([R1.reshape(-1), [1, -2, 3.]])
        zz = np.concatenate([Rz.reshape(-1), [2, 0, -1.]])
        R2 = R1 @ Rz @ rel
        t2 = p1[9:] + R1 @ zz[9:] + R1 @ Rz @ np.array([0.5, -1, 2.])
        br = ("taylor", "smallw") if nm == "identity" else ("pi%d" % (2 - k), "fullw")
        nm = "exact_" + (nm if nm == "identity" else "pi_" + nm)
        put(F_BETWEEN_POSE3, nm, [p1, np.concatenate([R2.reshape(-1), t2])], zz, MODE_DIRECT, -1, br)
        Rp = R1 @ rel
        put(F_PRIOR_POSE3, nm, [p1], np.concatenate([Rp.reshape(-1), p1[9:] + R1 @ np.array([0.5, -1, 2.])]), MODE_DIRECT, 1, br)
        put(F_PRIOR_CAM, nm, [np.concatenate([p1, CAL])],
            np.concatenate([Rp.reshape(-1), p1[9:] + R1 @ np.array([0.5, -1, 2.]), CAL]), MODE_DIRECT, 1, br)
    # a prior on its own value: R^T R is symmetric, w = 0 exactly
    g = _f64(_base(1))
    put(F_PRIOR_POSE3, "exact_self", [g], g, MODE_DIRECT, 1, ("taylor", "smallw"))
    put(F_BETWEEN_POSE3, "exact_self", [g, g], [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.], MODE_DIRECT, -1, ("taylor", "smallw"))

    # ---- Pose2
    pi64 = float(np.pi)
    stored = [pi64, -pi64, pi64 - 1e-12, -(pi64 - 1e-12), 3.5, 7.0, -7.0]
    for i, th in enumerate(stored):
        a = [0.5 + i, -1.25, th]
        b = [1.5 - i, 0.75, 0.4 - 0.3 * i]
        put(F_BETWEEN_POSE2, "stored_%.17g" % th, [a, b], [0.3, -0.2, 0.9])
        put(F_BETWEEN_POSE2, "stored2_%.17g" % th, [b, a], [0.3, -0.2, -0.6])
        put(F_PRIOR_POSE2, "stored_%.17g" % th, [a], [0.4, -1.0, 0.5])
        put(F_PRIOR_POSE2, "meas_%.17g" % th, [b], [0.4, -1.0, th])
    for nm, rel, mode in [("pi", pi64, MODE_ANGLE), ("-pi", -pi64, MODE_ANGLE), ("pi-1e-12", pi64 - 1e-12, MODE_DIRECT),
                          ("pi+1e-12", pi64 + 1e-12, MODE_DIRECT), ("-pi+1e-12", -pi64 + 1e-12, MODE_DIRECT),
                          ("-pi-1e-12", -pi64 - 1e-12, MODE_DIRECT)]:
        # exactly +-pi: theta1 = 0 and a zero measured angle keep the relative angle the stored number itself
        t1, zt = (0.0, 0.0) if mode == MODE_ANGLE else (0.25, 0.5)
        put(F_BETWEEN_POSE2, "rel_" + nm, [[1.0, 2.0, t1], [-0.5, 0.25, t1 + zt + rel]], [0.7, 0.1, zt], mode, shift=mode != MODE_ANGLE)
        put(F_PRIOR_POSE2, "rel_" + nm, [[1.0, 2.0, t1]], [-0.5, 0.25, t1 + rel], mode, shift=mode != MODE_ANGLE)

    # ---- bearing-range
    x = [1.0, -2.0, 0.7]
    c, s = np.cos(0.7), np.sin(0.7)
    put(F_BEARING_RANGE_2D, "on_pose", [x, x[:2]], [0.3, 0.0], branch=("bguard", "rguard"), shift=False)
    put(F_BEARING_RANGE_2D, "n_0.9e-5", [x, [1.0 + 0.9e-5 * 0.6, -2.0 + 0.9e-5 * 0.8]], [0.2, 1e-5], branch=("bguard", "rfull"), shift=False)
    put(F_BEARING_RANGE_2D, "n_1.1e-5", [x, [1.0 + 1.1e-5 * 0.6, -2.0 + 1.1e-5 * 0.8]], [0.2, 1e-5], branch=("bfull", "rfull"), shift=False)
    put(F_BEARING_RANGE_2D, "r_1e-11", [[0.0, 0.0, 0.7], [0.6e-11, 0.8e-11]], [0.2, 0.0], branch=("bguard", "rguard"), shift=False)
    put(F_BEARING_RANGE_2D, "behind", [x, [1.0 - 3 * c, -2.0 - 3 * s]], [3.0, 2.5], branch=("bfull", "rfull"))
    put(F_BEARING_RANGE_2D, "behind_meas_pi", [x, [1.0 - 3 * c, -2.0 - 3 * s]], [pi64, 2.5], branch=("bfull", "rfull"))
    put(F_BEARING_RANGE_2D, "behind_meas_-pi", [x, [1.0 - 3 * c, -2.0 - 3 * s]], [-pi64, 2.5], branch=("bfull", "rfull"))
    put(F_BEARING_RANGE_2D, "ahead_meas_pi", [[1.0, -2.0, 0.0], [4.0, -2.0]], [pi64, 2.5], MODE_ANGLE, branch=("bfull", "rfull"), shift=False)
    put(F_BEARING_RANGE_2D, "ahead_meas_-pi", [[1.0, -2.0, 0.0], [4.0, -2.0]], [-pi64, 2.5], MODE_ANGLE, branch=("bfull", "rfull"), shift=False)
    put(F_BEARING_RANGE_2D, "ordinary", [x, [3.0, 1.0]], [0.4, 3.0], branch=("bfull", "rfull"))

    # ---- projection: K with skew; the camera of the exact cases is a signed permutation at the origin, so q = R^T p exactly
    K = [520.0, 480.0, 1.75, 320.0, 240.0]
    Rc = np.array([0, 0, 1, 1, 0, 0, 0, 1, 0.])  # columns: camera x = world y, y = world z, z = world x
    cam0 = np.concatenate([Rc, [0, 0, 0.]])
    Rm = Rc.reshape(3, 3)
    gen = _f64(_base(0))
    Rg, tg = gen[:9].reshape(3, 3), gen[9:]
    sens = _f64((_rot(V([.2, -.3, .1]), M("0.3")), V([.1, -.05, .2])))
    sens_id = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.])
    pts = [("qz_1e-12", Rm @ np.array([0.5e-12, -0.25e-12, 1e-12]), cam0, "front", False),
           ("qz_0", Rm @ np.array([0.3, -0.2, 0.0]), cam0, "behind", False),
           ("qz_-1", tg + Rg @ np.array([0.3, -0.2, -1.0]), gen, "behind", True),
           ("on_axis", Rm @ np.array([0.0, 0.0, 2.5]), cam0, "front", True),
           ("ordinary", tg + Rg @ np.array([0.7, -0.4, 3.0]), gen, "front", True),
           ("wide", tg + Rg @ np.array([2.1, 1.6, 2.0]), gen, "front", True)]
    for nm, pt, cam, br, sh in pts:
        put(F_PROJECTION, nm, [cam, pt], [300.0, 250.0] + K, branch=(br,), shift=sh)
        # body_P_sensor: the exact cases keep the identity sensor, the others a general one (the point is given in the body frame's camera)
        if sh:
            body = _f64(compose3(pose3(cam), inverse3(pose3(sens))))
            put(F_PROJECTION_BPS, nm, [body, pt], np.concatenate([[300.0, 250.0], K, sens]), branch=(br,), shift=sh)
        else:
            put(F_PROJECTION_BPS, nm, [cam, pt], np.concatenate([[300.0, 250.0], K, sens_id]), branch=(br,), shift=sh)
        put(F_SFM2, nm, [cam, pt, K], [300.0, 250.0], branch=(br,), shift=sh)
        put(F_SFM, nm, [np.concatenate([cam, [450.0, 0.05, 0.01, 3.0, -2.0]]), pt], [30.0, -25.0], branch=(br,), shift=sh)
    # Cal3Bundler radial terms: k1 = -0.3, k2 = 0.2 at image radius about 1
    for nm, q in [("bundler_r1", [0.8, -0.6, 1.0]), ("bundler_r1_far", [2.4, 1.9, 3.0])]:
        put(F_SFM, nm, [np.concatenate([gen, [450.0, -0.3, 0.2, 3.0, -2.0]]), tg + Rg @ np.array(q)], [30.0, -25.0], branch=("front",))

    # ---- fill every type to ROWS_PER_TYPE with translation-shifted repeats
    for ft, rows in T.items():
        src = [r for r in rows if r["shift"]]
        assert src and len(rows) <= ROWS_PER_TYPE, (ft, len(rows))
        j = 0
        while len(rows) < ROWS_PER_TYPE:
            r, j = src[j % len(src)], j + 1
            rows.append(_shifted(r, 1 + j // len(src) + (j % 7)))
    return T


def _shift_value(vtype, v, sh):
    v = v.copy()
    if vtype in (POSE3, CAM_BUNDLER):
        v[9:12] += sh
    elif vtype == POINT3:
        v[:3] += sh
    elif vtype in (POSE2, POINT2):
        v[:2] += sh[:2]
    return v


def _shifted(r, j):
    sh, ft = _shift3(j), r["ftype"]
    q = dict(r, name="%s_shift%d" % (r["name"], j), base=False)
    q["vals"] = [_shift_value(t, v, sh) for t, v in zip(FACTOR_VARS[ft], r["vals"])]
    if ft in (F_PRIOR_POSE3, F_PRIOR_CAM):
        q["meas"] = _shift_value(POSE3, r["meas"], sh)
    if ft == F_PRIOR_POSE2:
        q["meas"] = _shift_value(POSE2, r["meas"], sh)
    return q


def retract_cases():
    """{vtype: [(name, stored value, delta)]}: |w|^2 in {0, 1e-20, 9.61e-6, 1.024e-5 (either side of 1e-5), 1, pi^2, (2 pi)^2, 40}, v != 0,
    non-identity bases, both translation scales; Pose2 d_theta in {+-pi, 2 pi} among ordinary ones"""
    out = {POSE3: [], CAM_BUNDLER: [], POSE2: []}
    th2 = [("0", M(0)), ("1e-20", M("1e-20")), ("9.61e-6", M("9.61e-6")), ("1.024e-5", M("1.024e-5")), ("1", M(1)), ("pi^2", PI ** 2),
           ("(2pi)^2", 4 * PI ** 2), ("40", M(40))]
    n = 0
    for nm, t2 in th2:
        for xname, ax in AXES + [("tie", TIE)]:
            size = 1 if n % 2 == 0 else 1000
            w = sc(mp.sqrt(t2) / norm(V(ax)), V(ax))
            d = np.array([float(x) for x in w] + [0.4 * size, -0.7 * size, 0.2 * size])
            base = _base(n)
            base = _f64((base[0], sc(size, base[1])))
            out[POSE3].append(("w2_%s_%s_t%g" % (nm, xname, size), base, d))
            if xname in ("x", "tie"):
                out[CAM_BUNDLER].append(("w2_%s_%s_t%g" % (nm, xname, size), np.concatenate([base, CAL]),
                                         np.concatenate([d, [2.5, -0.01, 0.003]])))
            n += 1
    pi64 = float(np.pi)
    for i, dth in enumerate([pi64, -pi64, 2 * pi64, 0.0, 0.3, -7.0]):
        for th in (0.4, pi64, -3.0):
            out[POSE2].append(("dth_%.17g_th_%.17g" % (dth, th), np.array([1.0 + i, -2.0, th]), np.array([0.5, -0.25 * (i + 1), dth])))
    return out


ROBUST_DEFAULT_K = {1: 1.3998, 2: 1.345, 3: 0.1, 4: 4.6851, 5: 2.9846, 6: 1.0, 7: 1.0, 8: 1.0}


def robust_cases():
    """[(kind, k, d)]: d in {0, 0.99 k, k exactly, 1.01 k, 10 k} for each m-estimator; the factor is a PRIOR_POINT3 with Unit noise on
    the point (d, 0, 0) with a zero prior, whose whitened error is (d, 0, 0) exactly"""
    return [(kind, k, d) for kind, k in ROBUST_DEFAULT_K.items() for d in (0.0, 0.99 * k, k, 1.01 * k, 10 * k)]
