"""numpy restatement of the reference's smart projection factors, on top of triangulation_restatement.py: the checker of the device's smart
factors (include/lmgpu.h, "smart projection factors").
  SmartProjectionFactor::decideIfTriangulate / triangulateSafe   gtsam/slam/SmartProjectionFactor.h:127-184 (the cache rule; Pose3::equals
                                                                 -> fpEqual, gtsam/base/Vector.cpp:42-77, without the relative test)
  totalReprojectionError / error                                 :411-439
  createHessianFactor                                            :198-237 with CameraSet::SchurComplement, gtsam/geometry/CameraSet.h:145-216
  LevenbergMarquardtOptimizer / GaussNewtonOptimizer             the control flow of gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:121-308 and
                                                                 NonlinearOptimizer::defaultOptimize on the DENSE pose system, with the reference's
                                                                 order of calls: constructor error, per iteration linearize, per trial lambda one
                                                                 error evaluation iff the damped system was solved and the linear cost did not rise
A pose is 12 doubles (R row-major 9, t 3); values are a dict key -> pose.  A Graph holds smart factors and PriorFactor<Pose3>s in graph order.

Decisions that select a branch are recorded like in triangulation_restatement (`dec` lists): status decisions with its margins, the cache test
as ("cache", |a - b|, threshold, threshold) per entry and ("cache_call", the largest |a - b| of the call, threshold, threshold)."""
import numpy as np

import triangulation_restatement as tr

EPS = np.finfo(float).eps


# ---------------------------------------------------------------- Pose3
def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def so3_expmap(w):
    th2 = w @ w
    W = skew(w)
    if th2 <= EPS:
        return np.eye(3) + W
    th = np.sqrt(th2)
    return np.eye(3) + (np.sin(th) / th) * W + ((1 - np.cos(th)) / th2) * (W @ W)


def so3_logmap(R):
    tr_ = np.trace(R)
    if tr_ + 1.0 < 1e-3:
        raise NotImplementedError("rotation near pi")
    tr_3 = tr_ - 3.0
    if tr_3 < -1e-6:
        th = np.arccos((tr_ - 1.0) / 2.0)
        mag = th / (2.0 * np.sin(th))
    else:
        mag = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0
    return mag * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def pose(R, t):
    return np.concatenate([np.asarray(R, dtype=float).reshape(9), np.asarray(t, dtype=float).reshape(3)])


def Rt(p):
    return p[:9].reshape(3, 3), p[9:12]


def compose(a, b):
    Ra, ta = Rt(a)
    Rb, tb = Rt(b)
    return pose(Ra @ Rb, ta + Ra @ tb)


def between(a, b):
    Ra, ta = Rt(a)
    Rb, tb = Rt(b)
    return pose(Ra.T @ Rb, Ra.T @ (tb - ta))


def pose3_expmap(xi):
    """Pose3::Expmap (gtsam/geometry/Pose3.cpp, GTSAM_POSE3_EXPMAP)"""
    w, v = xi[:3], xi[3:]
    R = so3_expmap(w)
    th2 = w @ w
    if th2 > EPS:
        t_par = w * (w @ v)
        wxv = np.cross(w, v)
        t = (wxv - R @ wxv + t_par) / th2
    else:
        t = v
    return pose(R, t)


def pose3_logmap(p):
    """Pose3::Logmap"""
    R, T = Rt(p)
    w = so3_logmap(R)
    t = np.linalg.norm(w)
    if t < 1e-10:
        return np.concatenate([w, T])
    W = skew(w / t)
    Tan = np.tan(0.5 * t)
    WT = W @ T
    u = T - (0.5 * t) * WT + (1 - t / (2.0 * Tan)) * (W @ WT)
    return np.concatenate([w, u])


def retract(p, xi):
    return compose(p, pose3_expmap(xi))


def ypr(y, p, r):
    """Rot3::Ypr = Rz(y) Ry(p) Rx(r)"""
    cx, sx, cy, sy, cz, sz = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    return Rz @ Ry @ Rx


def fp_equal(a, b, tol):
    """fpEqual(a, b, tol, check_relative_also = false); DOUBLE_MIN_NORMAL = min() + 1.0 == 1.0"""
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if np.isinf(a) or np.isinf(b):
        return bool(np.isinf(a) and np.isinf(b))
    return abs(a - b) <= tol


# ---------------------------------------------------------------- projection with both Jacobians
def project_jac(p12, K5, point):
    """PinholePose<Cal3_S2>::project2(point, Dpose, Dpoint) (PinholePose.h:90-109, CalibratedCamera.cpp:27-46, 116-136).  None behind the camera."""
    R, t = Rt(p12)
    q = R.T @ (point - t)
    if q[2] <= 0:
        return None
    d = 1.0 / q[2]
    u, v = q[0] * d, q[1] * d
    fx, fy, s, u0, v0 = K5
    uv = np.array([fx * u + s * v + u0, fy * v + v0])
    Dpi = np.array([[fx, s], [0.0, fy]])
    Dpose = np.array([[u * v, -1 - u * u, v, -d, 0, d * u], [1 + v * v, -u * v, -u, 0, -d, d * v]])
    Dpoint = d * np.array([R.T[0] - u * R.T[2], R.T[1] - v * R.T[2]])
    return uv, Dpi @ Dpose, Dpi @ Dpoint


class SmartParams:
    """SmartProjectionParams with HESSIAN / ZERO_ON_DEGENERACY; triangulation: tr.Params"""

    def __init__(self, triangulation=None, retriangulationThreshold=1e-5):
        self.triangulation = triangulation or tr.Params()
        self.retriangulationThreshold = retriangulationThreshold


class SmartFactor:
    def __init__(self, keys, zs, K5, sigma, params=None):
        self.keys = [int(k) for k in keys]
        self.zs = [np.asarray(z, dtype=float) for z in zs]
        self.K5 = np.asarray(K5, dtype=float)
        self.sigma = float(sigma)
        self.params = params or SmartParams()
        self.reset()
        self.dec = None  # a list: decisions are recorded

    def reset(self):
        self.cache = None  # cameraPosesTriangulation_
        self.status, self.point = tr.DEGENERATE, None
        self.retriangulated = False

    def cams(self, values):
        return [np.concatenate([values[k], self.K5]) for k in self.keys]

    def triangulate_safe(self, values):
        """the member triangulateSafe, :173-184"""
        self.retriangulated = False
        if len(self.keys) < 2:
            self.status, self.point = tr.DEGENERATE, None
            return
        poses = [values[k].copy() for k in self.keys]
        re = self.cache is None
        if not re:
            thr = self.params.retriangulationThreshold
            for a, b in zip(poses, self.cache):
                for x, y in zip(a, b):
                    if self.dec is not None:
                        self.dec.append(("cache", abs(x - y), thr, thr))
                    if not fp_equal(x, y, thr):
                        re = True
            if self.dec is not None:  # the call's decision as a whole: the largest difference against the threshold
                self.dec.append(("cache_call", max(abs(x - y) for a, b in zip(poses, self.cache) for x, y in zip(a, b)), thr, thr))
        if re:
            self.cache = poses
            d = [] if self.dec is not None else None
            self.status, self.point, _ = tr.triangulate_safe(self.cams(values), tr.S2, self.zs, self.params.triangulation, d)
            if d:
                self.dec.extend(d)
            self.retriangulated = True

    def _FEb(self, values):
        m = len(self.keys)
        F, E, b = np.zeros((m, 2, 6)), np.zeros((2 * m, 3)), np.zeros(2 * m)
        for j, k in enumerate(self.keys):
            r = project_jac(values[k], self.K5, self.point)
            if r is None:  # (GenericProjectionFactor's behaviour; see include/lmgpu.h, "Deviation")
                b[2 * j:2 * j + 2] = -2.0 * self.K5[0] / self.sigma
                continue
            uv, Dp, Dx = r
            F[j], E[2 * j:2 * j + 2], b[2 * j:2 * j + 2] = Dp / self.sigma, Dx / self.sigma, -(uv - self.zs[j]) / self.sigma
        return F, E, b

    def error(self, values):
        """:411-439"""
        self.triangulate_safe(values)
        if self.status != tr.VALID:
            return 0.0
        _, _, b = self._FEb(values)
        return 0.5 * (b @ b)

    def hessian(self, values):
        """createHessianFactor: the augmented information matrix (6 m + 1) x (6 m + 1)"""
        self.triangulate_safe(values)
        return self.hessian_at_cache(values)

    def hessian_at_cache(self, values):
        m = len(self.keys)
        N = 6 * m + 1
        if self.status != tr.VALID:
            return np.zeros((N, N))
        F, E, b = self._FEb(values)
        Fd = np.zeros((2 * m, 6 * m))
        for j in range(m):
            Fd[2 * j:2 * j + 2, 6 * j:6 * j + 6] = F[j]
        P = np.linalg.inv(E.T @ E)
        Q = np.eye(2 * m) - E @ P @ E.T
        A = np.zeros((N, N))
        A[:N - 1, :N - 1] = Fd.T @ Q @ Fd
        A[:N - 1, N - 1] = A[N - 1, :N - 1] = Fd.T @ Q @ b
        A[N - 1, N - 1] = b @ Q @ b
        return A


class Prior:
    """PriorFactor<Pose3> with a diagonal model: error = -Local(x, prior) whitened, H = I (PriorFactor.h:98-102)"""

    def __init__(self, key, prior12, sigmas6):
        self.keys = [int(key)]
        self.prior = np.asarray(prior12, dtype=float)
        self.inv = 1.0 / np.broadcast_to(np.asarray(sigmas6, dtype=float), (6,))

    def _b(self, values):
        return self.inv * pose3_logmap(between(values[self.keys[0]], self.prior))  # = -whitened error

    def error(self, values):
        b = self._b(values)
        return 0.5 * (b @ b)

    def hessian(self, values):
        A, b = np.diag(self.inv), self._b(values)
        out = np.zeros((7, 7))
        out[:6, :6], out[:6, 6], out[6, :6], out[6, 6] = A.T @ A, A.T @ b, A.T @ b, b @ b
        return out


class Graph:
    def __init__(self, factors, order):
        """factors in graph order; order: the pose keys in the order of the dense system's blocks"""
        self.factors, self.order = list(factors), [int(k) for k in order]
        self.col = {k: 6 * i for i, k in enumerate(self.order)}

    def smart(self):
        return [f for f in self.factors if isinstance(f, SmartFactor)]

    def error(self, values):
        return float(sum(f.error(values) for f in self.factors))

    def linearize(self, values):
        """-> (H, g, f): linear error at x is 0.5 (x'Hx - 2 g'x + f)"""
        n = 6 * len(self.order)
        H, g, c = np.zeros((n, n)), np.zeros(n), 0.0
        for f in self.factors:
            A = f.hessian(values)
            idx = np.concatenate([np.arange(self.col[k], self.col[k] + 6) for k in f.keys])
            H[np.ix_(idx, idx)] += A[:-1, :-1]
            g[idx] += A[:-1, -1]
            c += A[-1, -1]
        return H, g, c

    def retract(self, values, delta):
        return {k: retract(values[k], delta[self.col[k]:self.col[k] + 6]) if k in self.col else values[k] for k in values}


def lin_error(H, g, c, x):
    return 0.5 * (x @ H @ x - 2.0 * (g @ x) + c)


def solve(H, g, lam):
    """the damped system (H + lam I) x = g by Cholesky; None where it is not positive definite (IndeterminantLinearSystemException)"""
    try:
        L = np.linalg.cholesky(H + lam * np.eye(len(g)))
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, g))


class LMParams:
    def __init__(self):
        self.maxIterations, self.relativeErrorTol, self.absoluteErrorTol, self.errorTol = 100, 1e-5, 1e-5, 0.0
        self.lambdaInitial, self.lambdaFactor, self.lambdaUpperBound, self.lambdaLowerBound = 1e-5, 10.0, 1e5, 0.0
        self.minModelFidelity, self.useFixedLambdaFactor = 1e-3, True


def check_convergence(p, cur, new):
    """NonlinearOptimizer.cpp:182-231"""
    if new <= p.errorTol:
        return True
    dec = cur - new
    return bool(dec / cur <= p.relativeErrorTol or dec <= p.absoluteErrorTol)


class LM:
    """LevenbergMarquardtOptimizer on a Graph; trace: per tryLambda (lambda, lin_err0, lin_err1 | None, new error | None, accepted, delta | None)"""

    def __init__(self, graph, values, params=None):
        self.g, self.values, self.p = graph, dict(values), params or LMParams()
        self.error = graph.error(self.values)  # the constructor's error evaluation
        self.lam, self.factor, self.iterations, self.inner = self.p.lambdaInitial, self.p.lambdaFactor, 0, 0
        self.trace = []
        self.ctl = []  # the loop's own decisions as (name, value, bound, scale), like the `dec` lists

    def iterate(self):
        p = self.p
        H, g, c = self.g.linearize(self.values)
        while True:
            self.inner += 1
            x = solve(H, g, self.lam)
            ok = stop = False
            newErr = l1 = None
            if x is not None:
                l0, l1 = 0.5 * c, lin_error(H, g, c, x)
                lcc = l0 - l1
                if lcc >= 0:
                    newVals = self.g.retract(self.values, x)
                    newErr = self.g.error(newVals)
                    cost = self.error - newErr
                    self.ctl.append(("linearizedCostChange", lcc, EPS * l0, max(abs(l0), abs(l1))))
                    if lcc > EPS * l0:
                        mf = cost / lcc
                        self.ctl.append(("modelFidelity", mf, p.minModelFidelity, max(abs(mf), p.minModelFidelity)))
                        ok = mf > p.minModelFidelity
                    self.ctl.append(("stopSearchingLambda", abs(cost), p.relativeErrorTol * self.error, max(abs(cost), p.relativeErrorTol * self.error)))
                    if abs(cost) < p.relativeErrorTol * self.error:
                        stop = True
            self.trace.append((self.lam, 0.5 * c, l1, newErr, ok, x))
            if ok:
                if p.useFixedLambdaFactor:
                    lam = self.lam / self.factor
                else:
                    lam = self.lam * max(1.0 / 3.0, 1.0 - (2.0 * mf - 1.0) ** 3)
                    self.factor *= 2.0
                self.lam = max(p.lambdaLowerBound, lam)
                self.values, self.error = newVals, newErr
                self.iterations += 1
                return
            if stop:
                return
            self.lam *= self.factor
            if not p.useFixedLambdaFactor:
                self.factor *= 2.0
            if self.lam >= p.lambdaUpperBound:
                return

    def optimize(self):
        """defaultOptimize, NonlinearOptimizer.cpp:62-117; history: (error, lambda) after every iterate"""
        p = self.p
        hist = []
        cur = self.error
        if cur <= p.errorTol or self.iterations >= p.maxIterations:
            return hist
        new = cur
        while True:
            cur = new
            self.iterate()
            new = self.error
            hist.append((self.error, self.lam))
            if not (self.iterations < p.maxIterations and not check_convergence(p, cur, new) and np.isfinite(cur)):
                break
        return hist


def gn_step(graph, values):
    """GaussNewtonOptimizer::iterate's step: the undamped solve; (delta | None, lin_err0, lin_err1 | None)"""
    H, g, c = graph.linearize(values)
    x = solve(H, g, 0.0)
    return x, 0.5 * c, None if x is None else lin_error(H, g, c, x)
