"""numpy restatement of the reference's triangulation (gtsam/geometry/triangulation.h, triangulation.cpp) for PinholeCamera<Cal3Bundler> and
PinholeCamera<Cal3_S2>: the checker of lmgpu_triangulate_batch / lmgpu_triangulate_landmarks.  numpy.linalg.svd for the DLT, the per-point
Levenberg-Marquardt of triangulateNonlinear with the control flow of LevenbergMarquardtOptimizer (the one oracle/lm_oracle.cpp restates for
the whole graph), Cal3Bundler::calibrate's fixed-point loop.

A camera is 17 doubles: Pose3 packing (R row-major 9, t 3) + (f, k1, k2, u0, v0) for model BUNDLER, + (fx, fy, s, u0, v0) for model S2.

Every comparison whose outcome selects a branch is recorded in `dec` (a list, optional) as (name, value, bound, scale): a case is fit for a
device parity test only if |value - bound| >= 1e-3 * scale for all of them, so that a last-bit difference cannot select another branch.
`scale` is the magnitude of the terms that enter the comparison."""
import numpy as np

BUNDLER, S2 = 0, 1
VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT, CALIBRATE_FAILED = 0, 1, 2, 3, 4, 5
EPS = np.finfo(float).eps


class Underconstrained(Exception):
    """TriangulationUnderconstrainedException"""


class Cheirality(Exception):
    """TriangulationCheiralityException"""


class CalibrateFailed(Exception):
    """the std::runtime_error of Cal3Bundler::calibrate (Cal3Bundler.cpp:120-123)"""


class Params:
    """TriangulationParameters (triangulation.h:562-609) + the one inverse sigma of the shared isotropic noise model (0: Unit)"""

    def __init__(self, rankTolerance=1.0, enableEPI=False, landmarkDistanceThreshold=-1.0, dynamicOutlierRejectionThreshold=-1.0, noise_inv_sigma=0.0):
        self.rankTolerance, self.enableEPI = rankTolerance, enableEPI
        self.landmarkDistanceThreshold, self.dynamicOutlierRejectionThreshold = landmarkDistanceThreshold, dynamicOutlierRejectionThreshold
        self.noise_inv_sigma = noise_inv_sigma


def _note(dec, name, value, bound, scale):
    if dec is not None:
        dec.append((name, float(value), float(bound), float(scale)))


def pose_of(cam):
    return cam[:9].reshape(3, 3), cam[9:12]


def K_of(cam, model):
    """the pinhole part: Cal3_S2::K, or Cal3::K of a Cal3Bundler (fx = fy = f, s = 0)"""
    c = cam[12:17]
    if model == BUNDLER:
        return np.array([[c[0], 0, c[3]], [0, c[0], c[4]], [0, 0, 1.0]])
    return np.array([[c[0], c[2], c[3]], [0, c[1], c[4]], [0, 0, 1.0]])


def projection_matrix(cam, model):
    """PinholeCamera::cameraProjectionMatrix, PinholeCamera.h:316-318: K * pose.inverse().matrix()[0:3, :]"""
    R, t = pose_of(cam)
    return K_of(cam, model) @ np.hstack([R.T, (-R.T @ t).reshape(3, 1)])


def uncalibrate(cam, model, pn, jac=False):
    """Cal3Bundler::uncalibrate (Cal3Bundler.cpp:64-90) / Cal3_S2::uncalibrate, with Dp"""
    c = cam[12:17]
    x, y = pn
    if model == BUNDLER:
        f, k1, k2, u0, v0 = c
        r = x * x + y * y
        g = 1.0 + (k1 + k2 * r) * r
        uv = np.array([u0 + f * (g * x), v0 + f * (g * y)])
        if not jac:
            return uv
        a = 2.0 * (k1 + 2.0 * k2 * r)
        return uv, f * np.array([[g + a * x * x, a * x * y], [a * x * y, g + a * y * y]])
    fx, fy, s, u0, v0 = c
    uv = np.array([fx * x + s * y + u0, fy * y + v0])
    return (uv, np.array([[fx, s], [0.0, fy]])) if jac else uv


def calibrate_bundler(cam, pi, dec=None):
    """Cal3Bundler::calibrate, Cal3Bundler.cpp:93-128: at most 10 passes, break at distance2(uncalibrate(pn), pi) <= 1e-5"""
    f, k1, k2, u0, v0 = cam[12:17]
    inv = np.array([(pi[0] - u0) / f, (pi[1] - v0) / f])
    px, py = inv
    it = 0
    while True:
        rr = px * px + py * py
        g = 1 + k1 * rr + k2 * rr * rr
        pn = inv / g
        d = np.linalg.norm(uncalibrate(cam, BUNDLER, pn) - pi)
        _note(dec, "calibrate", d, 1e-5, max(d, 1e-5))
        if d <= 1e-5:
            break
        px, py = pn
        it += 1
        if not it < 10:
            break
    if it >= 10:
        raise CalibrateFailed()
    return pn


def undistort(cam, model, z, dec=None):
    """undistortMeasurementInternal, triangulation.h:252-268: nothing for Cal3_S2"""
    if model == S2:
        return np.asarray(z, dtype=float)
    pn = calibrate_bundler(cam, np.asarray(z, dtype=float), dec)
    return (K_of(cam, model) @ np.array([pn[0], pn[1], 1.0]))[:2]


def project(cam, model, p, jac=False, dec=None):
    """PinholeCamera::project2 (PinholeCamera.h:283-300; PinholeBase::project2 CalibratedCamera.cpp:116-136).  None where the reference throws
    CheiralityException."""
    R, t = pose_of(cam)
    q = R.T @ (p - t)
    _note(dec, "cheirality", q[2], 0.0, np.linalg.norm(p - t))
    if q[2] <= 0:
        return None
    d = 1.0 / q[2]
    pn = np.array([q[0] * d, q[1] * d])
    if not jac:
        return uncalibrate(cam, model, pn)
    uv, Dp = uncalibrate(cam, model, pn, True)
    Rt = R.T
    Dpn = d * np.array([Rt[0] - pn[0] * Rt[2], Rt[1] - pn[1] * Rt[2]])  # PinholeBase::Dpoint :37-46
    return uv, Dp @ Dpn


def dlt_matrix(cams, model, zs_undistorted):
    """triangulateHomogeneousDLT, triangulation.cpp:27-50"""
    A = np.zeros((2 * len(cams), 4))
    for i, (cam, z) in enumerate(zip(cams, zs_undistorted)):
        P = projection_matrix(cam, model)
        A[2 * i] = z[0] * P[2] - P[0]
        A[2 * i + 1] = z[1] * P[2] - P[1]
    return A


def dlt(A, rank_tol, dec=None):
    """DLT, gtsam/base/Matrix.cpp:556-574: rank = the number of the four singular values > rank_tol, v = the last right singular vector"""
    s, Vt = np.linalg.svd(A, full_matrices=True)[1:]
    s = np.concatenate([s, np.zeros(4 - len(s))])
    for sv in s:
        _note(dec, "rank", sv, rank_tol, max(sv, rank_tol, 1e3 * EPS * s[0]))
    return int((s > rank_tol).sum()), Vt[3]


def graph_error(cams, model, zs, p, w, dec=None):
    """NonlinearFactorGraph::error of triangulationGraph: 0.5 sum |whitened (project(p) - z)|^2; behind a camera the factor's error is
    (2 fx, 2 fx) (TriangulationFactor.h:122-136, PinholeCamera.h:321-323)"""
    e = 0.0
    for cam, z in zip(cams, zs):
        uv = project(cam, model, p, dec=dec)
        r = w * ((uv - z) if uv is not None else np.full(2, 2.0 * cam[12]))
        e += r @ r
    return 0.5 * e


def linearize(cams, model, zs, p, w, dec=None):
    J, b = np.zeros((2 * len(cams), 3)), np.zeros(2 * len(cams))
    for i, (cam, z) in enumerate(zip(cams, zs)):
        r = project(cam, model, p, jac=True, dec=dec)
        if r is None:
            b[2 * i:2 * i + 2] = -w * 2.0 * cam[12]
        else:
            J[2 * i:2 * i + 2] = w * r[1]
            b[2 * i:2 * i + 2] = -w * (r[0] - z)
    return J, b


def refine(cams, model, zs, x, inv_sigma=0.0, dec=None):
    """triangulateNonlinear -> optimize (triangulation.cpp:177-195): LevenbergMarquardtParams() with lambdaInitial 1, lambdaFactor 10,
    maxIterations 100, absoluteErrorTol 1; NonlinearOptimizer::defaultOptimize (NonlinearOptimizer.cpp:62-117) around
    LevenbergMarquardtOptimizer::iterate / tryLambda (LevenbergMarquardtOptimizer.cpp:121-308).  Returns (point, tryLambda calls)."""
    w = inv_sigma if inv_sigma > 0 else 1.0
    relTol, absTol, errTol, maxIt, minFid, lamUp, lamLo, factor = 1e-5, 1.0, 0.0, 100, 1e-3, 1e5, 0.0, 10.0
    x = np.array(x, dtype=float)
    err = graph_error(cams, model, zs, x, w, dec)
    lam, iterations, inner = 1.0, 0, 0
    if err <= errTol:
        return x, 0
    newError = err
    while True:
        currentError = newError
        J, b = linearize(cams, model, zs, x, w, dec)
        H, g = J.T @ J, J.T @ b
        oldLin = 0.5 * (b @ b)
        while True:  # while (!tryLambda())
            inner += 1
            step_ok, stop, nerr, xn = False, False, np.inf, x
            try:
                L = np.linalg.cholesky(H + lam * np.eye(3))
                delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
                solved = True
            except np.linalg.LinAlgError:
                solved = False
            if solved:
                r = J @ delta - b
                lcc = oldLin - 0.5 * (r @ r)
                scale = abs(g @ delta) + 0.5 * abs(delta @ H @ delta)
                _note(dec, "linearizedCostChange >= 0", lcc, 0.0, scale)
                if lcc >= 0:
                    xn = x + delta
                    nerr = graph_error(cams, model, zs, xn, w, dec)
                    costChange = err - nerr
                    _note(dec, "linearizedCostChange > eps oldLin", lcc, EPS * oldLin, scale)
                    if lcc > EPS * oldLin:
                        mf = costChange / lcc
                        _note(dec, "modelFidelity", mf, minFid, max(abs(mf), minFid))
                        step_ok = mf > minFid
                    _note(dec, "stopSearchingLambda", abs(costChange), relTol * err, max(abs(costChange), relTol * err))
                    if abs(costChange) < relTol * err:
                        stop = True
            if step_ok:
                x, err, lam = xn, nerr, max(lamLo, lam / factor)
                iterations += 1
                break
            elif not stop:
                lam *= factor
                if lam >= lamUp:
                    break
            else:
                break
        newError = err
        conv = newError <= errTol
        if not conv:  # checkConvergence, NonlinearOptimizer.cpp:182-231
            dec_abs = currentError - newError
            _note(dec, "relativeErrorTol", dec_abs / currentError, relTol, max(abs(dec_abs / currentError), relTol))
            _note(dec, "absoluteErrorTol", dec_abs, absTol, max(abs(dec_abs), absTol))
            conv = (dec_abs / currentError <= relTol) or (dec_abs <= absTol)
        if not (iterations < maxIt and not conv and np.isfinite(currentError)):
            break
    return x, inner


def triangulate_point3(cams, model, zs, rank_tol=1e-9, optimize=False, inv_sigma=0.0, dec=None, info=None):
    """triangulatePoint3<CAMERA>, triangulation.h:491-549, GTSAM_THROW_CHEIRALITY_EXCEPTION on"""
    if len(cams) < 2:
        raise Underconstrained()
    und = [undistort(c, model, z, dec) for c, z in zip(cams, zs)]
    rank, v = dlt(dlt_matrix(cams, model, und), rank_tol, dec)
    if rank < 3:
        raise Underconstrained()
    p = v[:3] / v[3]
    if optimize:
        p, inner = refine(cams, model, [np.asarray(z, dtype=float) for z in zs], p, inv_sigma, dec)
        if info is not None:
            info["iterations"] = inner
    for cam in cams:
        R, t = pose_of(cam)
        z = (R.T @ (p - t))[2]
        _note(dec, "cheirality", z, 0.0, np.linalg.norm(p - t))
        if z <= 0:
            raise Cheirality()
    return p


def triangulate_safe(cams, model, zs, params, dec=None):
    """triangulateSafe, triangulation.h:701-758 -> (status, point or None, tryLambda calls)"""
    info = {"iterations": 0}
    if len(cams) < 2:
        return DEGENERATE, None, 0
    try:
        p = triangulate_point3(cams, model, zs, params.rankTolerance, params.enableEPI, params.noise_inv_sigma, dec, info)
    except Underconstrained:
        return DEGENERATE, None, info["iterations"]
    except Cheirality:
        return BEHIND_CAMERA, None, info["iterations"]
    except CalibrateFailed:
        return CALIBRATE_FAILED, None, 0
    maxrep = 0.0
    for cam, z in zip(cams, zs):
        _, t = pose_of(cam)
        if params.landmarkDistanceThreshold > 0:
            d = np.linalg.norm(t - p)
            _note(dec, "landmarkDistanceThreshold", d, params.landmarkDistanceThreshold, max(d, params.landmarkDistanceThreshold))
            if d > params.landmarkDistanceThreshold:
                return FAR_POINT, None, info["iterations"]
        if params.dynamicOutlierRejectionThreshold > 0:
            maxrep = max(maxrep, np.linalg.norm(project(cam, model, p) - np.asarray(z, dtype=float)))
    if params.dynamicOutlierRejectionThreshold > 0:
        _note(dec, "dynamicOutlierRejectionThreshold", maxrep, params.dynamicOutlierRejectionThreshold,
              max(maxrep, params.dynamicOutlierRejectionThreshold))
        if maxrep > params.dynamicOutlierRejectionThreshold:
            return OUTLIER, None, info["iterations"]
    return VALID, p, info["iterations"]


def batch(cams, model, offsets, obs_cam, obs_z, params, dec=None):
    """triangulateSafe per landmark of a CSR batch -> points (n, 3; NaN unless VALID), status (n), tryLambda calls (n)"""
    cams, obs_z = np.asarray(cams, dtype=float).reshape(-1, 17), np.asarray(obs_z, dtype=float).reshape(-1, 2)
    n = len(offsets) - 1
    pts, st, it = np.full((n, 3), np.nan), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i in range(n):
        sel = range(offsets[i], offsets[i + 1])
        d = [] if dec is not None else None
        st[i], p, it[i] = triangulate_safe([cams[obs_cam[o]] for o in sel], model, [obs_z[o] for o in sel], params, d)
        if dec is not None:
            dec.append(d)
        if p is not None:
            pts[i] = p
    return pts, st, it


def worst_margin(decisions):
    """the smallest |value - bound| / scale of a list of recorded decisions (inf for none), and that decision"""
    worst, which = np.inf, None
    for d in decisions:
        name, value, bound, scale = d
        m = abs(value - bound) / scale if scale > 0 else np.inf
        if m < worst:
            worst, which = m, d
    return worst, which
