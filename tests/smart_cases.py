"""Inputs of the smart projection factor tests: the fixtures of gtsam/slam/tests/smartFactorScenarios.h and the scenes the device is compared
on (tests/test_gpu_smart.py).  A scene is a dict
    values {key: pose12}, order [pose keys in elimination order],
    factors [("smart", keys, zs, K5, sigma, smart_restatement.SmartParams) | ("prior", key, pose12, sigma) | ("between", k1, k2, pose12, sigma)]
in graph order.  `restatement(scene)` builds the numpy checker's Graph (priors and smart factors only), `package(scene)` the
gtsam_personal_amd graph, values and ordering of the same inputs."""
import numpy as np

import smart_restatement as sr
import triangulation_cases as tc
import triangulation_restatement as tr

# ---------------------------------------------------------------- smartFactorScenarios.h:34-60, 94
LANDMARK1, LANDMARK2, LANDMARK3 = np.array([5, 0.5, 1.2]), np.array([5, -0.5, 1.2]), np.array([3, 0, 3.0])
LEVEL_POSE = sr.pose(sr.ypr(-np.pi / 2, 0.0, -np.pi / 2), [0, 0, 1])
POSE_RIGHT = sr.compose(LEVEL_POSE, sr.pose(np.eye(3), [1, 0, 0]))
POSE_ABOVE = sr.compose(LEVEL_POSE, sr.pose(np.eye(3), [0, -1, 0]))
WRONG_WAY = sr.pose(sr.ypr(np.pi / 2, 0.0, -np.pi / 2), [0, 0, 1])  # testTriangulation.cpp:330
_F = 640 / (2.0 * np.tan(np.deg2rad(60.0) / 2.0))
K_FOV = np.array([_F, _F, 0.0, 320.0, 240.0])  # Cal3_S2(fov = 60, w = 640, h = 480), Cal3_S2.cpp
K2 = np.array([1500.0, 1200.0, 0.0, 640.0, 480.0])
SIGMA = 0.1
X1, X2, X3 = [(ord("X") << 56) | i for i in (1, 2, 3)]


def project(p12, K5, point):
    return sr.project_jac(p12, K5, np.asarray(point, dtype=float))[0]


def zero_on_degeneracy(**tri):
    thr = tri.pop("retriangulationThreshold", 1e-5)
    return sr.SmartParams(tr.Params(**tri), thr)


def every_change(**tri):
    """retriangulationThreshold 0: a factor re-triangulates iff a pose entry changed at all.  The threshold of the scenes that the device runs
    Levenberg-Marquardt on: the steps of a converging optimizer pass through every magnitude, so no positive threshold keeps every cache
    test of such a run a factor of 10 away from it, while "changed at all" is decided alike by the device and the restatement as long as
    the largest change of a call is far above the last bit (checked in tests/test_smart_reference.py)"""
    return zero_on_degeneracy(retriangulationThreshold=0.0, **tri)


def smart(keys, poses, K5, landmark, params=None, sigma=SIGMA, noise=None):
    zs = [project(p, K5, landmark) for p in poses]
    if noise is not None:
        zs = [z + n for z, n in zip(zs, noise)]
    return ("smart", list(keys), zs, np.asarray(K5, dtype=float), sigma, params or zero_on_degeneracy())


def factors_scene():
    """testSmartProjectionPoseFactor.cpp:336-414"""
    K = np.array([100.0, 100, 0, 0, 0])
    p1, p2 = sr.pose(np.eye(3), [0, 0, 0]), sr.pose(np.eye(3), [1, 0, 0])
    return dict(values={X1: p1, X2: p2}, order=[X1, X2], factors=[smart([X1, X2], [p1, p2], K, [0, 0, 10.0])])


def factors_expected_information():
    """:385-406: A1, A2 scaled by 10 / sigma, G = 0.5 A'A, g = 0, f = 0"""
    A = np.concatenate([np.array([-10.0, 0, 0, 0, 1, 0]), np.array([10.0, 0, 1, 0, -1, 0])]) * 10.0 / SIGMA
    out = np.zeros((13, 13))
    out[:12, :12] = 0.5 * np.outer(A, A)
    return out


NOISE_POSE = sr.pose(sr.ypr(-np.pi / 100, 0.0, -np.pi / 100), [0.1, 0.1, 0.1])


def three_poses_scene(perturbed=True, K5=K2, params=None):
    """3poses_smart_projection_factor, :275-333: three factors over (x1, x2, x3), priors on x1, x2, x3 started off pose_above"""
    poses = [LEVEL_POSE, POSE_RIGHT, POSE_ABOVE]
    keys = [X1, X2, X3]
    fs = [smart(keys, poses, K5, lm, params) for lm in (LANDMARK1, LANDMARK2, LANDMARK3)]
    fs += [("prior", X1, LEVEL_POSE, 0.10), ("prior", X2, POSE_RIGHT, 0.10)]
    x3 = sr.compose(POSE_ABOVE, NOISE_POSE) if perturbed else POSE_ABOVE
    return dict(values={X1: LEVEL_POSE, X2: POSE_RIGHT, X3: x3}, order=keys, factors=fs)


PRINTED_X3 = sr.pose([[0, -0.0314107591, 0.99950656], [-0.99950656, -0.0313952598, -0.000986635786], [0.0314107591, -0.999013364, -0.0313952598]],
                     [0.1, -0.1, 1.9])  # :324-327


def five_status_scene(thr=0.0):
    """one graph with every status: VALID, FAR_POINT, OUTLIER, DEGENERATE (one observation), DEGENERATE (rank), BEHIND_CAMERA; priors on all.
    thr: the retriangulationThreshold of every factor (0: re-triangulate whenever a pose entry changed at all, see EVERY_CHANGE)"""
    zod = lambda **kw: zero_on_degeneracy(retriangulationThreshold=thr, **kw)  # noqa: E731
    plain = zod()  # shared by the four factors without a threshold of their own: one group of mixed observation counts
    X4, X5 = [(ord("X") << 56) | i for i in (4, 5)]
    poses3, keys3 = [LEVEL_POSE, POSE_RIGHT, POSE_ABOVE], [X1, X2, X3]
    fs = [smart(keys3, poses3, K2, LANDMARK1, plain),
          smart(keys3, poses3, K2, LANDMARK1, zod(landmarkDistanceThreshold=2.0)),
          smart(keys3, poses3, K2, [5, -0.5, 1.0], zod(dynamicOutlierRejectionThreshold=1.0),
                noise=[np.array([10.0, 10.0]), np.zeros(2), np.zeros(2)]),
          smart([X1], [LEVEL_POSE], K2, LANDMARK1, plain),
          smart([X1, X5], [LEVEL_POSE, LEVEL_POSE], K2, LANDMARK1, plain)]
    bc = smart([X1, X2, X4], [LEVEL_POSE, POSE_RIGHT, LEVEL_POSE], K2, LANDMARK1, plain)
    bc[2][2] = np.array([400.0, 400.0])  # the wrong-way camera's measurement, testTriangulation.cpp:337-339
    fs.append(bc)
    values = {X1: LEVEL_POSE, X2: POSE_RIGHT, X3: sr.compose(POSE_ABOVE, NOISE_POSE), X4: WRONG_WAY, X5: LEVEL_POSE.copy()}
    order = [X1, X2, X3, X4, X5]
    fs += [("prior", k, {X1: LEVEL_POSE, X2: POSE_RIGHT, X3: POSE_ABOVE, X4: WRONG_WAY, X5: LEVEL_POSE}[k], 0.10) for k in order]
    return dict(values=values, order=order, factors=fs)


FIVE_STATUS = (tr.VALID, tr.FAR_POINT, tr.OUTLIER, tr.DEGENERATE, tr.DEGENERATE, tr.BEHIND_CAMERA)


def ring_scene(degrees, seed=5, n_cams=24, sigma_px=0.5, perturb=1e-3, params=None):
    """24 ring cameras (triangulation_cases.ring_cameras) with one calibration, priors on all, one smart factor per entry of `degrees`
    over that many distinct cameras; the poses start slightly off the truth.  All factors share ONE parameter object, so they reach the
    device in one lmgpu_add_smart_factors call and its triangulation launches hold many lanes of mixed observation counts"""
    params = params or zero_on_degeneracy()
    rng = np.random.default_rng(seed)
    cams = tc.ring_cameras(n_cams, tr.S2, rng)
    K5 = cams[0, 12:17].copy()
    keys = [(ord("X") << 56) | i for i in range(n_cams)]
    truth = {k: cams[i, :12].copy() for i, k in enumerate(keys)}
    fs = []
    for d in degrees:
        lm = rng.uniform(-4, 4, 3)
        sel = np.sort(rng.choice(n_cams, d, replace=False))
        noise = [rng.normal(0, sigma_px, 2) for _ in sel]
        fs.append(smart([keys[i] for i in sel], [truth[keys[i]] for i in sel], K5, lm, params, sigma=1.0, noise=noise))
    fs += [("prior", k, truth[k], 0.05) for k in keys]
    values = {k: sr.retract(truth[k], perturb * rng.normal(0, 1, 6)) for k in keys}
    return dict(values=values, order=keys, factors=fs)


def restatement(scene):
    fs = []
    for f in scene["factors"]:
        if f[0] == "smart":
            fs.append(sr.SmartFactor(f[1], f[2], f[3], f[4], f[5]))
        elif f[0] == "prior":
            fs.append(sr.Prior(f[1], f[2], f[3]))
        else:
            raise NotImplementedError(f[0])
    return sr.Graph(fs, scene["order"]), {k: v.copy() for k, v in scene["values"].items()}


def package_params(p):
    import gtsam_personal_amd as gpa
    from gtsam_personal_amd import smart as S
    out = gpa.SmartProjectionParams(S.HESSIAN, S.ZERO_ON_DEGENERACY, retriangulationTh=p.retriangulationThreshold)
    t = p.triangulation
    out.triangulation = gpa.TriangulationParameters(t.rankTolerance, t.enableEPI, t.landmarkDistanceThreshold, t.dynamicOutlierRejectionThreshold,
                                                    noiseModel=(t.noise_inv_sigma or None))
    return out


def package(scene, explicit_points=None):
    """-> (graph, values, ordering, smart factor objects).  explicit_points: a list of points, one per smart factor (None: skip it): the same
    scene with POINT3 variables and GenericProjectionFactors instead of smart factors (landmark keys L(i), eliminated first)."""
    import gtsam_personal_amd as gpa
    from gtsam_personal_amd import graph as G
    g, v = gpa.NonlinearFactorGraph(), gpa.Values()
    for k, p in scene["values"].items():
        v.insert(k, G.POSE3, p)
    cache, objs, lms = {}, [], []
    i_smart = 0
    for f in scene["factors"]:
        if f[0] == "smart":
            if explicit_points is None:
                if id(f[5]) not in cache:
                    cache[id(f[5])] = package_params(f[5])
                o = gpa.SmartProjectionPoseFactor(G.noiseModel.Isotropic.Sigma(2, f[4], smart=False), f[3], cache[id(f[5])])
                o.add(f[2], f[1])
                g.add_SmartProjectionPoseFactor(o)
                objs.append(o)
            elif explicit_points[i_smart] is not None:
                lk = G.L(i_smart)
                v.insert(lk, G.POINT3, explicit_points[i_smart])
                lms.append(lk)
                for k, z in zip(f[1], f[2]):
                    g.add_GenericProjectionFactor(z, G.noiseModel.Isotropic.Sigma(2, f[4], smart=False), k, lk, f[3])
            i_smart += 1
        elif f[0] == "prior":
            R, t = sr.Rt(f[2])
            g.add_PriorFactorPose3(f[1], R, t, G.noiseModel.Isotropic.Sigma(6, f[3], smart=False))
        elif f[0] == "between":
            R, t = sr.Rt(f[3])
            g.add_BetweenFactorPose3(f[1], f[2], R, t, G.noiseModel.Isotropic.Sigma(6, f[4], smart=False))
    return g, v, gpa.Ordering(lms + list(scene["order"])), objs
