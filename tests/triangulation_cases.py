"""Inputs of the triangulation tests: the scenes of gtsam/geometry/tests/testTriangulation.cpp with their known answers, and the batches
the device is compared on (tests/test_gpu_triangulation.py).  Every batch is a dict
    name, model, cams (n, 17), offsets (n_points + 1), obs_cam, obs_z (n_obs, 2), params (triangulation_restatement.Params)
and `expected(case)` is the restatement's answer for it, computed once per process and shared by the tests."""
import functools
import os

import numpy as np

import triangulation_restatement as r
from gtsam_personal_amd import graph as G
from gtsam_personal_amd.datasets import SfmData, bal_graph, pose3_compose, rot3_ypr
from gtsam_personal_amd.synthetic import make_bal

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUNDLER, S2 = r.BUNDLER, r.S2


def cam17(R, t, c5):
    return np.concatenate([np.asarray(R, dtype=float).reshape(9), np.asarray(t, dtype=float), np.asarray(c5, dtype=float)])


# ---------------------------------------------------------------- testTriangulation.cpp:36-59
K_SHARED = (1500, 1200, 0.1, 640, 480)
UPRIGHT = rot3_ypr(-np.pi / 2, 0.0, -np.pi / 2)
POSE1 = (UPRIGHT, np.array([0.0, 0, 1]))
POSE2 = pose3_compose(POSE1[0], POSE1[1], np.eye(3), np.array([1.0, 0, 0]))
POSE3 = pose3_compose(POSE1[0], POSE1[1], rot3_ypr(0.1, 0.2, 0.1), np.array([0.1, -2, -0.1]))  # :313
POSE4 = (rot3_ypr(np.pi / 2, 0.0, -np.pi / 2), np.array([0.0, 0, 1]))                           # :330, facing the wrong way
LANDMARK = np.array([5, 0.5, 1.2])
BUNDLER_CAL = (1500, 0.1, 0.2, 640, 480)  # :267
K1, K2, K3, K4 = (1500, 1200, 0, 640, 480), (1600, 1300, 0, 650, 440), (700, 500, 0, 640, 480), (700, 500, 0, 640, 480)  # :431-479
NOISE1, NOISE2, NOISE3 = np.array([0.1, 0.5]), np.array([-0.2, 0.3]), np.array([0.1, -0.1])


def scene(model, cals, noisy=(False, False, False), wrong_way=False, n=2, z3_offset=NOISE3):
    """cameras at POSE1.. with the given calibrations, the landmark's projections (+ the test file's noise)"""
    poses = [POSE1, POSE2, POSE3, POSE4][:4 if wrong_way else n]
    cams = [cam17(R, t, cals[i]) for i, (R, t) in enumerate(poses)]
    zs = []
    for i, cam in enumerate(cams[:3]):
        z = r.project(cam, model, LANDMARK)
        if noisy[i]:
            z = z + (NOISE1, NOISE2, z3_offset)[i]
        zs.append(z)
    if wrong_way:
        zs.append(np.array([400.0, 400.0]))
    return cams, zs


def single(name, model, cams, zs, params):
    m = len(cams)
    return dict(name=name, model=model, cams=np.array(cams).reshape(-1, 17), offsets=np.array([0, m], dtype=np.int32),
                obs_cam=np.arange(m, dtype=np.int32), obs_z=np.array(zs, dtype=float).reshape(-1, 2), params=params)


def merge(name, cases):
    """single-landmark cases with the same model and params as one batch"""
    cams, off, oc, oz = [], [0], [], []
    for c in cases:
        assert c["model"] == cases[0]["model"]
        base = sum(len(x) for x in cams)
        cams.append(c["cams"])
        oc.append(c["obs_cam"] + base)
        oz.append(c["obs_z"])
        off.append(off[-1] + len(c["obs_cam"]))
    return dict(name=name, model=cases[0]["model"], cams=np.concatenate(cams), offsets=np.array(off, dtype=np.int32),
                obs_cam=np.concatenate(oc).astype(np.int32), obs_z=np.concatenate(oz), params=cases[0]["params"])


def known_scene_batches(model):
    """the known-answer scenes as device batches (one per parameter set).  The noise-free scenes run without refinement only: at a residual of
    rounding size every accept test of the LM is decided by the last bit (test_decision_margins would reject them)."""
    cal = [K_SHARED] * 4 if model == S2 else [BUNDLER_CAL] * 4
    dist = [K1, K2, K3, K4] if model == S2 else [(1500, 0.1, 0.2, 640, 480), (1600, 0.05, 0.1, 650, 440), (700, -0.1, 0.05, 640, 480), (700, 0, 0, 640, 480)]
    P = r.Params
    out = []
    for tag, opt in (("dlt", False), ("epi", True)):
        p9 = P(rankTolerance=1e-9, enableEPI=opt)
        items = [single("twoPoses noisy", model, *scene(model, cal, (True, True, False)), p9),
                 single("fourPoses three noisy cameras", model, *scene(model, cal, (True, True, True), n=3), p9),
                 single("distinct Ks noisy", model, *scene(model, dist, (True, True, False)), p9),
                 single("distinct Ks three cameras", model, *scene(model, dist, (True, True, True), n=3), p9),
                 single("wrong way", model, *scene(model, cal, (True, True, True), wrong_way=True), p9),
                 single("distinct Ks wrong way", model, *scene(model, dist, (True, True, True), wrong_way=True), p9)]
        if not opt:
            items += [single("twoPoses", model, *scene(model, cal), p9), single("distinct Ks", model, *scene(model, dist), p9),
                      single("twoIdenticalPoses", model, [cam17(*POSE1, cal[0])] * 2, [r.project(cam17(*POSE1, cal[0]), model, LANDMARK)] * 2, p9),
                      single("onePose", model, [cam17(np.eye(3), np.zeros(3), cal[0])], [np.zeros(2)], p9)]
        out.append(merge(f"known scenes {tag} model {model}", items))
    # outliersAndFarLandmarks :515-569
    two, three = scene(model, dist), scene(model, dist, (False, False, True), n=3, z3_offset=np.array([10.0, -10.0]))
    out += [single(f"far 10 model {model}", model, *two, P(1.0, False, 10)), single(f"far 4 model {model}", model, *two, P(1.0, False, 4)),
            single(f"outlier 100 model {model}", model, *three, P(1.0, False, 10, 100)),
            single(f"outlier 5 model {model}", model, *three, P(1.0, False, 10, 5))]
    return out


# ---------------------------------------------------------------- synthetic batches
def lookat(eye, target, up=np.array([0.0, 0, 1])):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1), eye


def ring_cameras(n, model, rng, distortion=1.0):
    cams = []
    for i in range(n):
        a = 2 * np.pi * i / n
        R, t = lookat(np.array([30 * np.cos(a), 30 * np.sin(a), rng.uniform(-3, 3)]), np.zeros(3))
        if model == BUNDLER:
            c5 = (500 + 20 * rng.uniform(-1, 1), distortion * 1e-2 * rng.uniform(-1, 1), distortion * 1e-3 * rng.uniform(-1, 1), 320 + rng.uniform(-5, 5),
                  240 + rng.uniform(-5, 5))
        else:
            c5 = (500 + 20 * rng.uniform(-1, 1), 480 + 20 * rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), 320 + rng.uniform(-5, 5), 240 + rng.uniform(-5, 5))
        cams.append(cam17(R, t, c5))
    return np.array(cams)


def ring_batch(name, model, degrees, params, seed, n_cams=24, sigma=0.5, distortion=1.0):
    """landmarks in a box at the centre of a ring of cameras; landmark i is seen by degrees[i] distinct cameras; sigma: pixel noise (a scalar
    or one per landmark)"""
    rng = np.random.default_rng(seed)
    cams = ring_cameras(n_cams, model, rng, distortion)
    sig = np.broadcast_to(np.asarray(sigma, dtype=float), (len(degrees),))
    off, oc, oz, pts = [0], [], [], rng.uniform(-8, 8, (len(degrees), 3))
    for i, d in enumerate(degrees):
        sel = np.sort(rng.choice(n_cams, d, replace=False))
        for ci in sel:
            oc.append(ci)
            oz.append(r.project(cams[ci], model, pts[i]) + rng.normal(0, sig[i], 2))
        off.append(off[-1] + d)
    return dict(name=name, model=model, cams=cams, offsets=np.array(off, dtype=np.int32), obs_cam=np.array(oc, dtype=np.int32),
                obs_z=np.array(oz, dtype=float).reshape(-1, 2), params=params, truth=pts)


def prefix(case, n):
    """the first n landmarks of a batch"""
    k = case["offsets"][n]
    return dict(case, name=f"{case['name']} first {n}", offsets=case["offsets"][:n + 1], obs_cam=case["obs_cam"][:k], obs_z=case["obs_z"][:k])


COUNTS = (1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def counts_batch(model):
    rng = np.random.default_rng(5 + model)
    return ring_batch(f"counts model {model}", model, rng.integers(2, 6, 257), r.Params(rankTolerance=1.0), seed=11 + model)


@functools.lru_cache(maxsize=None)
def degrees_batch(model):
    return ring_batch(f"degrees 0 1 2 3 17 model {model}", model, [0, 1, 2, 3, 17, 2, 0, 3, 17, 1], r.Params(rankTolerance=1e-9), seed=21 + model)


@functools.lru_cache(maxsize=None)
def degree70_batch(model):
    deg = [2] * 64
    deg[5] = 70
    return ring_batch(f"degree 70 model {model}", model, deg, r.Params(rankTolerance=1e-9), seed=31 + model, n_cams=80)


DIST_THR, OUT_THR = 45.0, 6.0


@functools.lru_cache(maxsize=None)
def mixed_status_batch(model):
    """one wave with every status: VALID lanes beside a landmark of one observation, one seen twice by the same camera, one behind a
    camera, an outlier, a far point, one both behind a camera and beyond the distance threshold of another (BEHIND_CAMERA), one both far
    and an outlier (FAR_POINT) and, for Cal3Bundler, one whose calibrate does not converge"""
    c = ring_batch(f"mixed statuses model {model}", model, [3] * 40, r.Params(1e-9, False, DIST_THR, OUT_THR), seed=41 + model)
    cams, rng = list(c["cams"]), np.random.default_rng(43)
    off, oc, oz = list(c["offsets"]), list(c["obs_cam"]), [z for z in c["obs_z"]]

    def add(cam_ids, zs):
        oc.extend(cam_ids)
        oz.extend(zs)
        off.append(off[-1] + len(cam_ids))

    def seen(p, ids, noise=0.3):
        return [r.project(cams[i], model, p) + rng.normal(0, noise, 2) for i in ids]

    p = np.array([1.0, -2.0, 0.5])
    add([3], seen(p, [3]))                                   # 40 DEGENERATE: one observation
    add([3, 3], [r.project(cams[3], model, p)] * 2)          # 41 DEGENERATE: the same camera twice
    # 42 BEHIND_CAMERA: a camera at the ring looking outward, its measurement anything
    Rb, tb = lookat(np.array([30.0, 0, 0]), np.array([60.0, 0, 0]))
    cams.append(cam17(Rb, tb, cams[0][12:17]))
    back = len(cams) - 1
    add([2, 9, back], seen(p, [2, 9]) + [np.array([300.0, 200.0])])
    # 43 OUTLIER: one measurement 40 pixels off
    zs = seen(p, [1, 6, 12])
    zs[2] = zs[2] + np.array([40.0, -30.0])
    add([1, 6, 12], zs)
    # 44 FAR_POINT: 40 above the centre
    far = np.array([0.0, 0.0, 40.0])
    add([0, 8, 16], seen(far, [0, 8, 16]))
    # 45 behind `back` and far from the others: BEHIND_CAMERA
    add([0, 8, back], seen(far, [0, 8]) + [np.array([300.0, 200.0])])
    # 46 far and an outlier: FAR_POINT
    zs = seen(far, [0, 8, 16])
    zs[1] = zs[1] + np.array([60.0, 60.0])
    add([0, 8, 16], zs)
    want = [r.DEGENERATE, r.DEGENERATE, r.BEHIND_CAMERA, r.OUTLIER, r.FAR_POINT, r.BEHIND_CAMERA, r.FAR_POINT]
    if model == BUNDLER:  # 47 CALIBRATE_FAILED: a camera whose distortion makes the fixed-point iteration diverge at this pixel
        bad = cams[4].copy()
        bad[13:15] = (4.0, 9.0)
        cams.append(bad)
        add([2, len(cams) - 1, 11], seen(p, [2]) + [bad[15:17] + np.array([450.0, 380.0])] + seen(p, [11]))
        want.append(r.CALIBRATE_FAILED)
    for _ in range(64 - (len(off) - 1)):  # VALID lanes after them, same wave
        ids = np.sort(rng.choice(24, 3, replace=False))
        add(list(ids), seen(rng.uniform(-8, 8, 3), ids))
    c.update(cams=np.array(cams), offsets=np.array(off, dtype=np.int32), obs_cam=np.array(oc, dtype=np.int32), obs_z=np.array(oz).reshape(-1, 2),
             want_special=want)
    return c


@functools.lru_cache(maxsize=None)
def refine_batch(model, inv_sigma=0.0):
    """one wave whose lanes need different numbers of tryLambda calls: pixel noise from 0.3 to 25 per landmark"""
    rng = np.random.default_rng(57 + model)
    deg = rng.integers(2, 7, 64)
    return ring_batch(f"refinement model {model} inv_sigma {inv_sigma}", model, deg, r.Params(1e-9, True, noise_inv_sigma=inv_sigma),
                      seed=53 + model, sigma=np.geomspace(0.3, 25.0, 64))


@functools.lru_cache(maxsize=None)
def crossing_batch(model):
    """landmarks a little in front of a close camera that sees them far off its axis, with a gross measurement error there: trial steps of
    the refinement land behind that camera and take the factor's constant-error branch.  Candidates are drawn until 16 of them do so in the
    restatement, end VALID and keep every decision 5e-3 clear of its boundary."""
    rng = np.random.default_rng(61 + model)
    cams = list(ring_cameras(8, model, rng))
    off, oc, oz = [0], [], []
    for _ in range(4000):
        p = rng.uniform(-3, 3, 3)
        d = rng.normal(0, 1, 3)
        depth = rng.uniform(0.05, 0.2)
        eye = p + depth * d / np.linalg.norm(d)
        R, t = lookat(eye, p + 0.5 * depth * rng.uniform(-1, 1, 3))
        close = cam17(R, t, cams[0][12:17])
        if model == BUNDLER:
            close[13:15] = 0.0  # no distortion: calibrate converges at any pixel
        if r.project(close, model, p) is None:
            continue
        ids = [0, 3, 5]
        zs = [r.project(cams[k], model, p) + rng.normal(0, 1.0, 2) for k in ids]
        zc = r.project(close, model, p)
        zs.append(zc + rng.uniform(300, 3000) * (zc - close[15:17]) / np.linalg.norm(zc - close[15:17]))
        dec = []
        st, _, _ = r.triangulate_safe([cams[k] for k in ids] + [close], model, zs, r.Params(1e-9, True), dec)
        crossed = sum(1 for x in dec if x[0] == "cheirality" and x[1] <= 0)
        if st != r.VALID or crossed == 0 or r.worst_margin(dec)[0] < 5e-3:
            continue
        cams.append(close)
        oc += ids + [len(cams) - 1]
        oz += zs
        off.append(len(oc))
        if len(off) == 17:
            break
    assert len(off) == 17
    return dict(name=f"crossing model {model}", model=model, cams=np.array(cams), offsets=np.array(off, dtype=np.int32),
                obs_cam=np.array(oc, dtype=np.int32), obs_z=np.array(oz).reshape(-1, 2), params=r.Params(1e-9, True))


@functools.lru_cache(maxsize=None)
def distortion_batch():
    """Cal3Bundler with strong distortion: calibrate takes several passes"""
    return ring_batch("strong distortion", BUNDLER, [3] * 70, r.Params(1e-9, False), seed=72, distortion=60.0)


# ---------------------------------------------------------------- graphs (handle form)
def graph_batch(name, graph, values, ordering, params):
    """the batch lmgpu_triangulate_landmarks works on: the POINT3 variables in the order of `ordering`, the observations of each in
    graph-index order, cameras = the current values.  Returns (case, point keys)."""
    pts = [int(k) for k in ordering if values.type(k) == G.POINT3]
    obs = {k: [] for k in pts}
    cam_index, cams, model = {}, [], None
    for ftype, _, gi, keys, meas, _, _ in graph.buckets():
        if ftype not in (G.F_SFM, G.F_PROJECTION):
            continue
        m = BUNDLER if ftype == G.F_SFM else S2
        assert model in (None, m)
        model = m
        for g, ks, ms in zip(gi, keys, meas):
            ck, pk = int(ks[0]), int(ks[1])
            cam = values.at(ck)[:17] if m == BUNDLER else np.concatenate([values.at(ck)[:12], ms[2:7]])
            key = (ck, tuple(ms[2:7]) if m == S2 else ())
            if key not in cam_index:
                cam_index[key] = len(cams)
                cams.append(cam)
            obs[pk].append((int(g), cam_index[key], ms[:2]))
    off, oc, oz = [0], [], []
    for k in pts:
        for _, ci, z in sorted(obs[k], key=lambda e: e[0]):
            oc.append(ci)
            oz.append(z)
        off.append(len(oc))
    case = dict(name=name, model=model if model is not None else BUNDLER, cams=np.array(cams).reshape(-1, 17), offsets=np.array(off, dtype=np.int32),
                obs_cam=np.array(oc, dtype=np.int32), obs_z=np.array(oz, dtype=float).reshape(-1, 2), params=params)
    return case, pts


@functools.lru_cache(maxsize=None)
def bal_small():
    return make_bal(n_cam=5, n_pt=130, obs_per_point=3, seed=3)


@functools.lru_cache(maxsize=None)
def bal_medium():
    return make_bal(n_cam=20, n_pt=1000, obs_per_point=10, seed=42)


@functools.lru_cache(maxsize=None)
def dubrovnik():
    db = SfmData.FromBalFile(os.path.join(GOLD, "dubrovnik-3-7-pre.txt"))
    graph, initial = bal_graph(db, camera_key=G.C)
    return graph, initial, None, G.Ordering.Schur(graph, initial)


@functools.lru_cache(maxsize=None)
def projection_graph():
    """POSE3 + POINT3 + GenericProjectionFactor<Pose3, Point3, Cal3_S2>, two calibrations"""
    rng = np.random.default_rng(81)
    cams = ring_cameras(6, S2, rng)
    graph, values = G.NonlinearFactorGraph(), G.Values()
    for i, c in enumerate(cams):
        values.insert_pose3(G.X(i), c[:9].reshape(3, 3), c[9:12])
    Ks = [cams[0][12:17], cams[1][12:17]]
    unit = G.noiseModel.Unit.Create(2)
    for j in range(70):
        p = rng.uniform(-8, 8, 3)
        values.insert_point3(G.L(j), p + rng.normal(0, 0.05, 3))
        for i in np.sort(rng.choice(6, 2 + j % 3, replace=False)):
            K = Ks[(i + j) % 2]
            z = r.project(np.concatenate([cams[i][:12], K]), S2, p) + rng.normal(0, 0.5, 2)
            graph.add_GenericProjectionFactor(z, unit, G.X(i), G.L(j), K)
    ordering = G.Ordering([G.L(j) for j in range(70)] + [G.X(i) for i in range(6)])
    return graph, values, None, ordering


FAR_BAL, FAR_PROJECTION = 32.0, 31.0  # landmarkDistanceThreshold of the handle tests that need landmarks of two statuses
GRAPHS = {"bal_small": bal_small, "dubrovnik": dubrovnik, "projection": projection_graph, "bal_medium": bal_medium}


@functools.lru_cache(maxsize=None)
def graph_case(which, epi=False, dist_thr=-1.0):
    """(batch, point keys) of a graph at its initial values; dist_thr > 0 turns part of the landmarks into FAR_POINT"""
    graph, values, _, ordering = GRAPHS[which]()
    return graph_batch(f"{which} epi {epi} far {dist_thr}", graph, values, ordering,
                       r.Params(rankTolerance=1.0, enableEPI=epi, landmarkDistanceThreshold=dist_thr))


def gpu_parity_cases():
    """every batch the device is compared on (test_decision_margins checks each point of each of them)"""
    out = []
    for model in (BUNDLER, S2):
        out += known_scene_batches(model)
        out += [counts_batch(model), degrees_batch(model), degree70_batch(model), mixed_status_batch(model), refine_batch(model, 0.0),
                refine_batch(model, 10.0), crossing_batch(model)]
    out.append(distortion_batch())
    for which in ("bal_small", "dubrovnik", "projection"):
        out += [graph_case(which, False)[0], graph_case(which, True)[0]]
    out += [graph_case("bal_small", False, FAR_BAL)[0], graph_case("projection", True, FAR_PROJECTION)[0]]
    out += [graph_case("bal_medium", False)[0], graph_case("bal_medium", True)[0]]
    return out


_EXPECTED = {}


def expected(case):
    """(points, status, tryLambda calls, decisions per point) of the restatement, computed once per batch"""
    if case["name"] not in _EXPECTED:
        dec = []
        _EXPECTED[case["name"]] = r.batch(case["cams"], case["model"], case["offsets"], case["obs_cam"], case["obs_z"], case["params"], dec) + (dec,)
    return _EXPECTED[case["name"]]
