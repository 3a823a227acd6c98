"""The numpy restatement of the reference's triangulation (tests/triangulation_restatement.py) reproduces the known answers of
gtsam/geometry/tests/testTriangulation.cpp at that file's own tolerances; the inputs of the device parity tests keep every branch decision
clear of its boundary and are well conditioned; the new ABI surface exists and refuses what it must without a device.  No GPU needed."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import triangulation_cases as c
import triangulation_restatement as r
from gtsam_personal_amd import (LevenbergMarquardtOptimizer, NonlinearFactorGraph, Ordering, TriangulationParameters, TriangulationResult, Values,
                                _lib, graph as G, noiseModel)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2, BUNDLER = c.S2, c.BUNDLER
NOISY = (4.995, 0.499167, 1.19814)


def _close(expected, actual, tol):
    """assert_equal(Point3, Point3, tol)"""
    d = np.abs(np.asarray(expected, dtype=float) - np.asarray(actual, dtype=float)).max()
    assert d <= tol, d


# ---------------------------------------------------------------- known answers
def test_two_poses():
    """testTriangulation.cpp:63-94"""
    cal = [c.K_SHARED] * 2
    cams, zs = c.scene(S2, cal)
    _close(c.LANDMARK, r.triangulate_point3(cams, S2, zs, 1e-9, False), 1e-7)  # :72
    _close(c.LANDMARK, r.triangulate_point3(cams, S2, zs, 1e-9, True), 1e-7)   # :78
    cams, zs = c.scene(S2, cal, (True, True, False))
    _close(NOISY, r.triangulate_point3(cams, S2, zs, 1e-9, False), 1e-4)       # :87
    _close(NOISY, r.triangulate_point3(cams, S2, zs, 1e-9, True), 1e-4)        # :93


def test_two_poses_bundler():
    """:265-293"""
    cal = [c.BUNDLER_CAL] * 2
    cams, zs = c.scene(BUNDLER, cal)
    _close(c.LANDMARK, r.triangulate_point3(cams, BUNDLER, zs, 1e-9, True), 1e-7)  # :283
    cams, zs = c.scene(BUNDLER, cal, (True, True, False))
    _close((4.995, 0.499167, 1.19847), r.triangulate_point3(cams, BUNDLER, zs, 1e-9, True), 1e-3)  # :292


@pytest.mark.parametrize("cals", [[c.K_SHARED] * 4, [c.K1, c.K2, c.K3, c.K4]], ids=["fourPoses", "fourPoses_distinct_Ks"])
def test_four_poses(cals):
    """:296-342 and :430-490"""
    _close(c.LANDMARK, r.triangulate_point3(*_cz(c.scene(S2, cals)), 1e-9), 1e-2)                               # :301 / :448
    _close(c.LANDMARK, r.triangulate_point3(*_cz(c.scene(S2, cals, (True, True, False))), 1e-9), 1e-2)          # :310 / :457
    three = _cz(c.scene(S2, cals, (True, True, True), n=3))
    _close(c.LANDMARK, r.triangulate_point3(*three, 1e-9), 1e-2)                                                 # :322 / :470
    _close(c.LANDMARK, r.triangulate_point3(*three, 1e-9, True), 1e-2)                                           # :327 / :475
    cams, zs = c.scene(S2, cals, (True, True, True), wrong_way=True)
    assert r.project(cams[3], S2, c.LANDMARK) is None                                                            # :334 / :483
    with pytest.raises(r.Cheirality):                                                                            # :339 / :487
        r.triangulate_point3(cams, S2, zs, 1e-9)


def _cz(scene):
    return scene[0], S2, scene[1]


def test_outliers_and_far_landmarks():
    """:515-569"""
    cals = [c.K1, c.K2, c.K3]
    cams, zs = c.scene(S2, cals)
    st, p, _ = r.triangulate_safe(cams, S2, zs, r.Params(1.0, False, 10))
    assert st == r.VALID
    _close(c.LANDMARK, p, 1e-2)                                                       # :536-537
    assert r.triangulate_safe(cams, S2, zs, r.Params(1.0, False, 4))[0] == r.FAR_POINT  # :544
    cams, zs = c.scene(S2, cals, (False, False, True), n=3, z3_offset=np.array([10.0, -10.0]))
    assert r.triangulate_safe(cams, S2, zs, r.Params(1.0, False, 10, 100))[0] == r.VALID   # :561
    assert r.triangulate_safe(cams, S2, zs, r.Params(1.0, False, 10, 5))[0] == r.OUTLIER   # :568


def test_underconstrained():
    """twoIdenticalPoses :572-584, onePose :587-596"""
    cam = c.cam17(*c.POSE1, c.K_SHARED)
    z = r.project(cam, S2, c.LANDMARK)
    with pytest.raises(r.Underconstrained):
        r.triangulate_point3([cam, cam], S2, [z, z])
    with pytest.raises(r.Underconstrained):
        r.triangulate_point3([c.cam17(np.eye(3), np.zeros(3), c.K_SHARED)], S2, [np.zeros(2)])
    assert r.triangulate_safe([cam, cam], S2, [z, z], r.Params(1e-9))[0] == r.DEGENERATE


def test_calibrate_known_behaviour():
    """Cal3Bundler::calibrate inverts uncalibrate (testCal3Bundler.cpp's calibrate round trip) and gives up after 10 passes"""
    cam = c.cam17(np.eye(3), np.zeros(3), c.BUNDLER_CAL)
    pn = np.array([0.2, -0.15])
    dec = []
    got = r.calibrate_bundler(cam, r.uncalibrate(cam, BUNDLER, pn), dec)
    assert np.abs(got - pn).max() < 1e-7 and 2 <= len(dec) <= 10
    bad = c.cam17(np.eye(3), np.zeros(3), (500, 4.0, 9.0, 0, 0))
    with pytest.raises(r.CalibrateFailed):
        r.calibrate_bundler(bad, np.array([450.0, 380.0]))


# ---------------------------------------------------------------- the device parity inputs
CASES = {case["name"]: case for case in c.gpu_parity_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_decision_margins(name):
    """no branch decision of any point of a device parity batch lies within 1e-3 (relative) of its boundary: the singular values against
    rank_tol, every LM accept / stop test, every calibrate break test, the cheirality signs, both thresholds"""
    _, _, _, dec = c.expected(CASES[name])
    for i, d in enumerate(dec):
        m, which = r.worst_margin(d)
        assert m >= 1e-3, (name, i, m, which)


@pytest.mark.parametrize("name", sorted(CASES))
def test_conditioning(name):
    """a relative perturbation of all inputs by 1e-13 moves the restatement's point by at most 1e-8 relative: the conditioning that makes
    the device's 1e-6 bound attainable"""
    case = CASES[name]
    pts, st, _, _ = c.expected(case)
    rng = np.random.default_rng(1)
    cams = case["cams"] * (1 + 1e-13 * rng.choice([-1.0, 1.0], case["cams"].shape))
    z = case["obs_z"] * (1 + 1e-13 * rng.choice([-1.0, 1.0], case["obs_z"].shape))
    pts2, st2, _ = r.batch(cams, case["model"], case["offsets"], case["obs_cam"], z, case["params"])
    assert np.array_equal(st, st2)
    ok = st == r.VALID
    if ok.any():
        move = np.linalg.norm(pts2[ok] - pts[ok], axis=1) / np.linalg.norm(pts[ok], axis=1)
        assert move.max() <= 1e-8, (name, int(np.argmax(move)), move.max())


def test_special_lanes_of_the_mixed_wave():
    for model in (BUNDLER, S2):
        case = c.mixed_status_batch(model)
        _, st, _, _ = c.expected(case)
        want = case["want_special"]
        assert list(st[40:40 + len(want)]) == want
        assert (st[:40] == r.VALID).all() and (st[40 + len(want):] == r.VALID).all()


def test_refinement_cases_exercise_what_they_claim():
    for model in (BUNDLER, S2):
        _, _, it0, _ = c.expected(c.refine_batch(model, 0.0))
        _, _, it1, _ = c.expected(c.refine_batch(model, 10.0))
        assert len(set(it0.tolist())) >= 2 and it0.min() >= 1            # lanes of one wave with different tryLambda counts
        assert it1.sum() != it0.sum() and it1.max() != it0.max()         # the noise model moves the stopping iteration
        _, st, _, dec = c.expected(c.crossing_batch(model))
        assert (st == r.VALID).all()
        assert all(any(d[0] == "cheirality" and d[1] <= 0 for d in dd) for dd in dec)  # every lane takes the constant-error branch
    _, st, _, dec = c.expected(c.distortion_batch())
    passes = [sum(1 for d in dd if d[0] == "calibrate") for dd in dec]
    assert max(passes) >= 4 * 3 and (st == r.VALID).all()                # calibrate: four passes and more per observation


# ---------------------------------------------------------------- ABI and Python
TRI_SYMBOLS = ("lmgpu_triangulate_batch", "lmgpu_triangulate_landmarks", "lmgpu_num_points3", "lmgpu_get_triangulation_stats")


def test_symbols_exported_and_declared():
    lib = ct.CDLL(_lib.LIB_PATH)
    h = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    assert sorted(n for n in _lib.SYMBOLS if "triangulat" in n or n == "lmgpu_num_points3") == sorted(TRI_SYMBOLS)
    for name in TRI_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, h), name


def test_python_enums_and_defaults_match_header():
    h = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    val = lambda name: int(re.search(r"\b%s = (\d+)" % name, h).group(1))  # noqa: E731
    for i, name in enumerate(("VALID", "DEGENERATE", "BEHIND_CAMERA", "OUTLIER", "FAR_POINT", "CALIBRATE_FAILED")):
        assert val("LMGPU_TRI_" + name) == getattr(_lib, "LMGPU_TRI_" + name) == getattr(TriangulationResult, name) == getattr(r, name) == i
    assert val("LMGPU_NUM_FACTOR_TYPES") == 14 and val("LMGPU_NUM_VAR_TYPES") == 7  # no new factor or variable type
    p = TriangulationParameters()  # triangulation.h:584-595
    assert (p.rankTolerance, p.enableEPI, p.landmarkDistanceThreshold, p.dynamicOutlierRejectionThreshold, p.useLOST, p.noiseModel) == \
        (1.0, False, -1.0, -1.0, False, None)
    cp = p._c()
    assert (cp.rankTolerance, cp.enableEPI, cp.useLOST, cp.landmarkDistanceThreshold, cp.dynamicOutlierRejectionThreshold, cp.noise_inv_sigma) == \
        (1.0, 0, 0, -1.0, -1.0, 0.0)
    assert TriangulationParameters(noiseModel=noiseModel.Isotropic.Sigma(2, 0.1))._c().noise_inv_sigma == 10.0
    assert ct.sizeof(_lib.lmgpu_triangulation_params) == 40 and ct.sizeof(_lib.lmgpu_triangulation_stats) == 48
    res = TriangulationResult(0, [1, 2, 3])
    assert res.valid() and not (res.degenerate() or res.outlier() or res.farPoint() or res.behindCamera()) and list(res.get()) == [1, 2, 3]
    assert TriangulationResult(4).farPoint() and TriangulationResult(3).outlier() and TriangulationResult(2).behindCamera()
    with pytest.raises(RuntimeError):
        TriangulationResult(1).get()


def _batch_rc(model=0, n_cams=2, n_points=1, off=(0, 2), oc=(0, 1), **kw):
    lib = _lib.load()
    cams = np.zeros((max(n_cams, 1), 17))
    off, oc = np.array(off, dtype=np.int32), np.array(oc, dtype=np.int32)
    z, pts, st = np.zeros((max(len(oc), 1), 2)), np.zeros((max(n_points, 1), 3)), np.zeros(max(n_points, 1), dtype=np.int32)
    cp = TriangulationParameters(**kw)._c()
    dp, ip = (lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))), (lambda a: a.ctypes.data_as(ct.POINTER(ct.c_int32)))
    return lib.lmgpu_triangulate_batch(0, model, n_cams, dp(cams), n_points, ip(off), ip(oc), dp(z), ct.byref(cp), dp(pts), ip(st))


def test_batch_refusals_need_no_device():
    assert _batch_rc(useLOST=True) == _lib.LMGPU_INVALID
    assert _batch_rc(oc=(0, 2)) == _lib.LMGPU_INVALID and _batch_rc(oc=(-1, 1)) == _lib.LMGPU_INVALID  # camera index out of range
    assert _batch_rc(n_points=2, off=(0, 2, 1)) == _lib.LMGPU_INVALID                                  # offsets that decrease
    assert _batch_rc(n_points=-1) == _lib.LMGPU_INVALID
    assert _batch_rc(model=2) == _lib.LMGPU_INVALID and _batch_rc(model=-1) == _lib.LMGPU_INVALID       # unknown camera model
    assert _batch_rc(n_points=0, off=(0,), oc=()) == _lib.LMGPU_OK


def _structure_handle(extra):
    """two cameras, one pose, one calibration, three points; SFM factors on P(0), P(1); `extra` adds the rest"""
    g, v = NonlinearFactorGraph(), Values()
    unit = noiseModel.Unit.Create(2)
    for i in range(2):
        v.insert_camera(G.C(i), np.eye(3), [float(i), 0, 0], 500, 0, 0)
    v.insert_pose3(G.X(0), np.eye(3), [0.0, 1, 0])
    v.insert_cal3_s2(G.symbol("k", 0), 500, 500, 0, 0, 0)
    for j in range(3):
        v.insert_point3(G.P(j), [0.0, 0, 5 + j])
    for j in range(2):
        for i in range(2):
            g.add_GeneralSFMFactor([1.0, 2.0], unit, G.C(i), G.P(j))
    extra(g, unit)
    order = Ordering([G.P(0), G.P(1), G.P(2), G.C(0), G.C(1), G.X(0), G.symbol("k", 0)])
    return LevenbergMarquardtOptimizer(g, v, order, device=-1)


def _landmarks_rc(opt, **kw):
    cp = TriangulationParameters(**kw)._c()
    rc = opt.lib.lmgpu_triangulate_landmarks(opt._h, ct.byref(cp), 0, None, None, None)
    return rc, opt.lib.lmgpu_last_error(opt._h).decode()


def test_structure_only_handle():
    K = (500, 500, 0, 0, 0)
    prior = lambda g, unit: (g.add_GenericProjectionFactor([1.0, 2.0], unit, G.X(0), G.P(2), K),  # noqa: E731
                             g.add_PriorFactorCal3_S2(G.symbol("k", 0), K, noiseModel.Unit.Create(5)))
    opt = _structure_handle(prior)  # P(2) has PROJECTION factors only: a legal structure
    assert opt.lib.lmgpu_num_points3(opt._h) == opt.num_points3() == 3
    rc, msg = _landmarks_rc(opt)
    assert rc == _lib.LMGPU_INVALID and "lmgpu_set_values" in msg  # the structure passes; a device = -1 handle has no values
    rc, msg = _landmarks_rc(opt, useLOST=True)
    assert rc == _lib.LMGPU_INVALID and "LOST" in msg
    st = _lib.lmgpu_triangulation_stats()
    assert opt.lib.lmgpu_get_triangulation_stats(opt._h, ct.byref(st)) == _lib.LMGPU_INVALID  # no call has run

    mixed = lambda g, unit: (g.add_GenericProjectionFactor([1.0, 2.0], unit, G.X(0), G.P(1), K),  # noqa: E731
                             g.add_GenericProjectionFactor([1.0, 2.0], unit, G.X(0), G.P(2), K),
                             g.add_PriorFactorCal3_S2(G.symbol("k", 0), K, noiseModel.Unit.Create(5)))
    rc, msg = _landmarks_rc(_structure_handle(mixed))
    assert rc == _lib.LMGPU_INVALID and "both SFM and PROJECTION" in msg and "slot 1" in msg

    bps = lambda g, unit: (g.add_GenericProjectionFactor([1.0, 2.0], unit, G.X(0), G.P(2), K, body_P_sensor=(np.eye(3), np.zeros(3))),  # noqa: E731
                           g.add_PriorFactorCal3_S2(G.symbol("k", 0), K, noiseModel.Unit.Create(5)))
    rc, msg = _landmarks_rc(_structure_handle(bps))
    assert rc == _lib.LMGPU_INVALID and "PROJECTION_BPS / SFM2" in msg and "slot 2" in msg

    sfm2 = lambda g, unit: g.add_GeneralSFMFactor2([1.0, 2.0], unit, G.X(0), G.P(2), G.symbol("k", 0))  # noqa: E731
    rc, msg = _landmarks_rc(_structure_handle(sfm2))
    assert rc == _lib.LMGPU_INVALID and "PROJECTION_BPS / SFM2" in msg and "slot 2" in msg
