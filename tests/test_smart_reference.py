"""CPU tests of the smart projection factors: the numpy restatement (tests/smart_restatement.py) against the known answers of
gtsam/slam/tests/testSmartProjectionPoseFactor.cpp at that file's tolerances, the margins of every decision the GPU tests' inputs take,
the dense-algebra identity the integration rests on, and the C ABI's refusals on a structure-only handle.  No GPU."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import smart_cases as sc
import smart_restatement as sr
import triangulation_restatement as tr
from gtsam_personal_amd import _lib
from gtsam_personal_amd import smart as S
from gtsam_personal_amd import (GaussNewtonOptimizer, LevenbergMarquardtOptimizer, NonlinearFactorGraph, Ordering, SmartProjectionParams,
                                SmartProjectionPoseFactor, Values, noiseModel)
from gtsam_personal_amd import graph as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_params_defaults_and_setters():
    """testSmartProjectionPoseFactor.cpp:85-93 and SmartFactorParams.h:60-66"""
    p = SmartProjectionParams()
    assert abs(p.getRetriangulationThreshold() - 1e-5) <= 1e-7
    p.setRetriangulationThreshold(1e-3)
    assert abs(p.getRetriangulationThreshold() - 1e-3) <= 1e-7
    q = SmartProjectionParams()
    assert (q.getLinearizationMode(), q.getDegeneracyMode()) == (S.HESSIAN, S.IGNORE_DEGENERACY)
    assert not q.getThrowCheirality() and not q.getVerboseCheirality()
    t = q.getTriangulationParameters()
    assert (t.rankTolerance, t.enableEPI, t.landmarkDistanceThreshold, t.dynamicOutlierRejectionThreshold) == (1.0, False, -1.0, -1.0)
    q.setRankTolerance(10)
    q.setEnableEPI(True)
    q.setLandmarkDistanceThreshold(2.0)
    q.setDynamicOutlierRejectionThreshold(3.0)
    assert (t.rankTolerance, t.enableEPI, t.landmarkDistanceThreshold, t.dynamicOutlierRejectionThreshold) == (10, True, 2.0, 3.0)
    with pytest.raises(ValueError, match="IGNORE_DEGENERACY"):
        q._c()
    q.setDegeneracyMode(S.ZERO_ON_DEGENERACY)
    c = q._c()
    assert (c.linearizationMode, c.degeneracyMode, c.triangulation.enableEPI) == (0, 1, 1)
    q.setLinearizationMode(S.JACOBIAN_SVD)
    with pytest.raises(ValueError, match="JACOBIAN_SVD"):
        q._c()


def test_noiseless():
    """:108-163: zero error at the ground truth"""
    poses = [sc.LEVEL_POSE, sc.POSE_RIGHT]
    f = sc.smart([sc.X1, sc.X2], poses, sc.K_FOV, sc.LANDMARK1)
    g, v = sc.restatement(dict(values={sc.X1: poses[0], sc.X2: poses[1]}, order=[sc.X1, sc.X2], factors=[f]))
    assert abs(g.error(v)) <= 1e-7
    assert g.smart()[0].status == tr.VALID
    assert np.allclose(g.smart()[0].point, sc.LANDMARK1, atol=1e-7)


def test_factors_known_answers():
    """:336-414"""
    g, v = sc.restatement(sc.factors_scene())
    f = g.smart()[0]
    A = f.hessian(v)
    assert f.status == tr.VALID and np.allclose(f.point, [0, 0, 10], atol=1e-9)
    assert np.allclose(A, sc.factors_expected_information(), atol=1e-6)
    H, gg, c = g.linearize(v)
    assert abs(sr.lin_error(H, gg, c, np.zeros(12))) <= 1e-6
    assert abs(sr.lin_error(H, gg, c, np.ones(12)) - 2500) <= 1e-6


def test_three_poses():
    """:275-333"""
    scene = sc.three_poses_scene()
    assert np.allclose(scene["values"][sc.X3], sc.PRINTED_X3, atol=1e-9)
    g0, v0 = sc.restatement(sc.three_poses_scene(perturbed=False))
    assert abs(g0.error(v0)) <= 1e-9
    g, v = sc.restatement(scene)
    lm = sr.LM(g, v)
    lm.optimize()
    assert np.allclose(lm.values[sc.X3], sc.POSE_ABOVE, atol=1e-6)


def test_landmark_distance_and_outlier_rejection_turn_factors_off():
    """:610-666, :669-732: every factor is off (the result is not valid, or it is valid with zero gradient) and x3 does not move"""
    far = sc.zero_on_degeneracy(landmarkDistanceThreshold=2.0)
    scene = sc.three_poses_scene(K5=sc.K_FOV, params=far)
    g, v = sc.restatement(scene)
    lm = sr.LM(g, v)
    lm.optimize()
    assert [f.status for f in g.smart()] == [tr.FAR_POINT] * 3
    assert np.allclose(lm.values[sc.X3], scene["values"][sc.X3], atol=1e-9)

    out = sc.zero_on_degeneracy(landmarkDistanceThreshold=1e10, dynamicOutlierRejectionThreshold=1.0)
    scene = sc.three_poses_scene(perturbed=False, K5=sc.K_FOV, params=out)
    poses, keys = [sc.LEVEL_POSE, sc.POSE_RIGHT, sc.POSE_ABOVE], [sc.X1, sc.X2, sc.X3]
    scene["factors"].insert(3, sc.smart(keys, poses, sc.K_FOV, [5, -0.5, 1.0], out, noise=[np.array([10.0, 10.0]), np.zeros(2), np.zeros(2)]))
    g, v = sc.restatement(scene)
    lm = sr.LM(g, v)
    lm.optimize()
    assert [f.status for f in g.smart()] == [tr.VALID, tr.VALID, tr.VALID, tr.OUTLIER]
    assert np.allclose(lm.values[sc.X3], sc.POSE_ABOVE, atol=1e-9)


def test_check_hessian():
    """:833-912"""
    d = sr.pose(sr.ypr(-0.05, 0.0, -0.05), [0, 0, 0])  # Rot3::RzRyRx(-0.05, 0, -0.05)
    pose2 = sr.compose(sc.LEVEL_POSE, d)
    pose3 = sr.compose(pose2, d)
    poses, keys = [sc.LEVEL_POSE, pose2, pose3], [sc.X1, sc.X2, sc.X3]
    prm = sc.zero_on_degeneracy(rankTolerance=10)
    fs = [sc.smart(keys, poses, sc.K_FOV, lm, prm) for lm in (sc.LANDMARK1, sc.LANDMARK2, sc.LANDMARK3)]
    x3 = sr.compose(pose3, sc.NOISE_POSE)
    printed = sr.pose([[0.00563056869, -0.130848107, 0.991386438], [-0.991390265, -0.130426831, -0.0115837907],
                       [0.130819108, -0.98278564, -0.130455917]], [0.0897734171, -0.110201006, 0.901022872])
    assert np.allclose(x3, printed, atol=1e-9)
    g, v = sc.restatement(dict(values={sc.X1: poses[0], sc.X2: pose2, sc.X3: x3}, order=keys, factors=fs))
    H, gg, _ = g.linearize(v)
    cum = sum(f.hessian(v) for f in g.smart())
    assert np.allclose(H, cum[:18, :18], atol=1e-6) and np.allclose(gg, cum[:18, 18], atol=1e-6)
    # (the three cameras of that test share one centre: no factor's result is valid there and under ZERO_ON_DEGENERACY the sums are zero; the same
    # identity on cameras that are apart)
    assert all(f.status != tr.VALID for f in g.smart())
    g, v = sc.restatement(sc.three_poses_scene())
    H, gg, _ = g.linearize(v)
    cum = sum(f.hessian(v) for f in g.factors[:3])
    pri = np.zeros((19, 19))
    for f in g.factors[3:]:
        idx = np.r_[np.arange(g.col[f.keys[0]], g.col[f.keys[0]] + 6), 18]
        pri[np.ix_(idx, idx)] += f.hessian(v)
    assert [f.status for f in g.smart()] == [tr.VALID] * 3 and np.linalg.norm(cum) > 1.0
    assert np.allclose(H, (cum + pri)[:18, :18], atol=1e-6) and np.allclose(gg, (cum + pri)[:18, 18], atol=1e-6)


def test_cache_rule():
    """SmartProjectionFactor.h:127-184: no re-triangulation within the threshold, one beyond it, m < 2 leaves the cache alone"""
    scene = sc.three_poses_scene(params=sc.zero_on_degeneracy(retriangulationThreshold=1e-3))
    g, v = sc.restatement(scene)
    f = g.smart()[0]
    f.error(v)
    assert f.retriangulated
    p0 = f.point.copy()
    v[sc.X3] = v[sc.X3].copy()
    v[sc.X3][9] += 1e-4
    f.error(v)
    assert not f.retriangulated and np.array_equal(f.point, p0)
    v[sc.X3][9] += 1e-2
    f.error(v)
    assert f.retriangulated and not np.array_equal(f.point, p0)
    one = sr.SmartFactor([sc.X1], [np.zeros(2)], sc.K2, 0.1)
    one.error(v)
    assert one.status == tr.DEGENERATE and one.cache is None and one.error(v) == 0.0


def gpu_scenes():
    """every scene of tests/test_gpu_smart.py that is compared with the restatement"""
    import test_gpu_smart as t
    return t.parity_scenes()


def test_gpu_inputs_are_clear_of_every_boundary():
    """status decisions through the `dec` margins of triangulation_restatement (>= 1e-3 of their scale); cache tests a factor of 10 either side"""
    worst = np.inf
    for name, scene, steps in gpu_scenes():
        g, v = sc.restatement(scene)
        for f in g.smart():
            f.dec = []
        lm = steps(g, v)
        for d in (lm.ctl if lm is not None else []):  # the decisions of the Levenberg-Marquardt loop itself
            assert abs(d[1] - d[2]) >= 1e-3 * d[3], (name, d)
        for f in g.smart():
            for d in f.dec:
                if d[0] == "cache_call":
                    # threshold 0 (smart_cases.every_change): "any entry changed"; the largest change is nothing or far above the last bit
                    assert d[2] > 0 or d[1] == 0 or d[1] >= 1e-12, (name, d)
                elif d[0] == "cache":
                    if d[2] > 0:
                        assert d[1] <= d[2] / 10 * (1 + 1e-9) or d[1] >= d[2] * 10 * (1 - 1e-9), (name, d)  # (1e-9: the rounding of x + 1e-4 - x)
                else:
                    m = abs(d[1] - d[2]) / d[3] if d[3] > 0 else np.inf
                    worst = min(worst, m)
                    assert m >= 1e-3, (name, d)
    print(f"smallest status margin over the GPU inputs: {worst:.3g}")


def test_five_status_scene():
    g, v = sc.restatement(sc.five_status_scene())
    for f in g.smart():
        f.dec = []
    e = g.error(v)
    assert tuple(f.status for f in g.smart()) == sc.FIVE_STATUS
    margins = [tr.worst_margin([d for d in f.dec if not d[0].startswith("cache")])[0] for f in g.smart()]
    print("five-status margins:", margins)
    assert min(margins) >= 0.1
    valid_alone = g.smart()[0].error(v)
    priors = sum(f.error(v) for f in g.factors if isinstance(f, sr.Prior))
    assert abs(e - (valid_alone + priors)) <= 1e-12 * max(1.0, e)
    for f in g.smart()[1:]:
        assert not f.hessian(v).any()
    lm = sr.LM(g, v)
    lm.iterate()
    assert lm.trace[0][5] is not None  # the dense system is solvable: nothing indeterminate


def test_gn_step_equals_pose_part_of_explicit_landmark_step():
    """the identity the hidden-point integration rests on: eliminating each triangulated point from the Jacobian system of the explicit graph
    gives the smart graph's system.  Dense algebra, 1e-9 relative."""
    scene = sc.ring_scene([2, 3, 5, 9], seed=11)
    g, v = sc.restatement(scene)
    step, _, _ = sr.gn_step(g, v)
    smart = g.smart()
    n = 6 * len(g.order)
    npt = len(smart)
    rows = []
    for i, f in enumerate(smart):
        assert f.status == tr.VALID
        F, E, b = f._FEb(v)
        for j, k in enumerate(f.keys):
            A = np.zeros((2, n + 3 * npt + 1))
            A[:, g.col[k]:g.col[k] + 6] = F[j]
            A[:, n + 3 * i:n + 3 * i + 3] = E[2 * j:2 * j + 2]
            A[:, -1] = b[2 * j:2 * j + 2]
            rows.append(A)
    for f in g.factors:
        if isinstance(f, sr.Prior):
            A = np.zeros((6, n + 3 * npt + 1))
            A[:, g.col[f.keys[0]]:g.col[f.keys[0]] + 6] = np.diag(f.inv)
            A[:, -1] = f._b(v)
            rows.append(A)
    A = np.vstack(rows)
    x = np.linalg.lstsq(A[:, :-1], A[:, -1], rcond=None)[0]
    assert np.linalg.norm(x[:n] - step) <= 1e-9 * np.linalg.norm(step)


def test_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    lib = _lib.load()
    for name in ("lmgpu_add_smart_factors", "lmgpu_num_smart_factors", "lmgpu_smart_get_points", "lmgpu_smart_get_hessian", "lmgpu_smart_reset",
                 "lmgpu_get_smart_stats"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert "LMGPU_NUM_FACTOR_TYPES = 14" in header


# ---------------------------------------------------------------- refusals, on a handle without a device
def _handle(types=(G.POSE3, G.POSE3, G.POINT3), world_size=1):
    lib = _lib.load()
    h = ct.c_void_p()
    cfg = _lib.lmgpu_config(-1, 0, world_size, 0)
    assert lib.lmgpu_create(ct.byref(cfg), ct.byref(h)) == 0
    keys = np.arange(1, len(types) + 1, dtype=np.uint64)
    t = np.array(types, dtype=np.int32)
    assert lib.lmgpu_set_variables(h, len(t), keys.ctypes.data_as(ct.POINTER(ct.c_uint64)), t.ctypes.data_as(_lib._I)) == 0
    return lib, h


def _add(lib, h, offsets=(0, 2), slots=(0, 1), inv_sigma=(10.0,), lin=0, deg=1, lost=0, gi=(0,)):
    p = _lib.lmgpu_smart_params(lin, deg, 1e-5, _lib.lmgpu_triangulation_params(1.0, 0, lost, -1.0, -1.0, 0.0))
    n = len(offsets) - 1
    gi_, off, sl = np.array(gi, dtype=np.int32), np.array(offsets, dtype=np.int32), np.array(slots, dtype=np.int32)
    z, K5, isg = np.zeros(2 * max(1, len(slots))), np.tile(sc.K2, n), np.array(inv_sigma, dtype=np.float64)
    rc = lib.lmgpu_add_smart_factors(h, n, gi_.ctypes.data_as(_lib._I), off.ctypes.data_as(_lib._I), sl.ctypes.data_as(_lib._I),
                                     z.ctypes.data_as(_lib._D), K5.ctypes.data_as(_lib._D), isg.ctypes.data_as(_lib._D), ct.byref(p))
    return rc, (lib.lmgpu_last_error(h) or b"").decode()


@pytest.mark.parametrize("kw, word", [
    (dict(lin=1), "linearizationMode"), (dict(lin=3), "linearizationMode"), (dict(deg=0), "degeneracyMode"), (dict(deg=2), "degeneracyMode"),
    (dict(lost=1), "useLOST"), (dict(slots=(0, 2)), "POSE3"), (dict(slots=(0, 0)), "twice"), (dict(offsets=(0, 0), slots=()), "without observations"),
    (dict(offsets=(0, 2, 1), slots=(0, 1), inv_sigma=(1.0, 1.0), gi=(0, 1)), "decreasing"), (dict(inv_sigma=(0.0,)), "inv_sigma"),
    (dict(inv_sigma=(-1.0,)), "inv_sigma"), (dict(slots=(0, 7)), "unknown slot")])
def test_add_smart_factors_refusals(kw, word):
    lib, h = _handle()
    rc, msg = _add(lib, h, **kw)
    assert rc == _lib.LMGPU_INVALID and word in msg, (rc, msg)
    assert lib.lmgpu_num_smart_factors(h) == -1
    # nothing was added: the handle finalizes as one without smart factors
    gi, sl, m = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), sc.LEVEL_POSE.copy()
    assert lib.lmgpu_add_factor_bucket(h, 4, 1, gi.ctypes.data_as(_lib._I), sl.ctypes.data_as(_lib._I), m.ctypes.data_as(_lib._D), 0, None) == 0
    sl2, m2 = np.array([1, 2], dtype=np.int32), np.concatenate([np.zeros(2), sc.K2])
    gi2 = np.ones(1, dtype=np.int32)
    assert lib.lmgpu_add_factor_bucket(h, 7, 1, gi2.ctypes.data_as(_lib._I), sl2.ctypes.data_as(_lib._I), m2.ctypes.data_as(_lib._D), 0, None) == 0
    assert lib.lmgpu_finalize_structure(h) == _lib.LMGPU_OK
    assert lib.lmgpu_num_smart_factors(h) == 0 and lib.lmgpu_total_dim(h) == 15
    lib.lmgpu_destroy(h)


def test_world_size_refused():
    lib, h = _handle(world_size=2)
    rc, msg = _add(lib, h)
    assert rc == _lib.LMGPU_INVALID and "world_size" in msg
    lib.lmgpu_destroy(h)


def test_public_factor_types_stay_at_14():
    lib, h = _handle()
    gi, sl, m, nz = np.zeros(1, dtype=np.int32), np.array([0, 2], dtype=np.int32), np.zeros(7), np.ones(2)
    rc = lib.lmgpu_add_factor_bucket(h, 14, 1, gi.ctypes.data_as(_lib._I), sl.ctypes.data_as(_lib._I), m.ctypes.data_as(_lib._D), 2,
                                     nz.ctypes.data_as(_lib._D))
    assert rc == _lib.LMGPU_INVALID
    lib.lmgpu_destroy(h)


def _structure_only(scene):
    g, v, order, objs = sc.package(scene)
    return LevenbergMarquardtOptimizer(g, v, order, device=-1), objs


def test_structure_and_refusals_on_a_smart_handle():
    scene = sc.five_status_scene()
    opt, objs = _structure_only(scene)
    lib, h = opt.lib, opt._h
    assert opt.num_smart_factors() == 6
    # five hidden points (the one-observation factor has none) are no part of the packed vectors
    assert lib.lmgpu_total_dim(h) == 6 * 5 and lib.lmgpu_total_store(h) == 12 * 5
    # the front taps show them: one leaf front per hidden point
    leaves = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert sum(1 for f in leaves if f["nf"] == 3) == 5

    def refused(rc):
        msg = (lib.lmgpu_last_error(h) or b"").decode()
        return rc == _lib.LMGPU_INVALID and "smart projection factors" in msg

    pcg = _lib.lmgpu_pcg_params(1, 1, 500, 501, 1e-3, 1e-3)
    assert refused(lib.lmgpu_set_linear_solver(h, _lib.LMGPU_SOLVER_PCG, ct.byref(pcg)))
    assert refused(lib.lmgpu_gnc_enable(h, 1, 0))
    r, c = ct.c_int32(), ct.c_int32()
    assert refused(lib.lmgpu_get_jacobian(h, 0, None, ct.byref(r), ct.byref(c)))
    n = ct.c_int32()
    assert refused(lib.lmgpu_get_jacobians(h, ct.byref(n), None, None, None, None, None))
    tp = _lib.lmgpu_triangulation_params(1.0, 0, 0, -1.0, -1.0, 0.0)
    assert refused(lib.lmgpu_triangulate_landmarks(h, ct.byref(tp), 0, None, None, None))
    g = np.zeros(30)
    assert refused(lib.lmgpu_gradient(h, g.ctypes.data_as(_lib._D)))
    st = _lib.lmgpu_lm_state()
    assert lib.lmgpu_dl_iterate(h, ct.byref(st)) == _lib.LMGPU_INVALID
    cov = np.zeros(36)
    assert lib.lmgpu_marginal_covariance(h, 0, cov.ctypes.data_as(_lib._D)) == _lib.LMGPU_INVALID
    assert lib.lmgpu_hessian_diagonal(h, g.ctypes.data_as(_lib._D)) == _lib.LMGPU_INVALID
    m = ct.c_int32()
    assert lib.lmgpu_smart_get_hessian(h, 3, ct.byref(m), None) == _lib.LMGPU_OK and m.value == 1
    assert lib.lmgpu_smart_get_hessian(h, 6, ct.byref(m), None) == _lib.LMGPU_INVALID  # a prior's graph index
    opt.close()


def test_pcg_before_finalize_is_refused():
    g, v, order, _ = sc.package(sc.factors_scene())
    from gtsam_personal_amd import BlockJacobiPreconditionerParameters, LevenbergMarquardtParams, PCGSolverParameters
    p = LevenbergMarquardtParams()
    p.linearSolverType, p.iterativeParams = "ITERATIVE", PCGSolverParameters(BlockJacobiPreconditionerParameters())
    with pytest.raises(_lib.LmgpuError, match="smart projection factors"):
        LevenbergMarquardtOptimizer(g, v, order, p, device=-1)


def test_python_surface_without_a_device():
    prm = SmartProjectionParams()
    f = SmartProjectionPoseFactor(noiseModel.Isotropic.Sigma(2, 0.1), sc.K2, prm)
    f.add(np.array([1.0, 2.0]), sc.X1)
    f.add([np.array([3.0, 4.0]), np.array([5.0, 6.0])], [sc.X2, sc.X3])
    assert f.keys() == [sc.X1, sc.X2, sc.X3] and f.size() == 3 and f.isDegenerate() and not f.isValid()
    with pytest.raises(ValueError):
        f.add(np.zeros(2), sc.X1)
    with pytest.raises(ValueError):
        SmartProjectionPoseFactor(noiseModel.Diagonal.Sigmas([0.1, 0.2]), sc.K2, prm)
    g = NonlinearFactorGraph()
    g.add_PriorFactorPose3(sc.X1, np.eye(3), np.zeros(3), noiseModel.Isotropic.Sigma(6, 0.1))
    g.add_SmartProjectionPoseFactor(f)
    assert g.size() == 2 and g.smart_factors()[0][0] == 1
    assert g.keys() == [sc.X1, sc.X2, sc.X3] and Ordering.Natural(g) == [sc.X1, sc.X2, sc.X3]
    assert g.factor_keys_in_graph_order()[1] == (sc.X1, sc.X2, sc.X3)
    v = Values()
    for k in (sc.X1, sc.X2, sc.X3):
        v.insert(k, G.POSE3, sc.LEVEL_POSE)
    for cls in (LevenbergMarquardtOptimizer, GaussNewtonOptimizer):
        with pytest.raises(ValueError, match="IGNORE_DEGENERACY"):  # the reference's default mode is not bound
            cls(g, v, Ordering.Natural(g), device=-1)
    prm.setDegeneracyMode(S.ZERO_ON_DEGENERACY)
    opt = LevenbergMarquardtOptimizer(g, v, Ordering.Natural(g), device=-1)
    assert opt.num_smart_factors() == 1
    opt.close()
    # a graph without smart factors: 0 after finalize
    g2 = NonlinearFactorGraph()
    g2.add_PriorFactorPose3(sc.X1, np.eye(3), np.zeros(3), noiseModel.Isotropic.Sigma(6, 0.1))
    v2 = Values()
    v2.insert(sc.X1, G.POSE3, sc.LEVEL_POSE)
    opt = LevenbergMarquardtOptimizer(g2, v2, Ordering.Natural(g2), device=-1)
    assert opt.num_smart_factors() == 0
    opt.close()
