"""Batched triangulation on the device (lmgpu_triangulate_batch, lmgpu_triangulate_landmarks; kernels_triangulation.hpp) against the numpy
restatement (tests/triangulation_restatement.py) on identical inputs: statuses equal, points at the project's parity bound of 1e-6
relative (per point), tryLambda counts of the refinement equal.  Every input is one whose branch decisions test_triangulation_reference.py
found clear of their boundaries.  Each test prints the margin it reached."""
import ctypes as ct

import numpy as np
import pytest

import oracle_harness as oh
import triangulation_cases as c
import triangulation_restatement as r
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, LevenbergMarquardtOptimizer, LevenbergMarquardtParams, NonlinearFactorGraph,
                                Ordering, PCGSolverParameters, TriangulationCheiralityException, TriangulationParameters,
                                TriangulationUnderconstrainedException, Values, _lib, graph as G, noiseModel, triangulatePoint3, triangulateSafe,
                                triangulateSafeBatch)
from gtsam_personal_amd.triangulation import CAL3_BUNDLER, CAL3_S2

pytestmark = pytest.mark.gpu
TOL = 1e-6
MODELS = (c.BUNDLER, c.S2)


def tparams(p, **over):
    """the restatement's Params as TriangulationParameters"""
    t = TriangulationParameters(p.rankTolerance, p.enableEPI, p.landmarkDistanceThreshold, p.dynamicOutlierRejectionThreshold,
                                noiseModel=p.noise_inv_sigma if p.noise_inv_sigma > 0 else None)
    for k, v in over.items():
        setattr(t, k, v)
    return t


def run(case):
    return triangulateSafeBatch(case["cams"], case["model"], case["offsets"], case["obs_cam"], case["obs_z"], tparams(case["params"]),
                                return_stats=True)


def check(name, got_pts, got_st, want_pts, want_st, stats=None, want_it=None):
    assert np.array_equal(got_st, want_st), (name, np.flatnonzero(got_st != want_st)[:8], got_st[got_st != want_st][:8], want_st[got_st != want_st][:8])
    ok = want_st == r.VALID
    assert np.isnan(got_pts[~ok]).all()
    worst = 0.0
    if ok.any():
        worst = float((np.linalg.norm(got_pts[ok] - want_pts[ok], axis=1) / np.linalg.norm(want_pts[ok], axis=1)).max())
    line = f"{name}: {len(want_st)} points, statuses {np.bincount(want_st, minlength=6).tolist()}, worst relative point error {worst:.3e}"
    if stats is not None:
        assert stats.n_points == len(want_st) and stats.n_status == np.bincount(want_st, minlength=6).tolist()
        if want_it is not None:
            line += f", tryLambda calls max {stats.max_iterations} sum {stats.sum_iterations}, device {stats.device_ms:.3f} ms"
            assert (stats.max_iterations, stats.sum_iterations) == (int(want_it.max(initial=0)), int(want_it.sum())), (name, stats.max_iterations,
                                                                                                                         stats.sum_iterations)
    print(line)
    assert worst <= TOL, (name, worst)


def compare(case):
    pts, st, stats = run(case)
    want_pts, want_st, want_it, _ = c.expected(case)
    check(case["name"], pts, st, want_pts, want_st, stats, want_it)
    return pts, st, stats


# ---------------------------------------------------------------- lmgpu_triangulate_batch
@pytest.mark.parametrize("model", MODELS)
def test_known_scenes(model):
    """the scenes of testTriangulation.cpp, both camera models: twoPoses, fourPoses with the camera facing the wrong way, distinct Ks,
    outliersAndFarLandmarks with its four parameter sets, twoIdenticalPoses, onePose"""
    batches = c.known_scene_batches(model)
    for case in batches:
        compare(case)
    st = [c.expected(b)[1][0] for b in batches[2:]]
    assert st == [r.VALID, r.FAR_POINT, r.VALID, r.OUTLIER]


def test_python_interface_on_the_known_scenes():
    cams, zs = c.scene(c.S2, [c.K_SHARED] * 4)
    p = triangulatePoint3(cams, zs, rank_tol=1e-9)
    assert np.abs(p - c.LANDMARK).max() <= 1e-7  # testTriangulation.cpp:72
    cams, zs = c.scene(c.BUNDLER, [c.BUNDLER_CAL] * 4, (True, True, False))
    p = triangulatePoint3(cams, zs, rank_tol=1e-9, optimize=True, camera_model=CAL3_BUNDLER)
    assert np.abs(p - np.array([4.995, 0.499167, 1.19847])).max() <= 1e-3  # :292
    cams, zs = c.scene(c.S2, [c.K_SHARED] * 4, (True, True, True), wrong_way=True)
    with pytest.raises(TriangulationCheiralityException):  # :339
        triangulatePoint3(cams, zs, camera_model=CAL3_S2)
    assert triangulateSafe(cams, zs, TriangulationParameters(1e-9)).behindCamera()
    with pytest.raises(TriangulationUnderconstrainedException):  # :594
        triangulatePoint3([c.cam17(np.eye(3), np.zeros(3), c.K_SHARED)], [np.zeros(2)])


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", c.COUNTS)
def test_landmark_counts_at_wave_and_block_edges(model, n):
    full = c.counts_batch(model)
    want_pts, want_st, _, _ = c.expected(full)
    pts, st, stats = run(c.prefix(full, n))
    assert len(st) == n
    check(f"{full['name']} first {n}", pts, st, want_pts[:n], want_st[:n], stats)


def test_zero_points():
    pts, st, stats = triangulateSafeBatch(np.zeros((0, 17)), CAL3_S2, [0], [], np.zeros((0, 2)), return_stats=True)
    assert pts.shape == (0, 3) and st.shape == (0,) and stats.n_points == 0 and sum(stats.n_status) == 0


@pytest.mark.parametrize("model", MODELS)
def test_degrees_0_1_2_3_17_in_one_batch(model):
    _, st, _ = compare(c.degrees_batch(model))
    assert list(st) == [1, 1, 0, 0, 0, 0, 1, 0, 0, 1]


@pytest.mark.parametrize("model", MODELS)
def test_degree_70_among_degree_2_lands_at_its_own_index(model):
    """the degree sort moves landmark 5 to the end of the launch order; every result must come back at its original index"""
    case = c.degree70_batch(model)
    pts, st, _ = compare(case)
    want = c.expected(case)[0]
    assert st[5] == r.VALID and np.linalg.norm(pts[5] - want[5]) <= TOL * np.linalg.norm(want[5])
    assert np.linalg.norm(pts[5] - case["truth"][5]) < 0.05  # 70 observations: close to the generating point


@pytest.mark.parametrize("model", MODELS)
def test_statuses_mixed_inside_one_wave(model):
    case = c.mixed_status_batch(model)
    _, st, _ = compare(case)
    want = case["want_special"]
    assert list(st[40:40 + len(want)]) == want  # behind + far -> BEHIND_CAMERA, far + outlier -> FAR_POINT, Cal3Bundler: status 5
    assert set(want) >= {1, 2, 3, 4} and (st[:40] == 0).all() and (st[40 + len(want):] == 0).all()


@pytest.mark.parametrize("model", MODELS)
def test_refinement_iteration_counts_differ_by_lane_and_noise_model(model):
    _, _, s0 = compare(c.refine_batch(model, 0.0))
    _, _, s1 = compare(c.refine_batch(model, 10.0))
    assert (s0.max_iterations, s0.sum_iterations) != (s1.max_iterations, s1.sum_iterations)


@pytest.mark.parametrize("model", MODELS)
def test_refinement_crossing_behind_a_camera(model):
    compare(c.crossing_batch(model))


def test_bundler_strong_distortion():
    compare(c.distortion_batch())


def test_two_consecutive_calls_are_bitwise_equal():
    case = c.refine_batch(c.BUNDLER, 0.0)
    a, b = run(case), run(case)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- lmgpu_triangulate_landmarks
def _optimizer(which, pcg=False):
    graph, values, _, ordering = c.GRAPHS[which]()
    params = LevenbergMarquardtParams()
    if pcg:
        params.linearSolverType = "ITERATIVE"
        params.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    return LevenbergMarquardtOptimizer(graph, values, ordering, params, device=0), graph, ordering


def _packed(opt):
    out = np.empty(opt._nstore)
    opt._check(opt.lib.lmgpu_get_values(opt._h, out.ctypes.data_as(ct.POINTER(ct.c_double))))
    return out


def _point_offsets(opt):
    return [int(opt._voff[i]) for i, t in enumerate(opt._types) if t == G.POINT3]


def _handle_against_batch_and_restatement(which, epi, dist_thr, pcg=False):
    case, keys = c.graph_case(which, epi, dist_thr)
    opt, graph, ordering = _optimizer(which, pcg)
    if pcg:
        assert opt.num_fronts() == 0
    tp = tparams(case["params"])
    before = _packed(opt)
    res = opt.triangulate_landmarks(tp, write=False)
    assert res.keys == keys and opt.num_points3() == len(keys)
    assert np.array_equal(_packed(opt), before)  # write_values = 0: bitwise unchanged
    want_pts, want_st, want_it, _ = c.expected(case)
    check(case["name"] + (" pcg" if pcg else ""), res.points, res.status, want_pts, want_st, res.stats, want_it)
    assert res.n_valid == int((want_st == 0).sum())
    if case["model"] == c.BUNDLER:  # the same cameras and measurements through the stand-alone form: bit for bit
        pts, st, _ = run(case)
        assert np.array_equal(pts, res.points, equal_nan=True) and np.array_equal(st, res.status)
    again = opt.triangulate_landmarks(tp, write=False)
    assert np.array_equal(again.points, res.points, equal_nan=True) and np.array_equal(again.status, res.status)
    # write_values = 1 changes exactly the VALID points
    res2 = opt.triangulate_landmarks(tp, write=True)
    assert np.array_equal(res2.points, res.points, equal_nan=True)
    after, want_after = _packed(opt), before.copy()
    for i, off in enumerate(_point_offsets(opt)):
        if res.status[i] == 0:
            want_after[off:off + 3] = res.points[i]
    assert np.array_equal(after, want_after)
    err = ct.c_double()
    opt._check(opt.lib.lmgpu_error(opt._h, ct.byref(err)))
    want_err = oh.OracleProblem(graph, opt.values(), ordering).error()
    print(f"{case['name']}: error after the write {err.value:.9g}, oracle {want_err:.9g}")
    assert abs(err.value - want_err) <= 1e-9 * max(1.0, abs(want_err))
    opt.close()


@pytest.mark.parametrize("which,epi,dist_thr", [("bal_small", False, -1.0), ("bal_small", True, -1.0), ("bal_small", False, c.FAR_BAL),
                                                ("dubrovnik", False, -1.0), ("dubrovnik", True, -1.0)])
def test_handle_form_sfm(which, epi, dist_thr):
    _handle_against_batch_and_restatement(which, epi, dist_thr)


@pytest.mark.parametrize("epi,dist_thr", [(False, -1.0), (True, -1.0), (True, c.FAR_PROJECTION)])
def test_handle_form_projection_factors(epi, dist_thr):
    _handle_against_batch_and_restatement("projection", epi, dist_thr)


def test_handle_form_on_a_pcg_finalized_handle():
    _handle_against_batch_and_restatement("bal_small", True, -1.0, pcg=True)


@pytest.mark.parametrize("epi", [False, True])
def test_medium_case(epi):
    case, _ = c.graph_case("bal_medium", epi)
    opt, _, _ = _optimizer("bal_medium")
    res = opt.triangulate_landmarks(tparams(case["params"]), write=False)
    want_pts, want_st, want_it, _ = c.expected(case)
    check(case["name"], res.points, res.status, want_pts, want_st, res.stats, want_it)
    opt.close()


class _NoValues(LevenbergMarquardtOptimizer):
    def set_values(self, values):
        pass


def test_refusals_with_their_messages():
    opt, graph, ordering = _optimizer("bal_small")
    cp = TriangulationParameters()._c()

    def refused(o):
        rc = o.lib.lmgpu_triangulate_landmarks(o._h, ct.byref(cp), 0, None, None, None)
        return rc, o.lib.lmgpu_last_error(o._h).decode()

    opt._check(opt.lib.lmgpu_gnc_enable(opt._h, 1, 0))
    rc, msg = refused(opt)
    assert rc == _lib.LMGPU_INVALID and "GNC is enabled" in msg
    opt._check(opt.lib.lmgpu_gnc_enable(opt._h, 0, 0))
    assert refused(opt)[0] == _lib.LMGPU_OK
    opt.close()
    # a finalized device handle that has never been given values
    nv = _NoValues.__new__(_NoValues)
    with pytest.raises(_lib.LmgpuError):
        nv.__init__(graph, c.GRAPHS["bal_small"]()[1], ordering, device=0)  # lmgpu_lm_init refuses: no values
    rc, msg = refused(nv)
    assert rc == _lib.LMGPU_INVALID and "lmgpu_set_values" in msg
    nv.close()
    # a point with both SFM and PROJECTION factors
    g, v = NonlinearFactorGraph(), Values()
    unit = noiseModel.Unit.Create(2)
    v.insert_camera(G.C(0), np.eye(3), [0.0, 0, 0], 500, 0, 0)
    v.insert_pose3(G.X(0), np.eye(3), [1.0, 0, 0])
    v.insert_point3(G.P(0), [0.0, 0, 5])
    g.add_GeneralSFMFactor([0.0, 0.0], unit, G.C(0), G.P(0))
    g.add_GenericProjectionFactor([-100.0, 0.0], unit, G.X(0), G.P(0), (500, 500, 0, 0, 0))
    g.add_PriorFactorPose3(G.X(0), np.eye(3), [1.0, 0, 0], noiseModel.Unit.Create(6))
    mixed = LevenbergMarquardtOptimizer(g, v, Ordering([G.P(0), G.C(0), G.X(0)]), device=0)
    rc, msg = refused(mixed)
    assert rc == _lib.LMGPU_INVALID and "both SFM and PROJECTION" in msg
    mixed.close()
