"""InitializePose3 on the device against the numpy restatement (tests/init_pose3_restatement.py) on identical inputs, at the project's
parity bound of 1e-6 relative: rotations compared as matrices, poses as packed values."""
import ctypes as ct
import os

import numpy as np
import pytest

import init_pose3_cases as c
import init_pose3_restatement as r
import oracle_harness as oh
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, GaussNewtonOptimizer, GaussNewtonParams, InitializePose3,
                                LevenbergMarquardtParams, NonlinearFactorGraph, Ordering, PCGSolverParameters, Values, _lib, noiseModel)
from gtsam_personal_amd.datasets import chain_initial_pose3, load3D
from gtsam_personal_amd.init_pose3 import _Session

pytestmark = pytest.mark.gpu
GOLD = c.GOLD
TOL = 1e-6


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.linalg.norm(a - b) / max(1e-300, np.linalg.norm(b)))


def stack(d, keys=None):
    keys = sorted(d) if keys is None else keys
    return np.stack([np.asarray(d[k]).reshape(-1) for k in keys])


def stack_values(v):
    return np.stack([v.at(k) for k in v.keys()])


def _file_graph(name):
    return c.with_prior(load3D(os.path.join(GOLD, name))[0])


def _inputs():
    return {"graph": c.graph, "graph2": c.graph2, "pose3example": lambda: _file_graph("pose3example.txt"), "grid": lambda: c.grid()[0],
            "sphere2500_head": lambda: _file_graph("sphere2500_head.txt")}


@pytest.mark.parametrize("name", ["graph", "graph2", "pose3example", "grid", "sphere2500_head"])
def test_chordal_and_poses_match_restatement(name):
    g = _inputs()[name]()
    edges = r.extract(g)
    want_R = r.orientations_chordal(edges)
    got_R = InitializePose3.initializeOrientations(g)
    assert sorted(got_R) == sorted(want_R)
    print(name, "rotations", rel(stack(got_R), stack(want_R)))
    assert rel(stack(got_R), stack(want_R)) <= TOL
    want = r.compute_poses(want_R, edges)
    got = InitializePose3.initialize(g)
    assert got.keys() == want.keys()
    print(name, "poses", rel(stack_values(got), stack_values(want)))
    assert rel(stack_values(got), stack_values(want)) <= TOL
    # the pieces one by one give the same as the fused call
    pg = InitializePose3.buildPose3graph(g)
    got2 = InitializePose3.computePoses(InitializePose3.computeOrientationsChordal(pg), pg)
    assert pg.size() == len(edges) + 1  # computePoses added the anchor's prior, like the reference
    assert rel(stack_values(got2), stack_values(got)) <= 1e-12


@pytest.mark.parametrize("which", ["sphere2500_colamd", "sphere2500_metis"])
def test_sphere2500_full_with_committed_orderings(which):
    g = _file_graph("sphere2500.txt")
    fx = np.load(os.path.join(GOLD, "slam_orderings.npz"))
    order = [int(k) for k in fx[which]] + [r.ANCHOR]
    edges = r.extract(g)
    want_R = r.orientations_chordal(edges)
    got_R = InitializePose3.initializeOrientations(g, ordering=order)
    print(which, "rotations", rel(stack(got_R), stack(want_R)))
    assert rel(stack(got_R), stack(want_R)) <= TOL
    want = r.compute_poses(want_R, edges, True, order)
    got = InitializePose3.initialize(g, ordering=order)
    print(which, "poses", rel(stack_values(got), stack_values(want)))
    assert rel(stack_values(got), stack_values(want)) <= TOL
    # the anchor elsewhere in the ordering, and the natural ordering: the same result up to round-off
    alt = InitializePose3.initializeOrientations(g, ordering=[r.ANCHOR] + order[:-1])
    assert rel(stack(alt), stack(got_R)) <= 1e-9
    if which.endswith("colamd"):
        nat = InitializePose3.initializeOrientations(g)
        assert rel(stack(nat), stack(got_R)) <= 1e-9


def test_jacobian_tap_of_chordal_factor():
    """lmgpu_get_jacobian of a chordal factor = [-I9 M9 0] whitened; the prior = [I9 vec(I3)]"""
    pg = InitializePose3.buildPose3graph(c.graph2())
    gfg = InitializePose3.buildLinearOrientationGraph(pg)
    rows = r.linear_orientation_rows(r.extract(c.graph2()))
    assert gfg.size() == len(rows) == 7
    for i, (keys, As, b) in enumerate(rows):
        f = gfg.at(i)
        assert tuple(f.keys()) == keys
        want = np.hstack(list(As) + [b.reshape(9, 1)])
        assert f.augmentedJacobian().shape == want.shape
        assert np.abs(f.augmentedJacobian() - want).max() <= 1e-15 * max(1.0, np.abs(want).max()), i
    assert np.count_nonzero(gfg.at(3).augmentedJacobian()) == 0  # zero precision: a factor of zero rows
    # the raw tap on the fused object's orientation handle
    s = _Session(pg)
    try:
        s.chordal()
        h = s.handle(0)
        rr, cc = ct.c_int32(), ct.c_int32()
        assert s.lib.lmgpu_get_jacobian(h, 0, None, ct.byref(rr), ct.byref(cc)) == 0 and (rr.value, cc.value) == (9, 19)
        out = np.empty(9 * 19)
        assert s.lib.lmgpu_get_jacobian(h, 0, out.ctypes.data_as(ct.POINTER(ct.c_double)), ct.byref(rr), ct.byref(cc)) == 0
        keys, As, b = rows[0]
        assert np.abs(out.reshape(19, 9).T - np.hstack(list(As) + [b.reshape(9, 1)])).max() <= 1e-15
    finally:
        s.close()


def _close(expected, actual, tol):
    assert np.abs(np.asarray(expected) - np.asarray(actual)).max() <= tol, np.abs(np.asarray(expected) - np.asarray(actual)).max()


@pytest.mark.parametrize("g", [c.graph, c.graph2])
def test_known_answers_chordal(g):
    """testInitializePose3.cpp:98-121 on the device"""
    rots = InitializePose3.computeOrientationsChordal(InitializePose3.buildPose3graph(g()))
    for k, (R, _) in c.POSES.items():
        _close(R, rots[k], 1e-6)


def test_known_answers_gradient_1_and_10_iterations():
    """:173-248 on the device"""
    pg = InitializePose3.buildPose3graph(c.graph())
    rots, it, mg = InitializePose3.computeOrientationsGradient(pg, c.perturbed_guess(), 1, False, return_info=True)
    assert it == 1
    for k, M in c.ITER1.items():
        _close(M, rots[k], 1e-5)
    want, _, trace = r.orientations_gradient(r.extract(c.graph()), c.rots_of(c.perturbed_guess()), 1, False)
    assert rel(stack(rots), stack(want)) <= TOL and abs(mg - trace[-1]) <= TOL * trace[-1]
    rots, it, mg = InitializePose3.computeOrientationsGradient(pg, c.perturbed_guess(), 10, False, return_info=True)
    assert it == 10
    for k, M in c.iter10_expected().items():
        _close(M, rots[k], c.ITER10_TOL[k])
    want, _, trace = r.orientations_gradient(r.extract(c.graph()), c.rots_of(c.perturbed_guess()), 10, False)
    assert rel(stack(rots), stack(want)) <= TOL and abs(mg - trace[-1]) <= TOL * trace[-1]


def test_known_answers_poses():
    """posesWithGivenGuess :251-262 and initializePoses :265-276 on the device"""
    init = InitializePose3.initialize(c.graph(), c.true_guess())
    assert init.keys() == sorted(c.POSES)
    for k, (R, t) in c.POSES.items():
        _close(np.concatenate([R.reshape(9), t]), init.at(k), 1e-6)
    g, in_file = c.grid()
    init = InitializePose3.initialize(g)
    assert init.keys() == in_file.keys()
    for k in in_file.keys():
        _close(in_file.at(k), init.at(k), 0.1)


def test_closest_to_known_answer_on_device():
    """testSO3.cpp:54-68 through normalizeRelaxedRotations (which projects the TRANSPOSE of the column-major relaxed matrix)"""
    M = 3 * np.array([[0.79067393, 0.6051136, -0.0930814], [0.4155925, -0.64214347, -0.64324489], [-0.44948549, 0.47046326, -0.75917576]])
    expected = np.array([[0.790687, 0.605096, -0.0931312], [0.415746, -0.642355, -0.643844], [-0.449411, 0.47036, -0.759468]])
    rng = np.random.default_rng(1)
    relaxed = {7: M.reshape(9), r.ANCHOR: np.eye(3).reshape(9)}  # ClosestTo(M) <- relaxed vector = M row-major
    for k in range(8, 40):
        relaxed[k] = rng.standard_normal(9)  # general matrices, both signs of the determinant
    got = InitializePose3.normalizeRelaxedRotations(relaxed)
    assert r.ANCHOR not in got and len(got) == 33
    _close(expected, got[7], 1e-6)
    want = r.normalize_relaxed(relaxed)
    for k in want:
        assert rel(got[k], want[k]) <= TOL, k
        assert abs(np.linalg.det(got[k]) - 1.0) <= 1e-12


@pytest.mark.parametrize("set_ref_frame", [False, True])
def test_gradient_runs_to_its_stop_rule(set_ref_frame):
    """Input: init_pose3_cases.ring() (12 poses on a ring about z with one chord, noisy measurements, a prior on pose 0; guess = yaw-only
    rotations off by 0.3 sin(3 i) rad).  The restatement stops after 39 iterations; its maxGrad is 5.1688e-3 at iteration 38 and
    4.8294e-3 at the stopping one, 3.4 % either side of 5e-3 (asserted on the CPU in test_init_pose3_reference.py), so round-off cannot
    move the stop.  The device must stop at the same iteration, not later, and agree with the restatement there."""
    g, guess = c.ring()
    want, it, trace = r.orientations_gradient(r.extract(g), c.rots_of(guess), 10000, set_ref_frame)
    got, git, mg = InitializePose3.computeOrientationsGradient(InitializePose3.buildPose3graph(g), guess, 10000, set_ref_frame, return_info=True)
    print("stop", it, git, trace[-2:], mg)
    assert git == it
    assert abs(mg - trace[-1]) <= TOL * trace[-1]
    assert rel(stack(got), stack(want)) <= TOL
    # maxIter below the stop: exactly maxIter iterations
    got, git, mg = InitializePose3.computeOrientationsGradient(InitializePose3.buildPose3graph(g), guess, 30, set_ref_frame, return_info=True)
    want, it, trace = r.orientations_gradient(r.extract(g), c.rots_of(guess), 30, set_ref_frame)
    assert git == it == 30 and abs(mg - trace[-1]) <= TOL * trace[-1] and rel(stack(got), stack(want)) <= TOL
    # the whole pipeline in gradient mode
    pw = r.initialize(g, c.rots_of(guess), True)
    pg = InitializePose3.initialize(g, guess, True)
    assert rel(stack_values(pg), stack_values(pw)) <= TOL


def test_gradient_on_sphere2500_head_matches_restatement():
    g = _file_graph("sphere2500_head.txt")
    guess = chain_initial_pose3(g)
    want, it, trace = r.orientations_gradient(r.extract(g), c.rots_of(guess), 25, True)
    got, git, mg = InitializePose3.computeOrientationsGradient(InitializePose3.buildPose3graph(g), guess, 25, True, return_info=True)
    assert git == it == 25
    assert rel(stack(got), stack(want)) <= TOL and abs(mg - trace[-1]) <= TOL * trace[-1]


def test_chordal_through_pcg_agrees_with_cholesky():
    """the tolerance of test_gpu_pcg.py's PCG-against-direct comparison: 1e-7 relative, BlockJacobi, eps 1e-14"""
    pg = InitializePose3.buildPose3graph(_file_graph("sphere2500_head.txt"))
    direct = InitializePose3.computeOrientationsChordal(pg)
    p = LevenbergMarquardtParams()
    p.linearSolverType = "ITERATIVE"
    p.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    p.iterativeParams.epsilon_rel, p.iterativeParams.epsilon_abs, p.iterativeParams.maxIterations = 1e-14, 1e-28, 20000
    pcg = InitializePose3.computeOrientationsChordal(pg, params=p)
    print("pcg vs cholesky", rel(stack(pcg), stack(direct)))
    assert rel(stack(pcg), stack(direct)) <= 1e-7
    # the generic path (CHORDAL_BETWEEN / PRIOR_VEC9 buckets on an ordinary handle), both solvers: the step IS the relaxed solution
    relaxed_want = r.relaxed_orientations(r.extract(pg))
    for params in (None, p):
        opt = InitializePose3._orientation_problem(pg, None, params)
        opt.linearize()
        by_key, _, _, _ = opt.solve(0.0)
        assert rel(stack(by_key), stack(relaxed_want)) <= TOL
        opt.close()


def test_gaussian_and_diagonal_noise_give_the_restatements_precision():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((6, 6))
    gauss = noiseModel.Gaussian.Information(A @ A.T + 6 * np.eye(6))
    diag = noiseModel.Diagonal.Sigmas([0.3, 0.1, 0.2, 0.5, 0.4, 0.6])
    iso = noiseModel.Isotropic.Sigma(6, 0.25)
    unit = noiseModel.Unit.Create(6)
    g = NonlinearFactorGraph()
    models = [gauss, diag, iso, unit, gauss]
    for (a, b), m in zip(((c.x0, c.x1), (c.x1, c.x2), (c.x2, c.x3), (c.x2, c.x0), (c.x0, c.x3)), models):
        R, t = c.between(c.POSES[a], c.POSES[b])
        g.add_BetweenFactorPose3(a, b, R @ r.expmap(0.05 * rng.standard_normal(3)), t, m)
    g.add_PriorFactorPose3(c.x0, c.R0, c.p0, diag)
    pg = InitializePose3.buildPose3graph(g)
    gfg = InitializePose3.buildLinearOrientationGraph(pg)
    edges = r.extract(g)
    want_p = [r.rotation_precision(e[4]) for e in edges]
    assert abs(want_p[0] - gauss.data[0, 0]) < 1e-15 and want_p[1] == 1 / 0.3 and want_p[2] == 4.0 and want_p[3] == 1.0
    for i, p in enumerate(want_p):
        got = gfg.at(i).getA(0)[0, 0] ** 2  # A1 = -sqrt(p) I9
        assert abs(got - p) <= 1e-14 * p, (i, got, p)
    got_R = InitializePose3.initializeOrientations(g)
    assert rel(stack(got_R), stack(r.orientations_chordal(edges))) <= TOL
    assert rel(stack_values(InitializePose3.initialize(g)), stack_values(r.initialize(g))) <= TOL


def test_rejected_inputs_leave_the_object_usable():
    lib = _lib.load()
    ip = ct.c_void_p()
    cfg = _lib.lmgpu_config(0, 0, 1, 0)
    assert lib.lmgpu_init_pose3_create(ct.byref(cfg), ct.byref(ip)) == 0
    u64 = lambda a: np.asarray(a, dtype=np.uint64).ctypes.data_as(ct.POINTER(ct.c_uint64))
    dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))
    i32 = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_int32))
    ident = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    try:
        # only a prior: no Pose3 between factor
        gi = np.array([0], dtype=np.int32)
        assert lib.lmgpu_init_pose3_add_factors(ip, 4, 1, i32(gi), u64([0]), dp(ident), 0, None) == 0
        o = np.array([0], dtype=np.uint64)
        assert lib.lmgpu_init_pose3_finalize(ip, 1, u64(o)) == _lib.LMGPU_INVALID
        assert lib.lmgpu_init_pose3_num_poses(ip) == -1
        assert lib.lmgpu_init_pose3_orientations_chordal(ip, None) == _lib.LMGPU_INVALID
        # a between factor 0 -> 1; an ordering with a variable (2) that has no factor, then one that misses a factor's key
        gi = np.array([1], dtype=np.int32)
        meas = ident.copy()
        meas[9] = 1.0
        assert lib.lmgpu_init_pose3_add_factors(ip, 2, 1, i32(gi), u64([0, 1]), dp(meas), 0, None) == 0
        assert lib.lmgpu_init_pose3_add_factors(ip, 7, 1, i32(gi), u64([0, 1]), dp(meas), 0, None) == 0  # dropped silently
        assert lib.lmgpu_init_pose3_finalize(ip, 3, u64([0, 1, 2])) == _lib.LMGPU_INVALID
        assert b"no factor" in lib.lmgpu_init_pose3_last_error(ip)
        assert lib.lmgpu_init_pose3_finalize(ip, 1, u64([0])) == _lib.LMGPU_INVALID
        assert lib.lmgpu_init_pose3_finalize(ip, 2, u64([1, 1])) == _lib.LMGPU_INVALID
        # still usable
        assert lib.lmgpu_init_pose3_finalize(ip, 2, u64([1, 0])) == 0
        assert lib.lmgpu_init_pose3_num_poses(ip) == 2 and lib.lmgpu_init_pose3_num_factors(ip) == 2
        poses = np.empty((2, 12))
        assert lib.lmgpu_init_pose3_initialize(ip, None, 0, dp(poses)) == 0
        assert np.abs(poses[0] - meas).max() <= 1e-12 and np.abs(poses[1] - ident).max() <= 1e-12  # order of the ordering: key 1, key 0
        assert lib.lmgpu_init_pose3_orientations_gradient(ip, None, 10, 0, None, None, None) == _lib.LMGPU_INVALID
        assert lib.lmgpu_init_pose3_initialize(ip, None, 0, dp(poses)) == 0
    finally:
        lib.lmgpu_init_pose3_destroy(ip)
    # gradient mode without a prior: the anchor has no edge (the reference throws)
    g = NonlinearFactorGraph()
    g.add_BetweenFactorPose3(0, 1, np.eye(3), [1.0, 0, 0], noiseModel.Unit.Create(6))
    guess = Values()
    guess.insert_pose3(0, np.eye(3), np.zeros(3))
    guess.insert_pose3(1, np.eye(3), np.zeros(3))
    with pytest.raises(_lib.LmgpuError, match="anchor has no edge"):
        InitializePose3.computeOrientationsGradient(g, guess, 5, True)
    # chordal without a prior: the relaxation is indeterminate, as GaussianFactorGraph::optimize throws in the reference
    with pytest.raises(_lib.IndeterminantLinearSystemException):
        InitializePose3.initializeOrientations(g)


def test_sphere2500_end_to_end():
    """The chordal start has a lower graph error than the odometry chain, and Gauss-Newton on the device from the chordal start
    follows the CPU oracle's Gauss-Newton from the same start: same iteration count, error and values at 1e-6 relative."""
    g = _file_graph("sphere2500.txt")
    fx = np.load(os.path.join(GOLD, "slam_orderings.npz"))
    order = [int(k) for k in fx["sphere2500_colamd"]]
    init = InitializePose3.initialize(g, ordering=order + [r.ANCHOR])
    chain = chain_initial_pose3(g)
    e_init, e_chain = oh.OracleProblem(g, init, order).error(), oh.OracleProblem(g, chain, order).error()
    print("graph error: chordal", e_init, "chain", e_chain)
    assert e_init < e_chain
    params = GaussNewtonParams()
    opt = GaussNewtonOptimizer(g, init, order, params, device=0)
    orc = oh.OracleProblem(g, init, order)
    orc.lm_init(params)
    assert abs(opt.error() - e_init) <= TOL * e_init
    opt.optimize()
    assert orc.gn_optimize(params) == 0
    so = orc.lm_state()
    print("GN from the chordal start: iterations", so["iterations"], "error", so["error"])
    assert opt.iterations() == so["iterations"]
    assert abs(opt.error() - so["error"]) <= 1e-6 * max(1e-12, abs(so["error"])) + 1e-12
    # values: the parity bound of this file and of tests/test_gpu_fullsize.py for this data set, 1e-6 relative on packed values -- over all
    # poses and for every single pose.  (An absolute 1e-7 per entry, as the small graphs of test_gpu_parity.py use, is not that bound
    # here: translations are of the order of 100, and one entry of pose 2327 differs by 1.3e-7 = 1.3e-9 of the pose's norm between two
    # FP64 eliminations of this step, which raises the error fourfold.)
    vo, vg = orc.values(), opt.values()
    keys = sorted(vo)
    worst = max(rel(vg.at(k), vo[k]) for k in keys)
    print("GN values: all poses", rel(np.stack([vg.at(k) for k in keys]), np.stack([vo[k] for k in keys])), "worst pose", worst)
    assert rel(np.stack([vg.at(k) for k in keys]), np.stack([vo[k] for k in keys])) <= TOL
    assert worst <= TOL
