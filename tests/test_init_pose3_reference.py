"""The numpy restatement of InitializePose3 (tests/init_pose3_restatement.py) reproduces gtsam/slam/tests/testInitializePose3.cpp at
that file's own tolerances, and the new ABI surface exists.  No GPU needed."""
import ctypes as ct
import os
import re

import numpy as np

import init_pose3_cases as c
import init_pose3_restatement as r
from gtsam_personal_amd import _lib, graph as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(expected, actual, tol):
    """assert_equal(Matrix, Matrix, tol): every entry within tol"""
    assert np.abs(np.asarray(expected) - np.asarray(actual)).max() <= tol, np.abs(np.asarray(expected) - np.asarray(actual)).max()


def test_orientations():
    """testInitializePose3.cpp:98-108"""
    rots = r.orientations_chordal(r.extract(c.graph()))
    assert sorted(rots) == sorted(c.POSES)
    for k, (R, _) in c.POSES.items():
        _close(R, rots[k], 1e-6)


def test_orientations_precisions():
    """:111-121, two factors of zero precision"""
    edges = r.extract(c.graph2())
    assert [r.rotation_precision(e[4]) for e in edges] == [1.0, 1.0, 1.0, 0.0, 0.0, 10.0]
    rots = r.orientations_chordal(edges)
    for k, (R, _) in c.POSES.items():
        _close(R, rots[k], 1e-6)


def test_rotation_precision_per_noise_kind():
    """:48-51 restated for Unit, Isotropic, Diagonal and full Gaussian models"""
    nm = G.noiseModel
    assert r.rotation_precision(nm.Unit.Create(6)) == 1.0
    assert r.rotation_precision(nm.Isotropic.Sigma(6, 0.1)) == 10.0
    assert r.rotation_precision(nm.Diagonal.Sigmas([0.5, 1, 2, 3, 4, 5])) == 2.0
    A = np.random.default_rng(0).standard_normal((6, 6))
    info = A @ A.T + 6 * np.eye(6)
    assert abs(r.rotation_precision(nm.Gaussian.Information(info)) - np.linalg.cholesky(info).T[0, 0]) < 1e-15


def test_orientations_gradient_symbolic_graph():
    """:124-153"""
    adj = r.symbolic_graph(r.extract(c.graph()))
    assert adj[c.x0] == [0, 3, 4, 5]
    assert adj[c.x1] == [0, 1]
    assert adj[c.x2] == [1, 2, 3]
    assert adj[c.x3] == [2, 4]
    assert len(adj) == 5  # this includes the anchor


def test_single_gradient():
    """:156-170"""
    R2 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    _close([0, 0, 1.962658662803917], r.gradient_tron(np.eye(3), R2, 6.010534238540223, 1.0), 1e-6)
    a, b, _ = r.gradient_constants(1)
    assert abs(a - 6.010534238540223) < 1e-12 and b == 1.0


def test_iteration_gradient():
    """:173-211"""
    rots, it, _ = r.orientations_gradient(r.extract(c.graph()), c.rots_of(c.perturbed_guess()), 1, False)
    assert it == 1
    for k, M in c.ITER1.items():
        _close(M, rots[k], 1e-5)


def test_orientations_gradient_10_iterations():
    """:214-248 against simpleGraph10gradIter.txt"""
    rots, it, _ = r.orientations_gradient(r.extract(c.graph()), c.rots_of(c.perturbed_guess()), 10, False)
    assert it == 10
    for k, M in c.iter10_expected().items():
        _close(M, rots[k], c.ITER10_TOL[k])


def test_poses_with_given_guess():
    """:251-262 (initialize(graph, givenPoses): chordal, the guess is not used)"""
    init = r.initialize(c.graph(), c.rots_of(c.true_guess()), False)
    assert init.keys() == sorted(c.POSES)
    for k, (R, t) in c.POSES.items():
        _close(np.concatenate([R.reshape(9), t]), init.at(k), 1e-6)


def test_initialize_poses_grid():
    """:265-276"""
    g, in_file = c.grid()
    init = r.initialize(g)
    assert init.keys() == in_file.keys()
    for k in in_file.keys():
        _close(in_file.at(k), init.at(k), 0.1)


def test_closest_to():
    """gtsam/geometry/tests/testSO3.cpp:54-68"""
    M = np.array([[0.79067393, 0.6051136, -0.0930814], [0.4155925, -0.64214347, -0.64324489], [-0.44948549, 0.47046326, -0.75917576]])
    expected = np.array([[0.790687, 0.605096, -0.0931312], [0.415746, -0.642355, -0.643844], [-0.449411, 0.47036, -0.759468]])
    _close(expected, r.closest_to(3 * M), 1e-6)


def test_ring_stop_rule_has_margin():
    """the gradient-mode input of the GPU stop-rule test: maxGrad at the stopping iteration and at the one before are both clear of 5e-3"""
    g, guess = c.ring()
    for srf in (False, True):
        _, it, trace = r.orientations_gradient(r.extract(g), c.rots_of(guess), 10000, srf)
        assert it == len(trace) and it > 22
        assert trace[-1] < 5e-3 * (1 - 0.02) and trace[-2] > 5e-3 * (1 + 0.02), (it, trace[-2:])


def test_init_pose3_symbols_exported():
    lib = ct.CDLL(_lib.LIB_PATH)
    names = [n for n in _lib.SYMBOLS if n.startswith("lmgpu_init_pose3_")]
    assert len(names) == 14
    for name in names:
        assert hasattr(lib, name), name


def test_python_enums_match_header():
    h = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    val = lambda name: int(re.search(r"\b%s = (\d+)" % name, h).group(1))
    assert val("LMGPU_VEC9") == G.VEC9 == 6 and val("LMGPU_NUM_VAR_TYPES") == len(G.VAR_DIM) == 7
    assert val("LMGPU_F_CHORDAL_BETWEEN") == G.F_CHORDAL_BETWEEN == 12 and val("LMGPU_F_PRIOR_VEC9") == G.F_PRIOR_VEC9 == 13
    assert val("LMGPU_NUM_FACTOR_TYPES") == len(G.FACTOR_ROWS) == len(G.FACTOR_ARITY) == len(G.FACTOR_MEAS) == len(G.FACTOR_VARS) == 14
    assert val("LMGPU_CAL3_S2") == 5 and val("LMGPU_F_PRIOR_CAL3_S2") == 11  # existing values do not move
    assert G.VAR_DIM[G.VEC9] == G.VAR_STORE_DEV[G.VEC9] == 9 and G.FACTOR_ROWS[12] == G.FACTOR_ROWS[13] == 9
    assert int(re.search(r"LMGPU_INIT_POSE3_ANCHOR_KEY (\d+)", h).group(1)) == _lib.LMGPU_INIT_POSE3_ANCHOR_KEY == r.ANCHOR


def test_build_pose3_graph_mirror():
    """the Python mirror's buildPose3graph (host bookkeeping) against the restatement's extraction"""
    from gtsam_personal_amd import InitializePose3
    pg = InitializePose3.buildPose3graph(c.graph())
    assert pg.size() == 6
    assert pg.factor_keys_in_graph_order()[5] == (r.ANCHOR, c.x0)
    for a, b in zip(r.extract(pg), r.extract(c.graph())):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
