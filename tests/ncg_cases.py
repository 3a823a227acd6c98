"""TEST INFRASTRUCTURE: the graphs of the nonlinear conjugate gradient tests (tests/test_ncg_reference.py, tests/test_gpu_ncg.py)
and the restatement's results on them, computed once per process."""
from __future__ import annotations

import functools
import math
import os

import numpy as np

import ncg_restatement as nr
from gtsam_personal_amd import NonlinearFactorGraph, Values, noiseModel
from gtsam_personal_amd.datasets import chain_initial_pose3, load3D, pose3_compose, rot3_expmap
from gtsam_personal_amd.synthetic import make_bal

GOLD = os.path.join(os.path.dirname(__file__), "golden")

# ---- the tolerances of tests/test_gpu_ncg.py, measured on the CPU (tests/test_ncg_reference.py::test_measured_constants_hold
# measures them again).
# The branch `testError >= newError` of lineSearch makes the bracket sequence depend on the last bits of the error.  Probe: the
# restatement run as it is and with every error it evaluates multiplied by (1 +- 1e-15) (seeds 1, 2, 3).  Measured spread of alpha of
# the first line search and of the error after 1..5 iterations on five_pose, pose3_head and bal_small: 0 (bitwise equal; the errors a
# search compares differ by far more than 1e-15 relative until the bracket is ~1e-8 wide, and it stops at ~1.4e-5).
# The bracket tolerance tau implies: the search returns the midpoint of a bracket of width < tau (|testStep| + |newStep|) <= 2 tau
# |minStep| around the minimiser, i.e. alpha is determined to 2 tau = 2e-5 relative.  The larger of the two, times 10:
SPREAD_MEASURED = 0.0
BRACKET_RTOL = 2 * nr.TAU
ALPHA_RTOL = 10 * max(SPREAD_MEASURED, BRACKET_RTOL)  # 2e-4
ERROR_RTOL = 10 * max(SPREAD_MEASURED, BRACKET_RTOL)  # 2e-4
PERTURB_SEEDS = (1, 2, 3)
SEARCH_GRAPHS = ("five_pose", "pose3_head", "bal_small")
# The evaluation count of the first line search, probed the same way at eps = 1e-12 (the figure tests/test_gpu_ncg.py holds graph_error to
# the NCG error by): the graphs on which the count stays as it is under seeds 1, 2, 3 -- there the device's count must EQUAL the
# restatement's (measured: all three; tests/test_ncg_reference.py::test_trial_counts_are_robust).
TRIALS_EPS = 1e-12
TRIALS_EXACT_GRAPHS = ("five_pose", "pose3_head", "bal_small")
# beta of every trace row (test_each_direction_method_matches_its_restatement).  The device's alpha of a search lies within BRACKET_RTOL of
# the restatement's, and every later gradient, hence every later beta, follows the alpha before it.  Probe: the restatement with every
# search's alpha multiplied by (1 + BRACKET_RTOL), by (1 - BRACKET_RTOL), and by (1 +- BRACKET_RTOL) with the sign drawn per search (seeds
# 1, 2, 3), four iterations, four methods, five_pose and five_pose_huber.  BETA_SPREAD_MEASURED = the largest |beta' - beta| / max(|beta|,
# BETA_FLOOR) over all of those rows (tests/test_ncg_reference.py::test_beta_spread_holds measures it again); the tolerance is ten times it.
BETA_FLOOR = 1e-3  # a beta below this (a clamped or nearly clamped one) is compared absolutely against this scale
BETA_SPREAD_MEASURED = 2.8e-3  # 2.79e-3, five_pose, Hestenes-Stiefel: beta follows the gradient at a line minimum, where alpha's 2e-5 counts
BETA_RTOL = 10 * BETA_SPREAD_MEASURED
BETA_GRAPHS = ("five_pose", "five_pose_huber")



def five_pose(huber=False):
    """generateProblem() of gtsam/nonlinear/tests/testNonlinearConjugateGradientOptimizer.cpp:26-69; huber: a Huber model around
    the loop closure's noise"""
    g = NonlinearFactorGraph()
    g.add_PriorFactorPose2(1, [0.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    odo = noiseModel.Diagonal.Sigmas([0.2, 0.2, 0.1])
    g.add_BetweenFactorPose2(1, 2, [2.0, 0.0, 0.0], odo)
    g.add_BetweenFactorPose2(2, 3, [2.0, 0.0, math.pi / 2], odo)
    g.add_BetweenFactorPose2(3, 4, [2.0, 0.0, math.pi / 2], odo)
    g.add_BetweenFactorPose2(4, 5, [2.0, 0.0, math.pi / 2], odo)
    loop = noiseModel.Diagonal.Sigmas([0.2, 0.2, 0.1])
    if huber:
        loop = noiseModel.Robust.Create(noiseModel.mEstimator.Huber.Create(1.345), loop)
    g.add_BetweenFactorPose2(5, 2, [2.0, 0.0, math.pi / 2], loop)
    v = Values()
    v.insert_pose2(1, 0.5, 0.0, 0.2)
    v.insert_pose2(2, 2.3, 0.1, -0.2)
    v.insert_pose2(3, 4.1, 0.1, math.pi / 2)
    v.insert_pose2(4, 4.0, 2.0, math.pi)
    v.insert_pose2(5, 2.1, 2.1, -math.pi / 2)
    return g, v


def pose2_chain(n=86):
    """a prior and n - 1 odometry factors along a gentle arc, perturbed start: 3 n scalars (86 poses = 258 straddle a 256-thread block)"""
    rng = np.random.default_rng(11)
    g, v = NonlinearFactorGraph(), Values()
    g.add_PriorFactorPose2(0, [0.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    odo = noiseModel.Diagonal.Sigmas([0.2, 0.2, 0.1])
    x = y = th = 0.0
    for i in range(n):
        v.insert_pose2(i, x + rng.normal(0, 0.1), y + rng.normal(0, 0.1), th + rng.normal(0, 0.05))
        if i + 1 < n:
            g.add_BetweenFactorPose2(i, i + 1, [1.0, 0.0, 0.05], odo)
            x, y, th = x + math.cos(th), y + math.sin(th), th + 0.05
    return g, v


def pose3_head(n=30):
    """the factors of tests/golden/sphere2500_head.txt (edges only) among its first n poses, a prior on pose 0, and the
    odometry-chained initial estimate moved by seeded noise (the chained one has zero error on a graph without loop closures)"""
    graph, _ = load3D(os.path.join(GOLD, "sphere2500_head.txt"))
    initial = chain_initial_pose3(graph)
    keep = set(initial.keys()[:n])
    rng = np.random.default_rng(5)
    g, v = NonlinearFactorGraph(), Values()
    for k in sorted(keep):
        R, t = initial.at(k)[:9].reshape(3, 3), initial.at(k)[9:12]
        Rn, tn = pose3_compose(R, t, rot3_expmap(rng.normal(0, 0.03, 3)), rng.normal(0, 0.05, 3))
        v.insert_pose3(k, Rn, tn)
    rec = [None] * graph.size()
    for ftype, _, gi, keys, meas, _, models in graph.buckets():
        for i, gidx in enumerate(gi.tolist()):
            rec[gidx] = (ftype, keys[i], meas[i], models[i])
    for r in rec:
        if r is not None and all(int(k) in keep for k in r[1]):
            g._add(r[0], [r[1]], [r[2]], r[3])
    k0 = sorted(keep)[0]
    g.add_PriorFactorPose3(k0, initial.at(k0)[:9].reshape(3, 3), initial.at(k0)[9:12], noiseModel.Diagonal.Sigmas([0.1, 0.1, 0.1, 0.3, 0.3, 0.3]))
    return g, v


def bal_small():
    """3 cameras / 20 points: the GeneralSFMFactor kernels of their own"""
    graph, initial, _, _ = make_bal(n_cam=3, n_pt=20, obs_per_point=3, seed=3)
    return graph, initial


def self_calibration():
    """SelfCalibrationExample's graph as tests/test_sfm2.py builds it (three-variable factors)"""
    from test_sfm2 import self_calibration as sc
    return sc(n_poses=4, n_points=6)


GRAPHS = {
    "five_pose": five_pose,
    "chain86": pose2_chain,
    "pose3_head": pose3_head,
    "bal_small": bal_small,
    "self_calibration": self_calibration,
    "five_pose_huber": lambda: five_pose(huber=True),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def restated_gradient(name):
    graph, initial = problem(name)
    s = nr.OracleSystem(graph)
    return s.by_key(initial, s.gradient(initial))


@functools.lru_cache(maxsize=None)
def restated_line_search(name, seed=None):
    """(alpha, trials, bracket) of the first line search (direction = gradient); seed: the perturbed run"""
    graph, initial = problem(name)
    s = nr.OracleSystem(graph, perturb=None if seed is None else np.random.default_rng(seed))
    st = {}
    alpha = nr.line_search(s, initial, s.gradient(initial), st)
    return alpha, st["trials"], st["bracket"]


@functools.lru_cache(maxsize=None)
def restated_trials(name, seed=None):
    """evaluations of the first line search; seed: with every error multiplied by (1 +- TRIALS_EPS)"""
    graph, initial = problem(name)
    s = nr.OracleSystem(graph, perturb=None if seed is None else np.random.default_rng(seed), eps=TRIALS_EPS)
    st = {}
    nr.line_search(s, initial, s.gradient(initial), st)
    return st["trials"]


BETA_MOVES = ("up", "down", 1, 2, 3)


@functools.lru_cache(maxsize=None)
def restated_betas(name, method, move=None, max_iterations=4):
    """beta of every trace row; move: every search's alpha times (1 + BRACKET_RTOL) ("up"), (1 - BRACKET_RTOL) ("down"), or with the sign
    drawn per search from the seed `move`"""
    graph, initial = problem(name)
    rng = np.random.default_rng(move) if isinstance(move, int) else None
    fn = {None: None, "up": lambda a: a * (1 + BRACKET_RTOL), "down": lambda a: a * (1 - BRACKET_RTOL)}.get(
        move, lambda a: a * (1 + (BRACKET_RTOL if rng.integers(0, 2) else -BRACKET_RTOL)))
    trace = []
    nr.nonlinear_conjugate_gradient(nr.OracleSystem(graph), initial, nr.Params(maxIterations=max_iterations), False, method, False, trace, fn)
    return tuple(r[1] for r in trace)


def beta_distance(got, want):
    return abs(got - want) / max(abs(want), BETA_FLOOR)


@functools.lru_cache(maxsize=None)
def restated_run(name, max_iterations, method=nr.POLAK_RIBIERE, gradient_descent=False, seed=None, single=False):
    """(error after the run, iterations, trace) of nonlinearConjugateGradient with NonlinearOptimizerParams' default tolerances"""
    graph, initial = problem(name)
    s = nr.OracleSystem(graph, perturb=None if seed is None else np.random.default_rng(seed))
    trace = []
    values, it = nr.nonlinear_conjugate_gradient(s, initial, nr.Params(maxIterations=max_iterations), single, method, gradient_descent, trace)
    return nr.OracleSystem(graph).error(values), it, tuple(trace), values
