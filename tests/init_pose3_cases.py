"""Inputs shared by the InitializePose3 tests: the graphs of gtsam/slam/tests/testInitializePose3.cpp:36-89 and their known answers."""
from __future__ import annotations

import os

import numpy as np

from gtsam_personal_amd.datasets import load3D, rot3_expmap, rot3_ypr
from gtsam_personal_amd.graph import NonlinearFactorGraph, Values, noiseModel, symbol

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
x0, x1, x2, x3 = (symbol("x", i) for i in range(4))
R0, R1, R2, R3 = (rot3_expmap([0.0, 0.0, a]) for a in (0.0, 1.570796, 3.141593, 4.712389))
p0, p1, p2, p3 = (np.array(p, dtype=float) for p in ([0, 0, 0], [1, 2, 0], [0, 2, 0], [-1, 1, 0]))
POSES = {x0: (R0, p0), x1: (R1, p1), x2: (R2, p2), x3: (R3, p3)}


def between(a, b):
    (Ra, ta), (Rb, tb) = a, b
    return Ra.T @ Rb, Ra.T @ (tb - ta)


def graph():
    """simple::graph(), testInitializePose3.cpp:61-70"""
    model = noiseModel.Isotropic.Sigma(6, 0.1)
    g = NonlinearFactorGraph()
    for a, b in ((x0, x1), (x1, x2), (x2, x3), (x2, x0), (x0, x3)):
        g.add_BetweenFactorPose3(a, b, *between(POSES[a], POSES[b]), model)
    g.add_PriorFactorPose3(x0, R0, p0, model)
    return g


def _iso_precision(dim, p):
    """noiseModel::Isotropic::Precision(dim, p) = Variance(dim, 1 / p): sigma = 1 / sqrt(p); p = 0 gives an infinite sigma"""
    from gtsam_personal_amd.graph import N_ISO, N_UNIT, NoiseModel
    if p == 1.0:
        return NoiseModel(dim, N_UNIT)
    return NoiseModel(dim, N_ISO, np.inf if p == 0 else 1.0 / np.sqrt(p))


def graph2():
    """simple::graph2(), :72-88: two factors with zero information"""
    g = NonlinearFactorGraph()
    one, zero = _iso_precision(6, 1.0), _iso_precision(6, 0.0)
    for a, b in ((x0, x1), (x1, x2), (x2, x3)):
        g.add_BetweenFactorPose3(a, b, *between(POSES[a], POSES[b]), one)
    g.add_BetweenFactorPose3(x2, x0, rot3_ypr(0.1, 0.0, 0.1), [0.0, 0.0, 0.0], zero)
    g.add_BetweenFactorPose3(x0, x3, rot3_ypr(0.5, -0.2, 0.2), [10.0, 20.0, 30.0], zero)
    g.add_PriorFactorPose3(x0, R0, p0, noiseModel.Isotropic.Sigma(6, 0.1))
    return g


def perturbed_guess():
    """givenPoses of iterationGradient / orientationsGradient, :176-182"""
    Rp = rot3_expmap([0.01, 0.01, 0.01])
    v = Values()
    v.insert_pose3(x0, R0, p0)
    v.insert_pose3(x1, R0 @ Rp, p0)
    v.insert_pose3(x2, R0 @ Rp.T, p0)
    v.insert_pose3(x3, R0 @ Rp, p0)
    return v


def true_guess():
    v = Values()
    for k, (R, t) in POSES.items():
        v.insert_pose3(k, R, t)
    return v


def rots_of(values):
    return {k: values.at(k)[:9].reshape(3, 3) for k in values.keys()}


# the four matrices printed in iterationGradient, :188-210
ITER1 = {
    x0: np.array([[0.999435813876064, -0.033571481675497, 0.001004768630281], [0.033572116359134, 0.999436104312325, -0.000621610948719],
                  [-0.000983333645009, 0.000654992453817, 0.999999302019670]]),
    x1: np.array([[0.999905367545392, -0.010866391403031, 0.008436675399114], [0.010943459008004, 0.999898317528125, -0.009143047050380],
                  [-0.008336465609239, 0.009234508232789, 0.999922610604863]]),
    x2: np.array([[0.998936644682875, 0.045376417678595, -0.008158469732553], [-0.045306446926148, 0.998936408933058, 0.008566024448664],
                  [0.008538487960253, -0.008187284445083, 0.999930028850403]]),
    x3: np.array([[0.999898767273093, -0.010834701971459, 0.009223038487275], [0.010911315499947, 0.999906044037258, -0.008297366559388],
                  [-0.009132272433995, 0.008397162077148, 0.999923041673329]]),
}
ITER10_TOL = {x0: 1e-4, x1: 1e-4, x2: 1e-3, x3: 1e-4}  # :238-247


def iter10_expected():
    """rotations of vertices 1..4 of simpleGraph10gradIter.txt = x0..x3 (:233-247)"""
    _, vals = load3D(os.path.join(GOLD, "simpleGraph10gradIter.txt"))
    return {k: vals.at(i + 1)[:9].reshape(3, 3) for i, k in enumerate((x0, x1, x2, x3))}


def grid():
    """initializePoses, :265-276: pose3example-grid with a Unit prior on pose 0; returns (graph, posesInFile)"""
    g, vals = load3D(os.path.join(GOLD, "pose3example-grid.txt"))
    g.add_PriorFactorPose3(0, np.eye(3), np.zeros(3), noiseModel.Unit.Create(6))
    return g, vals


def with_prior(g):
    g.add_PriorFactorPose3(0, np.eye(3), np.zeros(3), noiseModel.Unit.Create(6))
    return g


# gradient mode to its stop rule: a ring of N poses about z with one chord, started from the identity everywhere
def ring(n=12, seed=3):
    rng = np.random.default_rng(seed)
    Rs = [rot3_expmap([0.05 * np.sin(i), 0.04 * np.cos(2 * i), 2 * np.pi * i / n]) for i in range(n)]
    model = noiseModel.Isotropic.Sigma(6, 0.1)
    g = NonlinearFactorGraph()
    for i in range(n):
        j = (i + 1) % n
        noise = rot3_expmap(0.02 * rng.standard_normal(3))
        g.add_BetweenFactorPose3(i, j, Rs[i].T @ Rs[j] @ noise, [1.0, 0.0, 0.0], model)
    g.add_BetweenFactorPose3(0, n // 2, Rs[0].T @ Rs[n // 2], [0.0, 1.0, 0.0], model)
    g.add_PriorFactorPose3(0, Rs[0], np.zeros(3), model)
    guess = Values()
    for i in range(n):
        guess.insert_pose3(i, rot3_expmap([0.0, 0.0, 2 * np.pi * i / n + 0.3 * np.sin(3 * i)]), np.zeros(3))
    return g, guess
