"""TEST INFRASTRUCTURE: the inputs of the TranslationRecovery tests, shared by the CPU file (restatement against the reference's known
answers) and the GPU file (device against restatement).  The known-answer scenes are those of tests/testTranslationRecovery.cpp in the
reference tree; an edge is (key1, key2, z, Noise | None) as in translation_recovery_restatement."""
import os

import numpy as np

import translation_recovery_restatement as trr
from gtsam_personal_amd.datasets import SfmData

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bal():
    db = SfmData.FromBalFile(os.path.join(GOLD, "dubrovnik-3-7-pre.txt"))
    pos = {j: np.asarray(cam[1], dtype=float) for j, cam in enumerate(db.cameras)}
    rel = trr.simulate(pos, [(0, 1), (0, 2), (1, 2)])
    Ta, Tb, Tc = pos[0], pos[1], pos[2]
    expected = {0: (np.zeros(3), 1e-9), 1: (2 * rel[0][2], 1e-9), 2: ((Tc - Ta) * (2.0 / np.linalg.norm(Tb - Ta)), 1e-4)}
    return dict(rel=rel, scale=2.0, betweens=[], expected=expected)


def _scene(pos, edges, scale, expected, tol, betweens=()):
    return dict(rel=trr.simulate(pos, edges), scale=scale, betweens=list(betweens), expected={k: (np.asarray(v, dtype=float), tol) for k, v in expected.items()})


P3 = {0: [0, 0, 0], 1: [2, 0, 0], 3: [1, -1, 0]}
P4 = {0: [0, 0, 0], 1: [2, 0, 0], 2: [2, 0, 0], 3: [1, -1, 0]}


def known_answers():
    """name -> dict(rel, scale, betweens, expected {key: (Point3, the reference test's tolerance)}); assert_equal's default is 1e-9"""
    return {
        "BAL": _bal(),
        "TwoPoseTest": _scene({0: [0, 0, 0], 1: [2, 0, 0]}, [(0, 1)], 3.0, {0: [0, 0, 0], 1: [3, 0, 0]}, 1e-8),
        "ThreePoseTest": _scene(P3, [(0, 1), (1, 3), (3, 0)], 3.0, {0: [0, 0, 0], 1: [3, 0, 0], 3: [1.5, -1.5, 0]}, 1e-8),
        "ThreePosesIncludingZeroTranslation": _scene({0: [0, 0, 0], 1: [2, 0, 0], 2: [2, 0, 0]}, [(0, 1), (1, 2)], 3.0,
                                                     {0: [0, 0, 0], 1: [3, 0, 0], 2: [3, 0, 0]}, 1e-8),
        "FourPosesIncludingZeroTranslation": _scene(P4, [(0, 1), (1, 2), (1, 3), (3, 0)], 4.0,
                                                    {0: [0, 0, 0], 1: [4, 0, 0], 2: [4, 0, 0], 3: [2, -2, 0]}, 1e-8),
        "ThreePosesWithZeroTranslation": _scene({0: [0, 0, 0], 1: [0, 0, 0], 2: [0, 0, 0]}, [(0, 1), (1, 2), (2, 0)], 4.0,
                                                {0: [0, 0, 0], 1: [0, 0, 0], 2: [0, 0, 0]}, 1e-8),
        "ThreePosesWithOneSoftConstraint": _scene(P3, [(0, 1), (0, 3), (1, 3)], 0.0, {0: [0, 0, 0], 1: [2, 0, 0], 3: [1, -1, 0]}, 1e-4,
                                                  [(0, 3, np.array([1.0, -1, 0]), trr.Noise.isotropic(1e-2))]),
        # the reference's (0, 1) between carries Constrained::All(3, 1e2): an isotropic model of the same sigma as the soft case stands in
        "NodeWithBetweenFactorAndNoMeasurements": _scene({**P3, 4: [1, 2, 1]}, [(0, 1), (0, 3), (1, 3)], 0.0,
                                                         {0: [0, 0, 0], 1: [2, 0, 0], 3: [1, -1, 0], 4: [1, 2, 1]}, 1e-4,
                                                         [(0, 1, np.array([2.0, 0, 0]), trr.Noise.isotropic(1e-2)), (0, 4, np.array([1.0, 2, 1]), None)]),
    }


NOISY_MAX_ITERATIONS = 5  # the iterations of noisy_scene whose every decision is clear of its bound (test_noisy_scene_decisions_have_margin)


def noisy_scene(n=40, m=120, seed=5, spread=0.2, sigma=0.2):
    """n nodes on a deterministic point cloud, m edges (a ring plus chords), directions turned away from the truth by a fixed rule so that the
    optimum keeps an error of order one to ten (sigma 0.2 against perturbations of order `spread`); two of its first five iterations reject
    trial steps and raise lambda.  Isotropic noise on two thirds of the edges, a diagonal model on the rest.
    -> (rel, initial values {key: Point3}, positions)"""
    rng = np.random.RandomState(seed)
    pos = {i: np.array([4 * np.cos(2 * np.pi * i / n), 4 * np.sin(2 * np.pi * i / n), 0.0]) + rng.uniform(-1, 1, 3) for i in range(n)}
    pairs = [(i, (i + 1) % n) for i in range(n)]
    k = 2
    while len(pairs) < m:
        for i in range(n):
            if len(pairs) < m:
                pairs.append((i, (i + k) % n))
        k += 3
    rel = []
    for e, (a, b) in enumerate(pairs):
        d = pos[b] - pos[a] + spread * np.linalg.norm(pos[b] - pos[a]) * rng.uniform(-1, 1, 3)
        noise = trr.Noise.isotropic(sigma) if e % 3 else trr.Noise.diagonal([sigma, 2 * sigma, 1.5 * sigma])
        rel.append((a, b, d / np.linalg.norm(d), noise))
    init = {i: pos[i] + 0.3 * rng.uniform(-1, 1, 3) for i in range(n)}
    return rel, init, pos


def complete_graph(n=60, seed=3):
    """every pair of n nodes, exact directions, isotropic noise: its elimination ends in one dense front of 3 n columns"""
    rng = np.random.RandomState(seed)
    pos = {i: rng.uniform(-5, 5, 3) for i in range(n)}
    edges = [(a, b) for a in range(n) for b in range(a + 1, n)]
    rel = trr.simulate(pos, edges)
    init = {i: pos[i] + 0.2 * rng.uniform(-1, 1, 3) for i in range(n)}
    return rel, init, pos
