"""TEST INFRASTRUCTURE: the inputs the GNC tests share (CPU restatement tests and device tests build exactly the same problems)."""
import os

import numpy as np

from gtsam_personal_amd import NonlinearFactorGraph, Ordering, Values, X, noiseModel
from gtsam_personal_amd.datasets import load2D
from gtsam_personal_amd.synthetic import make_bal

GOLD = os.path.join(os.path.dirname(__file__), "golden")
B2 = 4.605170185988091  # 0.5 * chi2inv(0.99, 2): the default threshold of the reference's Point2 toy graph


def toy_graph(robust=True):
    """sharedRobustFactorGraphWithOutliers (tests/smallExample.h:406-427) with PriorFactor<Point3> (third coordinate 0) in place of
    PriorFactor<Point2>: three priors at the origin and one at (1, 0, 0), Isotropic sigma 0.1 under a Geman-McClure loss"""
    g = NonlinearFactorGraph()
    m = noiseModel.Isotropic.Sigma(3, 0.1)
    if robust:
        m = noiseModel.Robust.Create(noiseModel.mEstimator.GemanMcClure.Create(1.0), m)
    for z in ([0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]):
        g.add_PriorFactorPoint3(X(1), z, m)
    return g


def point_values(p):
    v = Values()
    v.insert_point3(X(1), p)
    return v


W100_OUTLIER = (90, 50)  # the reference's outlier
# The LM-base / TLS run on the reference's outlier is chaotic in the restatement itself: perturbing the initial values by 1e-13 changes
# its outer iteration count (29 -> 28) and moves the result by 15 (tests/test_gnc_reference.py measures this).  Its discrete outcome
# cannot be compared between two implementations, so that one case uses another wrong loop closure with the same measurement and noise,
# for which a 1e-10 perturbation moves the result by 3e-11.
W100_OUTLIER_OF_CASE = {("LM", 1): (20, 70)}


def w100(outlier=True, pair=W100_OUTLIER):
    """testGncOptimizer.cpp:737-758: w100.graph + a prior on pose 0 (sigmas 0.01) [+ BetweenFactor<Pose2>(pair, Pose2(), (0.1, 0.1, 0.01))]"""
    graph, initial = load2D(os.path.join(GOLD, "w100.graph"))
    graph.add_PriorFactorPose2(0, [0.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.01, 0.01, 0.01]))
    if outlier:
        graph.add_BetweenFactorPose2(pair[0], pair[1], [0.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.1, 0.1, 0.01]))
    return graph, initial, Ordering.Natural(graph)


def w100_case(base, loss):
    return w100(True, W100_OUTLIER_OF_CASE.get((base, loss), W100_OUTLIER))


def perturbed(values, eps, seed=1):
    """every coordinate moved by eps relative + eps absolute (uniform, seeded)"""
    rng = np.random.default_rng(seed)
    out = values.copy()
    for k in out.keys():
        x = out.at(k)
        out.update(k, x * (1 + eps * rng.uniform(-1, 1, x.shape)) + eps * rng.uniform(-1, 1, x.shape))
    return out


BAL_SEED, BAL_SHARE, BAL_PIXELS = 7, 0.05, 40.0


def bal_with_outliers(n_cam=12, n_pt=300, obs_per_point=8, seed=BAL_SEED, share=BAL_SHARE, pixels=BAL_PIXELS):
    """synthetic BAL graph (synthetic.make_bal) in which `share` of the measurements are displaced by `pixels` .. 2 `pixels` in a random
    direction; returns (graph, initial, ordering, displaced: bool per graph index)"""
    graph, initial, _, ordering = make_bal(n_cam=n_cam, n_pt=n_pt, obs_per_point=obs_per_point, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    out = NonlinearFactorGraph()
    displaced = np.zeros(graph.size(), dtype=bool)
    for ftype, _, gi, keys, meas, _, models in graph.buckets():
        meas = meas.copy()
        if ftype == 0:
            pick = rng.random(len(gi)) < share
            ang = rng.uniform(0, 2 * np.pi, len(gi))
            rad = rng.uniform(pixels, 2 * pixels, len(gi))
            meas[pick, 0] += (rad * np.cos(ang))[pick]
            meas[pick, 1] += (rad * np.sin(ang))[pick]
            displaced[gi[pick]] = True
        assert (np.diff(gi) == 1).all() and gi[0] == out.size()
        out._add(ftype, keys, meas, models[0])
    return out, initial, ordering, displaced
