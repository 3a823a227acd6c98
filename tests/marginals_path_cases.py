"""Small graphs for the marginal path walk (csrc/kernels_marginals.hpp): one builder per shape the walk can go wrong
at.  Each returns (graph, values, ordering); tests/test_marginals_path_reference.py reads their structure on device = -1 handles,
tests/test_gpu_marginals_path.py their covariances on the device."""
import os

import numpy as np

from gtsam_personal_amd import NonlinearFactorGraph, Ordering, Values, noiseModel
from gtsam_personal_amd.datasets import chain_initial_pose3, load3D, rot3_expmap

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_S2 = (520.0, 510.0, 0.3, 320.0, 240.0)


def single_variable():
    g, v = NonlinearFactorGraph(), Values()
    g.add_PriorFactorPose2(7, [1.0, 2.0, 0.3], noiseModel.Diagonal.Sigmas([0.3, 0.2, 0.1]))
    v.insert_pose2(7, 1.1, 1.9, 0.25)
    return g, v, Ordering([7])


def pose2_chain(n=5, first_key=1, loop=False, robust=False, seed=3):
    """odometry chain with a prior on its first pose; robust: Huber around every between factor, values off the measurements"""
    rng = np.random.default_rng(seed)
    g, v = NonlinearFactorGraph(), Values()
    odo = noiseModel.Diagonal.Sigmas([0.2, 0.2, 0.1])
    if robust:
        odo = noiseModel.Robust.Create(noiseModel.mEstimator.Huber.Create(0.5), odo)
    g.add_PriorFactorPose2(first_key, [0.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    for i in range(n - 1):
        g.add_BetweenFactorPose2(first_key + i, first_key + i + 1, [2.0, 0.0, 0.1], odo)
    if loop:
        g.add_BetweenFactorPose2(first_key + n - 1, first_key, [-1.5, 0.4, -0.2], odo)
    for i in range(n):
        e = rng.normal(0, [0.3, 0.3, 0.1]) if robust else rng.normal(0, [0.05, 0.05, 0.02])
        v.insert_pose2(first_key + i, 2.0 * i + e[0], e[1], 0.1 * i + e[2])
    return g, v, Ordering(list(range(first_key, first_key + n)))


def forest():
    """two components: two roots, no path crosses from one to the other"""
    g, v, o = pose2_chain(4, first_key=1)
    g2, v2, o2 = pose2_chain(3, first_key=11, seed=5)
    for (ftype, _, gi, keys, meas, _, models) in g2.buckets():
        for k, m, mod in zip(keys.tolist(), meas, models):
            if len(k) == 1:
                g.add_PriorFactorPose2(k[0], m, mod)
            else:
                g.add_BetweenFactorPose2(k[0], k[1], m, mod)
    for k in o2:
        v.insert_pose2(k, *v2.at(k))
    return g, v, Ordering(list(o) + list(o2))


def dense_clique(n=4):
    """every pair of n poses tied: ONE front with n frontal variables (first / middle / last of it are queried)"""
    rng = np.random.default_rng(8)
    g, v = NonlinearFactorGraph(), Values()
    g.add_PriorFactorPose2(1, [0.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    pos = rng.normal(0, 2.0, (n, 3))
    for i in range(n):
        v.insert_pose2(1 + i, *pos[i])
        for j in range(i + 1, n):
            g.add_BetweenFactorPose2(1 + i, 1 + j, rng.normal(0, 1.0, 3), noiseModel.Diagonal.Sigmas([0.2, 0.3, 0.1]))
    return g, v, Ordering(list(range(1, n + 1)))


def _camera_ring(n_pose, n_pt, seed):
    rng = np.random.default_rng(seed)
    poses = [(rot3_expmap(rng.normal(0, 0.05, 3)), np.array([0.8 * i, 0.1 * rng.normal(), 0.0])) for i in range(n_pose)]
    pts = np.column_stack([rng.uniform(-1, 0.8 * n_pose, n_pt), rng.uniform(-1.5, 1.5, n_pt), rng.uniform(4.0, 7.0, n_pt)])
    return poses, pts


def _project(R, t, K, p):
    q = R.T @ (p - t)
    fx, fy, s, u0, v0 = K
    return np.array([fx * q[0] / q[2] + s * q[1] / q[2] + u0, fy * q[1] / q[2] + v0])


def projection(n_pose=3, n_pt=7, seed=1):
    """Pose3 + Point3 under GenericProjectionFactor<Pose3, Point3, Cal3_S2> (6 / 3), points first"""
    poses, pts = _camera_ring(n_pose, n_pt, seed)
    g, v = NonlinearFactorGraph(), Values()
    px = noiseModel.Isotropic.Sigma(2, 1.5)
    for i, (R, t) in enumerate(poses):
        v.insert_pose3(100 + i, R, t)
        g.add_PriorFactorPose3(100 + i, R, t, noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.05, 0.2, 0.2, 0.2]))
    for j, p in enumerate(pts):
        v.insert_point3(j, p)
        for i, (R, t) in enumerate(poses):
            if (i + j) % 3 != 2:
                g.add_GenericProjectionFactor(_project(R, t, K_S2, p), px, 100 + i, j, K_S2)
    g.add_PriorFactorPoint3(0, pts[0], noiseModel.Isotropic.Sigma(3, 0.5))
    return g, v, Ordering(list(range(n_pt)) + [100 + i for i in range(n_pose)])


def calibrated_sfm(n_pose=3, n_pt=6, seed=2):
    """GeneralSFMFactor2<Cal3_S2>: poses, points and ONE shared calibration (dimension 5), eliminated last"""
    poses, pts = _camera_ring(n_pose, n_pt, seed)
    g, v = NonlinearFactorGraph(), Values()
    px = noiseModel.Isotropic.Sigma(2, 1.0)
    v.insert_cal3_s2(500, *K_S2)
    g.add_PriorFactorCal3_S2(500, K_S2, noiseModel.Diagonal.Sigmas([20.0, 20.0, 0.5, 10.0, 10.0]))
    for i, (R, t) in enumerate(poses):
        v.insert_pose3(100 + i, R, t)
        g.add_PriorFactorPose3(100 + i, R, t, noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.05, 0.2, 0.2, 0.2]))
    for j, p in enumerate(pts):
        v.insert_point3(j, p)
        for i, (R, t) in enumerate(poses):
            g.add_GeneralSFMFactor2(_project(R, t, K_S2, p), px, 100 + i, j, 500)
    return g, v, Ordering(list(range(n_pt)) + [100 + i for i in range(n_pose)] + [500])


def vec9_chain(n=4):
    """the linear orientation graph of InitializePose3: VEC9 variables, chordal between factors, a prior on the anchor"""
    rng = np.random.default_rng(6)
    g, v = NonlinearFactorGraph(), Values()
    g.add_PriorFactorVec9(0, np.eye(3).reshape(9), noiseModel.Isotropic.Sigma(9, 0.1))
    for i in range(n):
        v.insert_vec9(i, rot3_expmap(rng.normal(0, 0.4, 3)).reshape(9))
    for i in range(n - 1):
        g.add_ChordalBetweenFactor(i, i + 1, rot3_expmap(rng.normal(0, 0.4, 3)), 1.0 + i)
    g.add_ChordalBetweenFactor(0, n - 1, rot3_expmap(rng.normal(0, 0.4, 3)), 0.7)
    return g, v, Ordering(list(range(n)))


def sphere_head_natural():
    """the first 300 poses of sphere2500 in natural order: the path of pose 0 crosses LDS fronts of 19 columns and more and the HBM fronts"""
    g, _ = load3D(os.path.join(GOLDEN, "sphere2500_head.txt"))
    v = chain_initial_pose3(g)
    g.add_PriorFactorPose3(0, np.eye(3), np.zeros(3), noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]))
    return g, v, Ordering.Natural(g)


def sphere_head_with_leaf():
    """the same with one more pose hung on pose 0 by a single odometry factor and eliminated first: its front has 13 columns (a
    register-size front, at most 16), its path then runs through the LDS fronts and the HBM fronts of the graph above.  (In natural order
    the smallest front of sphere2500's head alone has 19 columns.)"""
    g, v, o = sphere_head_natural()
    leaf = max(int(k) for k in o) + 1
    dR, dt = rot3_expmap(np.array([0.01, 0.02, -0.03])), np.array([0.3, -0.2, 0.1])
    R0, t0 = np.asarray(v.at(0)[:9]).reshape(3, 3), np.asarray(v.at(0)[9:12])
    v.insert_pose3(leaf, R0 @ dR, t0 + R0 @ dt)
    g.add_BetweenFactorPose3(0, leaf, dR, dt, noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.05, 0.1, 0.1, 0.1]))
    return g, v, Ordering([leaf] + list(o)), leaf


def pose3_chain(n):
    """Pose3 odometry in natural order: the path of pose 0 runs through every clique of the tree"""
    g, v = NonlinearFactorGraph(), Values()
    model = noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.05, 0.1, 0.1, 0.1])
    dR, dt = rot3_expmap(np.array([0.02, -0.01, 0.05])), np.array([1.0, 0.05, 0.0])
    R, t = np.eye(3), np.zeros(3)
    g.add_PriorFactorPose3(0, R, t, noiseModel.Diagonal.Sigmas([0.01, 0.01, 0.01, 0.02, 0.02, 0.02]))
    for i in range(n):
        v.insert_pose3(i, R, t)
        if i + 1 < n:
            g.add_BetweenFactorPose3(i, i + 1, dR, dt, model)
            R, t = R @ dR, t + R @ dt
    return g, v, Ordering(list(range(n)))


def gauge_freedom():
    """two poses, one odometry factor, no prior: the information matrix is singular (tests/test_gpu_marginals.py)"""
    g, v = NonlinearFactorGraph(), Values()
    g.add_BetweenFactorPose2(1, 2, [2.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([1.0, 1.0, 1.0]))
    v.insert_pose2(1, 0.0, 0.0, 0.0)
    v.insert_pose2(2, 2.0, 0.0, 0.0)
    return g, v, Ordering([1, 2])


# the structure-only checks walk these (name -> builder); the full-size shapes are built by the GPU test alone
SMALL = {
    "single": single_variable,
    "chain": pose2_chain,
    "loop": lambda: pose2_chain(6, loop=True),
    "forest": forest,
    "dense_clique": dense_clique,
    "projection": projection,
    "calibrated_sfm": calibrated_sfm,
    "vec9": vec9_chain,
    "pose3_chain": lambda: pose3_chain(12),
    "robust": lambda: pose2_chain(5, robust=True),
}
