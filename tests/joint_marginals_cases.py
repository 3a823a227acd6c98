"""Small graphs for the cross-covariance walk (csrc/kernels_marginals.hpp, marginal_cross_kernel) beside those of
tests/marginals_path_cases.py: trees that BRANCH, which a chain in natural order never does.  Each returns (graph, values, ordering)."""
from gtsam_personal_amd import NonlinearFactorGraph, Ordering, Values, noiseModel


def pose2_comb():
    """Pose2 tree 1 - 2 - 3 - 5 - 6 with 7 hung on 3 and 4 hung on 5, a prior on 6, eliminated in the order 1 2 7 3 4 5 6 (no fill: the
    Bayes tree is the graph).  From pose 1 the junctions lie at three depths: with 2 and 3 on its own path, with 7 at the front of 3,
    with 4 at the root; the path of 1 (15 scalars) is longer than that of 4 (9) and of 7 (12)."""
    g, v = NonlinearFactorGraph(), Values()
    odo = noiseModel.Diagonal.Sigmas([0.2, 0.25, 0.1])
    g.add_PriorFactorPose2(6, [6.0, 0.6, 0.3], noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    for a, b, dx in ((1, 2, 1.0), (2, 3, 1.1), (7, 3, 0.7), (3, 5, 0.9), (4, 5, 1.3), (5, 6, 1.0)):
        g.add_BetweenFactorPose2(a, b, [dx, 0.05 * a, 0.1 - 0.02 * b], odo)
    for k in range(1, 8):
        v.insert_pose2(k, 1.0 * k, 0.1 * k * (-1) ** k, 0.05 * k)
    return g, v, Ordering([1, 2, 7, 3, 4, 5, 6])
