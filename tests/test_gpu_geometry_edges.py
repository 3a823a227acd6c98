"""The HIP factor and retract kernels on the singular branches of the geometry (relative rotations at 0 and pi, the Expmap Taylor
switch, Pose2 angles at +-pi, the bearing / range guards, cheirality, Cal3Bundler's radial terms, the m-estimators at d = k), against
the 50-digit reference of tests/geometry_reference.py as stored in tests/golden/geometry_edges.npz.  Only the fixture is read here.

One graph per variable family and bucket size: every case is a factor on variables of its own, so a bucket evaluates its cases in
one launch; the bucket sizes 1, 64, 65 and 129 put the ragged tail on the wave and block edges of the 128-lane generic kernel (the
fixture repeats the cases with shifted translations up to 129 rows per factor type).  linearize() + jacobian(g) is the JAC = true
path, graph_error() the JAC = false one; both must give the fixture's error.

Tolerances: 16 x the floor of the quantity, the floor being the CPU oracle's own deviation from the 50-digit value over the case
table (measured by tests/test_geometry_reference.py, stored in the fixture; never below one ulp), relative to max(1, |expected|) per
case, and never above the project's 1e-9 (geometry_edges.tolerance)."""
import numpy as np
import pytest

import geometry_edges as ge
from gtsam_personal_amd import LevenbergMarquardtOptimizer, Ordering
from gtsam_personal_amd.graph import (CAM_BUNDLER, F_BEARING_RANGE_2D, F_BETWEEN_POSE2, F_BETWEEN_POSE3, F_PRIOR_CAM, F_PRIOR_POSE2,
                                      F_PRIOR_POSE3, F_PROJECTION, F_PROJECTION_BPS, F_SFM, F_SFM2, POSE2, POSE3)

pytestmark = pytest.mark.gpu

FAMILIES = {"pose3": (F_BETWEEN_POSE3, F_PRIOR_POSE3, F_PROJECTION, F_PROJECTION_BPS, F_SFM2),
            "camera": (F_SFM, F_PRIOR_CAM),
            "pose2": (F_BETWEEN_POSE2, F_PRIOR_POSE2, F_BEARING_RANGE_2D)}


@pytest.fixture(scope="module")
def fx():
    return ge.load()


def _optimizer(graph, values):
    return LevenbergMarquardtOptimizer(graph, values, Ordering.Natural(graph), device=0)


@pytest.mark.parametrize("n", ge.BUCKET_SIZES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_factor_edges(fx, family, n):
    graph, values, order = ge.build_factor_graph(fx, FAMILIES[family], n)
    opt = _optimizer(graph, values)
    opt.linearize()
    bad, half, expected, slack = [], 0.0, 0.0, 0.0
    for g, (ft, i) in enumerate(order):
        J = opt.jacobian(g)
        de, dH, derr = ge.factor_deviation(fx, ft, i, J)
        te = ge.tolerance(fx["floor_e"][ft, fx["f%d_mode" % ft][i]])
        tH, terr = ge.tolerance(fx["floor_H"][ft]), ge.tolerance(fx["floor_err"][ft])
        if not (de <= te and dH <= tH and derr <= terr):
            bad.append("type %d case %s: e %.3g (tol %.3g)  H %.3g (tol %.3g)  error %.3g (tol %.3g)"
                       % (ft, fx["f%d_name" % ft][i], de, te, dH, tH, derr, terr))
        half += 0.5 * float(J[:, -1] @ J[:, -1])
        expected += fx["f%d_err" % ft][i]
        slack += terr * max(1.0, fx["f%d_err" % ft][i])
    assert not bad, "\n".join(bad)
    err = opt.graph_error()
    assert abs(err - expected) <= slack, (err, expected, slack)
    assert abs(err - half) <= slack, (err, half, slack)


@pytest.mark.parametrize("kind", range(1, 9))
def test_robust_edges(fx, kind):
    """d in {0, 0.99 k, k, 1.01 k, 10 k} through lmgpu_add_factor_bucket_robust: [A b] = sqrt(weight) [I -e], error = sum of the losses"""
    graph, values, rows = ge.build_robust_graph(fx, kind)
    opt = _optimizer(graph, values)
    opt.linearize()
    tol = ge.tolerance(fx["floor_rb"][0])
    for g, i in enumerate(rows):
        J = opt.jacobian(g)
        assert np.all(np.isfinite(J)), (kind, fx["b_d"][i])
        assert ge._dev(J, fx["b_J"][i].reshape(3, 4)) <= tol, (kind, fx["b_d"][i], J, fx["b_J"][i])
    err, expected = opt.graph_error(), float(fx["b_loss"][rows].sum())
    assert np.isfinite(err)
    assert abs(err - expected) <= ge.tolerance(fx["floor_rb"][1]) * max(1.0, expected), (kind, err, expected)


@pytest.mark.parametrize("vt", (POSE2, POSE3, CAM_BUNDLER))
def test_retract_edges(fx, vt):
    """|w|^2 at 0, either side of the Taylor switch 1e-5, pi^2, (2 pi)^2 and 40; Pose2 d_theta at +-pi and 2 pi"""
    graph, values, delta = ge.build_retract_graph(fx, vt)
    opt = _optimizer(graph, values)
    opt.retract(np.concatenate([delta[k] for k in opt.ordering]))
    got, tol, bad = opt.values(), ge.tolerance(fx["floor_x"][vt]), []
    for k, exp in enumerate(fx["r%d_exp" % vt]):
        d, ortho = ge.retract_deviation(vt, got.at(k), exp)
        if not (d <= tol and ortho <= ge.ORTHO_TOL):
            bad.append("case %s: value %.3g (tol %.3g)  R^T R - I %.3g (tol %.3g)" % (fx["r%d_name" % vt][k], d, tol, ortho, ge.ORTHO_TOL))
    assert not bad, "\n".join(bad)
