"""CPU checks of the GNC feature: the plain-Python restatement (tests/gnc_restatement.py) pinned to the reference's own known answers
(tests/testGncOptimizer.cpp, each with its line), lmgpu_chi2inv through ctypes (host code), the exported C ABI and the Python
parameter objects.  No device needed."""
import ctypes as ct
import os

import numpy as np
import pytest

import gnc_cases as gc
import gnc_restatement as gr
import oracle_harness as oh
from gtsam_personal_amd import (GaussNewtonParams, GncGaussNewtonParams, GncLMParams, GncLossType, GncOptimizer, LevenbergMarquardtParams,
                                NonlinearFactorGraph, Ordering, X, noiseModel)
from gtsam_personal_amd.graph import VAR_STORE

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gtsam_personal_amd", "liblmgpu.so")
ORD = [X(1)]


def test_chi2inv():
    """testGncOptimizer.cpp:634-637 (MATLAB: chi2inv(0.997, 1), chi2inv(0.997, 3)); the library's host implementation to 1e-9"""
    assert abs(gr.chi2inv(0.997, 1) - 8.807468393511950) < 1e-9
    assert abs(gr.chi2inv(0.997, 3) - 13.931422665512077) < 1e-9
    lib = ct.CDLL(LIB)
    lib.lmgpu_chi2inv.restype = ct.c_double
    lib.lmgpu_chi2inv.argtypes = [ct.c_double, ct.c_int32]
    assert abs(lib.lmgpu_chi2inv(0.997, 1) - 8.807468393511950) < 1e-9
    assert abs(lib.lmgpu_chi2inv(0.997, 3) - 13.931422665512077) < 1e-9
    assert abs(GncOptimizer.Chi2inv(0.997, 1) - 8.807468393511950) < 1e-9
    for alpha in (0.5, 0.9, 0.99, 0.999):
        for d in (1, 2, 3, 6, 9):
            assert abs(lib.lmgpu_chi2inv(alpha, d) - gr.chi2inv(alpha, d)) < 1e-9 * gr.chi2inv(alpha, d)


def test_default_thresholds():
    """:663-680: 0.5 * chi2inv(0.99, dim) = 5.672433365072185 / 4.605170185988091 / 3.317448300510607 for 3 / 2 / 1 rows, to 1e-3"""
    assert np.allclose(gr.default_thresholds(gc.toy_graph()), 5.672433365072185, atol=1e-3)
    assert abs(0.5 * gr.chi2inv(0.99, 2) - 4.605170185988091) < 1e-3
    assert abs(0.5 * gr.chi2inv(0.99, 1) - 3.317448300510607) < 1e-3


def test_toy_graph_errors_and_gm_weights():
    """:352-385: the outlier's error is 50; GM weights at mu 1, barcSq 1 -> (1/51)^2, at mu 2, barcSq 5 -> (10/60)^2"""
    g = gc.toy_graph()
    r = gr.factor_errors(g, gc.point_values([0, 0, 0]), ORD)
    assert np.allclose(r, [0, 0, 0, 50.0], atol=1e-9)
    w = gr.calculate_weights(r, np.full(4, 1.0), 1.0, gr.GM)
    assert np.allclose(w, [1, 1, 1, (1.0 / 51.0) ** 2], atol=1e-9)
    w = gr.calculate_weights(r, np.full(4, 5.0), 2.0, gr.GM)
    assert np.allclose(w, [1, 1, 1, (10.0 / 60.0) ** 2], atol=1e-9)


def test_toy_graph_tls_weights():
    """:388-409: TLS at mu 1 -> [1, 1, 1, 0] (threshold = the reference's 2-dof default)"""
    r = gr.factor_errors(gc.toy_graph(), gc.point_values([0, 0, 0]), ORD)
    assert np.allclose(gr.calculate_weights(r, np.full(4, gc.B2), 1.0, gr.TLS), [1, 1, 1, 0], atol=1e-9)


def tls2_graph():
    g = NonlinearFactorGraph()
    g.add_PriorFactorPoint3(X(1), [1.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([1.0, 1.0, 1.0]))
    return g


@pytest.mark.parametrize("barc,expected,tol", [(0.51, 1.0, 1e-9), (0.49, 0.0, 1e-9), (0.5, 0.5, 1e-5)])
def test_tls2_threshold_cases(barc, expected, tol):
    """:412-478: one factor of error 0.5, mu 1e6: inlier / outlier / undecided"""
    r = gr.factor_errors(tls2_graph(), gc.point_values([0, 0, 0]), ORD)
    assert abs(r[0] - 0.5) < 1e-12
    assert abs(gr.calculate_weights(r, [barc], 1e6, gr.TLS)[0] - expected) < tol


def test_initialize_and_update_mu():
    """:174-263: GM mu_init = 2 * rmax / barcSq = 100 / barcSq; TLS barcSq / (2 rmax - barcSq); updateMu; a graph without outliers: -1"""
    r = gr.factor_errors(gc.toy_graph(), gc.point_values([0, 0, 0]), ORD)
    b = np.full(4, gc.B2)
    assert abs(gr.initialize_mu(r, b, gr.GM) - 2 * 50.0 / gc.B2) < 1e-9
    assert abs(gr.initialize_mu(r, b, gr.TLS) - gc.B2 / (100.0 - gc.B2)) < 1e-12
    assert gr.initialize_mu(np.zeros(4), b, gr.TLS) == -1.0
    assert gr.initialize_mu(np.array([1e9]), [1.0], gr.TLS) == 1e-6
    assert gr.update_mu(5.0, gr.GM, 1.4) == 5.0 / 1.4 and gr.update_mu(1.2, gr.GM, 1.4) == 1.0 and gr.update_mu(5.0, gr.TLS, 1.4) == 7.0


def test_convergence_checks():
    """:266-350: cost (relative 1e-5), weights (TLS, binary to 1e-4), mu (GM, 1)"""
    assert gr.check_cost(1.0, 1.0 + 1e-6, 1e-5) and not gr.check_cost(1.0, 1.1, 1e-5)
    assert gr.check_weights(np.array([1, 0, 1.0]), gr.TLS, 1e-4) and not gr.check_weights(np.array([1, 0.5, 1.0]), gr.TLS, 1e-4)
    assert not gr.check_weights(np.array([1, 0, 1.0]), gr.GM, 1e-4)
    assert gr.check_mu(1.0, gr.GM) and not gr.check_mu(1.1, gr.GM) and not gr.check_mu(1.0, gr.TLS)
    assert gr.check_convergence(2.0, np.array([0.5]), 1.0, 1.0, gr.TLS, 1e-5, 1e-4)


def test_optimize_toy():
    """:529-560: Gauss-Newton with the Geman-McClure loss stays near the mean of the four priors -- without the loss it IS the mean
    (0.25, 0, 0); GNC with a GN base and TLS reaches (0, 0, 0) to 1e-3"""
    g, p0 = gc.toy_graph(robust=False), gc.point_values([3, 3, 0])
    orc = oh.OracleProblem(g, p0, ORD)
    gn = GaussNewtonParams()
    orc.lm_init(gn)
    orc.gn_optimize(gn)
    assert np.allclose(orc.values()[X(1)], [0.25, 0, 0], atol=1e-9)
    res = gr.gnc_optimize(gc.toy_graph(), p0, ORD, "GN", gn, loss=gr.TLS, barc=np.full(4, gc.B2))
    assert np.allclose(res["values"][X(1)], [0, 0, 0], atol=1e-3)
    assert np.allclose(res["weights"], [1, 1, 1, 0], atol=1e-3)


@pytest.mark.parametrize("loss", [gr.GM, gr.TLS])
def test_optimize_toy_known_inliers(loss):
    """:563-632: known inliers {0, 1, 2}, initial (1, 0): GM with threshold 1 and TLS with the default threshold reach (0, 0, 0) to 1e-3
    with the three known weights at 1 (TLS: the fourth at 0); with threshold 100 all are inliers and the result is the mean (0.25, 0, 0)"""
    g, p0, gn = gc.toy_graph(), gc.point_values([1, 0, 0]), GaussNewtonParams()
    res = gr.gnc_optimize(g, p0, ORD, "GN", gn, loss=loss, known_in=[0, 1, 2], barc=np.full(4, 1.0 if loss == gr.GM else gc.B2))
    assert np.allclose(res["values"][X(1)], [0, 0, 0], atol=1e-3)
    assert np.allclose(res["weights"][:3], [1, 1, 1], atol=1e-9)
    if loss == gr.TLS:
        assert abs(res["weights"][3]) < 1e-9
    res = gr.gnc_optimize(g, p0, ORD, "GN", gn, loss=gr.TLS, known_in=[0, 1, 2], barc=np.full(4, 100.0))
    assert np.allclose(res["weights"], [1, 1, 1, 1], atol=1e-9)
    assert np.allclose(res["values"][X(1)], [0.25, 0, 0], atol=1e-3)


# (known inliers, known outliers, loss, initial weights): the blocks of knownInliersAndOutliers (:776-863) and setWeights (:866-944); all
# with setInlierCostThresholds(1.0), initial (1, 0), GN base; expected result (0, 0) to 1e-3 and final weights [1, 1, 1, 0]
TOY_KNOWN_AND_WEIGHTS = [
    ([0, 1, 2], [3], gr.GM, None),           # :785-811 everything known: early exit
    ([2, 0], [3], gr.GM, None),              # :814-839
    ([], [3], gr.GM, None),                  # :842-862
    ([], [], gr.TLS, [0.5, 0.5, 0.5, 0.5]),  # :873-891
    ([], [], gr.TLS, [0.0, 0.0, 1.0, 1.0]),  # :893-914 bad initialization: the outlier as inlier
    ([2, 0], [3], gr.TLS, [0.5, 0.5, 0.5, 0.5]),  # :916-943
]


@pytest.mark.parametrize("kin,kout,loss,w0", TOY_KNOWN_AND_WEIGHTS)
def test_optimize_toy_known_inliers_and_outliers_and_set_weights(kin, kout, loss, w0):
    """:776-944 on the restatement.  Weight tolerances as there: 1e-9 (`tol`), 1e-5 for the one free weight of a GM run.  The first block
    is the early exit 'all measurements are known' (GncOptimizer.h:196-215): no outer iteration, the weights stay the initial ones"""
    res = gr.gnc_optimize(gc.toy_graph(), gc.point_values([1, 0, 0]), ORD, "GN", GaussNewtonParams(), loss=loss, known_in=kin, known_out=kout,
                          barc=np.full(4, 1.0), weights=w0)
    assert np.allclose(res["values"][X(1)], [0, 0, 0], atol=1e-3)
    assert np.allclose(res["weights"], [1, 1, 1, 0], atol=1e-5 if loss == gr.GM else 1e-9)
    if len(kin) + len(kout) == 4:
        assert (res["stop"], res["iterations"]) == (5, 0)
    else:
        assert res["stop"] in (1, 2, 3)


def test_known_outlier_with_large_threshold():
    """only the outlier known, threshold 100: the three free factors are inliers, the known outlier keeps weight 0"""
    res = gr.gnc_optimize(gc.toy_graph(), gc.point_values([3, 3, 0]), ORD, "GN", GaussNewtonParams(), loss=gr.TLS, known_out=[3],
                          barc=np.full(4, 100.0))
    assert np.allclose(res["weights"], [1, 1, 1, 0], atol=1e-9) and np.allclose(res["values"][X(1)], [0, 0, 0], atol=1e-3)


def inlier_only_graph():
    g = NonlinearFactorGraph()
    for _ in range(3):
        g.add_PriorFactorPoint3(X(1), [0.0, 0.0, 0.0], noiseModel.Isotropic.Sigma(3, 0.1))
    return g


def test_small_residuals_stop_at_initialisation():
    """GncOptimizer.h:192-215 with initializeMu's -1 (:298-307): every residual at the initial values is below its threshold, TLS needs no
    robustification: no outer iteration, the result is the first base optimizer run's, weights 1"""
    res = gr.gnc_optimize(inlier_only_graph(), gc.point_values([0.01, 0, 0]), ORD, "GN", GaussNewtonParams(), loss=gr.TLS)
    assert (res["stop"], res["iterations"], res["mu"]) == (4, 0, -1.0)
    assert np.allclose(res["values"][X(1)], [0, 0, 0], atol=1e-9) and np.allclose(res["weights"], 1.0)


def test_gn_max_iterations_zero_returns_initial():
    """solverParameterParsing :102-123: a base optimizer that may not iterate returns the initial values"""
    gn = GaussNewtonParams()
    gn.maxIterations = 0
    res = gr.gnc_optimize(gc.toy_graph(), gc.point_values([3, 3, 0]), ORD, "GN", gn, loss=gr.TLS, barc=np.full(4, gc.B2))
    assert np.allclose(res["values"][X(1)][:3], [3, 3, 0])


def _lm_values(graph, initial, ordering):
    orc = oh.OracleProblem(graph, initial, ordering)
    p = LevenbergMarquardtParams()
    orc.lm_init(p)
    orc.lm_optimize(p)
    return orc.values()


def _max_diff(a, b):
    return max(float(np.abs(a[k] - b[k]).max()) for k in a)


SMALL_POSE_GRAPH_CASES = [("GN", gr.TLS), ("LM", gr.TLS), ("GN", gr.GM), ("LM", gr.GM)]


def small_pose_graph_restatement(base, loss, pair=None, eps=0.0):
    graph, initial, ordering = gc.w100_case(base, loss) if pair is None else gc.w100(True, pair)
    if eps:
        initial = gc.perturbed(initial, eps)
    bp = GaussNewtonParams() if base == "GN" else LevenbergMarquardtParams()
    return gr.gnc_optimize(graph, initial, ordering, base, bp, loss=loss)


def _outcome_shift(a, b):
    """(same discrete outcome, largest weight difference, largest value difference) of two runs"""
    return ((a["iterations"], a["stop"]) == (b["iterations"], b["stop"]), float(np.abs(a["weights"] - b["weights"]).max()),
            _max_diff(a["values"], b["values"]))


@pytest.mark.parametrize("base,loss", SMALL_POSE_GRAPH_CASES)
def test_optimize_small_pose_graph(base, loss):
    """:737-773: GNC with a Gauss-Newton base and default parameters (TLS) on w100 + one outlier equals LM on the outlier-free graph to
    1e-3 per coordinate, and LM with the outlier does not.  That is the reference's own case and criterion; the restatement of the other
    three combinations does NOT meet it (measured distance to the clean LM solution: GN/GM 1.8e-3 after 30 outer iterations, LM/GM 15.3
    -- its cost test stops the loop in outer iteration 0, mu = 21221; LM/TLS ends with every weight at 1), so for them only the device-
    versus-restatement comparison of tests/test_gpu_gnc.py applies.
    For all four the input must make the outcome comparable between two implementations:
      * every convergence test of every outer iteration is at least 1e-3 (relative) away from flipping, and
      * the run is not chaotic: initial values perturbed by 1e-10 (the agreement of the per-factor errors the project asks of two
        implementations) give the same outer iteration count and stop reason, and weights and values within 1e-7, a tenth of the 1e-6
        the device comparison allows.
    Of the four only GN / TLS and GN / GM actually reject the outlier on w100; with an LM base rejection is exercised by the synthetic
    BAL case (test_bal_outlier_classification_restatement and its device counterpart).  None of the stable wrong loop closures tried
    for LM / TLS ((10, 60), (20, 70), (5, 95), (99, 0), (50, 52)) ends with the outlier rejected.
    An input that misses either is changed, not the tolerance: gnc_cases.W100_OUTLIER_OF_CASE (see test_reference_outlier_is_chaotic_...)."""
    graph, initial, ordering = gc.w100_case(base, loss)
    g0, _, _ = gc.w100(outlier=False)
    expected = _lm_values(g0, initial, ordering)
    assert _max_diff(expected, _lm_values(graph, initial, ordering)) > 1e-3
    res = small_pose_graph_restatement(base, loss)
    print(base, loss, "distance to clean LM", _max_diff(expected, res["values"]), "outer iterations", res["iterations"], "stop", res["stop"])
    if (base, loss) == ("GN", gr.TLS):
        assert _max_diff(expected, res["values"]) < 1e-3
        assert res["weights"][-1] < 0.5 and (res["weights"][:-1] > 0.5).all()
    else:  # the facts that keep the criterion from being asserted: if one of them changes, this test says so
        assert _max_diff(expected, res["values"]) > 1e-3
        if (base, loss) == ("GN", gr.GM):
            assert _max_diff(expected, res["values"]) < 3e-3 and (res["iterations"], res["stop"]) == (30, 3)
        if (base, loss) == ("LM", gr.GM):
            assert (res["iterations"], res["stop"]) == (0, 1) and res["mu"] > 1e4  # the cost test ends the loop in outer iteration 0
        if (base, loss) == ("LM", gr.TLS):
            assert res["stop"] == 2 and (res["weights"] == 1.0).all()  # ends with every weight at 1: the outlier is NOT rejected
    assert min(min(m) for m in res["margins"]) >= 1e-3, res["margins"]
    same, dw, dv = _outcome_shift(res, small_pose_graph_restatement(base, loss, eps=1e-10))
    print("   shift under a 1e-10 perturbation: same outcome", same, "weights", dw, "values", dv)
    assert same and dw <= 1e-7 and dv <= 1e-7, (same, dw, dv)


def test_reference_outlier_is_chaotic_under_lm_tls():
    """why the LM / TLS case does not use the reference's outlier (90, 50): there a perturbation of the initial values by 1e-13 already
    changes the restatement's own discrete outcome or moves its result by far more than 1e-6 (measured: 29 -> 28 outer iterations,
    weights by 1.0, values by 15.2)"""
    a = small_pose_graph_restatement("LM", gr.TLS, pair=gc.W100_OUTLIER)
    b = small_pose_graph_restatement("LM", gr.TLS, pair=gc.W100_OUTLIER, eps=1e-13)
    same, dw, dv = _outcome_shift(a, b)
    print("same outcome", same, "weights", dw, "values", dv)
    assert not same or dw > 1e-6 or dv > 1e-6


def test_bal_outlier_classification_restatement():
    """the synthetic BAL graph with displaced measurements, LM base, TLS: the restatement itself separates displaced from untouched
    measurements except for at most 1 % of the factors"""
    graph, initial, ordering, displaced = gc.bal_with_outliers()
    res = gr.gnc_optimize(graph, initial, ordering, "LM", LevenbergMarquardtParams(), loss=gr.TLS)
    wrong = int(((res["weights"] < 0.5) != displaced).sum())
    assert displaced.sum() > 0.02 * graph.size()
    assert wrong <= 0.01 * graph.size(), (wrong, graph.size())
    assert min(min(m) for m in res["margins"]) >= 1e-3, res["margins"]


def test_gnc_symbols_exported():
    lib = ct.CDLL(LIB)
    for name in ("lmgpu_chi2inv", "lmgpu_gnc_enable", "lmgpu_gnc_set_inlier_cost_thresholds", "lmgpu_gnc_set_known", "lmgpu_gnc_set_weights",
                 "lmgpu_gnc_get_weights", "lmgpu_gnc_get_inlier_cost_thresholds", "lmgpu_gnc_initialize_mu", "lmgpu_gnc_calculate_weights",
                 "lmgpu_gnc_optimize", "lmgpu_gnc_get_trace"):
        assert hasattr(lib, name), name


def test_python_parameter_defaults():
    """GncParams.h:69-73"""
    for cls, base in ((GncLMParams, LevenbergMarquardtParams), (GncGaussNewtonParams, GaussNewtonParams)):
        p = cls()
        assert (p.lossType, p.maxIterations, p.muStep, p.relativeCostTol, p.weightsTol) == (GncLossType.TLS, 100, 1.4, 1e-5, 1e-4)
        assert p.knownInliers == [] and p.knownOutliers == [] and isinstance(p.baseOptimizerParams, base)
    p = GncLMParams()
    p.setKnownInliers([2, 0])  # GncParams.h:122-138: append and sort; both lists on one object as testGncOptimizer.cpp:795-796
    p.setKnownOutliers([3])
    p.setKnownInliers([1])
    assert p.knownInliers == [0, 1, 2] and p.knownOutliers == [3]


def test_constructor_checks_raise_before_any_handle():
    """GncOptimizer.h:75-99: raised before the library is asked for a device"""
    g, p0 = gc.toy_graph(), gc.point_values([3, 3, 0])
    p = GncGaussNewtonParams()
    p.knownInliers, p.knownOutliers = [0, 1], [1, 3]
    with pytest.raises(RuntimeError, match="BOTH"):
        GncOptimizer(g, p0, p, ORD)
    p.knownInliers, p.knownOutliers = [4], []
    with pytest.raises(RuntimeError, match="known inliers"):
        GncOptimizer(g, p0, p, ORD)
    p.knownInliers, p.knownOutliers = [], [7]
    with pytest.raises(RuntimeError, match="known outliers"):
        GncOptimizer(g, p0, p, ORD)
