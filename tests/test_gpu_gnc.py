"""Device checks of the GNC feature through the public interface, against the plain-Python restatement (tests/gnc_restatement.py, which
rebuilds a weighted graph per outer iteration and runs the frozen CPU oracle on it)."""
import ctypes as ct

import numpy as np
import pytest

import gnc_cases as gc
import gnc_restatement as gr
import oracle_harness as oh
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, GaussNewtonParams, GncGaussNewtonParams, GncLMParams, GncLossType,
                                GncOptimizer, LevenbergMarquardtOptimizer, LevenbergMarquardtParams, NonlinearFactorGraph, PCGSolverParameters, X,
                                _lib)
from test_gnc_reference import SMALL_POSE_GRAPH_CASES, TOY_KNOWN_AND_WEIGHTS, inlier_only_graph, small_pose_graph_restatement, tls2_graph

pytestmark = pytest.mark.gpu
ORD = [X(1)]


def _gnc(graph, initial, ordering, base="GN", loss=gr.TLS, known_in=(), known_out=(), base_params=None):
    p = GncGaussNewtonParams(base_params) if base == "GN" else GncLMParams(base_params)
    p.setLossType(loss)
    p.setKnownInliers(known_in)
    p.setKnownOutliers(known_out)
    return GncOptimizer(graph, initial, p, ordering)


def _vals_dict(values):
    return {k: values.at(k) for k in values.keys()}


def _max_diff(a, b):
    return max(float(np.abs(np.asarray(a[k])[:len(b[k])] - b[k][:len(a[k])]).max()) for k in a)


# ---------------------------------------------------------------- 1. kernel level
def _kernel_level(graph, initial, ordering, known_in, known_out, barc):
    n = graph.size()
    exists = [r is not None for r in gr.records(graph)]
    r = gr.factor_errors(graph, initial, ordering)
    for loss in (gr.GM, gr.TLS):
        gnc = _gnc(graph, initial, ordering, "LM", loss, known_in, known_out)
        gnc.setInlierCostThresholds(barc)
        assert np.array_equal(gnc.getInlierCostThresholds()[exists], np.asarray(barc)[exists])
        mu_d, mu_r = gnc.initializeMu(), gr.initialize_mu(r, barc, loss, exists)
        print("loss", loss, "mu device", mu_d, "restatement", mu_r)
        assert abs(mu_d - mu_r) <= 1e-9 * abs(mu_r)
        for mu in (mu_r, 3.7 * mu_r, 0.31 * mu_r + 0.05):
            w_d = gnc.calculateWeights(initial, mu)
            w_r = gr.calculate_weights(r, barc, mu, loss, known_in, known_out, exists)
            print("   mu", mu, "max weight difference", np.abs(w_d - w_r).max())
            assert w_d.shape == (n,) and np.abs(w_d - w_r).max() <= 1e-9
        gnc.close()


def test_kernels_w100():
    """initializeMu and calculateWeights on w100 + outlier: per-factor thresholds, known inliers and outliers, factors with r = 0 (a
    duplicate prior the initial values satisfy exactly) and an empty graph slot at the end (resize)"""
    graph, initial, ordering = gc.w100(outlier=True)
    graph.add_PriorFactorPose2(0, initial.at(0), gc.noiseModel.Diagonal.Sigmas([0.01, 0.01, 0.01]))  # r = 0 at the initial values
    graph.resize(graph.size() + 1)
    n = graph.size()
    rng = np.random.default_rng(3)
    barc = rng.uniform(0.5, 8.0, n)
    _kernel_level(graph, initial, ordering, [1, 5, 17], [2, 40], barc)


def test_kernels_bal():
    """the same on the synthetic BAL graph with displaced measurements (seed, share and displacement: gnc_cases)"""
    graph, initial, ordering, _ = gc.bal_with_outliers()
    rng = np.random.default_rng(4)
    _kernel_level(graph, initial, ordering, [0, 9, 100], [3, 77, 500], rng.uniform(0.5, 8.0, graph.size()))


# ---------------------------------------------------------------- 2. the weighted graph in linearize / error / solve / iterate
@pytest.mark.parametrize("case", ["w100", "bal"])
def test_weighted_graph_parity(case):
    """with weights from setWeights (random in [0, 1], some exactly 0 and 1): error to 1e-10 relative, hessianDiagonal / solve / one LM
    iterate at test_gpu_parity.py's tolerances, and for DIAG and UNIT buckets every factor's [A b] to 1e-9 -- against the oracle on
    the weighted graph the restatement builds"""
    if case == "w100":
        graph, initial, ordering = gc.w100(outlier=True)
    else:
        graph, initial, ordering, _ = gc.bal_with_outliers()
    n = graph.size()
    rng = np.random.default_rng(11)
    w = rng.uniform(0, 1, n)
    w[rng.choice(n, n // 10, replace=False)] = 1.0
    zero = rng.choice(np.arange(1, n - 2), 3, replace=False)  # a few removed factors (every variable keeps other factors)
    w[zero] = 0.0
    gnc = _gnc(graph, initial, ordering, "LM")
    gnc.setWeights(w)
    assert np.array_equal(gnc.getWeights(), w)
    opt = gnc.base()
    gw, _ = gr.weighted_graph(graph, w)
    orc = oh.OracleProblem(gw, initial, ordering)
    e_d, e_o = opt.graph_error(), orc.error()
    print("error device", e_d, "oracle", e_o)
    assert abs(e_d - e_o) <= 1e-10 * abs(e_o)
    opt.linearize()
    orc.linearize()
    for i in range(n):
        assert np.allclose(opt.jacobian(i), orc.jacobian(i), rtol=1e-9, atol=1e-9), i
    hd, ho = opt.hessian_diagonal(), orc.hessian_diagonal()
    for k in ho:
        assert np.allclose(hd[k], ho[k], rtol=1e-9, atol=1e-9)
    dk, _, l0, l1 = opt.solve(1e-3)
    rc, do, o0, o1 = orc.solve(1e-3)
    assert rc == 0
    num = np.sqrt(sum(float(((dk[k] - do[k]) ** 2).sum()) for k in do))
    den = np.sqrt(sum(float((do[k] ** 2).sum()) for k in do))
    print("solve relative difference", num / den)
    assert num <= 1e-8 * den
    assert abs(l0 - o0) <= 1e-9 * abs(o0) and abs(l1 - o1) <= 1e-8 * abs(o1) + 1e-12
    params = LevenbergMarquardtParams()
    cp = params._c()
    opt._check(opt.lib.lmgpu_lm_init(opt._h, ct.byref(cp), ct.byref(opt.state)))
    opt.iterate()
    orc.lm_init(params)
    orc.lm_iterate(params)
    st = orc.lm_state()
    assert abs(opt.error() - st["error"]) <= 1e-6 * abs(st["error"]) and opt.lambda_() == st["lambda_"]
    assert _max_diff(_vals_dict(opt.values()), orc.values()) <= 1e-6
    gnc.close()


# ---------------------------------------------------------------- 3. the toy-graph known answers on the device
def test_toy_known_answers():
    """testGncOptimizer.cpp:352-478, :529-632, :776-945 through GncOptimizer on the device (PriorFactor<Point3>, third coordinate 0)"""
    g, at0 = gc.toy_graph(), gc.point_values([0, 0, 0])
    gnc = _gnc(g, at0, ORD, "GN", gr.GM)
    assert np.allclose(gnc.getInlierCostThresholds(), 5.672433365072185, atol=1e-3)  # :663-680
    assert abs(gnc.base().graph_error() - 50.0) < 1e-9  # Robust stripped, weights 1
    gnc.setInlierCostThresholds(1.0)
    assert np.allclose(gnc.calculateWeights(at0, 1.0), [1, 1, 1, (1 / 51.0) ** 2], atol=1e-9)
    gnc.setInlierCostThresholds(5.0)
    assert np.allclose(gnc.calculateWeights(at0, 2.0), [1, 1, 1, (10 / 60.0) ** 2], atol=1e-9)
    assert abs(gnc.initializeMu() - 2 * 50.0 / 5.0) < 1e-9
    gnc.close()
    gnc = _gnc(g, at0, ORD, "GN", gr.TLS)
    gnc.setInlierCostThresholds(gc.B2)
    assert np.allclose(gnc.calculateWeights(at0, 1.0), [1, 1, 1, 0], atol=1e-9)
    assert abs(gnc.initializeMu() - gc.B2 / (100.0 - gc.B2)) < 1e-12
    assert gnc.checkConvergence(2.0, np.array([0.5]), 1.0, 1.0) and not gnc.checkWeightsConvergence(np.array([1, 0.5]))
    assert gnc.updateMu(5.0) == 7.0 and not gnc.checkMuConvergence(1.0)
    gnc.close()
    for barc, expected, tol in ((0.51, 1.0, 1e-9), (0.49, 0.0, 1e-9), (0.5, 0.5, 1e-5)):
        gnc = _gnc(tls2_graph(), at0, ORD, "GN", gr.TLS)
        gnc.setInlierCostThresholds(barc)
        assert abs(gnc.calculateWeights(at0, 1e6)[0] - expected) < tol
        gnc.close()
    p0 = gc.point_values([3, 3, 0])
    gnc = _gnc(g, p0, ORD, "GN", gr.TLS)
    gnc.setInlierCostThresholds(gc.B2)
    assert np.allclose(gnc.optimize().at(X(1)), [0, 0, 0], atol=1e-3)
    assert np.allclose(gnc.getWeights(), [1, 1, 1, 0], atol=1e-3)
    gnc.close()
    p1 = gc.point_values([1, 0, 0])
    gnc = _gnc(g, p1, ORD, "GN", gr.GM, known_in=[0, 1, 2])
    gnc.setInlierCostThresholds(1.0)
    assert np.allclose(gnc.optimize().at(X(1)), [0, 0, 0], atol=1e-3) and np.allclose(gnc.getWeights()[:3], 1.0, atol=1e-9)
    gnc.close()
    gnc = _gnc(g, p1, ORD, "GN", gr.TLS, known_in=[0, 1, 2])
    gnc.setInlierCostThresholds(gc.B2)
    assert np.allclose(gnc.optimize().at(X(1)), [0, 0, 0], atol=1e-3) and np.allclose(gnc.getWeights(), [1, 1, 1, 0], atol=1e-9)
    gnc.setInlierCostThresholds(100.0)
    gnc.setWeights(np.ones(4))
    assert np.allclose(gnc.optimize().at(X(1)), [0.25, 0, 0], atol=1e-3) and np.allclose(gnc.getWeights(), [1, 1, 1, 1], atol=1e-9)
    gnc.close()
    gnc = _gnc(g, p0, ORD, "GN", gr.TLS, known_out=[3])
    gnc.setInlierCostThresholds(100.0)
    assert np.allclose(gnc.optimize().at(X(1)), [0, 0, 0], atol=1e-3) and np.allclose(gnc.getWeights(), [1, 1, 1, 0], atol=1e-9)
    gnc.close()
    gnc = _gnc(g, p0, ORD, "GN", gr.TLS)
    gnc.setInlierCostThresholds(gc.B2)
    gnc.setWeights([1, 1, 1, 0])
    assert np.allclose(gnc.optimize().at(X(1)), [0, 0, 0], atol=1e-3) and np.allclose(gnc.getWeights(), [1, 1, 1, 0], atol=1e-3)
    gnc.close()
    gn = GaussNewtonParams()
    gn.maxIterations = 0  # solverParameterParsing :102-123: the initial values and their error come back
    gnc = _gnc(g, p0, ORD, "GN", gr.TLS, base_params=gn)
    assert np.allclose(gnc.optimize().at(X(1)), [3, 3, 0]) and gnc.base().iterations() == 0
    gnc.close()


@pytest.mark.parametrize("kin,kout,loss,w0", TOY_KNOWN_AND_WEIGHTS)
def test_toy_known_inliers_and_outliers_and_set_weights(kin, kout, loss, w0):
    """knownInliersAndOutliers (testGncOptimizer.cpp:776-863) and setWeights (:866-944) on the device: the reference's expectations
    (result (0, 0) to 1e-3, final weights [1, 1, 1, 0]) and, against the restatement, the same outer iteration count, stop reason and
    base optimizer iterations.  The first block is the early exit 'nothing unknown' (GncOptimizer.h:196-215): stop 5, no outer
    iteration, the weights stay the initial ones and the values are the first base optimizer run's."""
    g, p1 = gc.toy_graph(), gc.point_values([1, 0, 0])
    ref = gr.gnc_optimize(g, p1, ORD, "GN", GaussNewtonParams(), loss=loss, known_in=kin, known_out=kout, barc=np.full(4, 1.0), weights=w0)
    gnc = _gnc(g, p1, ORD, "GN", loss, known_in=kin, known_out=kout)
    gnc.setInlierCostThresholds(1.0)
    if w0 is not None:
        gnc.setWeights(w0)
    result = gnc.optimize()
    w = gnc.getWeights()
    assert np.allclose(result.at(X(1)), [0, 0, 0], atol=1e-3)
    assert np.allclose(w, [1, 1, 1, 0], atol=1e-5 if loss == gr.GM else 1e-9)
    assert (gnc.result.iterations, gnc.result.stop) == (ref["iterations"], ref["stop"])
    assert gnc.result.base_iterations_total == ref["base_iterations_total"]
    assert np.abs(w - ref["weights"]).max() <= 1e-9 and np.abs(result.at(X(1)) - ref["values"][X(1)]).max() <= 1e-9
    if len(kin) + len(kout) == 4:
        assert (gnc.result.stop, gnc.result.iterations, len(gnc.trace())) == (5, 0, 0)
    gnc.close()


def test_small_residuals_stop_at_initialisation():
    """mu <= 0 at initialisation (GncOptimizer.h:192-215, initializeMu's -1): stop 4, no outer iteration, the values are the first base
    optimizer run's, the weights stay 1; under GM the same graph runs the loop (mu = 2 r_max / barcSq > 0)"""
    g, p = inlier_only_graph(), gc.point_values([0.01, 0, 0])
    gnc = _gnc(g, p, ORD, "GN", gr.TLS)
    assert gnc.initializeMu() == -1.0
    result = gnc.optimize()
    assert (gnc.result.stop, gnc.result.iterations, gnc.result.mu, len(gnc.trace())) == (4, 0, -1.0, 0)
    assert np.allclose(result.at(X(1)), [0, 0, 0], atol=1e-9) and np.array_equal(gnc.getWeights(), np.ones(3))
    assert gnc.result.base_iterations_total == gnc.base().iterations() > 0
    gnc.close()
    gnc = _gnc(g, p, ORD, "GN", gr.GM)
    gnc.optimize()
    ref = gr.gnc_optimize(g, p, ORD, "GN", GaussNewtonParams(), loss=gr.GM)
    assert gnc.result.stop in (1, 3) and (gnc.result.iterations, gnc.result.stop) == (ref["iterations"], ref["stop"])
    gnc.close()


def test_weight_change_invalidates_linear_graph():
    """a linear graph handed out before setWeights / calculateWeights carries the old weights: reading it afterwards is refused, and so
    is the C tap until the next linearize"""
    g, at0 = gc.toy_graph(), gc.point_values([0.5, 0, 0])
    gnc = _gnc(g, at0, ORD, "GN", gr.TLS)
    opt = gnc.base()
    lin = opt.linearize()
    gnc.setWeights([1, 0.25, 1, 1])
    with pytest.raises(_lib.LmgpuError):
        lin.at(1)
    r, c = ct.c_int32(), ct.c_int32()
    buf = np.zeros(12)
    assert opt.lib.lmgpu_get_jacobian(opt._h, 1, buf.ctypes.data_as(ct.POINTER(ct.c_double)), ct.byref(r), ct.byref(c)) == _lib.LMGPU_INVALID
    lin = opt.linearize()
    assert np.allclose(lin.at(1).augmentedJacobian(), 0.5 * lin.at(0).augmentedJacobian(), atol=1e-15)
    gnc.close()


# ---------------------------------------------------------------- 4. optimizeSmallPoseGraph
@pytest.mark.parametrize("base,loss", SMALL_POSE_GRAPH_CASES)
def test_small_pose_graph(base, loss):
    """w100 + outlier on the device against the restatement: same number of outer iterations and same stop reason, mu identical to 1e-12
    relative after every outer iteration, final values and final cost within 1e-6, weights within 1e-6 absolute.  The reference's own
    criterion (1e-3 per coordinate to LM on the outlier-free graph, testGncOptimizer.cpp:737-773) is asserted for the reference's own
    case, GN base with TLS; the restatement of the other three does not meet it itself (figures in tests/test_gnc_reference.py).

    The LM / TLS case runs on another wrong loop closure than the reference's (gnc_cases.W100_OUTLIER_OF_CASE): on the reference's the
    restatement itself is chaotic (a 1e-13 perturbation changes its outer iteration count), so no two implementations can agree there;
    the CPU file asserts the stability of every input used here."""
    ref = small_pose_graph_restatement(base, loss)
    graph, initial, ordering = gc.w100_case(base, loss)
    gnc = _gnc(graph, initial, ordering, base, loss)
    result = gnc.optimize()
    tr, w = gnc.trace(), gnc.getWeights()
    print(base, loss, "outer iterations", gnc.result.iterations, ref["iterations"], "stop", gnc.result.stop, ref["stop"], "base iterations",
          gnc.result.base_iterations_total, ref["base_iterations_total"])
    print("max weight difference", np.abs(w - ref["weights"]).max(), "value difference", _max_diff(_vals_dict(result), ref["values"]),
          "cost", gnc.result.cost, ref["cost"])
    for i, (a, b) in enumerate(zip(tr, ref["trace"])):
        print("   outer", i, "mu", a[0], b[0], "cost", a[1], b[1], "max |w - round w|", a[2], b[2], "base iterations", int(a[5]))
    assert (gnc.result.iterations, gnc.result.stop) == (ref["iterations"], ref["stop"])
    assert len(tr) == len(ref["trace"])
    for a, b in zip(tr, ref["trace"]):
        assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0])
    assert abs(gnc.result.mu - ref["mu"]) <= 1e-12 * abs(ref["mu"])
    assert _max_diff(_vals_dict(result), ref["values"]) <= 1e-6
    assert abs(gnc.result.cost - ref["cost"]) <= 1e-6 * max(1.0, abs(ref["cost"]))
    assert np.abs(w - ref["weights"]).max() <= 1e-6
    if (base, loss) == ("GN", gr.TLS):
        g0, _, _ = gc.w100(outlier=False)
        orc = oh.OracleProblem(g0, initial, ordering)
        p = LevenbergMarquardtParams()
        orc.lm_init(p)
        orc.lm_optimize(p)
        assert _max_diff(_vals_dict(result), orc.values()) < 1e-3
    gnc.close()


# ---------------------------------------------------------------- 5. BAL with outliers
def test_bal_outliers():
    """LM base, TLS: displaced measurements end below 0.5, untouched ones above, except for at most 1 % of the factors; the final error
    on the inlier factors is within 1e-6 relative of the restatement's"""
    graph, initial, ordering, displaced = gc.bal_with_outliers()
    gnc = _gnc(graph, initial, ordering, "LM", gr.TLS)
    result = gnc.optimize()
    w = gnc.getWeights()
    wrong = int(((w < 0.5) != displaced).sum())
    print("misclassified", wrong, "of", graph.size(), "outer iterations", gnc.result.iterations, "stop", gnc.result.stop)
    assert wrong <= 0.01 * graph.size()
    ref = gr.gnc_optimize(graph, initial, ordering, "LM", LevenbergMarquardtParams(), loss=gr.TLS)
    assert (gnc.result.iterations, gnc.result.stop) == (ref["iterations"], ref["stop"])
    inl = ~displaced
    r_d = gr.factor_errors(graph, result, ordering)
    vals = initial.copy()
    for k, v in ref["values"].items():
        vals.update(k, v)
    r_r = gr.factor_errors(graph, vals, ordering)
    print("inlier error device", r_d[inl].sum(), "restatement", r_r[inl].sum())
    assert abs(r_d[inl].sum() - r_r[inl].sum()) <= 1e-6 * r_r[inl].sum()
    gnc.close()


# ---------------------------------------------------------------- 6. PCG
def test_small_pose_graph_pcg():
    """the GN / TLS w100 case under LMGPU_SOLVER_PCG (block-Jacobi, epsilon_rel 1e-10): rounded final weights equal the Cholesky run's,
    values within 1e-4"""
    graph, initial, ordering = gc.w100(outlier=True)
    a = _gnc(graph, initial, ordering, "GN", gr.TLS)
    va, wa = a.optimize(), a.getWeights()
    a.close()
    gn = GaussNewtonParams()
    gn.linearSolverType = "ITERATIVE"
    gn.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    gn.iterativeParams.epsilon_rel, gn.iterativeParams.epsilon_abs, gn.iterativeParams.maxIterations = 1e-10, 1e-30, 5000
    b = _gnc(graph, initial, ordering, "GN", gr.TLS, base_params=gn)
    vb, wb = b.optimize(), b.getWeights()
    st = b.base().pcg_stats()
    print("PCG residual of the last solve: gamma", st["gamma"], "threshold", st["threshold"], "iterations", st["iterations"])
    assert np.array_equal(np.round(wa), np.round(wb))
    assert _max_diff(_vals_dict(va), _vals_dict(vb)) <= 1e-4
    b.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    g, p0 = gc.toy_graph(), gc.point_values([3, 3, 0])
    opt = LevenbergMarquardtOptimizer(g, p0, ORD, LevenbergMarquardtParams())
    lib, h = opt.lib, opt._h
    U = ct.POINTER(ct.c_uint64)
    D = ct.POINTER(ct.c_double)
    buf = np.ones(8)
    mu = ct.c_double()
    gp, bp, res = _lib.lmgpu_gnc_params(1, 100, 0, 1.4, 1e-5, 1e-4), LevenbergMarquardtParams()._c(), _lib.lmgpu_gnc_result()
    # before lmgpu_gnc_enable
    assert lib.lmgpu_gnc_set_weights(h, 4, buf.ctypes.data_as(D)) == _lib.LMGPU_INVALID and b"not enabled" in lib.lmgpu_last_error(h)
    assert lib.lmgpu_gnc_get_weights(h, 4, buf.ctypes.data_as(D)) == _lib.LMGPU_INVALID
    assert lib.lmgpu_gnc_initialize_mu(h, 1, ct.byref(mu)) == _lib.LMGPU_INVALID
    assert lib.lmgpu_gnc_calculate_weights(h, 1, 1.0) == _lib.LMGPU_INVALID
    assert lib.lmgpu_gnc_optimize(h, ct.byref(gp), ct.byref(bp), None, ct.byref(res)) == _lib.LMGPU_INVALID
    assert lib.lmgpu_gnc_enable(h, 1, 3) == _lib.LMGPU_INVALID  # graph_size below the largest graph index + 1
    assert lib.lmgpu_gnc_enable(h, 1, 4) == _lib.LMGPU_OK
    both_in, both_out = np.array([0, 1], dtype=np.uint64), np.array([1, 3], dtype=np.uint64)
    assert lib.lmgpu_gnc_set_known(h, 2, both_in.ctypes.data_as(U), 2, both_out.ctypes.data_as(U)) == _lib.LMGPU_INVALID
    assert b"BOTH" in lib.lmgpu_last_error(h)
    far = np.array([4], dtype=np.uint64)
    assert lib.lmgpu_gnc_set_known(h, 1, far.ctypes.data_as(U), 0, None) == _lib.LMGPU_INVALID and b"known inliers" in lib.lmgpu_last_error(h)
    assert lib.lmgpu_gnc_set_known(h, 0, None, 1, far.ctypes.data_as(U)) == _lib.LMGPU_INVALID and b"known outliers" in lib.lmgpu_last_error(h)
    assert lib.lmgpu_gnc_set_weights(h, 5, buf.ctypes.data_as(D)) == _lib.LMGPU_INVALID and b"does not match" in lib.lmgpu_last_error(h)
    assert lib.lmgpu_gnc_set_inlier_cost_thresholds(h, 3, buf.ctypes.data_as(D), 0.0) == _lib.LMGPU_INVALID
    assert lib.lmgpu_gnc_initialize_mu(h, 2, ct.byref(mu)) == _lib.LMGPU_INVALID and b"unknown loss" in lib.lmgpu_last_error(h)
    gp.baseOptimizer = 2  # Dogleg
    assert lib.lmgpu_gnc_optimize(h, ct.byref(gp), ct.byref(bp), None, ct.byref(res)) == _lib.LMGPU_INVALID
    assert b"Dogleg" in lib.lmgpu_last_error(h)
    assert lib.lmgpu_gnc_enable(h, 0, 0) == _lib.LMGPU_OK
    # world_size > 1: a structure of a two-rank handle refuses GNC
    opt2 = LevenbergMarquardtOptimizer(g, p0, ORD, LevenbergMarquardtParams(), device=-1, world_size=2)
    assert opt2.lib.lmgpu_gnc_enable(opt2._h, 1, 4) == _lib.LMGPU_INVALID and b"single-rank" in opt2.lib.lmgpu_last_error(opt2._h)
    opt2.close()
    gnc2 = None
    with pytest.raises(RuntimeError):
        gnc2 = _gnc(g, p0, ORD)
        gnc2.setWeights(np.ones(5))
    gnc2.close()
    # the handle still optimizes (Robust is back: Geman-McClure around sigma 0.1)
    cp = opt.params._c()
    opt._check(lib.lmgpu_lm_init(h, ct.byref(cp), ct.byref(opt.state)))
    opt.optimize()
    orc = oh.OracleProblem(g, p0, ORD)
    orc.lm_init(opt.params)
    orc.lm_optimize(opt.params)
    assert _max_diff(_vals_dict(opt.values()), orc.values()) <= 1e-6
    opt.close()


# ---------------------------------------------------------------- 8. off means off
def test_off_means_off():
    """a handle that had GNC enabled, run and disabled again gives LM results bit-equal to a handle that never had it"""
    graph, initial, ordering = gc.w100(outlier=True)
    a = LevenbergMarquardtOptimizer(graph, initial, ordering, LevenbergMarquardtParams())
    va = a.optimize()
    ja = a.linearize()
    ja = [ja.at(i).augmentedJacobian() for i in (0, 150, 301)]
    gnc = _gnc(graph, initial, ordering, "LM", gr.TLS)
    gnc.optimize()
    b = gnc.base()
    b._check(b.lib.lmgpu_gnc_enable(b._h, 0, 0))
    b.set_values(initial)
    cp = b.params._c()
    b._check(b.lib.lmgpu_lm_init(b._h, ct.byref(cp), ct.byref(b.state)))
    vb = b.optimize()
    jb = b.linearize()
    jb = [jb.at(i).augmentedJacobian() for i in (0, 150, 301)]
    assert (a.error(), a.iterations(), a.lambda_()) == (b.error(), b.iterations(), b.lambda_())
    for k in va.keys():
        assert np.array_equal(va.at(k), vb.at(k))
    for x, y in zip(ja, jb):
        assert np.array_equal(x, y)
    a.close()
    gnc.close()
