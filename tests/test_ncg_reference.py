"""The nonlinear conjugate gradient restatement (tests/ncg_restatement.py) against the reference's own known answers
(gtsam/nonlinear/tests/testNonlinearConjugateGradientOptimizer.cpp), the line search on a one-dimensional quadratic, the measured
constants tests/test_gpu_ncg.py compares the device with, and the C ABI's names.  No device."""
import math
import os
import re

import pytest

import ncg_cases as nc
import ncg_restatement as nr
from gtsam_personal_amd import DirectionMethod, _lib
from ncg_cases import BRACKET_RTOL, ERROR_RTOL, PERTURB_SEEDS, SEARCH_GRAPHS, SPREAD_MEASURED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optimize_reaches_the_reference_answer():
    """TEST(NonlinearConjugateGradientOptimizer, Optimize) :72-86: maxIterations 500, default direction method, error < 1e-4"""
    err, it, trace, _ = nc.restated_run("five_pose", 500)
    print("error", err, "iterations", it)
    assert abs(err) < 1e-4 and it <= 500


@pytest.mark.parametrize("method", [nr.FLETCHER_REEVES, nr.POLAK_RIBIERE, nr.HESTENES_STIEFEL, nr.DAI_YUAN])
def test_direction_methods_reach_the_reference_answer(method):
    """TEST(NonlinearConjugateGradientOptimizer, DirectionMethods) :244-284: maxIterations 500 for each of the four"""
    err, it, trace, _ = nc.restated_run("five_pose", 500, method=method)
    print("method", method, "error", err, "iterations", it, "most trials", max(r[3] for r in trace))
    assert abs(err) < 1e-4 and it <= 500
    assert max(r[3] for r in trace) < nr.MAX_TRIALS


@pytest.mark.parametrize("name", ["five_pose", "five_pose_huber"])
def test_direction_methods_are_told_apart(name):
    """what tests/test_gpu_ncg.py::test_each_direction_method_matches_its_restatement relies on: after four iterations the errors of
    the four methods differ pairwise by more than ten times the tolerance the device is compared under"""
    errs = [nc.restated_run(name, 4, method=m)[0] for m in (nr.FLETCHER_REEVES, nr.POLAK_RIBIERE, nr.HESTENES_STIEFEL, nr.DAI_YUAN)]
    print(name, errs)
    for i in range(4):
        for j in range(i):
            assert abs(errs[i] - errs[j]) > 10 * ERROR_RTOL * min(errs[i], errs[j])


@pytest.mark.parametrize("a,x0,c", [(1.0, 0.7, 0.0), (4.0, 3.5, 3.0), (250.0, -1.0, -0.25), (1e3, 10.9, 10.0)])
def test_line_search_on_a_quadratic(a, x0, c):
    """error = 0.5 a (x - c)^2: along the gradient the minimiser is alpha = -1 / a, inside the bracket [-1 / |g|, 0] when
    |x0 - c| <= 1.  The search keeps the minimiser inside its bracket and returns the midpoint once the bracket is narrower than
    tau (|testStep| + |newStep|) <= 2 tau |minStep|: |alpha + 1 / a| <= 2 tau / a (1 + 2 tau)."""
    s = nr.Quadratic1D(a, c)
    st = {}
    alpha = nr.line_search(s, x0, s.gradient(x0), st)
    want = -1.0 / a
    print("alpha", alpha, "want", want, "trials", st["trials"])
    assert st["bracket"][0] <= want <= st["bracket"][1]
    assert abs(alpha - want) <= 2 * nr.TAU * (1 + 2 * nr.TAU) * abs(want)
    assert st["trials"] < nr.MAX_TRIALS
    # the count the device's comment derives: 1 + ceil(log(2 tau r) / log(0.618)) with r = |alpha| |g| (one more for the rounding of r)
    r = abs(want) * abs(a * (x0 - c))
    assert st["trials"] <= 2 + math.ceil(math.log(2 * nr.TAU * r) / math.log(0.5 * (math.sqrt(5.0) - 1.0)))


def test_single_iteration_is_a_descent_step_and_one_conjugate_step():
    """iterate() (.cpp:71-80): singleIteration stops after the first pass whatever maxIterations says"""
    err, it, trace, _ = nc.restated_run("five_pose", 100, single=True)
    assert it == 1 and len(trace) == 2
    assert err == nc.restated_run("five_pose", 1)[0]


def test_early_exit_and_gradient_descent_switch():
    graph, initial = nc.problem("five_pose")
    s = nr.OracleSystem(graph)
    e0 = s.error(initial)
    values, it = nr.nonlinear_conjugate_gradient(s, initial, nr.Params(errorTol=e0 + 1.0), False)
    assert it == 0 and values is initial
    # gradient descent converges by the relative tolerance long before it reaches 1e-4 on this graph (0.00083 after 418 iterations):
    # no known-answer case for it; its first iterations are compared with the device instead
    err, it, trace, _ = nc.restated_run("five_pose", 5, gradient_descent=True)
    assert it == 5 and all(r[1] == 0.0 for r in trace)
    assert all(b[2] < a[2] for a, b in zip(trace, trace[1:]))


@pytest.mark.parametrize("name", SEARCH_GRAPHS)
def test_measured_constants_hold(name):
    """the spread the tolerances above were derived from, measured again; and the restatement's error decreases over the five
    iterations the device is compared on"""
    a0, t0, br = nc.restated_line_search(name)
    assert t0 < nr.MAX_TRIALS
    assert (br[1] - br[0]) <= BRACKET_RTOL * abs(a0) * (1 + BRACKET_RTOL)
    spread = 0.0
    for seed in PERTURB_SEEDS:
        a1, _, _ = nc.restated_line_search(name, seed)
        spread = max(spread, abs(a1 - a0) / abs(a0))
    errs = [nc.restated_run(name, k)[0] for k in range(1, 6)]
    for seed in PERTURB_SEEDS:
        for k in range(1, 6):
            spread = max(spread, abs(nc.restated_run(name, k, seed=seed)[0] - errs[k - 1]) / errs[k - 1])
    print(name, "alpha", a0, "trials", t0, "spread", spread, "errors", errs)
    assert spread <= SPREAD_MEASURED
    graph, initial = nc.problem(name)
    e0 = nr.OracleSystem(graph).error(initial)
    assert all(b < a for a, b in zip([e0] + errs, errs))


def test_trial_counts_are_robust():
    """the graphs on which tests/test_gpu_ncg.py asserts the device's evaluation count: the restatement's count of the first search is
    unchanged when every error moves by (1 +- 1e-12)"""
    robust = tuple(n for n in SEARCH_GRAPHS if all(nc.restated_trials(n, s) == nc.restated_trials(n) for s in PERTURB_SEEDS))
    print({n: nc.restated_trials(n) for n in SEARCH_GRAPHS})
    assert robust == nc.TRIALS_EXACT_GRAPHS
    assert all(nc.restated_trials(n) == nc.restated_line_search(n)[1] for n in SEARCH_GRAPHS)


def test_beta_spread_holds():
    """the spread behind BETA_RTOL, measured again: every trace row's beta with each search's alpha moved by +-BRACKET_RTOL"""
    worst = (0.0, None)
    for name in nc.BETA_GRAPHS:
        for method in (nr.FLETCHER_REEVES, nr.POLAK_RIBIERE, nr.HESTENES_STIEFEL, nr.DAI_YUAN):
            b0 = nc.restated_betas(name, method)
            assert b0 == tuple(r[1] for r in nc.restated_run(name, 4, method=method)[2]) and b0[0] == 0.0 and min(b0[1:]) > nc.BETA_FLOOR
            for move in nc.BETA_MOVES:
                d = max(nc.beta_distance(x, y) for x, y in zip(nc.restated_betas(name, method, move), b0))
                worst = max(worst, (d, (name, method, move)))
    print("beta spread", worst)
    assert worst[0] <= nc.BETA_SPREAD_MEASURED and nc.BETA_RTOL == 10 * nc.BETA_SPREAD_MEASURED
    assert worst[0] >= nc.BETA_SPREAD_MEASURED / 2  # the recorded figure is the measurement, not a loose cap


def test_python_enums_and_symbols_match_the_header():
    h = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    for name, want in (("LMGPU_NCG_FLETCHER_REEVES", nr.FLETCHER_REEVES), ("LMGPU_NCG_POLAK_RIBIERE", nr.POLAK_RIBIERE),
                       ("LMGPU_NCG_HESTENES_STIEFEL", nr.HESTENES_STIEFEL), ("LMGPU_NCG_DAI_YUAN", nr.DAI_YUAN)):
        m = re.search(name + r"\s*=\s*(\d+)", h)
        assert m and int(m.group(1)) == want == getattr(_lib, name)
    assert (DirectionMethod.FletcherReeves, DirectionMethod.PolakRibiere, DirectionMethod.HestenesStiefel, DirectionMethod.DaiYuan) == (0, 1, 2, 3)
    for name in ("lmgpu_gradient", "lmgpu_ncg_line_search", "lmgpu_ncg_iterate", "lmgpu_ncg_optimize", "lmgpu_ncg_get_trace",
                 "lmgpu_ncg_host_waits"):
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\(", h)
    fields = [f for f, _ in _lib.lmgpu_ncg_params._fields_]
    assert fields == ["direction_method", "gradient_descent", "max_iterations", "relative_error_tol", "absolute_error_tol", "error_tol"]
    m = re.search(r"typedef struct lmgpu_ncg_params \{[^}]*\}", h)
    assert m and [f for f in fields if f in m.group(0)] == fields
    # the trial bound the restatement checks against is the device code's
    src = open(os.path.join(ROOT, "gtsam_personal_amd", "csrc", "ncg.hpp")).read()
    assert int(re.search(r"#define NCG_MAX_TRIALS (\d+)", src).group(1)) == nr.MAX_TRIALS
