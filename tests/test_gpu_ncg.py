"""NonlinearConjugateGradientOptimizer on the device (lmgpu_gradient, lmgpu_ncg_*; kernels_ncg.hpp, ncg.hpp) against the float64
restatement of the reference (tests/ncg_restatement.py over the CPU oracle).  The restatement's results are computed once per
process (tests/ncg_cases.py); the tolerances on alpha and on the error are the measured constants of tests/ncg_cases.py, which
tests/test_ncg_reference.py measures again on the CPU."""
import ctypes as ct

import numpy as np
import pytest

import ncg_cases as nc
import ncg_restatement as nr
import oracle_harness as oh
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, DirectionMethod, GaussNewtonParams, LevenbergMarquardtOptimizer,
                                LevenbergMarquardtParams, NonlinearConjugateGradientOptimizer, Ordering, PCGSolverParameters, _lib)
from ncg_cases import ALPHA_RTOL, ERROR_RTOL, SEARCH_GRAPHS

pytestmark = pytest.mark.gpu

# Linear quantities, device against oracle: the norm-wise relative difference and the 1e-9 that tests/test_gpu_pcg.py allows between
# the device's PCG vectors and the restatement (its rel() / _compare), which is also the Jacobian parity figure of
# tests/test_gpu_parity.py; the gradient is a fixed-order sum of products of those Jacobian entries.
GRADIENT_RTOL = 1e-9


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.linalg.norm(a - b) / max(1e-300, np.linalg.norm(b)))


def _params(max_iterations=100, iterative=False):
    p = GaussNewtonParams()
    p.maxIterations = max_iterations
    if iterative:
        p.linearSolverType = "ITERATIVE"
        p.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    return p


def _opt(name, max_iterations=100, method=DirectionMethod.PolakRibiere, **kw):
    graph, initial = nc.problem(name)
    iterative = kw.pop("iterative", False)
    return NonlinearConjugateGradientOptimizer(graph, initial, _params(max_iterations, iterative), method, device=0, **kw)


def _packed_values(opt):
    out = np.empty(opt._nstore)
    opt._check(opt.lib.lmgpu_get_values(opt._h, out.ctypes.data_as(ct.POINTER(ct.c_double))))
    return out


@pytest.mark.parametrize("name", list(nc.GRAPHS))
def test_gradient_matches_restatement(name):
    """15 scalars (less than one workgroup), 258 (straddles a 256-thread block), Pose3, the GeneralSFMFactor kernels of their own,
    three-variable factors, and a Huber model (the reweighted [A b])"""
    opt = _opt(name)
    want = nc.restated_gradient(name)
    g = opt.gradient()
    got = opt.delta_by_key(g)
    assert sorted(got) == sorted(want)
    r = rel(np.concatenate([got[k] for k in sorted(want)]), np.concatenate([want[k] for k in sorted(want)]))
    print(name, "dim", g.size, "gradient rel", r)
    assert r <= GRADIENT_RTOL
    assert np.array_equal(opt.gradient(), g)  # fixed summation order: bitwise the same
    opt.close()


@pytest.mark.parametrize("name", SEARCH_GRAPHS)
def test_line_search_matches_restatement(name):
    opt = _opt(name)
    before = _packed_values(opt)
    alpha, trials = opt.line_search()
    want, want_trials, _ = nc.restated_line_search(name)
    print(name, "alpha", alpha, "restated", want, "rel", abs(alpha - want) / abs(want), "trials", trials, want_trials)
    assert np.array_equal(_packed_values(opt), before)
    assert 0 < trials < nr.MAX_TRIALS
    if name in nc.TRIALS_EXACT_GRAPHS:  # the restatement's count does not move with the last bits of the errors: the device's is the same
        assert trials == want_trials
    assert abs(alpha - want) <= ALPHA_RTOL * abs(want)
    assert opt.host_waits() == 1
    # the same search along the caller's copy of the gradient
    alpha2, trials2 = opt.line_search(opt.gradient())
    assert alpha2 == alpha and trials2 == trials
    opt.close()


@pytest.mark.parametrize("name", SEARCH_GRAPHS)
def test_iterations_match_restatement(name):
    """five calls of the full loop, maxIterations = 1..5, each from the initial values"""
    graph, initial = nc.problem(name)
    e0 = nr.OracleSystem(graph).error(initial)
    errs = []
    for k in range(1, 6):
        opt = _opt(name, k)
        opt.optimize()
        want, want_it, want_trace, _ = nc.restated_run(name, k)
        print(name, "maxIterations", k, "error", opt.error(), "restated", want, "rel", abs(opt.error() - want) / want)
        assert opt.iterations() == want_it == k
        assert abs(opt.error() - want) <= ERROR_RTOL * want
        tr = opt.trace()
        assert tr.shape == (k + 1, 4) and tr[-1, 2] == opt.error()
        assert all(0 < t < nr.MAX_TRIALS for t in tr[:, 3])
        assert opt.host_waits() <= 1 + (k + 1) + sum(1 for t in tr[:, 3] if t > 40) * 2
        assert abs(opt.graph_error() - opt.error()) <= 1e-12 * opt.error()
        errs.append(opt.error())
        opt.close()
    assert all(b < a for a, b in zip([e0] + errs, errs))  # monotone, as in the restatement (tests/test_ncg_reference.py)


METHODS = [DirectionMethod.FletcherReeves, DirectionMethod.PolakRibiere, DirectionMethod.HestenesStiefel, DirectionMethod.DaiYuan]


@pytest.mark.parametrize("method", METHODS)
def test_known_answer_on_the_device(method):
    """testNonlinearConjugateGradientOptimizer.cpp:72-86, 244-284: error < 1e-4 within 500 iterations, each direction method.
    (gradient_descent = 1 is left out: the restatement stops by the relative tolerance at 0.00083 after 418 iterations, it never
    gets below 1e-4 on this graph; its iterations are compared below.)"""
    opt = _opt("five_pose", 500, method)
    values = opt.optimize()
    want, want_it, _, _ = nc.restated_run("five_pose", 500, method=method)
    print("method", method, "error", opt.error(), "iterations", opt.iterations(), "restated", want, want_it)
    assert opt.error() < 1e-4 and opt.iterations() <= 500
    graph, _ = nc.problem("five_pose")
    assert oh.OracleProblem(graph, values, values.keys()).error() < 1e-4
    opt.close()


@pytest.mark.parametrize("name", ["five_pose", "five_pose_huber"])
@pytest.mark.parametrize("method", METHODS)
def test_each_direction_method_matches_its_restatement(name, method):
    """four iterations per method: the restatement's errors of the four methods lie more than 10 x ERROR_RTOL apart on these graphs
    (tests/test_ncg_reference.py::test_direction_methods_are_told_apart), so a method that is ignored or swapped fails here"""
    opt = _opt(name, 4, method)
    opt.optimize()
    want, want_it, want_trace, _ = nc.restated_run(name, 4, method=method)
    tr = opt.trace()
    print(name, "method", method, "error", opt.error(), "restated", want, "beta", tr[:, 1], [r[1] for r in want_trace])
    assert opt.iterations() == want_it == 4
    assert abs(opt.error() - want) <= ERROR_RTOL * want
    for k in range(1, 5):
        assert abs(tr[k, 2] - want_trace[k][2]) <= ERROR_RTOL * want_trace[k][2]
    assert tr[0, 1] == 0.0 == want_trace[0][1]
    for k in range(1, 5):  # beta of every row: the measured tolerance of tests/ncg_cases.py (alpha moves it through the next gradient)
        assert nc.beta_distance(tr[k, 1], want_trace[k][1]) <= nc.BETA_RTOL, (k, tr[k, 1], want_trace[k][1])
    opt.close()


def test_gradient_descent_switch_matches_restatement():
    opt = _opt("five_pose", 5, gradientDescent=True)
    opt.optimize()
    want, want_it, _, _ = nc.restated_run("five_pose", 5, gradient_descent=True)
    assert opt.iterations() == want_it == 5
    assert abs(opt.error() - want) <= ERROR_RTOL * want
    assert not opt.trace()[:, 1].any()
    opt.close()


def test_iterate_twice_equals_two_fresh_single_iterations():
    """iterate() starts over with a gradient-descent step each call (.cpp:71-80): the second call is a fresh single iteration from
    the first one's result"""
    a = _opt("five_pose")
    assert a.iterate() is None
    e1, v1 = a.error(), a.values()
    assert a.iterations() == 1 and a.trace().shape == (2, 4) and a.trace()[0, 1] == 0.0
    want1, _, _, _ = nc.restated_run("five_pose", 100, single=True)
    assert abs(e1 - want1) <= ERROR_RTOL * want1
    a.iterate()
    graph, _ = nc.problem("five_pose")
    b = NonlinearConjugateGradientOptimizer(graph, v1, _params(), device=0)
    assert b.error() == e1
    b.iterate()
    assert a.iterations() == 2 and b.iterations() == 1
    assert a.error() == b.error() and np.array_equal(_packed_values(a), _packed_values(b))
    assert a.error() < e1
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["pose3_head", "bal_small"])
def test_trace_is_independent_of_the_linear_solver(name):
    a = _opt(name, 4)
    b = _opt(name, 4, iterative=True)
    assert a.num_fronts() > 0 and b.num_fronts() == 0
    a.optimize()
    b.optimize()
    assert np.array_equal(a.trace(), b.trace()) and a.error() == b.error()
    assert np.array_equal(_packed_values(a), _packed_values(b))
    a.close()
    b.close()


def test_early_exit_leaves_the_values():
    opt = _opt("five_pose")
    e0 = opt.error()
    opt.params.errorTol = e0 + 1.0
    before = _packed_values(opt)
    opt.optimize()
    assert opt.iterations() == 0 and opt.error() == e0
    assert np.array_equal(_packed_values(opt), before)
    assert opt.trace().shape == (0, 4)
    opt.close()


def test_refused_states():
    graph, initial = nc.problem("five_pose")
    lib = _lib.load()
    cp = _lib.lmgpu_ncg_params(1, 0, 5, 1e-5, 1e-5, 0.0)
    g = np.zeros(15)
    gp = g.ctypes.data_as(ct.POINTER(ct.c_double))

    def refused(o):
        st = _lib.lmgpu_lm_state()
        a, n = ct.c_double(), ct.c_int32()
        for rc in (lib.lmgpu_ncg_optimize(o._h, ct.byref(cp), ct.byref(st)), lib.lmgpu_ncg_iterate(o._h, ct.byref(cp), ct.byref(st)),
                   lib.lmgpu_gradient(o._h, gp), lib.lmgpu_ncg_line_search(o._h, None, ct.byref(a), ct.byref(n))):
            assert rc == _lib.LMGPU_INVALID
            assert lib.lmgpu_last_error(o._h)

    # GNC enabled
    o = LevenbergMarquardtOptimizer(graph, initial, Ordering.Natural(graph), LevenbergMarquardtParams(), device=0)
    o._check(lib.lmgpu_gnc_enable(o._h, 1, graph.size()))
    refused(o)
    o._check(lib.lmgpu_gnc_enable(o._h, 0, 0))
    st = _lib.lmgpu_lm_state()
    assert lib.lmgpu_ncg_iterate(o._h, ct.byref(cp), ct.byref(st)) == _lib.LMGPU_OK  # and back
    o.close()
    # a communicator (one rank)
    o = LevenbergMarquardtOptimizer(graph, initial, Ordering.Natural(graph), LevenbergMarquardtParams(), device=0, split_root=True,
                                    comm_id=LevenbergMarquardtOptimizer.comm_unique_id())
    refused(o)
    o.close()
    # before lmgpu_set_values: a structure-only build of the same handle on the device
    o = LevenbergMarquardtOptimizer.__new__(LevenbergMarquardtOptimizer)
    o.lib, o._h = lib, ct.c_void_p()
    cfg = _lib.lmgpu_config(0, 0, 1, 0)
    assert lib.lmgpu_create(ct.byref(cfg), ct.byref(o._h)) == 0
    keys = np.array([1, 2], dtype=np.uint64)
    types = np.zeros(2, dtype=np.int32)
    assert lib.lmgpu_set_variables(o._h, 2, keys.ctypes.data_as(ct.POINTER(ct.c_uint64)), types.ctypes.data_as(ct.POINTER(ct.c_int32))) == 0
    gi, slots = np.zeros(1, dtype=np.int32), np.array([0, 1], dtype=np.int32)
    meas = np.array([1.0, 0.0, 0.0])
    ip = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_int32))  # noqa: E731
    assert lib.lmgpu_add_factor_bucket(o._h, 1, 1, ip(gi), ip(slots), meas.ctypes.data_as(ct.POINTER(ct.c_double)), 0, None) == 0
    assert lib.lmgpu_finalize_structure(o._h) == 0
    refused(o)
    o.close()


def test_python_class_reaches_the_known_answer():
    graph, initial = nc.problem("five_pose")
    p = GaussNewtonParams()
    p.maxIterations = 500
    opt = NonlinearConjugateGradientOptimizer(graph, initial, p)
    values = opt.optimize()
    assert oh.OracleProblem(graph, values, values.keys()).error() < 1e-4
    assert opt.iterations() <= 500 and opt.values().keys() == initial.keys()
    opt.close()
