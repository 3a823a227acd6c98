"""The kernels of the nonlinear conjugate gradient optimizer (csrc/kernels_ncg.hpp) and the queueing of csrc/ncg.hpp at their edges:
the cases of tests/ncg_edge_cases.py on the device, through the test hooks lmgpu_debug_ncg_* (liblmgpu_test.so) and on graphs.
  * vector cases: the device's dot-product partials, beta, new direction and ls_begin record against the long-double reference
    (tests/ncg_reference.py) at 16 x the floor of each (case, method, quantity); the rest of the record exact; two runs bit-equal;
  * control cases: every record of an error sequence equals the float64 restatement (ncg_restatement.ls_step) bit for bit;
  * ncg_reduce_stage1 / 2 against reduce_to (bit-equal), the long-double sum, and the skip flag;
  * ncg_gradient_kernel on the block, mixed and hub graphs of tests/pcg_cases.py against a long-double -(A^T b) on the device's Jacobians;
  * line searches of exactly 40, 41, 84 and 85 evaluations (the queue boundaries of NCG_TRIALS_FIRST / _MORE), the ascent direction, and
    the two searches that do not end (a minimiser at step 0 that stays resolved, an all-zero direction): the error return, and the handle
    after it.
What every comparison relies on is asserted without a device in tests/test_ncg_edges_reference.py."""
import ctypes as ct
import math

import numpy as np
import pytest

import ncg_cases as nc
import ncg_edge_cases as ec
import ncg_reference as ref
import ncg_restatement as nr
import pcg_cases as pc
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, GaussNewtonParams, NonlinearConjugateGradientOptimizer,
                                PCGSolverParameters, _lib)
from ncg_cases import ALPHA_RTOL
from test_gpu_ncg import GRADIENT_RTOL, _packed_values, rel

pytestmark = pytest.mark.gpu
_DP = ct.POINTER(ct.c_double)
NPART = 256  # NCG_MAXPART


def _dp(a):
    return a.ctypes.data_as(_DP)


def _record(c):
    return {f: (float(getattr(c, f)) if f not in ("done", "trials", "flag", "first") else int(getattr(c, f))) for f in nr.RECORD_FIELDS}


# ---------------------------------------------------------------- vector cases
def _device_direction(name, method, alias):
    c = ec.vector_case(name)
    lib = _lib.load(test_hooks=True)
    d = np.array(c["s"], dtype=np.float64)  # read by methods 0..3 and by the aliased form; overwritten by every form
    parts = np.zeros((5, NPART))
    npart, ctl = ct.c_int32(-1), _lib.lmgpu_debug_ncg_ctl()
    g, gp = np.array(c["g"]), np.array(c["gp"])
    rc = lib.lmgpu_debug_ncg_direction(0, c["n"], method, alias, _dp(g), _dp(gp), _dp(d), _dp(parts), ct.byref(npart), ct.byref(ctl))
    assert rc == 0
    assert np.array_equal(g, c["g"]) and np.array_equal(gp, c["gp"])
    return d, parts, npart.value, _record(ctl)


def _check_vector(name, method, alias, mid):
    c = ec.vector_case(name)
    want, floor = ec.vector_reference(name, method, alias)
    d, parts, npart, rec = _device_direction(name, method, alias)
    assert npart == ref.npart_of(c["n"])
    # the partials: rows of the dot products written up to npart (not at all by the set-direction form), beyond it never
    assert np.isnan(parts[:, npart:]).all()
    if method < 0:
        assert np.isnan(parts[:4]).all()
        dots = [math.nan] * 4
    else:
        assert np.isfinite(parts[:4, :npart]).all()
        dots = [parts[i, :npart].astype(ref.LD).sum() for i in range(4)]
    if np.isfinite(np.asarray(want["dir"], dtype=np.float64)).all():
        assert np.isfinite(parts[4, :npart]).all()
    got = dict(gg=dots[0], gd=dots[1], pp=dots[2], sd=dots[3], beta=rec["beta"], dir=d, dnorm=rec["dnorm"], minStep=rec["minStep"], newStep=rec["newStep"])
    miss = ref.misses(got, want, floor)
    print("%-16s %-9s beta %-22r dnorm %-22r miss / tolerance: %s" % (name, mid, rec["beta"], rec["dnorm"], " ".join("%s %.2g" % kv for kv in miss.items())))
    assert max(miss.values()) <= 1.0, (name, mid, miss)
    for q in ref.QUANTITIES:  # the tolerance used is never above the recorded one
        if floor["noise"] is None or q not in ref.NOISE_QUANTITIES:
            assert floor[q] <= ec.FLOORS[name][q] * 1.06
    # the record: given the device's own |direction| and beta, ls_begin bit for bit
    assert ref.same_bits(rec, nr.ls_begin(rec["dnorm"], rec["beta"])), (rec, nr.ls_begin(rec["dnorm"], rec["beta"]))
    if method < 0:
        assert rec["beta"] == 0.0 and np.array_equal(d, c["s"] if alias else c["g"])
    # the order of every sum is fixed: a second run gives the same bits
    d2, parts2, npart2, rec2 = _device_direction(name, method, alias)
    assert d2.tobytes() == d.tobytes() and parts2.tobytes() == parts.tobytes() and npart2 == npart and ref.same_bits(rec, rec2)


@pytest.mark.parametrize("name", ec.VECTOR_NAMES)
def test_vector_case(name):
    for (method, alias), mid in zip(ec.METHODS, ec.METHOD_IDS):
        _check_vector(name, method, alias, mid)


def test_zero_direction_record():
    """an all-zero direction into ls_begin: dnorm 0, minStep -inf, newStep and step NaN, nothing else moved"""
    for method, alias in ((-1, 0), (-1, 1), (1, 0)):
        _, _, _, rec = _device_direction("zero", method, alias)
        assert rec["dnorm"] == 0.0 and rec["minStep"] == -math.inf and rec["maxStep"] == 0.0 and math.isnan(rec["newStep"]) and math.isnan(rec["step"])
        assert (rec["newError"], rec["alpha"], rec["error"], rec["beta"]) == (0.0, 0.0, 0.0, 0.0)
        assert (rec["done"], rec["trials"], rec["flag"], rec["first"]) == (0, 0, 0, 1)


def test_infinite_and_nan_beta_reach_the_direction():
    """gp = 0: Fletcher-Reeves' g.g / 0 = +inf; the direction is +-inf where s is not zero and NaN (inf * 0) where it is, like the reference's"""
    c = ec.vector_case("pp0")
    d, _, _, rec = _device_direction("pp0", 0, 0)
    assert rec["beta"] == math.inf
    z = c["s"] == 0
    assert z.any() and np.isnan(d[z]).all() and np.array_equal(d[~z], np.where(c["s"][~z] > 0, np.inf, -np.inf))
    assert math.isnan(rec["dnorm"]) and math.isnan(rec["minStep"])
    d, _, _, rec = _device_direction("allzero_g", 0, 0)  # 0 / 0
    assert math.isnan(rec["beta"]) and np.isnan(d).all()
    for m in (1, 2, 3):  # the clamped formulas: the NaN quotient gives 0, the direction is g = 0
        d, _, _, rec = _device_direction("allzero_g", m, 0)
        assert rec["beta"] == 0.0 and not d.any() and rec["dnorm"] == 0.0


# ---------------------------------------------------------------- control cases
def _ctl(rec):
    c = _lib.lmgpu_debug_ncg_ctl()
    for f in nr.RECORD_FIELDS:
        setattr(c, f, rec[f])
    return c


@pytest.mark.parametrize("name", ec.CONTROL_NAMES)
def test_control_case_bit_for_bit(name):
    c = ec.control_case(name)
    lib = _lib.load(test_hooks=True)
    errors = np.array(c["errors"], dtype=np.float64)
    k = len(errors) - 1
    out = (_lib.lmgpu_debug_ncg_ctl * (k + 1))()
    cin = _ctl(c["rec0"])
    assert lib.lmgpu_debug_ncg_ls_control(0, ct.byref(cin), k, _dp(errors), 1, out) == 0
    for i, want in enumerate(c["records"]):
        got = _record(out[i])
        assert ref.same_bits(got, want), (name, i, errors[i], got, want)
    print(name, "records", k + 1, "done at", c["done_at"], "alpha", out[k].alpha)


# ---------------------------------------------------------------- the error reduction of a trial
@pytest.mark.parametrize("n", ec.REDUCE_SIZES)
def test_reduce_equals_reduce_to(n):
    lib = _lib.load(test_hooks=True)
    rng = np.random.default_rng([17, n])
    buf = rng.uniform(0.0, 2.0, n) ** 2  # error terms: non-negative
    want = buf.astype(ref.LD).sum()
    floor = max(ref.scalar_dist(buf[rng.permutation(n)].sum(), want) for _ in range(3))
    floor = max(floor, ref.scalar_dist(buf.sum(), want))
    floor = max(floor, ref.HALF_ULP) if floor > 0 else 0.0  # as ncg_reference.floors
    out = np.zeros(2)
    sentinel = -7.25
    for skip in (0, -1):
        assert lib.lmgpu_debug_ncg_reduce(0, n, _dp(buf), skip, sentinel, _dp(out)) == 0
        assert out[0].tobytes() == out[1].tobytes()
        d = ref.scalar_dist(out[0], want)
        print("n", n, "skip", skip, "sum", out[0], "distance", d, "floor", floor)
        assert d <= ref.FLOOR_FACTOR * floor
    first = out.copy()
    assert lib.lmgpu_debug_ncg_reduce(0, n, _dp(buf), 1, sentinel, _dp(out)) == 0
    assert out[0] == sentinel and out[1].tobytes() == first[1].tobytes()  # behind `done` the trial's error stays as it was


# ---------------------------------------------------------------- the gradient gather
def _edge_opt(graph, initial, max_iterations=100, iterative=False):
    p = GaussNewtonParams()
    p.maxIterations = max_iterations
    if iterative:
        p.linearSolverType = "ITERATIVE"
        p.iterativeParams = PCGSolverParameters(BlockJacobiPreconditionerParameters())
    return NonlinearConjugateGradientOptimizer(graph, initial, p, device=0)


@pytest.mark.parametrize("name", ec.GRADIENT_CASES)
def test_gradient_case(name):
    c = pc.case(name)
    opt = _edge_opt(c["graph"], c["initial"], iterative=True)
    lg = opt.linearize()
    want = {int(k): np.zeros(int(opt._xoff[i + 1] - opt._xoff[i]), dtype=ref.LD) for i, k in enumerate(opt.ordering)}
    for i in range(lg.size()):
        f = lg.at(i)
        if f is None:
            continue
        b = f.getb().astype(ref.LD)
        for j, k in enumerate(f.keys()):
            want[int(k)] -= f.getA(j).astype(ref.LD).T @ b
    g = opt.gradient()
    got = opt.delta_by_key(g)
    assert sorted(got) == sorted(want)
    keys = sorted(want)
    r = ref.vec_dist(np.concatenate([got[k] for k in keys]), np.concatenate([want[k] for k in keys]))
    print(name, "dim", g.size, "gradient distance", r)
    assert g.size == opt._ntot and r <= GRADIENT_RTOL
    assert np.array_equal(opt.gradient(), g)
    opt.close()


# ---------------------------------------------------------------- the queue boundaries
WAITS = {40: 1, 41: 2, 84: 2, 85: 3}


@pytest.mark.parametrize("trials", sorted(ec.RATIOS))
def test_search_of_exactly_this_many_trials(trials):
    graph, initial = ec.prior_problem(trials)
    want_alpha, want_trials = ec.prior_trials(ec.RATIOS[trials])
    assert want_trials == trials
    opt = _edge_opt(graph, initial)
    before = _packed_values(opt)
    alpha, n = opt.line_search()
    print("prior[%d]" % trials, "alpha", alpha, "restated", want_alpha, "trials", n, "host waits", opt.host_waits())
    assert n == trials
    assert opt.host_waits() == WAITS[trials]
    assert abs(alpha - want_alpha) <= ALPHA_RTOL * abs(want_alpha)
    assert np.array_equal(_packed_values(opt), before)
    assert opt.trace().shape == (1, 4) and opt.trace()[0, 0] == alpha and opt.trace()[0, 3] == trials
    opt.close()


def test_final_advance_uses_alpha_after_a_second_queue():
    """iterate() on the 41-trial graph: the surplus trials of the second queue are skipped behind `done`, and the final advance takes
    alpha, not the last trial's step.  Everything lies on the x axis: x1 = x0 + alpha0 g0 (g0 = x0), g1 = x1, d1 = g1 + beta1 g0,
    x2 = x1 + alpha1 d1, with the alphas and beta of the device's own trace; the last trial steps lie 1e-5 relative from the alphas."""
    graph, initial = ec.prior_problem(41)
    r = ec.RATIOS[41]
    opt = _edge_opt(graph, initial)
    alpha, n = opt.line_search()
    assert n == 41
    opt.iterate()
    tr = opt.trace()
    assert tr.shape == (2, 4) and tr[0, 3] == 41 and tr[0, 0] == alpha and tr[0, 1] == 0.0
    x1 = r + tr[0, 0] * r
    x2 = x1 + tr[1, 0] * (x1 + tr[1, 1] * r)
    got = _packed_values(opt)
    print("values", got, "host", x2, "x1", x1, "trace", tr)
    assert got.shape == (3,) and got[1] == 0.0 and got[2] == 0.0
    assert abs(got[0] - x2) <= 1e-12 * r
    assert abs(tr[0, 0] * r) * nr.TAU > 1e3 * 1e-12 * r  # a last trial step in alpha's place would move x1 by far more than the bound
    assert opt.error() == opt.graph_error() == tr[1, 2]
    assert opt.host_waits() >= 1 + 2 + 1
    opt.close()


def _raw_line_search(opt, direction):
    a, n = ct.c_double(math.nan), ct.c_int32(-1)
    d = np.ascontiguousarray(direction, dtype=np.float64)
    rc = opt.lib.lmgpu_ncg_line_search(opt._h, _dp(d), ct.byref(a), ct.byref(n))
    return rc, a.value, n.value, (opt.lib.lmgpu_last_error(opt._h) or b"").decode()


def _same_as_a_fresh_handle(opt, name):
    """an ordinary line search and optimize(3) on `opt` give the bits a fresh handle gives"""
    fresh = _edge_opt(*nc.problem(name), max_iterations=3)
    opt.params.maxIterations = 3
    assert opt.line_search() == fresh.line_search()
    opt.optimize()
    fresh.optimize()
    assert np.array_equal(opt.trace(), fresh.trace()) and opt.trace().shape == (4, 4)
    assert np.array_equal(_packed_values(opt), _packed_values(fresh)) and opt.error() == fresh.error()
    fresh.close()


def test_ascent_direction_ends_in_the_third_queue():
    """five_pose along -gradient.  In float64 this search ends (by ties, once the steps fall below the spacing of the values; the
    restatement after 102 evaluations: tests/test_ncg_edges_reference.py), in the third queue: three waits, alpha a step of no effect."""
    opt = _edge_opt(*nc.problem("five_pose"))
    before = _packed_values(opt)
    g = opt.gradient()
    rc, alpha, n, msg = _raw_line_search(opt, -g)
    print("ascent: rc", rc, "alpha", alpha, "trials", n, msg)
    assert rc == _lib.LMGPU_OK
    assert ec.ASCENT_TRIALS[0] < n <= ec.ASCENT_TRIALS[1] and opt.host_waits() == 3
    assert alpha < 0.0 and abs(alpha) * float(np.linalg.norm(g)) < 1e-15
    assert np.array_equal(_packed_values(opt), before)
    _same_as_a_fresh_handle(opt, "five_pose")
    opt.close()


def test_minimiser_at_zero_returns_the_error():
    """the prior's point AT the origin, direction (1, 0, 0): the search does not end; LMGPU_HIP_ERROR after NCG_MAX_TRIALS evaluations and
    three waits, the message names the bracket, the values stay, the handle goes on working"""
    from gtsam_personal_amd import NonlinearFactorGraph, Values, noiseModel
    graph, initial = NonlinearFactorGraph(), Values()
    graph.add_PriorFactorPoint3(0, [0.0, 0.0, 0.0], noiseModel.Unit.Create(3))
    initial.insert_point3(0, np.zeros(3))
    opt = _edge_opt(graph, initial)
    rc, alpha, n, msg = _raw_line_search(opt, [1.0, 0.0, 0.0])
    print("origin: rc", rc, msg)
    assert rc == _lib.LMGPU_HIP_ERROR and math.isnan(alpha) and n == -1
    assert "after %d trials" % nr.MAX_TRIALS in msg and "|direction| = 1" in msg and "bracket [-" in msg and ", 0]" in msg
    assert opt.host_waits() == 3
    assert not _packed_values(opt).any() and opt.graph_error() == 0.0
    rc2, _, _, msg2 = _raw_line_search(opt, [0.0, -2.0, 0.0])
    assert rc2 == _lib.LMGPU_HIP_ERROR and "|direction| = 2" in msg2 and opt.host_waits() == 3
    opt.close()


def test_zero_direction_returns_the_error():
    opt = _edge_opt(*nc.problem("five_pose"))
    before = _packed_values(opt)
    rc, alpha, n, msg = _raw_line_search(opt, np.zeros(15))
    print("zero direction: rc", rc, msg)
    assert rc == _lib.LMGPU_HIP_ERROR and math.isnan(alpha) and n == -1
    assert "after %d trials" % nr.MAX_TRIALS in msg and "|direction| = 0" in msg
    assert opt.host_waits() == 3
    assert np.array_equal(_packed_values(opt), before)
    _same_as_a_fresh_handle(opt, "five_pose")
    opt.close()
