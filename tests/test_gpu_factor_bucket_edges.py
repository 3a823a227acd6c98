"""The factor-bucket kernels of csrc/kernels_factors.hpp at their noise, launch and wave edges, against the long-double reference chain
of tests/factor_bucket_cases.py over the 50-digit unwhitened blocks of tests/golden/factor_bucket_edges.npz (only the fixture is read
here; tests/test_factor_bucket_reference.py checks the chain against mpmath and plants the defects these tests must catch):

  whiten        every factor type under Diagonal and Gaussian noise, a noise row of its own per factor, 1 / 127 / 128 / 129 factors
  sfm_blocks    the 256-lane SFM linearize (LDS tile, lin / 26 store, g < total guard) and error kernels on 255 / 256 / 257 / 513 factors
  robust        the eight m-estimators over Diagonal and Gaussian noise on 2-, 6- and 9-row factors, whitened |b| on both sides of k
  interleaved   eight buckets cycled one factor at a time (graph order != bucket order: epos, FacDesc.joff), also under GNC weights
  linear_error  every path of linear_error_kernel: staged (odd and padded pitch, one and two trips, ragged, one lane), direct (a shape
                above 32 doubles; mixed; same shape but not back to back), the 12-column form and the column loop, empty waves
  hessian_diag  a hub in all three column positions of 300 factors, ntot = 255 / 256 / 257
  reduce        1 ... 65 537 exactly representable terms: reduce_stage1 / 2 on both sides of their grid-stride switch
  retract       255 / 256 / 257 variables of every type, all types in one graph under a shuffled ordering

Tolerances: geometry_edges.tolerance(floor) = 16 x max(floor, 2^-52), never above 1e-9; the floor is the CPU oracle's own deviation
from the reference for that factor type, noise kind and m-estimator (stored in the fixture).  Deviations are relative to
max(1, |expected|) of that case and quantity.  retract has a one-ulp floor; reduce adds the rounding of its longest add chain.
The reductions are deterministic by design: a repeated call must return the same bits."""
import math

import numpy as np
import pytest

import factor_bucket_cases as fb
import geometry_edges as ge
from gtsam_personal_amd import LevenbergMarquardtOptimizer, Ordering
from gtsam_personal_amd.graph import CAM_BUNDLER, N_DIAG, N_GAUSS, N_UNIT, POSE2, POSE3
from gtsam_personal_amd.optimizer import GncLMParams, GncOptimizer

pytestmark = pytest.mark.gpu

WORST = {}   # largest device deviation per quantity, printed by the last test of the module


def _note(q, d):
    WORST[q] = max(WORST.get(q, 0.0), float(d))


@pytest.fixture(scope="module")
def fx():
    return fb.load()


def _optimizer(c):
    return LevenbergMarquardtOptimizer(c.graph, c.values, c.ordering, device=0)


def _check_linearization(fx, c, opt, blocks, solve=False):
    """linearize() + jacobian(g) of every factor, graph_error(), hessian_diagonal() (and solve()) of `opt` against the reference
    blocks; every call twice, the second returning the same bits"""
    opt.linearize()
    bad, slack = [], 0.0
    J = [opt.jacobian(g) for g in range(len(c.factors))]
    for g, (f, (Ab, err, _)) in enumerate(zip(c.factors, blocks)):
        i = fb.floor_index(f)
        tJ, te = ge.tolerance(fx["floor_J"][i]), ge.tolerance(fx["floor_err"][i])
        d = fb.dev(J[g], fb.to_f64(Ab))
        _note("[A b]", d)
        if not d <= tJ:
            bad.append("factor %d type %d case %d kind %d robust %d: [A b] %.3g (tol %.3g)" % (g, f["ft"], f["case"], i[1], i[2], d, tJ))
        slack += te * max(1.0, float(err))
        if not i[2]:    # without Robust the factor's error is 0.5 |b|^2 of its own (weighted) b
            de = fb.dev(0.5 * float(J[g][:, -1] @ J[g][:, -1]), float(err))
            _note("error", de)
            if not de <= te:
                bad.append("factor %d type %d case %d kind %d: 0.5 |b|^2 %.3g (tol %.3g)" % (g, f["ft"], f["case"], i[1], de, te))
    assert not bad, "%s\n%s" % (c.name, "\n".join(bad[:20]))
    expected = fb.fsum(b[1] for b in blocks)
    err = opt.graph_error()
    _note("error", abs(err - expected) / max(1.0, expected))
    assert abs(err - expected) <= slack, (c.name, err, expected, slack)
    # the Hessian diagonal, per variable
    rk = max(f["model"].robust_kind for f in c.factors)
    th, hd, ref = ge.tolerance(fx["floor_hdiag"][rk]), opt.hessian_diagonal(), c.hessian_diagonal(blocks)
    for k in ref:
        d = fb.dev(hd[k], fb.to_f64(ref[k]))
        _note("hessian diagonal", d)
        assert d <= th, (c.name, k, d, th)
    # bitwise repeats
    opt.linearize()
    assert all(np.array_equal(opt.jacobian(g), J[g]) for g in range(len(c.factors))), c.name
    assert opt.graph_error() == err, c.name
    hd2 = opt.hessian_diagonal()
    assert all(np.array_equal(hd[k], hd2[k]) for k in hd), c.name
    if solve:
        by_key, packed, e0, e1 = opt.solve(fb.LAMBDA)
        assert np.all(np.isfinite(packed)) and packed.size == c.values.dim()
        r0, r1 = c.linear_errors(blocks, by_key)   # at the RETURNED delta: the check does not depend on the factorisation
        for q, got, want in ((0, e0, r0), (1, e1, r1)):
            d = fb.dev(got, want)
            _note("e0 / e1", d)
            assert d <= ge.tolerance(fx["floor_lin"][q]), (c.name, "e%d" % q, got, want, d)
        _, packed2, f0, f1 = opt.solve(fb.LAMBDA)
        assert np.array_equal(packed, packed2) and (e0, e1) == (f0, f1), c.name
    return J, err


# ---------------------------------------------------------------- noise models at the block edges
@pytest.mark.parametrize("kind", (N_DIAG, N_GAUSS), ids=("diag", "gauss"))
@pytest.mark.parametrize("ft", fb.FACTOR_TYPES)
def test_whiten(fx, ft, kind):
    for n in fb.WHITEN_SIZES:
        c = fb.build(fx, "whiten_t%d_%s_n%d" % (ft, fb.KIND_NAME[kind], n))
        _check_linearization(fx, c, _optimizer(c), c.reference_blocks())


@pytest.mark.parametrize("n", fb.SFM_SIZES)
@pytest.mark.parametrize("kind", (N_UNIT, N_DIAG, N_GAUSS), ids=("unit", "diag", "gauss"))
def test_sfm_blocks(fx, kind, n):
    c = fb.build(fx, "sfm_%s_n%d" % (fb.KIND_NAME[kind], n))
    _check_linearization(fx, c, _optimizer(c), c.reference_blocks())


@pytest.mark.parametrize("rk", range(1, 9))
@pytest.mark.parametrize("kind", (N_DIAG, N_GAUSS), ids=("diag", "gauss"))
@pytest.mark.parametrize("ft", fb.ROBUST_TYPES)
def test_robust(fx, ft, kind, rk):
    c = fb.build(fx, "robust_t%d_%s_m%d" % (ft, fb.KIND_NAME[kind], rk))
    _check_linearization(fx, c, _optimizer(c), c.reference_blocks())


# ---------------------------------------------------------------- graph order against bucket order, GNC weights
def test_interleaved(fx):
    c = fb.build(fx, "interleaved")
    _check_linearization(fx, c, _optimizer(c), c.reference_blocks(), solve=True)


def test_interleaved_gnc(fx):
    """weights in [0, 1] (some exactly 0 and 1) through GncOptimizer.setWeights: [A b] carries sqrt(w), the error w; with the weights
    set back to one the results are those of the unweighted optimizer bit for bit"""
    c = fb.build(fx, "interleaved_gnc")
    plain = fb.build(fx, "interleaved")
    opt = _optimizer(plain)
    opt.linearize()
    J0 = [opt.jacobian(g) for g in range(len(plain.factors))]
    e0, h0 = opt.graph_error(), opt.hessian_diagonal()
    s0 = opt.solve(fb.LAMBDA)
    gnc = GncOptimizer(c.graph, c.values, GncLMParams(), c.ordering, device=0)
    gnc.setWeights(c.weights)
    assert np.array_equal(gnc.getWeights(), c.weights)
    _check_linearization(fx, c, gnc.base(), c.reference_blocks(), solve=True)
    gnc.setWeights(np.ones(len(c.factors)))
    base = gnc.base()
    base.linearize()
    assert all(np.array_equal(base.jacobian(g), J0[g]) for g in range(len(c.factors)))
    assert base.graph_error() == e0
    h1 = base.hessian_diagonal()
    assert all(np.array_equal(h0[k], h1[k]) for k in h0)
    s1 = base.solve(fb.LAMBDA)
    assert np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]


# ---------------------------------------------------------------- linear_error_kernel, hessian_diag_kernel
@pytest.mark.parametrize("name", fb.names("linear_error"))
def test_linear_error(fx, name):
    c = fb.build(fx, name)
    _check_linearization(fx, c, _optimizer(c), c.reference_blocks(), solve=True)


@pytest.mark.parametrize("ntot", fb.HDIAG_NTOT)
def test_hessian_diag(fx, ntot):
    c = fb.build(fx, "hdiag_ntot%d" % ntot)
    _check_linearization(fx, c, _optimizer(c), c.reference_blocks())


# ---------------------------------------------------------------- the two-stage reduction
def reduce_tolerance(n, total):
    """the one-ulp floor's tolerance plus the rounding of the longest add chain of reduce_stage1 / 2: ceil(n / (256 g)) + 8 +
    ceil(g / 256) + 8 additions with g = min(256, ceil(n / 256)), each at most 2^-53 of the sum"""
    g = min(256, -(-n // 256))
    return (ge.tolerance(ge.EPS) + (-(-n // (256 * g)) + 8 + -(-g // 256) + 8) * 2.0 ** -53) * max(1.0, total)


@pytest.mark.parametrize("n", fb.REDUCE_SIZES)
def test_reduce(n):
    graph, values, terms = fb.reduce_problem(n)
    opt = LevenbergMarquardtOptimizer(graph, values, Ordering.Natural(graph), device=0)
    total = math.fsum(terms)
    err = opt.graph_error()
    _note("reduce", abs(err - total) / max(1.0, total))
    assert abs(err - total) <= reduce_tolerance(n, total), (n, err, total)
    assert opt.graph_error() == err
    opt.linearize()
    for g in sorted({0, 254, 255, 256, 65535, n - 1} & set(range(n))):
        J, x = opt.jacobian(g), values.at(g)
        assert np.array_equal(J[:, :3], np.eye(3)) and np.array_equal(J[:, 3], 1.0 - x), (n, g)   # b = m - x, exact
    assert opt.graph_error() == err


# ---------------------------------------------------------------- retract
def _retract_deviation(vt, got, exp):
    if vt in (POSE2, POSE3, CAM_BUNDLER):
        return ge.retract_deviation(vt, got, exp)
    return fb.dev(got, exp), 0.0


@pytest.mark.parametrize("n", fb.RETRACT_SIZES)
def test_retract(fx, n):
    c = fb.build(fx, "retract_n%d" % n)
    opt = _optimizer(c)
    packed = np.concatenate([c.delta[k] for k in opt.ordering])
    opt.retract(packed)
    got, tol, bad = opt.values(), ge.tolerance(ge.EPS), []
    for k, (vt, exp) in c.expected.items():
        d, ortho = _retract_deviation(vt, got.at(k), exp)
        _note("retract", d)
        if not (d <= tol and ortho <= ge.ORTHO_TOL):
            bad.append("key %d type %d: value %.3g (tol %.3g)  R^T R - I %.3g (tol %.3g)" % (k, vt, d, tol, ortho, ge.ORTHO_TOL))
    assert not bad, "\n".join(bad[:20])
    # the same retraction from the same values gives the same bits
    opt.set_values(c.values)
    opt.retract(packed)
    again = opt.values()
    assert all(np.array_equal(got.at(k), again.at(k)) for k in c.expected)


def test_report_largest_deviations():
    """not a check: prints what the module measured (run with -s)"""
    for q in sorted(WORST):
        print("largest device deviation, %-16s %.3g" % (q, WORST[q]))
