"""CPU tests around the Dogleg's Bayes-tree products (csrc/kernels_bayes.hpp) and its host step (csrc/dogleg_step.hpp): no device.

  * the case set of bt_products_cases covers every edge value of the five kernels and of the slot table (front_info of structure-only
    handles against bt_products_cases.EDGES);
  * the floor: the float64 oracle's cliques, multiplied out in float64 numpy, against the extended-precision reference -A^T b /
    ||A x - alpha b||^2 - alpha^2 (||b||^2 - ||d||^2); 16 x floor <= 1e-9 per case;
  * a float64 numpy restatement of the five loops passes the tolerance as it is and misses it by more than 100 x with each of seven planted
    defects, each on a named case;
  * dogleg_trial_point / dogleg_radius_update (through lmgpu_selftest_dogleg_step) against np.longdouble at their thresholds;
  * the long-double restatement of one whole Dogleg iteration against the oracle's dl_iterate on bt_products_cases.RUNS: radius, error,
    step, trial count, and the branch of every trial as EXPECTED writes it down, under the margins that make those branches safe for a
    float64 implementation.

Measured (this module, float64 oracle against the restatement over all iterations of all fifteen runs): radius at most 4.4e-15, error at
most 1.9e-15, step at most 2.0e-11 (relative 2-norm; the late Newton steps, which shrink towards the rounding error of d); the trial counts
are equal.  The planted defects miss the tolerance by 1.9e6 x (the skipped column) to 3.2e12 x, the unchanged restatement stays below 3e-3 x."""
import ctypes as ct

import numpy as np
import pytest

import bt_products_cases as bc
from dense_reference import LD
from gtsam_personal_amd import LevenbergMarquardtOptimizer, _lib

EPS = float(np.finfo(np.float64).eps)


def _structure(name):
    c = bc.case(name)
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    keys = [opt.front(i, numeric=False)[0] for i in range(len(infos))]
    opt.close()
    return infos, keys


def test_cases_cover_every_edge():
    s = bc.summary({name: _structure(name) + (bc.slot_offsets(bc.case(name))[1],) for name in bc.CASES})
    missing = [edge for edge, seen in bc.EDGES.items() if not seen(s)]
    assert not missing, missing


def test_products_tap_refuses_a_handle_without_a_factor():
    c = bc.case("staging[31]")
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)
    with pytest.raises(_lib.LmgpuError, match="lmgpu_bt_products"):
        opt.bt_products(np.zeros(opt._ntot), 1.0)
    opt.close()


@pytest.mark.parametrize("name", list(bc.CASES))
def test_oracle_floor(name):
    fl = bc.oracle_floor(name)
    print(f"FLOOR {name:20s} gradient {fl['gradient']:.1e}  norm {fl['norm']:.1e}")
    assert bc.FACTOR * fl["gradient"] <= bc.CAP and bc.FACTOR * fl["norm"] <= bc.CAP, fl


# ---------------------------------------------------------------------------------------------------------------- planted defects
DEFECT_CASE = dict(zip(bc.DEFECTS, ("bin[65,73]", "bin[65,73]", "staging[31]", "medium_batch", "chain[576]", "children[5]", "children[5]")))
_restated = {}


def _restatement(name):
    """(restated fronts from the oracle's cliques, reference, gradient of the reference, tolerances) at the case's start"""
    if name not in _restated:
        c = bc.case(name)
        _, jac, cliques = bc.oracle_pass(c, 0)
        infos, _ = _structure(name)
        fl, widest = bc.oracle_floor(name), max(f["n"] for f in infos)
        ref = bc.ProductsReference(c, jac)
        _restated[name] = (bc.restated_fronts(infos, cliques), ref, ref.gradient(), bc.tolerance(fl["gradient"], widest), bc.tolerance(fl["norm"], widest))
    return _restated[name]


def _worst(name, defect):
    """(gradient deviation / tolerance, norm deviation / tolerance), worst over the probes"""
    fronts, ref, g_ref, tol_g, tol_n = _restatement(name)
    off, dims, ntot = bc.slot_offsets(bc.case(name))
    wg = wn = 0.0
    for x, alpha in bc.probes(ntot):
        s, g = bc.restated_products(fronts, off, dims, ntot, x, alpha, defect)
        wg, wn = max(wg, bc.gradient_deviation(g, g_ref) / tol_g), max(wn, bc.norm_deviation(s, ref.sq_norm(x, alpha)) / tol_n)
    return wg, wn


@pytest.mark.parametrize("name", sorted(set(DEFECT_CASE.values())))
def test_restatement_passes_as_it_is(name):
    wg, wn = _worst(name, None)
    print(f"{name}: gradient {wg:.2e} x tolerance, norm {wn:.2e} x tolerance")
    assert wg <= 1 and wn <= 1


@pytest.mark.parametrize("defect", bc.DEFECTS)
def test_planted_defect_misses_by_100(defect):
    name = DEFECT_CASE[defect]
    wg, wn = _worst(name, defect)
    print(f"DEFECT {defect!r} on {name}: gradient {wg:.1e} x tolerance, norm {wn:.1e} x tolerance")
    assert max(wg, wn) > 100, (defect, name, wg, wn)


# ---------------------------------------------------------------------------------------------------------------- dogleg_step.hpp
def _trial(delta, uu, nn, un):
    out = (ct.c_double * 2)()
    assert _lib.load().lmgpu_selftest_dogleg_step(0, (ct.c_double * 4)(delta, uu, nn, un), out) == 0
    return int(out[0]), out[1]


def _update(rho, delta, norm):
    out = (ct.c_double * 3)()
    assert _lib.load().lmgpu_selftest_dogleg_step(1, (ct.c_double * 3)(rho, delta, norm), out) == 0
    return out[0], bool(out[1]), bool(out[2])


def _next(x, up):
    return float(np.nextafter(x, np.inf if up else -np.inf))


def _tau_tolerance(delta, uu, nn, un):
    """a root of a tau^2 + b tau + c moves by (|da| tau^2 + |db| tau + |dc|) / |2 a tau + b| = ... / sqrt(b^2 - 4 a c); a, b, c are sums of
    uu, un, nn, delta^2 with a few roundings each, tau <= 1: 32 eps (uu + 2 |un| + nn + delta^2) / sqrt(disc), plus the division's own 4 eps"""
    uu, nn, un, dsq = LD(uu), LD(nn), LD(un), LD(delta) * LD(delta)
    a, b, c = uu - 2 * un + nn, 2 * (un - uu), uu - dsq
    return float(32 * EPS * (uu + 2 * abs(un) + nn + dsq) / np.sqrt(b * b - 4 * a * c) + 4 * EPS)


def test_trial_point_thresholds():
    """delta^2 equal to, one ulp below and one ulp above uu and nn: the comparisons are strict, so equality takes the later branch"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        delta = float(rng.uniform(0.01, 30))
        dsq = delta * delta
        ratio = float(rng.uniform(4, 25)) ** 2
        for uu, want in ((dsq, bc.BLEND), (_next(dsq, False), bc.BLEND), (_next(dsq, True), bc.STEEPEST)):
            nn = uu * ratio
            un = float(rng.uniform(uu, np.sqrt(uu * nn)))
            branch, scalar = _trial(delta, uu, nn, un)
            lb, ls = bc.trial_point_ld(delta, LD(uu), LD(nn), LD(un))
            assert branch == lb == want, (delta, uu, branch, lb, want)
            if want == bc.STEEPEST:
                assert abs(scalar - float(ls)) <= 4 * EPS and scalar < 1.0
            else:  # tau at the start of the segment: |x_u| = delta to an ulp, so tau is a rounding-sized number, not a negative one
                assert 0.0 <= scalar <= _tau_tolerance(delta, uu, nn, un), scalar
        for nn, want in ((dsq, bc.NEWTON), (_next(dsq, False), bc.NEWTON), (_next(dsq, True), bc.BLEND)):
            uu = nn / ratio
            un = float(rng.uniform(uu, np.sqrt(uu * nn)))
            branch, scalar = _trial(delta, uu, nn, un)
            lb, ls = bc.trial_point_ld(delta, LD(uu), LD(nn), LD(un))
            assert branch == lb == want, (delta, nn, branch, lb, want)
            if want == bc.NEWTON:
                assert scalar == 1.0
            else:  # tau at the end of the segment
                assert abs(scalar - 1.0) <= _tau_tolerance(delta, uu, nn, un), scalar


def test_trial_point_blend_against_long_double():
    """tau of Gram-consistent inputs (uu, nn, un of two random vectors, |x_N| / |x_u| >= 4) and the point it gives: on the sphere"""
    rng = np.random.default_rng(6)
    for _ in range(300):
        n = int(rng.integers(2, 40))
        u, v = rng.standard_normal(n), rng.standard_normal(n) * rng.uniform(4, 25)
        v *= max(1.0, 4.2 * np.linalg.norm(u) / np.linalg.norm(v))
        uu, nn, un = float(u @ u), float(v @ v), float(u @ v)
        delta = float(np.sqrt(uu) + rng.uniform(0.02, 0.98) * (np.sqrt(nn) - np.sqrt(uu)))
        branch, tau = _trial(delta, uu, nn, un)
        lb, lt = bc.trial_point_ld(delta, LD(uu), LD(nn), LD(un))
        assert branch == lb == bc.BLEND
        assert abs(tau - float(lt)) <= _tau_tolerance(delta, uu, nn, un), (tau, float(lt))
        t = LD(tau)
        radius = np.sqrt(LD(uu) * (1 - t) ** 2 + 2 * LD(un) * t * (1 - t) + LD(nn) * t * t)
        assert 0.0 <= tau <= 1.0 and abs(float(radius) - delta) <= 1e-12 * delta


# In exact arithmetic tau1 lies in [0, 1) whenever uu <= delta^2 < nn (the quadratic is <= 0 at 0 and > 0 at 1), and sqrt(b^2 - 4 a c) >= |b|
# survives rounding, so tau1 >= 0 always: the second root is only ever taken when tau1 ROUNDS above 1 + eps.  No Gram-consistent input out
# of 700000 random ones did (near-parallel x_u, x_N and delta^2 within three ulps of nn included); these two, found by a random search
# over (uu, nn, un) that no pair of vectors has (un^2 > uu nn), pin the window from both sides: (delta, uu, nn, un), takes the first root
WINDOW = (
    # tau1 evaluates to 1 + 1.66e-12 > 1 + eps: the second root, -22177.79...
    (("0x1.382c9a3881e1fp+7", "0x1.d26c0532f5390p+0", "0x1.7cacbfaf1ceb8p+14", "0x1.7cafa48d1eb33p+13"), False),
    # tau1 evaluates to 1 + eps exactly: still inside
    (("0x1.e7d4fd28e96edp+1", "0x1.48ffba39a0b68p+0", "0x1.d0ce0632f7202p+3", "0x1.9b9af95650dc5p+2"), True),
)


@pytest.mark.parametrize("inputs,first", WINDOW)
def test_trial_point_root_window(inputs, first):
    delta, uu, nn, un = (float.fromhex(x) for x in inputs)
    branch, tau = _trial(delta, uu, nn, un)
    assert branch == bc.BLEND
    a, b, c = LD(uu) - 2 * LD(un) + LD(nn), 2 * (LD(un) - LD(uu)), LD(uu) - LD(delta * delta)
    sq = np.sqrt(b * b - 4 * a * c)
    roots = ((-b + sq) / (2 * a), (-b - sq) / (2 * a))
    assert abs(float(roots[0]) - 1.0) < 1e-9 and float(roots[1]) < -1.0  # what the two cases are about
    want = float(roots[0 if first else 1])
    assert abs(tau - want) <= 1e-9 * abs(want), (tau, want)
    assert (tau == 1.0 + EPS) if first else (tau < -1.0)


def test_radius_update_thresholds():
    """rho at 0.75, 0.25, 0 and their neighbours, NaN; delta at 1e-5 and its neighbours; max(delta, 3 |dx_d|) from both sides"""
    rhos = [th2 for th in (0.75, 0.25, 0.0) for th2 in (_next(th, False), th, _next(th, True))] + [1.0, 0.5, 0.1, -1.0, -0.0, float("nan"), float("inf"), -float("inf")]
    deltas = [_next(1e-5, False), 1e-5, _next(1e-5, True), 0.3, 1000.0]
    for rho in rhos:
        for delta in deltas:
            for norm in (0.0, delta / 3, _next(delta / 3, True), 0.7 * delta, delta, 2.5 * delta):
                got = _update(rho, delta, norm)
                want = bc.radius_update_ld(rho, delta, LD(norm))
                assert got == (float(want[0]), want[1], want[2]), (rho, delta, norm, got, want)
                # and by the rules themselves
                halved = delta * 0.5 if delta > 1e-5 else delta
                if rho >= 0.75:
                    assert got == (max(delta, 3.0 * norm), False, True)
                elif rho >= 0.25:
                    assert got == (delta, False, True)
                elif rho >= 0.0:
                    assert got == (halved, False, True)
                else:  # rho < 0 or NaN
                    assert got == (halved, delta > 1e-5, delta > 1e-5)
                assert got[2] or (delta <= 1e-5 and not rho >= 0.0)  # moved = false only at the floor, and only while f rises
    assert _lib.load().lmgpu_selftest_dogleg_step(2, (ct.c_double * 4)(), (ct.c_double * 3)()) == -1
    assert _lib.load().lmgpu_selftest_dogleg_step(0, None, None) == -1


def test_radius_floor_ends_the_halving():
    """the loop of dl_iterate on a function that rises at every trial point: from 1000 the radius halves 27 times (1000 / 2^27 = 7.45e-6 is
    the first value not above 1e-5), then the step is dropped and the loop ends -- no graph decides this"""
    delta, trials = 1000.0, 0
    while True:
        delta, stay, moved = _update(-1.0, delta, 0.0)
        trials += 1
        if not stay:
            break
    assert (delta, moved, trials) == (1000.0 / 2 ** 27, False, 28)


# ---------------------------------------------------------------------------------------------------------------- one whole iteration
@pytest.mark.parametrize("name", list(bc.RUNS))
def test_restated_iteration_against_oracle(name):
    its, beyond = bc.restated_run(name)
    expected = bc.RUNS[name][3]
    assert len(its) == len(expected)
    for k, ((it, dev), want) in enumerate(zip(its, expected)):
        print(f"RUN {name:22s} iteration {k}: {bc.words(it):20s} |x_N| / |x_u| {it['ratio']:6.2f}  rho " + " ".join(f"{t['rho']:.3f}" for t in it["trials"])
              + f"  f {it['f_error']:.6g} -> {it['error']:.6g}  radius -> {it['delta']:.6g}  oracle: radius {dev['delta']:.1e} error {dev['error']:.1e} step {dev['step']:.1e}")
        assert bc.words(it) == want, (name, k)
        assert it["ratio"] >= bc.MARGIN_RATIO and bc.margins_hold(it), (name, k, it["trials"])
        assert dev["trials"] == len(it["trials"])
        assert all(bc.FACTOR * dev[q] <= bc.CAP for q in ("delta", "error", "step")), dev  # (what the device is then held to: 16 x these)
    # the run stops before the first iteration that fails a margin (or at MAX_ITERATIONS)
    assert beyond is None or not bc.margins_hold(beyond), name
