"""lds_front_group_kernel and lds_backsub_group_kernel (csrc/kernels_leaf.hpp: small leaf fronts four to a wave, 16 lanes each, on the way up
and on the way down) and the kernels they take the place of (lds_front_kernel<true>, lds_backsub_kernel; LMGPU_NO_LEAF_GROUPS and
LMGPU_NO_BACKSUB_GROUPS on the test library force them) on the cases of tests/leaf_group_cases.py: every front's [R S d] and delta
against the dense extended-precision reference built from the DEVICE's own Jacobians, with the harness and the tolerance rule of
tests/test_gpu_schur_edges.py -- per front max(16 x the oracle-vs-reference floor of the case, 64 n 2.2e-16), 16 x floor above 1e-9
fails the case.  Two passes (lambda = 1e-6 with identity damping; retract; lambda = 1e-2 with diagonal damping), each solve repeated
and bitwise equal.  Every run asserts through lmgpu_leaf_group_launches that the intended elimination kernel is the one that ran.

  every case                         the default form (product library); LMGPU_NO_LEAF_GROUPS; LMGPU_NO_BACKSUB_GROUPS; both switches
  GRAPH_CASES                        the four forms again with LMGPU_GRAPH=1 (lambda from device memory: the replayed launch sequence)
  FORM_CASES                         the elimination kernel with one wave per workgroup (LMGPU_LEAF_GROUP_THREADS=64; four by default)
  sfm_n3                             marginalCovariance of the point that carries the prior (the extra gradient term), rule of
                                     tests/test_gpu_lds_front_edges.py
  leaf_group_cases.single_observation_case   lambda = 0: the once-seen point fails; both elimination kernels report the same front

The leaf levels of sfm_counts and sfm_33 (a leaf of 135 separator columns) take lds_backsub_group_kernel<4, 9>, every other one <3, 6>.

Measured on an MI355X (deviation = max|X - X_ref| / max|X_ref| per front, worst over the leaves / over all fronts; relative 2-norm for
delta; device = worst over both passes and every form the case runs under; tolerance = of the narrowest front / of delta):
                      oracle floor          device                           tolerance
    case              [R S d]   delta       leaves    all fronts  delta
    sfm_counts        5.8e-14   1.3e-11     5.8e-15   5.8e-15     8.3e-12    9.2e-13 / 2.0e-10
    sfm_n1            3.0e-14   2.3e-12     2.1e-16   3.8e-14     1.4e-12    4.8e-13 / 3.7e-11
    sfm_n3            1.0e-14   9.9e-14     2.7e-16   2.4e-14     1.1e-13    3.1e-13 / 2.6e-12
    sfm_n4            7.0e-15   7.3e-14     3.4e-16   5.4e-15     1.5e-13    3.1e-13 / 2.6e-12
    sfm_n5            2.1e-15   1.6e-13     2.8e-16   2.5e-15     2.2e-13    3.1e-13 / 2.6e-12
    sfm_twice         1.2e-14   1.3e-13     2.1e-16   1.4e-14     6.5e-14    3.1e-13 / 2.6e-12   (generic elimination kernel in every form)
    sfm_33            5.0e-15   5.3e-14     2.8e-16   3.9e-15     4.1e-14    3.1e-13 / 2.6e-12   (generic elimination kernel in every form)
    planar            2.4e-13   8.4e-13     6.1e-16   2.2e-13     4.8e-13    3.8e-12 / 1.3e-11
    planar_pose       2.2e-13   5.8e-13     1.2e-15   2.1e-13     7.6e-13    3.5e-12 / 9.3e-12
    marginal (sfm_n3) oracle 1.3e-13, device 2.0e-13, tolerance 2.6e-12
The leaves themselves sit at a few ulp in either kernel; the "all fronts" column is the root and the 184-column point above them.
Every pass also reads each gather leaf's (rhs, rhs) corner back from the device (lmgpu_get_leaf_corner) and holds it against b'b - d'd of
the reference: worst |c - c_ref| / b'b over all cases and forms 7.1e-16.  The back-substitution form (none / <3, 6> / <4, 9>) is asserted
through lmgpu_backsub_group_launches in every run.
"""
import numpy as np
import pytest

import leaf_group_cases as lg
import lds_front_cases as lc
import schur_cases as sc
from gtsam_personal_amd import _lib
from test_gpu_parity import _check_linearize, _check_solve, _pair
from test_gpu_schur_edges import CAP, EPS, FACTOR, _reference

pytestmark = pytest.mark.gpu

OFF = "LMGPU_NO_LEAF_GROUPS"
OFF_B = "LMGPU_NO_BACKSUB_GROUPS"
GRAPH_CASES = ("sfm_counts", "sfm_n5", "planar_pose")
FORM_CASES = ("sfm_counts", "planar_pose")


def _corners(c, opt, ref, fronts, infos, fl):
    """the (rhs, rhs) corner b'b - d'd that every gather leaf hands to the root's Schur gather, read back from the device, against the
    reference's d and the device's own b.  Bound: d deviates by at most tol x max|X_ref| per entry (the front's [R S d] tolerance), so d'd
    by 2 sqrt(nf) tol max|X_ref| |d|; the two sums add 64 n eps b'b."""
    fk = c["graph"].factor_keys_in_graph_order()
    bsq = [float(np.sum(opt.jacobian(g)[:, -1] ** 2)) for g in range(len(fk))]
    worst = 0.0
    for i, f in enumerate(infos):
        if f["cls"] != 0:
            continue
        frontal = set(fronts[i][0][:fronts[i][1]])
        btb = sum(bsq[g] for g in range(len(fk)) if frontal & set(fk[g]))
        X = ref.front(i)
        d = np.asarray(X[:, -1], dtype=np.float64)
        want = btb - float(d @ d)
        tol = max(FACTOR * fl["rsd"], 64 * f["n"] * EPS)
        bound = 2 * np.sqrt(f["nf"]) * tol * float(np.abs(X).max()) * float(np.linalg.norm(d)) + 64 * f["n"] * EPS * btb
        got = opt.leaf_corner(i)
        assert abs(got - want) <= bound, (i, f, got, want, bound)
        assert float(d @ d) > 1e3 * bound  # the planted mistake (corner without - d'd) would miss by that much
        worst = max(worst, abs(got - want) / btb)
    return worst


def _run(name, groups=True, backsub_groups=True):
    c, fl = lg.case(name), lg.oracle_floor(name)
    assert FACTOR * fl["rsd"] <= CAP and FACTOR * fl["delta"] <= CAP, fl
    opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    assert opt.leaf_group_launches() == (lg.expected_group_launches(c) if groups else 0)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert opt.backsub_group_launches() == (lg.BACKSUB_FORMS[name] if backsub_groups else (0, 0))
    fronts = [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))]
    widest = max(f["n"] for f in infos)
    worst = [0.0, 0.0]
    for p, (lam, diagonal) in enumerate(lg.PASSES):
        _check_linearize(opt, orc, c["graph"])
        ref = _reference("leaf_group_" + name, c, opt, fronts, lam, diagonal)
        assert ref.residual < 1e-17
        dk = _check_solve(opt, orc, lam, diagonal)
        rsd = [opt.front(i)[1] for i in range(len(infos))]
        per_front, dd = sc.deviations(ref, lambda i: rsd[i], dk)
        tol_d = max(FACTOR * fl["delta"], 64 * widest * EPS)
        leaf_dev = max(d for d, f in zip(per_front, infos) if f["cls"] == 0)
        print(f"LGROW {name} pass {p} (lambda {lam:g}, {'diagonal' if diagonal else 'identity'}): [R S d] leaves {leaf_dev:.2e}, all fronts {max(per_front):.2e} "
              f"(tolerance of the narrowest {max(FACTOR * fl['rsd'], 64 * min(f['n'] for f in infos) * EPS):.2e}), delta {dd:.2e} (tolerance {tol_d:.2e}); "
              f"floor [R S d] {fl['rsd']:.2e}, delta {fl['delta']:.2e}")
        worst = [max(worst[0], max(per_front)), max(worst[1], dd)]
        for i, dev in enumerate(per_front):
            assert dev <= max(FACTOR * fl["rsd"], 64 * infos[i]["n"] * EPS), (name, p, i, infos[i], dev)
        assert dd <= tol_d, (name, p, dd)
        print(f"LGROW {name} pass {p}: leaf corners, worst |c - c_ref| / b'b {_corners(c, opt, ref, fronts, infos, fl):.2e}")
        dk2, _, _, _ = opt.solve(lam, diagonal)  # the same solve again: bitwise
        assert all(np.array_equal(dk[k], dk2[k]) for k in dk)
        assert all(np.array_equal(rsd[i], opt.front(i)[1]) for i in range(len(infos)))
        if p == 0:
            opt.retract()
            orc.retract({k: dk[k] for k in dk})
    opt.close()
    return worst


@pytest.mark.parametrize("name", list(lg.CASES))
def test_leaf_groups_against_dense_reference(name):
    _run(name)


# the switched forms (test library): the generic elimination kernel, the wave-per-front back-substitution, both
FORMS = {"no_leaf_groups": (OFF,), "no_backsub_groups": (OFF_B,), "neither": (OFF, OFF_B)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(lg.CASES))
def test_switched_forms_on_the_same_cases(monkeypatch, dev_switches, name, form):
    for sw in FORMS[form]:
        monkeypatch.setenv(sw, "1")
    _run(name, groups=OFF not in FORMS[form], backsub_groups=OFF_B not in FORMS[form])


@pytest.mark.parametrize("form", ["default"] + list(FORMS))
@pytest.mark.parametrize("name", GRAPH_CASES)
def test_leaf_groups_graph_replay(monkeypatch, dev_switches, name, form):
    monkeypatch.setenv("LMGPU_GRAPH", "1")
    for sw in FORMS.get(form, ()):
        monkeypatch.setenv(sw, "1")
    _run(name, groups=OFF not in FORMS.get(form, ()), backsub_groups=OFF_B not in FORMS.get(form, ()))


@pytest.mark.parametrize("name", FORM_CASES)
def test_leaf_group_kernel_one_wave_per_workgroup(monkeypatch, dev_switches, name):
    monkeypatch.setenv("LMGPU_LEAF_GROUP_THREADS", "64")
    _run(name)


def test_marginal_of_a_point_in_a_group_launch():
    import oracle_harness as oh
    from gtsam_personal_amd import Marginals
    from gtsam_personal_amd.graph import P
    c = lg.case("sfm_n3")
    key = P(1)  # the point with four cameras and the prior
    assert c["unary"][key] == [3]
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    assert orc.solve(0.0, False)[0] == 0
    oref = sc.reference(c, [orc.jacobian(g) for g in range(c["graph"].size())], [(k, nfk) for k, nfk, _, _ in orc.cliques()], 0.0, False)
    m = Marginals(c["graph"], c["initial"], c["ordering"])
    opt = m._opt
    assert opt.leaf_group_launches() == 1
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    opt.linearize()
    jac = [opt.jacobian(g) for g in range(c["graph"].size())]
    ref = sc.reference(c, jac, [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))], 0.0, False)
    assert ref.residual < 1e-17 and oref.residual < 1e-17
    want = lc.covariance_block(ref, key)
    floor = lc.block_deviation(orc.marginal_covariance(key, want.shape[0]), lc.covariance_block(oref, key))
    assert lc.FACTOR * floor <= lc.CAP
    tol = lc.marginal_tolerance(floor, max(f["n"] for f in infos))
    cov = m.marginalCovariance(key)
    dev = lc.block_deviation(cov, want)
    print(f"LGROW marginal sfm_n3: oracle floor {floor:.1e}  device {dev:.1e}  tolerance {tol:.1e}")
    assert dev <= tol, (dev, tol)
    assert np.array_equal(m.marginalCovariance(key), cov)
    m.close()


def test_underdetermined_leaf_reports_the_same_front(monkeypatch, dev_switches):
    """lambda = 0 and a point with a single observation: its third pivot is zero up to rounding (a pivot <= 0, or the pivot-exponent
    test).  A solver status (IndeterminantLinearSystemException), the same from both kernels"""
    from gtsam_personal_amd import LevenbergMarquardtOptimizer, LevenbergMarquardtParams
    c = lg.single_observation_case()
    slots = []
    for off in (False, True):
        if off:
            monkeypatch.setenv(OFF, "1")
        opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], LevenbergMarquardtParams(), device=0)
        assert opt.leaf_group_launches() == (0 if off else 1)
        opt.linearize()
        with pytest.raises(_lib.IndeterminantLinearSystemException) as e:
            opt.solve(0.0, False)
        slots.append(e.value.slot)
        dk, _, _, _ = opt.solve(1e-3, False)  # and the handle goes on working
        assert all(np.isfinite(v).all() for v in dk.values())
        opt.close()
    assert slots[0] == slots[1], slots
