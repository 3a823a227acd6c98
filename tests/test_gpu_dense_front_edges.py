"""The dense (HBM-class) front at its panel boundaries: the factorisation (panel_dataflow_kernel, diag_potrf_kernel + panel_trsm_kernel,
step_kernel, chain_kernel, front_tail_kernel, syrk_quadrants_kernel, syrk_mfma_kernel, the batched med_*_kernel) and the three
back-substitution forms (hbm_backsolve_blocks_kernel, hbm_backsolve_dataflow2_kernel, hbm_invert_diag_kernel +
hbm_backsolve_dataflow_kernel, with hbm_rhs_init_kernel in front of a front with separators) on the cases of tests/dense_front_cases.py:
every front's [R S d] and delta against the blocked extended-precision reference (tests/dense_reference.py) built from the DEVICE's own
Jacobians.

Per case: the fronts are the ones the case was built for (front_info); linearize (against the oracle); pass 0 = solve with
lambda = 1e-6, identity damping, compare; retract; pass 1 = solve with lambda = 1e-2, diagonal damping, over the previous R (which is
what shows a block left from the previous factorisation), compare again.  Each solve is repeated once with the launch counters on
(set_kernel_timing(1)): the repeat is bitwise equal in delta and in every front, and its `panel` / `syrk` / `chain` launch counts are the
ones the case's launch form has (dense_front_cases: `launches`, and front_launches for a form under a switch; the medium path is told
from the per-front path by the flop count its panel launches do not carry).  The 1e-6 comparison with the oracle (_check_solve) runs alongside.

Tolerance, per front: max(16 x the oracle-vs-reference floor of the case, 64 n 2.2e-16), n = front width; for delta n = the widest
front.  The floor is measured when the test runs; 16 x floor above 1e-9 fails the case.  test_dense_front_reference.py shows on the
CPU that a skipped 4-deep slice of one update tile, a missing lambda on one diagonal entry, a right-hand side that misses one panel
and a stale 16 x 16 block each miss this tolerance by more than 100 x.

The launch forms (dev_switches: the test library) are each compared with the REFERENCE at the same tolerance, not with the default
run: dense_front_cases.SWITCH_RUNS.

Measured on an MI355X (deviation = max|X - X_ref| / max|X_ref| over the fronts, relative 2-norm for delta; device = worst over both
passes; "worst form" = over the default form and every switch the case runs under).  Every repeated solve was bitwise equal, in every
form; every launch count was the expected one.  The device stays within 3 x the float64 oracle's own distance from the reference; every tolerance is the 64 n 2.2e-16 term:
                          oracle floor          device, default form  device, worst form    tolerance (front 0 / delta)
    case                  [R S d]   delta       [R S d]   delta       [R S d]   delta
    medium_batch          1.7e-15   1.1e-14     1.9e-15   1.3e-14     1.9e-15   1.3e-14     2.0e-12 / 3.6e-12
    one_panel[63]         3.9e-16   6.9e-15     5.4e-16   3.9e-15     5.4e-16   3.9e-15     2.0e-12 / 2.0e-12
    one_panel[64]         5.9e-16   1.7e-14     5.7e-16   2.5e-15     5.7e-16   2.5e-15     2.0e-12 / 2.0e-12
    one_panel[65]         7.0e-16   7.1e-15     7.7e-16   5.7e-15     7.7e-16   5.7e-15     2.0e-12 / 2.0e-12
    one_panel[128]        4.1e-16   8.9e-15     4.5e-16   6.6e-15     4.5e-16   6.6e-15     2.9e-12 / 2.9e-12
    one_panel[193]        1.4e-15   4.8e-14     1.4e-15   3.4e-14     1.4e-15   3.4e-14     2.7e-12 / 2.7e-12
    one_panel[255]        1.4e-15   3.1e-14     1.4e-15   1.5e-14     1.4e-15   1.5e-14     3.6e-12 / 3.6e-12
    one_panel[256]        1.4e-15   7.3e-15     1.3e-15   7.9e-15     1.3e-15   7.9e-15     3.6e-12 / 3.6e-12
    tail[257]             3.7e-16   7.8e-15     6.1e-16   1.1e-14     6.1e-16   1.1e-14     3.6e-12 / 3.6e-12
    tail[303]             9.5e-16   1.8e-14     1.1e-15   2.0e-14     1.1e-15   2.3e-14     4.3e-12 / 4.3e-12
    tail[304]             1.2e-15   1.5e-14     1.2e-15   1.7e-14     1.2e-15   1.7e-14     4.3e-12 / 4.3e-12
    tail[319]             1.1e-15   1.0e-14     1.4e-15   1.2e-14     1.4e-15   1.2e-14     4.5e-12 / 4.5e-12
    tail[320]             6.3e-16   8.4e-15     8.4e-16   9.5e-15     8.4e-16   9.5e-15     4.5e-12 / 4.5e-12
    tail[321]             1.2e-15   7.4e-15     9.5e-16   1.9e-14     9.5e-16   1.9e-14     4.5e-12 / 4.5e-12
    chain[576]            1.3e-15   1.6e-14     1.2e-15   1.6e-14     1.2e-15   1.6e-14     8.1e-12 / 8.1e-12
    chain[768]            2.1e-15   6.8e-15     2.2e-15   1.6e-14     2.2e-15   1.6e-14     1.1e-11 / 1.1e-11
    chain[771]            1.9e-15   2.7e-14     2.4e-15   2.9e-14     2.4e-15   2.9e-14     1.1e-11 / 1.1e-11
    chain[832]            3.3e-16   1.4e-14     4.7e-16   1.6e-14     6.7e-16   1.6e-14     1.2e-11 / 1.2e-11
    chain[900]            1.0e-15   6.2e-15     1.6e-15   5.7e-15     1.6e-15   5.8e-15     1.3e-11 / 1.3e-11
    chain[1088]           4.0e-15   1.8e-14     3.9e-15   2.0e-14     3.9e-15   2.0e-14     1.5e-11 / 1.5e-11
    beyond_1024           3.9e-15   1.7e-14     3.9e-15   1.4e-14     3.9e-15   1.4e-14     1.8e-11 / 1.8e-11
    separator[192,70]     1.7e-15   1.6e-14     1.9e-15   9.0e-15     1.9e-15   9.0e-15     3.7e-12 / 3.7e-12
    separator[300,138]    1.3e-15   8.4e-15     8.7e-16   6.8e-15     8.7e-16   6.8e-15     6.2e-12 / 6.2e-12
    separator[96,600]     1.6e-15   1.4e-14     2.3e-15   1.2e-14     2.3e-15   1.2e-14     9.8e-12 / 9.8e-12
    separator[1030,66]    1.9e-15   1.6e-14     2.1e-15   1.6e-14     2.1e-15   1.6e-14     1.5e-11 / 1.5e-11
The whole module takes 80 s, most of it the extended-precision references (14 s for beyond_1024, 9 s for chain[1088] and
separator[1030,66]; the reference is computed once per linearization and shared by the launch forms, which then take 0.2 .. 4 s).
"""
import hashlib

import numpy as np
import pytest

import dense_front_cases as dc
import schur_cases as sc
from test_gpu_parity import _check_linearize, _check_solve, _pair

pytestmark = pytest.mark.gpu

_refs = {}


def _reference(name, c, opt, fronts, lam, diagonal):
    """the reference from the device's tapped Jacobians, once per distinct linearization (the switches do not change it)"""
    lin = opt.linear_graph()
    jac = [lin.at(g).augmentedJacobian() for g in range(c["graph"].size())]
    digest = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in jac)).hexdigest()
    key = (name, lam, diagonal, digest, tuple((tuple(k), n) for k, n in fronts))
    if key not in _refs:
        _refs[key] = sc.reference(c, jac, fronts, lam, diagonal, block=dc.BLOCK)
    return _refs[key]


def _run(name, default_form, switch=None):
    c, fl = dc.case(name), dc.oracle_floor(name)
    assert dc.FACTOR * fl["rsd"] <= dc.CAP and dc.FACTOR * fl["delta"] <= dc.CAP, fl
    opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"]) for f in infos] == c["fronts"], infos
    fronts = [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))]
    tol_rsd, tol_d = dc.tolerances(fl, [f["n"] for f in infos])
    worst = [0.0, 0.0]
    for p, (lam, diagonal) in enumerate(dc.PASSES):
        _check_linearize(opt, orc, c["graph"])
        ref = _reference(name, c, opt, fronts, lam, diagonal)
        assert ref.residual < 1e-17
        dk = _check_solve(opt, orc, lam, diagonal)
        rsd = [opt.front(i)[1] for i in range(len(infos))]
        per_front, dd = sc.deviations(ref, lambda i: rsd[i], dk)
        print(f"{name} pass {p} (lambda {lam:g}, {'diagonal' if diagonal else 'identity'}): [R S d] " + ", ".join(f"{d:.2e}" for d in per_front)
              + " (tolerance " + ", ".join(f"{t:.2e}" for t in tol_rsd) + f"), delta {dd:.2e} (tolerance {tol_d:.2e})")
        worst = [max(worst[0], max(per_front)), max(worst[1], dd)]
        for i, dev in enumerate(per_front):
            assert dev <= tol_rsd[i], (name, p, i, infos[i], dev)
        assert dd <= tol_d, (name, p, dd)
        opt.set_kernel_timing(1)  # the same solve again, counted: bitwise
        dk2, _, _, _ = opt.solve(lam, diagonal)
        kt = opt.kernel_times()
        opt.set_kernel_timing(False)
        assert all(np.array_equal(dk[k], dk2[k]) for k in dk)
        assert all(np.array_equal(rsd[i], opt.front(i)[1]) for i in range(len(infos)))
        seen = dict(panel=kt["panel"]["launches"], syrk=kt["syrk"]["launches"], chain=kt["chain"]["launches"], panel_work=kt["panel"]["work"] > 0)
        print(f"{name} pass {p}: launches {seen}, backsub_hbm {kt['backsub_hbm']['launches']}")
        assert kt["backsub_hbm"]["launches"] >= 1
        expect = c["launches"] if default_form else dc.per_front_launches(c["fronts"], switch)
        assert seen == expect, (name, switch, seen, expect)
        if p == 0:
            opt.retract()
            orc.retract({k: dk[k] for k in dk})
    opt.close()
    print(f"ROW {name:20s} {fl['rsd']:.1e}  {fl['delta']:.1e}   {worst[0]:.1e}  {worst[1]:.1e}   {tol_rsd[0]:.1e} / {tol_d:.1e}")
    return worst


@pytest.mark.parametrize("name", list(dc.CASES))
def test_dense_front_against_reference(request, monkeypatch, name):
    switches = dc.case(name)["switches"]
    if switches:  # one_panel: the per-front path for a front the medium path would take
        request.getfixturevalue("dev_switches")
        for s in switches:
            monkeypatch.setenv(s, "1")
    _run(name, default_form=True)


@pytest.mark.parametrize("switch,name", [(sw, nm) for sw, names in dc.SWITCH_RUNS for nm in names],
                         ids=[f"{sw[0]}={sw[1]}-{nm}" for sw, names in dc.SWITCH_RUNS for nm in names])
def test_dense_front_launch_forms(monkeypatch, dev_switches, switch, name):
    monkeypatch.setenv(*switch)
    _run(name, default_form=False, switch=switch[0])
