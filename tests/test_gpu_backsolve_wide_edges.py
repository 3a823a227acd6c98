"""The root back-substitution's 128-row hops (hbm_backsolve_wide_kernel) at their block edges, on the cases of
tests/backsolve_wide_cases.py: roots of 1025, 1151, 1152, 1153 and 1280 frontal scalars and a non-root front (1153, 66), each through
the two passes of dense_front_cases.PASSES (lambda = 1e-6 with identity damping, then lambda = 1e-2 with diagonal damping over the
previous R, which is what shows an inverse block left from the previous factorisation).

As test_gpu_dense_front_edges.py: the fronts are asserted from front_info; every front's [R S d] and delta are held against the blocked
extended-precision reference (tests/dense_reference.py) built from the DEVICE's own Jacobians, at max(16 x the oracle's floor,
64 n 2.2e-16); every solve is repeated with the launch counters on and is bitwise equal, with the launch counts of the planner and at
least one `backsub_hbm` launch.  test_backsolve_wide_reference.py shows on the CPU that this comparison sees a dropped hop term, a
stale 16 x 16 inverse and a skipped fold at more than 100 x the tolerance.

The same cases run on the test library under LMGPU_BACKSOLVE_HOP64 (the 64-row form, hbm_backsolve_dataflow2_kernel) against the SAME
reference -- a second opinion on the cases, not a comparison of one form with the other.  The reference of a linearization is computed
once and shared by the two forms.

Measured on an MI355X (relative 2-norm of delta - delta_ref, worst of the two passes; every repeated solve bitwise equal, every launch
count the planner's; the [R S d] of the fronts is the factorisation's and the same in both forms, 1.6e-15 .. 7.0e-15):
    case                  oracle floor   128-row form   64-row form   tolerance
    root[1025]            1.3e-14        1.7e-14        1.7e-14       1.4e-11
    root[1151]            5.3e-14        2.4e-14        2.4e-14       1.6e-11
    root[1152]            2.6e-14        1.8e-14        1.9e-14       1.6e-11
    root[1153]            1.1e-14        4.3e-15        4.4e-15       1.6e-11
    root[1280]            4.1e-14        4.2e-14        4.2e-14       1.8e-11
    separator[1153,66]    1.6e-14        1.6e-14        1.6e-14       1.7e-11
A case takes 7 .. 14 s the first time (the two extended-precision references) and 2 .. 4 s under the second form.
"""
import numpy as np
import pytest

import backsolve_wide_cases as wc
import dense_front_cases as dc
import schur_cases as sc
from test_gpu_dense_front_edges import _reference
from test_gpu_parity import _check_linearize, _check_solve, _pair

pytestmark = pytest.mark.gpu


def _run(name):
    c, fl = wc.case(name), wc.oracle_floor(name)
    assert dc.FACTOR * fl["rsd"] <= dc.CAP and dc.FACTOR * fl["delta"] <= dc.CAP, fl
    opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"]) for f in infos] == c["fronts"], infos
    assert infos[0]["nf"] > 1024 and infos[0]["cls"] == 1  # the front under test takes the dataflow path of do_backsub
    fronts = [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))]
    tol_rsd, tol_d = dc.tolerances(fl, [f["n"] for f in infos])
    for p, (lam, diagonal) in enumerate(wc.PASSES):
        _check_linearize(opt, orc, c["graph"])
        ref = _reference("wide:" + name, c, opt, fronts, lam, diagonal)
        assert ref.residual < 1e-17
        dk = _check_solve(opt, orc, lam, diagonal)
        rsd = [opt.front(i)[1] for i in range(len(infos))]
        per_front, dd = sc.deviations(ref, lambda i: rsd[i], dk)
        print(f"{name} pass {p} (lambda {lam:g}, {'diagonal' if diagonal else 'identity'}): [R S d] " + ", ".join(f"{d:.2e}" for d in per_front)
              + " (tolerance " + ", ".join(f"{t:.2e}" for t in tol_rsd) + f"), delta {dd:.2e} (tolerance {tol_d:.2e})")
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
        assert seen == c["launches"], (name, seen, c["launches"])
        if p == 0:
            opt.retract()
            orc.retract({k: dk[k] for k in dk})
    opt.close()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_wide_hops_against_reference(name):
    _run(name)


@pytest.mark.parametrize("name", list(wc.CASES))
def test_hop64_against_reference(monkeypatch, dev_switches, name):
    monkeypatch.setenv(wc.SWITCH_HOP64, "1")
    _run(name)
