"""schur_var_kernel<1> / <8> (one walk per separator variable for its (v, v) and (v, rhs) blocks, the corner workgroup) and the form it
replaced (LMGPU_SCHUR_SPLIT_DIAG, test library: (v, v) and (v, rhs) as pair blocks + schur_factor_kernel + the scalar reduction), at the
walk's list boundaries: every front's [R S d] and delta against the dense extended-precision reference, with the harness and the
tolerance rule of tests/test_gpu_schur_edges.py -- per front max(16 x the oracle-vs-reference floor of the case, 64 n 2.2e-16), 16 x floor
above 1e-9 fails the case; two solves per damping, the repeat bitwise equal.

  var_lists (tests/schur_var_cases.py) and schur_cases.SWITCH_CASES   both forms, each also with LMGPU_NO_GATHER_WRITE (add mode)
  the other cases of schur_cases.CASES                                the split-diagonal form (test_gpu_schur_edges.py runs the default)

Measured (deviation as in test_gpu_schur_edges.py; device = worst over both solves and the four settings):
                      oracle floor          device                tolerance (root / delta)
    case              [R S d]   delta       [R S d]   delta
    var_lists         3.7e-14   1.1e-11     1.9e-14   4.1e-12     2.4e-12 / 1.7e-10
"""
import numpy as np
import pytest

import schur_cases as sc
import schur_var_cases as svc
from test_gpu_parity import _check_linearize, _check_solve, _pair
from test_gpu_schur_edges import CAP, EPS, FACTOR, PASSES, _reference

pytestmark = pytest.mark.gpu

SPLIT = "LMGPU_SCHUR_SPLIT_DIAG"
ADD = "LMGPU_NO_GATHER_WRITE"


def _case_and_floor(name):
    return (svc.case(), svc.oracle_floor()) if name == svc.NAME else (sc.case(name), sc.oracle_floor(name))


def _run(name):
    """test_gpu_schur_edges._run, for a case that need not be in schur_cases.CASES"""
    c, fl = _case_and_floor(name)
    assert FACTOR * fl["rsd"] <= CAP and FACTOR * fl["delta"] <= CAP, fl
    opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    fronts = [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))]
    widest = max(f["n"] for f in infos)
    worst = [0.0, 0.0]
    for p, (lam, diagonal) in enumerate(PASSES):
        _check_linearize(opt, orc, c["graph"])
        ref = _reference(name, c, opt, fronts, lam, diagonal)
        assert ref.residual < 1e-17
        dk = _check_solve(opt, orc, lam, diagonal)
        rsd = [opt.front(i)[1] for i in range(len(infos))]
        per_front, dd = sc.deviations(ref, lambda i: rsd[i], dk)
        tol_d = max(FACTOR * fl["delta"], 64 * widest * EPS)
        print(f"{name} pass {p} (lambda {lam:g}, {'diagonal' if diagonal else 'identity'}): [R S d] {max(per_front):.2e} (root {per_front[-1]:.2e}, "
              f"tolerance {max(FACTOR * fl['rsd'], 64 * infos[-1]['n'] * EPS):.2e}), delta {dd:.2e} (tolerance {tol_d:.2e}); "
              f"floor [R S d] {fl['rsd']:.2e}, delta {fl['delta']:.2e}")
        worst = [max(worst[0], max(per_front)), max(worst[1], dd)]
        for i, dev in enumerate(per_front):
            assert dev <= max(FACTOR * fl["rsd"], 64 * infos[i]["n"] * EPS), (name, p, i, infos[i], dev)
        assert dd <= tol_d, (name, p, dd)
        dk2, _, _, _ = opt.solve(lam, diagonal)  # the same solve again: bitwise
        assert all(np.array_equal(dk[k], dk2[k]) for k in dk)
        assert all(np.array_equal(rsd[i], opt.front(i)[1]) for i in range(len(infos)))
        if p == 0:
            opt.retract()
            orc.retract({k: dk[k] for k in dk})
    opt.close()
    return worst


@pytest.mark.parametrize("switches", [(), (ADD,), (SPLIT,), (SPLIT, ADD)], ids=["var", "var_add", "split_diag", "split_diag_add"])
@pytest.mark.parametrize("name", (svc.NAME,) + tuple(sc.SWITCH_CASES))
def test_schur_var_forms(monkeypatch, dev_switches, name, switches):
    for s in switches:
        monkeypatch.setenv(s, "1")
    _run(name)


@pytest.mark.parametrize("name", [n for n in sc.CASES if n not in sc.SWITCH_CASES])
def test_split_diagonal_form_on_the_remaining_cases(monkeypatch, dev_switches, name):
    monkeypatch.setenv(SPLIT, "1")
    _run(name)
