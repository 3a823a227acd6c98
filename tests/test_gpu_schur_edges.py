"""The Schur-form front assembly (schur_pairs_kernel<1> / <4>, schur_factor_kernel, zero_blocks_kernel, the lds_front_kernel<GATHER>
leaves and the host tables around gp_tmp / gv_tmp) at its list and shape boundaries: the cases of tests/schur_cases.py, every front's
[R S d] and delta against the dense extended-precision reference (tests/dense_reference.py) built from the DEVICE's own Jacobians.

Per case: linearize (against the oracle), solve with identity damping, compare; retract, linearize, solve with diagonal damping,
compare again -- the second factorisation runs over the previous R, which is what shows a block zero_blocks_kernel should have
cleared; two identical solves are bitwise equal (fixed-order sums).  lists, wide_leaves and dims_2_3 also run under
LMGPU_SCHUR_UNMASKED, LMGPU_NO_GATHER_WRITE and both.  The 1e-6 comparison with the oracle (_check_solve) runs alongside.

Tolerance, per front: max(16 x the oracle-vs-reference floor of the case, 64 n 2.2e-16), n = front width; for delta n = the widest
front.  The floor (float64, another summation order) is measured when the test runs; 16 x floor above 1e-9 fails the case.

Measured (deviation = max|X - X_ref| / max|X_ref| over the fronts, relative 2-norm for delta; device = worst over both solves and
all four switch settings):
                      oracle floor          device                tolerance (root / delta)
    case              [R S d]   delta       [R S d]   delta
    lists             1.8e-14   1.4e-12     4.3e-14   1.6e-12     2.2e-12 / 2.3e-11
    leaf_degrees      2.3e-15   3.7e-14     1.9e-15   2.8e-14     2.2e-12 / 2.2e-12
    wide_leaves       2.6e-14   1.9e-12     4.4e-14   6.5e-13     2.0e-12 / 3.1e-11
    vec9              5.6e-16   5.0e-16     4.2e-16   2.8e-15     2.0e-12 / 2.0e-12
    dims_2_3          2.3e-13   9.9e-13     2.1e-13   9.1e-13     3.6e-12 / 1.6e-11
    factor_counts     3.1e-14   2.1e-12     3.9e-14   2.2e-12     2.2e-12 / 3.3e-11
    many_hbm_fronts   2.4e-13   9.7e-13     2.4e-13   6.7e-13     3.9e-12 / 1.6e-11
"""
import hashlib

import numpy as np
import pytest

import schur_cases as sc
from test_gpu_parity import _check_linearize, _check_solve, _pair

pytestmark = pytest.mark.gpu

FACTOR, EPS, CAP = 16, 2.2e-16, 1e-9
PASSES = ((1e-3, False), (1e-2, True))
_refs = {}


def _reference(name, c, opt, fronts, lam, diagonal):
    """the reference from the device's tapped Jacobians, once per distinct linearization (the switches do not change it)"""
    lin = opt.linear_graph()
    jac = [lin.at(g).augmentedJacobian() for g in range(c["graph"].size())]
    digest = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in jac)).hexdigest()
    key = (name, lam, diagonal, digest, tuple((tuple(k), n) for k, n in fronts))
    if key not in _refs:
        _refs[key] = sc.reference(c, jac, fronts, lam, diagonal)
    return _refs[key]


def _run(name):
    c, fl = sc.case(name), sc.oracle_floor(name)
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
              f"tolerance {max(FACTOR * fl['rsd'], 64 * infos[-1]['n'] * EPS):.2e}), delta {dd:.2e} (tolerance {tol_d:.2e})")
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


@pytest.mark.parametrize("name", list(sc.CASES))
def test_schur_assembly_against_dense_reference(name):
    _run(name)


@pytest.mark.parametrize("switches", [("LMGPU_SCHUR_UNMASKED",), ("LMGPU_NO_GATHER_WRITE",), ("LMGPU_SCHUR_UNMASKED", "LMGPU_NO_GATHER_WRITE")],
                         ids=["unmasked", "no_gather_write", "both"])
@pytest.mark.parametrize("name", sc.SWITCH_CASES)
def test_schur_assembly_launch_forms(monkeypatch, dev_switches, name, switches):
    for s in switches:
        monkeypatch.setenv(s, "1")
    _run(name)


def test_vec9_zero_precision_factor_is_accepted():
    """a leaf factor of precision 0 (nine rows of zeros: the ABI allows it) goes through the gather like any other: the library
    accepts the graph (the vec9 case above compares its numbers); here only that its Jacobian really is zero on the device"""
    c = sc.case("vec9")
    (j, pos), = sc.VEC9_ZERO_PRECISION
    pair = {c["leaves"][j][0], c["leaves"][j][2][pos][0]}
    g = next(i for i, keys in enumerate(c["graph"].factor_keys_in_graph_order()) if set(keys) == pair)
    opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    opt.linearize()
    J = opt.jacobian(g)
    assert J.shape == (9, 19) and not J.any()
    opt.close()
