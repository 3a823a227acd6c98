"""The LDS-class fronts of csrc/kernels_front.hpp at their size edges: the factorisation (lds_front_tiny, lds_front_body inside
lds_front_kernel<false, 256>, lds_front_kernel<false, 1024>, lds_front_merged_kernel<256>, lds_front_merged_kernel<1024> and
level_fused_kernel<256>, with fill_upper_kernel in front of the merged launches) and the back-substitution (lds_backsub_kernel,
lds_backsub_wide_kernel, lds_backsub_merged_kernel) on the cases of tests/lds_front_cases.py: every front's [R S d] and delta against the
blocked extended-precision reference (tests/dense_reference.py) built from the DEVICE's own Jacobians.

Per case: the fronts are the ones the case was built for (front_info, level included); linearize (against the oracle); pass 0 = solve
with lambda = 1e-6, identity damping, compare; retract; pass 1 = solve with lambda = 1e-2, diagonal damping, over the previous state (which
is what shows an update matrix, an all-ones "not published" pattern or a ticket left from solve 1), compare again.  A solve that ends
with the indeterminate exception or with the dataflow-timeout status raises, and fails the case.  Each solve is repeated once with the
launch counters on (set_kernel_timing(1)): the repeat is bitwise equal in delta and in every front, and its `lds_front` / `backsub_lds` /
`panel` / `syrk` launch counts are those of lds_front_cases.launches, the restated dispatch -- the evidence that the intended form ran.
The 1e-6 comparison with the oracle (_check_solve) runs alongside.

Tolerance, per front: max(16 x the oracle-vs-reference floor of the case, 64 n 2.2e-16), n = front width; for delta n = the widest
front.  The floor is measured when the test runs; 16 x floor above 1e-9 fails the case.  test_lds_front_reference.py shows on the CPU
that each of six planted defects misses this tolerance by more than 100 x.

The launch forms (lds_front_cases.FORM_RUNS; dev_switches: the test library) are each compared with the REFERENCE at the same tolerance,
not with the default run.  Graph replay (LMGPU_GRAPH, read by both libraries; deep_chain replays by its depth) makes three solves: the
second is captured and replayed, the third replayed at the same state with another lambda; every counted repeat is an eager solve, so
each replay is also held bitwise against the eager launch sequence.  deep_chain runs once more with LMGPU_GRAPH=0.

The unit right-hand side (Marginals: the same kernels with the extra gradient term): marginalCovariance of one variable of a leaf front
and one of the root on lds_front_cases.MARGINAL_RUNS against the block of (R^T R)^-1 of the reference at lambda = 0, within
max(16 x the oracle's own marginal_covariance deviation from that block, 64 n 2.2e-16) relative to the block's largest entry.

Measured on an MI355X (deviation = max|X - X_ref| / max|X_ref| over the fronts, relative 2-norm for delta; device = worst over the passes;
"worst form" = over the default form and every switch the case runs under, their number in the last column).  Every repeated solve was
bitwise equal, in every form; every launch count was the restated one; no solve ended with the timeout status.  The device deviates by at
most 3.4e-14 ([R S d]) / 2.1e-12 (delta), the float64 oracle by 3.2e-14 / 2.0e-12:
                        oracle floor          device, default form  device, worst form    tolerance (front 0 / delta)   forms
    case                [R S d]   delta       [R S d]   delta       [R S d]   delta
    bin[24]             1.1e-15   9.9e-15     2.8e-15   9.5e-15     2.8e-15   9.5e-15     3.4e-13 / 3.4e-13             0
    bin[25]             2.2e-15   9.0e-15     8.4e-16   1.8e-14     2.4e-15   4.3e-14     3.5e-13 / 3.5e-13             3
    bin[48]             1.1e-15   7.3e-15     6.9e-16   6.2e-15     6.9e-16   6.2e-15     6.8e-13 / 6.8e-13             1
    bin[49]             1.4e-15   8.4e-15     1.4e-15   8.4e-15     1.4e-15   8.4e-15     6.9e-13 / 6.9e-13             1
    bin[72]             9.7e-16   1.4e-14     1.7e-15   8.9e-15     1.7e-15   8.9e-15     1.0e-12 / 1.0e-12             1
    bin[73]             7.2e-16   1.9e-14     5.5e-16   9.2e-15     5.5e-16   9.2e-15     1.0e-12 / 1.0e-12             1
    bin[96]             1.3e-15   6.8e-15     8.1e-16   8.1e-15     8.1e-16   8.1e-15     1.4e-12 / 1.4e-12             1
    bin[97]             1.2e-15   1.0e-14     7.6e-16   1.3e-14     7.6e-16   1.3e-14     1.4e-12 / 1.4e-12             1
    bin[120]            1.0e-15   3.7e-15     1.1e-15   4.6e-15     1.1e-15   4.6e-15     1.7e-12 / 1.7e-12             1
    bin[121]            8.8e-16   1.9e-14     1.5e-15   1.2e-14     1.5e-15   1.2e-14     1.7e-12 / 1.7e-12             1
    bin[64,74]          6.0e-16   8.3e-15     7.4e-16   7.6e-15     7.4e-16   7.6e-15     2.0e-12 / 2.0e-12             2
    bin[65,73]          8.4e-16   1.5e-14     8.4e-16   4.0e-15     8.4e-16   4.0e-15     2.0e-12 / 2.0e-12             3
    bin[3,135]          8.5e-16   1.6e-14     7.3e-16   1.7e-14     7.3e-16   1.7e-14     2.0e-12 / 2.0e-12             1
    bin[135,3]          1.2e-15   9.7e-15     9.8e-16   1.6e-14     9.8e-16   1.6e-14     2.0e-12 / 2.0e-12             1
    bin[16,122]         6.1e-16   9.3e-15     5.9e-16   4.2e-15     5.9e-16   4.2e-15     2.0e-12 / 2.0e-12             2
    bin_pooled          1.0e-15   1.6e-14     1.0e-15   1.2e-14     1.0e-15   1.2e-14     3.4e-13 / 1.4e-12             0
    pivots[2]           7.7e-16   1.7e-14     2.6e-15   2.5e-14     2.6e-15   2.5e-14     2.5e-13 / 2.7e-13             1
    pivots[3]           8.0e-16   6.6e-15     1.6e-15   1.9e-14     1.6e-15   1.9e-14     2.8e-13 / 2.8e-13             0
    pivots[5]           2.2e-15   1.8e-14     1.4e-15   1.6e-14     1.4e-15   1.6e-14     3.0e-13 / 3.0e-13             0
    pivots[7]           1.7e-15   1.4e-14     1.6e-15   2.0e-14     1.6e-15   2.0e-14     3.4e-13 / 3.4e-13             1
    pivots[8]           1.3e-15   5.9e-15     1.1e-15   1.2e-14     1.1e-15   1.2e-14     3.4e-13 / 3.4e-13             1
    pivots[9]           9.1e-16   5.3e-15     6.5e-16   2.9e-14     6.5e-16   2.9e-14     3.7e-13 / 3.7e-13             1
    pivots[11]          1.1e-15   9.2e-15     1.1e-15   2.5e-14     1.1e-15   2.5e-14     3.8e-13 / 3.8e-13             1
    pivots[12]          8.0e-16   1.6e-14     7.9e-16   8.7e-15     7.9e-16   8.7e-15     4.1e-13 / 4.1e-13             1
    pivots[13]          5.1e-16   3.1e-14     1.4e-15   3.6e-14     1.4e-15   3.6e-14     4.1e-13 / 4.9e-13             1
    pivots[15]          8.7e-16   7.8e-15     1.6e-15   5.4e-15     1.6e-15   5.4e-15     4.5e-13 / 4.5e-13             1
    pivots[16]          1.8e-15   1.2e-14     1.7e-15   8.1e-15     1.7e-15   8.1e-15     4.5e-13 / 4.5e-13             1
    pivots[17]          1.4e-15   1.1e-14     2.2e-15   6.4e-15     2.2e-15   6.4e-15     4.8e-13 / 4.8e-13             1
    pivots[31]          1.3e-15   1.1e-14     1.0e-15   9.0e-15     1.0e-15   9.0e-15     6.6e-13 / 6.6e-13             1
    pivots[32]          7.6e-16   6.8e-15     8.4e-16   4.2e-15     8.4e-16   4.2e-15     6.9e-13 / 6.9e-13             1
    pivots[33]          1.0e-15   8.0e-15     1.0e-15   1.5e-14     1.0e-15   1.5e-14     6.9e-13 / 6.9e-13             1
    pivots[47]          5.7e-16   5.9e-15     4.7e-16   4.9e-15     4.7e-16   4.9e-15     9.0e-13 / 9.0e-13             1
    pivots[48]          6.0e-16   1.7e-14     6.2e-16   1.1e-14     6.2e-16   1.1e-14     9.0e-13 / 9.0e-13             1
    pivots[49]          4.5e-16   7.0e-15     9.2e-16   8.6e-15     9.2e-16   8.6e-15     9.3e-13 / 9.3e-13             1
    pivots_wide[31]     1.2e-15   1.9e-14     1.2e-15   1.3e-14     1.2e-15   1.3e-14     1.3e-12 / 1.3e-12             1
    pivots_wide[32]     8.2e-16   9.8e-15     7.5e-16   6.0e-15     7.5e-16   6.0e-15     1.3e-12 / 1.3e-12             1
    pivots_wide[33]     6.4e-16   9.5e-15     1.1e-15   7.7e-15     1.1e-15   7.7e-15     1.3e-12 / 1.3e-12             1
    pivots_wide[47]     1.1e-15   8.9e-15     9.1e-16   7.8e-15     9.1e-16   7.8e-15     1.5e-12 / 1.5e-12             1
    pivots_wide[48]     1.5e-15   6.0e-15     1.9e-15   7.2e-15     1.9e-15   7.2e-15     1.5e-12 / 1.5e-12             1
    pivots_wide[49]     1.5e-15   1.1e-14     1.3e-15   8.0e-15     1.3e-15   8.0e-15     1.5e-12 / 1.5e-12             1
    tiny[15]            1.5e-15   2.8e-14     2.9e-15   6.8e-15     2.9e-15   1.4e-14     2.1e-13 / 4.5e-13             2
    tiny[16]            1.5e-15   1.8e-14     1.7e-15   7.0e-15     1.7e-15   9.0e-15     2.3e-13 / 2.9e-13             2
    tiny[17]            1.2e-15   4.6e-15     1.5e-15   1.5e-14     1.5e-15   3.3e-14     2.4e-13 / 2.4e-13             2
    tiny_tree           1.2e-15   8.9e-15     7.6e-16   1.2e-14     7.6e-16   1.2e-14     2.1e-13 / 2.3e-13             3
    tiny_sfm            9.5e-16   2.2e-14     1.5e-15   1.3e-14     1.5e-15   1.7e-14     2.1e-13 / 3.6e-13             2
    staging[31]         5.0e-15   3.2e-13     3.2e-15   1.8e-13     3.2e-15   1.8e-13     9.9e-14 / 5.0e-12             1
    staging[32]         3.0e-15   1.2e-13     3.6e-15   1.2e-13     3.6e-15   1.2e-13     9.9e-14 / 1.9e-12             1
    staging[33]         1.1e-15   8.2e-14     2.1e-15   3.7e-14     2.1e-15   3.7e-14     9.9e-14 / 1.3e-12             1
    staging[64]         3.2e-14   5.9e-13     3.4e-14   1.2e-12     3.4e-14   1.2e-12     5.1e-13 / 9.4e-12             1
    staging[65]         1.6e-14   2.0e-12     1.8e-14   2.1e-12     1.8e-14   2.1e-12     2.6e-13 / 3.2e-11             1
    staging_pose3[7]    6.9e-16   5.0e-15     9.4e-16   8.3e-14     9.4e-16   8.3e-14     1.8e-13 / 1.8e-13             1
    staging_pose3[8]    5.5e-16   5.4e-15     5.6e-16   3.9e-14     5.6e-16   3.9e-14     1.8e-13 / 1.8e-13             1
    staging_mixed       2.7e-15   2.3e-14     3.3e-15   3.3e-14     3.3e-15   3.3e-14     9.9e-14 / 3.7e-13             1
    staging[8,8]        2.9e-15   5.0e-15     2.6e-15   2.6e-14     2.6e-15   5.8e-14     2.4e-13 / 2.4e-13             2
    staging[9,8]        1.1e-15   1.2e-14     3.0e-15   2.3e-14     3.0e-15   2.3e-14     2.5e-13 / 2.5e-13             1
    children[1]         1.6e-15   7.8e-15     1.8e-15   1.4e-14     1.8e-15   1.4e-14     9.9e-14 / 3.1e-13             0
    children[2]         1.6e-15   3.4e-15     1.8e-15   6.7e-15     1.8e-15   6.7e-15     9.9e-14 / 3.1e-13             0
    children[3]         7.6e-16   1.1e-14     1.1e-15   1.0e-14     1.1e-15   1.0e-14     9.9e-14 / 3.1e-13             1
    children[4]         3.7e-15   4.7e-15     3.0e-15   5.4e-15     3.0e-15   5.4e-15     9.9e-14 / 3.1e-13             0
    children[5]         7.8e-16   5.7e-15     7.5e-16   5.5e-15     7.5e-16   5.5e-15     9.9e-14 / 3.1e-13             2
    children_wide       8.1e-16   1.5e-14     8.1e-16   2.0e-14     8.1e-16   2.0e-14     9.4e-13 / 2.0e-12             3
    backsub[63,15]      4.5e-16   8.1e-15     9.7e-16   1.2e-14     9.7e-16   1.2e-14     1.1e-12 / 1.1e-12             0
    backsub[128,8]      5.8e-16   4.7e-15     6.2e-16   8.3e-15     6.2e-16   8.3e-15     1.9e-12 / 1.9e-12             0
    backsub[129,6]      1.1e-15   1.5e-14     8.9e-16   1.1e-14     8.9e-16   1.1e-14     1.9e-12 / 1.9e-12             1
    backsub[14,124]     5.1e-16   6.4e-15     6.2e-16   1.5e-14     6.2e-16   1.5e-14     2.0e-12 / 2.0e-12             1
    backsub[15,123]     5.9e-16   8.0e-15     5.6e-16   4.8e-15     5.6e-16   4.8e-15     2.0e-12 / 2.0e-12             1
    backsub_mixed       2.1e-15   4.2e-15     2.0e-15   1.1e-14     2.4e-15   1.1e-14     3.5e-13 / 3.5e-13             2
    deep_chain          5.0e-16   4.2e-15     4.2e-16   1.9e-15     6.3e-16   2.7e-15     1.8e-13 / 1.8e-13             3
    fused_level         1.8e-15   1.4e-14     2.4e-15   1.2e-14     2.4e-15   1.2e-14     3.7e-12 / 3.7e-12             1
Marginal covariances (relative to the block's largest entry):
    tiny[16]     leaf: oracle floor 2.7e-15  device 1.8e-15  tolerance 2.3e-13
    tiny[16]     root: oracle floor 4.3e-15  device 8.1e-15  tolerance 2.3e-13
    bin[25]      leaf: oracle floor 1.2e-15  device 4.0e-15  tolerance 3.5e-13
    bin[25]      root: oracle floor 9.2e-16  device 5.1e-15  tolerance 3.5e-13
    children[3]  leaf: oracle floor 5.1e-16  device 2.8e-16  tolerance 3.1e-13
    children[3]  root: oracle floor 4.2e-15  device 5.5e-15  tolerance 3.1e-13
The whole module (151 tests) takes 7 s; no case takes more than 0.3 s (each reference 0.01 .. 0.1 s).
"""
import hashlib

import numpy as np
import pytest

import lds_front_cases as lc
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
        _refs[key] = sc.reference(c, jac, fronts, lam, diagonal, block=lc.BLOCK)
    return _refs[key]


def _run(name, form=None, passes=lc.PASSES):
    c, fl = lc.case(name), lc.oracle_floor(name, passes)
    assert lc.FACTOR * fl["rsd"] <= lc.CAP and lc.FACTOR * fl["delta"] <= lc.CAP, fl
    opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"], level=f["level"]) for f in infos] == c["fronts"], infos
    fronts = [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))]
    tol_rsd, tol_d = lc.tolerances(fl, [f["n"] for f in infos])
    expect = lc.launches(c["fronts"], **lc.FORM_ARGUMENT[form] if form else {})
    worst = [0.0, 0.0]
    for p, (lam, diagonal) in enumerate(passes):
        _check_linearize(opt, orc, c["graph"])
        ref = _reference(name, c, opt, fronts, lam, diagonal)
        assert ref.residual < 1e-17
        dk = _check_solve(opt, orc, lam, diagonal)  # (raises on the indeterminate exception and on the dataflow-timeout status)
        rsd = [opt.front(i)[1] for i in range(len(infos))]
        per_front, dd = sc.deviations(ref, lambda i: rsd[i], dk)
        print(f"{name} pass {p} (lambda {lam:g}, {'diagonal' if diagonal else 'identity'}): [R S d] " + ", ".join(f"{d:.2e}" for d in per_front)
              + " (tolerance " + ", ".join(f"{t:.2e}" for t in tol_rsd) + f"), delta {dd:.2e} (tolerance {tol_d:.2e})")
        worst = [max(worst[0], max(per_front)), max(worst[1], dd)]
        for i, dev in enumerate(per_front):
            assert dev <= tol_rsd[i], (name, p, i, infos[i], dev)
        assert dd <= tol_d, (name, p, dd)
        opt.set_kernel_timing(1)  # the same solve again, counted (and eager): bitwise
        dk2, _, _, _ = opt.solve(lam, diagonal)
        kt = opt.kernel_times()
        opt.set_kernel_timing(False)
        assert all(np.array_equal(dk[k], dk2[k]) for k in dk)
        assert all(np.array_equal(rsd[i], opt.front(i)[1]) for i in range(len(infos)))
        seen = {k: kt[k]["launches"] for k in ("lds_front", "panel", "syrk")}
        seen["backsub_lds"] = kt["backsub_lds"]["launches"]
        print(f"{name} pass {p}: launches {seen}")
        assert seen == expect, (name, form, seen, expect)
        if p == 0:  # (a third solve stays at the second's state: nearer the optimum delta shrinks towards d's rounding error)
            opt.retract()
            orc.retract({k: dk[k] for k in dk})
    opt.close()
    print(f"ROW {name:18s} {'default' if form is None else '='.join(form):22s} {fl['rsd']:.1e}  {fl['delta']:.1e}   {worst[0]:.1e}  {worst[1]:.1e}   {tol_rsd[0]:.1e} / {tol_d:.1e}")
    return worst


@pytest.mark.parametrize("name", list(lc.CASES))
def test_lds_front_against_reference(name):
    """the product library, no switch (deep_chain: merged both ways and replayed, so three solves)"""
    _run(name, passes=lc.GRAPH_PASSES if name == "deep_chain" else lc.PASSES)


@pytest.mark.parametrize("switch,name", [(sw, nm) for sw, names in lc.FORM_RUNS for nm in names],
                         ids=[f"{sw[0]}={sw[1]}-{nm}" for sw, names in lc.FORM_RUNS for nm in names])
def test_lds_front_launch_forms(monkeypatch, dev_switches, switch, name):
    monkeypatch.setenv(*switch)
    _run(name, form=switch)


@pytest.mark.parametrize("name", lc.GRAPH_RUNS)
def test_lds_front_graph_replay(monkeypatch, name):
    monkeypatch.setenv("LMGPU_GRAPH", "1")
    _run(name, form=("LMGPU_GRAPH", "1"), passes=lc.GRAPH_PASSES)


def test_deep_chain_without_graph(monkeypatch):
    monkeypatch.setenv("LMGPU_GRAPH", "0")
    _run("deep_chain", form=("LMGPU_GRAPH", "0"), passes=lc.GRAPH_PASSES)


@pytest.mark.parametrize("name,switch", lc.MARGINAL_RUNS, ids=[nm + ("" if sw is None else "-" + "=".join(sw)) for nm, sw in lc.MARGINAL_RUNS])
def test_lds_front_marginals(request, monkeypatch, name, switch):
    import oracle_harness as oh
    from gtsam_personal_amd import Marginals
    if switch:
        request.getfixturevalue("dev_switches")
        monkeypatch.setenv(*switch)
    c = lc.case(name)
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    assert orc.solve(0.0, False)[0] == 0
    oref = sc.reference(c, [orc.jacobian(g) for g in range(c["graph"].size())], [(k, nfk) for k, nfk, _, _ in orc.cliques()], 0.0, False, lc.BLOCK)
    m = Marginals(c["graph"], c["initial"], c["ordering"])
    opt = m._opt
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"], level=f["level"]) for f in infos] == c["fronts"], infos
    opt.linearize()
    jac = [opt.jacobian(g) for g in range(c["graph"].size())]
    ref = sc.reference(c, jac, [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))], 0.0, False, lc.BLOCK)
    assert ref.residual < 1e-17 and oref.residual < 1e-17
    widest = max(f["n"] for f in infos)
    expect = lc.launches(c["fronts"], **lc.FORM_ARGUMENT[switch] if switch else {})
    for key in lc.marginal_keys(c):
        want = lc.covariance_block(ref, key)
        floor = lc.block_deviation(orc.marginal_covariance(key, want.shape[0]), lc.covariance_block(oref, key))
        assert lc.FACTOR * floor <= lc.CAP
        tol = lc.marginal_tolerance(floor, widest)
        cov = m.marginalCovariance(key)
        dev = lc.block_deviation(cov, want)
        print(f"MROW {name:12s} {'root' if key == lc.marginal_keys(c)[1] else 'leaf'}: oracle floor {floor:.1e}  device {dev:.1e}  tolerance {tol:.1e}")
        assert dev <= tol, (name, key, dev, tol)
        opt.set_kernel_timing(1)  # once more, counted: one solve per column of the block, each in the form the case is listed for
        again = m.marginalCovariance(key)
        kt = opt.kernel_times()
        opt.set_kernel_timing(False)
        assert np.array_equal(again, cov)
        d = want.shape[0]
        assert (kt["lds_front"]["launches"], kt["backsub_lds"]["launches"]) == (d * expect["lds_front"], d * expect["backsub_lds"]), (kt, expect)
    m.close()
