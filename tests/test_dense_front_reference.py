"""CPU side of the dense-front panel-boundary cases (tests/dense_front_cases.py), without a GPU:

  * the blocked extended-precision reference against the row-at-a-time one on every schur_cases case;
  * per dense-front case: the reference's residual and the float64 oracle's distance from it (the floor the GPU test scales its
    tolerance from), 16 x floor under the 1e-9 cap, every front with the nf / n / parent / class it was built for (structure-only
    handle), and that the comparison SEES what it is for: a plain float64 blocked Cholesky of the same matrix with one planted defect
    misses the case's own tolerance by at least 100 x.

Blocked against row-at-a-time, max|R_b - R_u| / max|R_u| over [R d] -- measured, in units of eps n (eps = 1.08e-19, n = columns), at
lambda = 1e-3 identity / 1e-2 diagonal: lists (n = 4152) 0.064 / 0.005, leaf_degrees 0.056 / 0.036, wide_leaves 1.34 / 0.013, vec9 0.009 /
0.011, dims_2_3 0.26 / 0.018, factor_counts 0.65 / 0.033, many_hbm_fronts 0.36 / 0.004; asserted <= 4 eps n (the two sum the same
products in another order).  Residuals: blocked <= 1.0e-18, row-at-a-time <= 1.0e-19.

Per case -- measured.  time = BOTH references of the case (assembly, factorisation, whole-triangle residual, back-substitution) with
the oracle's two solves; beyond_1024 is the one case above 5 s per reference (5.9 s), and 1290 is ten rows above the smallest front
whose first update has more than 1024 columns.  The last column is the smallest of the six planted defects' deviations, in
tolerances (asserted >= 100).  Smallest over all cases, per defect: slice skipped in the first / middle / last block row 9.0e3 / 4.4e5 /
9.6e8, right-hand side 1.1e10, missing lambda 3.9e2, stale block 1.2e7:
    case                 time      floor [R S d], delta   tolerance (front 0 / delta)   smallest defect / tolerance
    medium_batch           1.5 s   1.7e-15  1.1e-14   2.0e-12 / 3.6e-12   2.5e+05
    one_panel[63]          0.1 s   3.9e-16  6.9e-15   2.0e-12 / 2.0e-12   1.3e+06
    one_panel[64]          0.1 s   5.9e-16  1.7e-14   2.0e-12 / 2.0e-12   1.4e+04
    one_panel[65]          0.1 s   7.0e-16  7.1e-15   2.0e-12 / 2.0e-12   9.2e+03
    one_panel[128]         0.1 s   4.1e-16  8.9e-15   2.9e-12 / 2.9e-12   2.2e+05
    one_panel[193]         0.1 s   1.4e-15  4.8e-14   2.7e-12 / 2.7e-12   3.5e+04
    one_panel[255]         0.2 s   1.4e-15  3.1e-14   3.6e-12 / 3.6e-12   1.8e+05
    one_panel[256]         0.2 s   1.4e-15  7.3e-15   3.6e-12 / 3.6e-12   5.2e+05
    tail[257]              0.2 s   3.7e-16  7.8e-15   3.6e-12 / 3.6e-12   6.2e+04
    tail[303]              0.3 s   9.5e-16  1.8e-14   4.3e-12 / 4.3e-12   2.1e+05
    tail[304]              0.3 s   1.2e-15  1.5e-14   4.3e-12 / 4.3e-12   4.0e+04
    tail[319]              0.3 s   1.1e-15  1.0e-14   4.5e-12 / 4.5e-12   3.8e+03
    tail[320]              0.3 s   6.3e-16  8.4e-15   4.5e-12 / 4.5e-12   1.3e+05
    tail[321]              0.4 s   1.2e-15  7.4e-15   4.5e-12 / 4.5e-12   1.2e+05
    chain[576]             1.5 s   1.3e-15  1.6e-14   8.1e-12 / 8.1e-12   9.6e+04
    chain[768]             3.3 s   2.1e-15  6.8e-15   1.1e-11 / 1.1e-11   5.1e+04
    chain[771]             3.5 s   1.9e-15  2.7e-14   1.1e-11 / 1.1e-11   3.9e+04
    chain[832]             4.0 s   3.3e-16  1.4e-14   1.2e-11 / 1.2e-11   2.1e+04
    chain[900]             4.4 s   1.0e-15  6.2e-15   1.3e-11 / 1.3e-11   5.3e+03
    chain[1088]            6.9 s   4.0e-15  1.8e-14   1.5e-11 / 1.5e-11   8.9e+03
    beyond_1024           11.8 s   3.9e-15  1.7e-14   1.8e-11 / 1.8e-11   5.9e+03
    separator[192,70]      0.1 s   1.7e-15  1.6e-14   3.7e-12 / 3.7e-12   4.5e+04
    separator[300,138]     0.7 s   1.3e-15  8.4e-15   6.2e-12 / 6.2e-12   5.0e+04
    separator[96,600]      2.1 s   1.6e-15  1.4e-14   9.8e-12 / 9.8e-12   3.7e+04
    separator[1030,66]     8.2 s   1.9e-15  1.6e-14   1.5e-11 / 1.5e-11   3.9e+02
"""
import time

import numpy as np
import pytest

import dense_front_cases as dc
import schur_cases as sc
from dense_reference import LD, FactorView, augmented_information
from gtsam_personal_amd import LevenbergMarquardtOptimizer

LD_EPS = float(np.finfo(LD).eps)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_blocked_reference_agrees_with_row_at_a_time(name):
    """on the Schur-assembly cases (sparse leaves in front of a dense root): same Jacobians, same fronts, both forms"""
    import oracle_harness as oh
    c = sc.case(name)
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    jac = [orc.jacobian(g) for g in range(c["graph"].size())]
    rc, _, _, _ = orc.solve(0.0, False)
    assert rc == 0
    fronts = [(keys, nfk) for keys, nfk, _, _ in orc.cliques()]
    for lam, diagonal in ((1e-3, False), (1e-2, True)):
        by_rows = sc.reference(c, jac, fronts, lam, diagonal)
        blocked = sc.reference(c, jac, fronts, lam, diagonal, block=dc.BLOCK)
        dev = float(np.abs(blocked.R - by_rows.R).max() / np.abs(by_rows.R).max())
        xb, xr = blocked._x, by_rows._x
        ddev = float(np.sqrt(((xb - xr) ** 2).sum() / (xr ** 2).sum()))
        print(f"{name} lambda {lam:g}: n {by_rows.n}, [R d] {dev:.2e} ({dev / (LD_EPS * by_rows.n):.2e} eps n), delta {ddev:.2e}, residual blocked {blocked.residual:.2e} "
              f"by rows {by_rows.residual:.2e}")
        assert blocked.residual < 1e-17 and by_rows.residual < 1e-17
        assert dev <= 4 * LD_EPS * by_rows.n, (name, lam, dev)


# ------------------------------------------------------------------------------------------------ a float64 factor with a defect
def _cholesky64(H, n, nb=16, skipped_slice=None, rhs_skips_panel=None, undamped=None):
    """[R d] (n, n + 1) of the float64 augmented matrix H: right-looking, panels of nb = 16 rows, trailing update in 16 x 16 tiles'
    arithmetic (one matrix product here).  One defect at a time:
      skipped_slice = (panel, tile row, tile column): rows 4..7 of that panel left out of the update of that 16 x 16 tile
      rhs_skips_panel = panel: the right-hand-side column not updated by that panel
      undamped = (j, lambda D_j): lambda D missing on diagonal entry j"""
    W = np.array(H, dtype=np.float64)
    if undamped is not None:
        W[undamped[0], undamped[0]] -= undamped[1]
    for p, j0 in enumerate(range(0, n, nb)):
        j1 = min(n, j0 + nb)
        for j in range(j0, j1):
            W[j, j:] /= np.sqrt(W[j, j])
            if j + 1 < j1:
                W[j + 1:j1, j + 1:] -= np.multiply.outer(W[j, j + 1:j1], W[j, j + 1:])
        P = W[j0:j1, j1:]
        U = P.T @ P
        if skipped_slice is not None and skipped_slice[0] == p:
            _, ti, tj = skipped_slice
            r = slice(max(16 * ti, j1) - j1, 16 * ti + 16 - j1)
            c = slice(max(16 * tj, j1) - j1, 16 * tj + 16 - j1)
            assert 16 * ti + 16 > j1 and ti <= tj and P.shape[0] >= 8
            U[r, c] -= P[4:8, r].T @ P[4:8, c]
        if rhs_skips_panel == p:
            U[:, -1] = 0
        W[j1:, j1:] -= U
    return np.triu(W)[:n]


def _defects(n, ranges):
    """the planted defects for a matrix of n columns + rhs: (label, keyword arguments of _cholesky64).  ranges: [lo, hi) of every
    front's frontal scalars: panel, tile row and tile column of a skipped slice lie within ONE front (blocks between two components are
    exact zeros, where no defect could show)"""
    last = (n - 1) // 16  # the tile row of the last frontal row; its panel is the one before it (16 rows: it has rows 4..7)
    lo, hi = next((lo, hi) for lo, hi in ranges if lo <= n // 2 < hi)
    mid = ((lo + hi) // 2) // 16  # the tile row in the middle of the front that holds the middle of the matrix
    first_in = (lo + 15) // 16  # the first panel that lies wholly inside the front of the middle tile
    picks = [("first", 0, 1, 2 if 16 * 2 + 8 < ranges[0][1] else 1),
             ("middle", (first_in + mid) // 2, mid, mid + 1 if 16 * (mid + 1) + 8 < hi else mid),
             ("last", last - 1, last, n // 16)]  # (column tile: the one that holds the right-hand side)
    out = []
    for label, p, ti, tj in picks:
        assert p < ti and 16 * p >= (0 if label == "first" else lo if label == "middle" else ranges[-1][0]), (label, p, ti, ranges)
        out.append((f"slice of 4 skipped, {label} block row (panel {p}, tile {ti},{tj})", dict(skipped_slice=(p, ti, tj))))
    out.append(("rhs column not updated by the middle panel", dict(rhs_skips_panel=(n // 2) // 16)))
    return out


def _margin(ref, view, fronts_rsd_tol, delta_tol):
    """the largest deviation / tolerance of a factor view against the reference, over the fronts and delta"""
    per_front, dd = sc.deviations(ref, view.front, view.delta())
    return max(max(d / t for d, t in zip(per_front, fronts_rsd_tol)), dd / delta_tol)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_dense_front_case(name):
    c = dc.case(name)
    # 2. boundaries: the fronts the case was built for, from a structure-only handle
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"]) for f in infos] == c["fronts"], infos
    if c["launches"]["panel_work"] and name not in ("separator[300,138]", "separator[96,600]"):  # (those two have a medium-path front beside a per-front one)
        assert dc.per_front_launches(c["fronts"]) == c["launches"], (dc.per_front_launches(c["fronts"]), c["launches"])
    # 1. floor: the oracle against the reference from its own Jacobians, both passes
    kept = []
    t0 = time.perf_counter()
    fl = sc.floor_of(c, dc.PASSES, dc.BLOCK, keep=kept)
    seconds = time.perf_counter() - t0
    tol_rsd, tol_delta = dc.tolerances(fl, [f["n"] for f in infos])
    print(f"{name}: reference {seconds:.1f} s for both passes (with the oracle's solves), residual {fl['residual']:.2e}; oracle vs reference [R S d] {fl['rsd']:.2e}, "
          f"delta {fl['delta']:.2e}; tolerance front 0 {tol_rsd[0]:.2e}, delta {tol_delta:.2e}")
    assert fl["residual"] < 1e-17
    # 3. cap: a condition on the inputs
    assert dc.FACTOR * fl["rsd"] <= dc.CAP and dc.FACTOR * fl["delta"] <= dc.CAP, fl
    # 4. the comparison sees what it is for
    import oracle_harness as oh
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    factors = list(zip(c["graph"].factor_keys_in_graph_order(), [orc.jacobian(g) for g in range(c["graph"].size())]))
    dims = sc.var_dims(c)
    (ref0, cl, _), (ref1, _, _) = kept
    fronts = ref0.fronts
    H = [augmented_information(factors, dims, lam, dg, fronts)[0].astype(np.float64) for lam, dg in dc.PASSES]
    n = ref0.n

    def view(R):
        return FactorView(R, ref0.off, dims, fronts)
    clean = [_margin(r, view(_cholesky64(h, n)), tol_rsd, tol_delta) for r, h in zip((ref0, ref1), H)]
    print(f"    the float64 factor without a defect: {clean[0]:.2e}, {clean[1]:.2e} of the tolerance")
    assert max(clean) <= 1.0, clean
    lam0 = dc.PASSES[0][0]
    margins = []
    ranges = [(ref0.off[keys[0]], ref0.off[keys[nfk - 1]] + dims[keys[nfk - 1]]) for keys, nfk in fronts]
    for label, kw in _defects(n, ranges) + [(f"lambda D missing on diagonal entry {n // 2}", dict(undamped=(n // 2, lam0)))]:
        margins.append((label, _margin(ref0, view(_cholesky64(H[0], n, **kw)), tol_rsd, tol_delta)))
    # one 16 x 16 block of the second factorisation left at its value from the first
    R0, R1 = _cholesky64(H[0], n), _cholesky64(H[1], n)
    b = 16 * ((n // 2) // 16)
    R1[b:b + 16, b + 16:b + 32] = R0[b:b + 16, b + 16:b + 32]
    margins.append((f"block ({b // 16},{b // 16 + 1}) left from the previous factorisation", _margin(ref1, view(R1), tol_rsd, tol_delta)))
    for label, m in margins:
        print(f"    {label}: {m:.2e} x the tolerance")
    print(f"ROW {name:20s} {seconds:5.1f} s   {fl['rsd']:.1e}  {fl['delta']:.1e}   {tol_rsd[0]:.1e} / {tol_delta:.1e}   {min(m for _, m in margins):.1e}")
    for label, m in margins:
        assert m >= 100, (name, label, m)
