"""CPU side of the wide-hop back-substitution cases (tests/backsolve_wide_cases.py), without a GPU, in the pattern of
test_dense_front_reference.py.

`wide_backsolve` restates in numpy / float64 what hbm_backsolve_wide_kernel (csrc/kernels_dense.hpp) computes for one dense front, block
by block of 128 rows, from the front's [R S d] and the 16 x 16 inverses of its diagonal tiles:
    X_B   = inv(R_BB), by the block back-substitution over 16-blocks:  X_hh = I_h;  X_gh = -I_g (sum_{k = g+1..h} R_gk X_kh)
            (the identity-padded partial last block: the padding inverts to itself and is left out here)
    M_B   = X_B R_{B,B+1}
    folds   acc = y_B - sum_{j = last .. B+2} R_Bj x_j, in that order
    u_B   = X_B acc
    x_B   = u_B - M_B x_{B+1}
Per case it shows
  (a) 16 x the oracle's floor stays under the 1e-9 cap of dense_front_cases (a condition on the seeds, checked before the GPU is),
  (b) the restatement, over a plain float64 Cholesky factor, meets the GPU test's tolerance on delta in both passes,
  (c) each of three planted defects misses that tolerance by more than 100 x: the M_B x_{B+1} term dropped for one block, one 16 x 16
      inverse left from the previous pass' factor, one 128-column fold skipped.
The fronts are asserted from a structure-only handle to be the ones the case was built for.

Measured (delta deviation in tolerances; the tolerance of delta is the 64 n 2.2e-16 term in every case):
    case                  floor [R S d], delta   tolerance   restatement (pass 0, 1)   dropped M x / stale inverse / skipped fold
    root[1025]            3.0e-15  1.3e-14   1.4e-11   3.1e-04  2.2e-04   8.8e+09 / 1.5e+08 / 9.1e+09
    root[1151]            5.2e-15  5.3e-14   1.6e-11   4.4e-04  1.9e-04   1.2e+10 / 1.2e+08 / 8.6e+09
    root[1152]            4.2e-15  2.6e-14   1.6e-11   2.5e-04  2.5e-04   9.1e+09 / 2.1e+08 / 1.2e+10
    root[1153]            1.6e-15  1.1e-14   1.6e-11   1.8e-04  2.7e-04   6.7e+09 / 2.7e+08 / 6.0e+09
    root[1280]            7.0e-15  4.1e-14   1.8e-11   3.4e-04  1.9e-04   5.4e+09 / 7.5e+07 / 5.1e+09
    separator[1153,66]    3.3e-15  1.6e-14   1.7e-11   5.2e-04  1.1e-04   3.9e+09 / 1.1e+08 / 9.1e+09
The six cases take 70 s, nearly all of it the extended-precision references.
"""
import numpy as np
import pytest

import backsolve_wide_cases as wc
import dense_front_cases as dc
import schur_cases as sc
from dense_reference import augmented_information
from gtsam_personal_amd import LevenbergMarquardtOptimizer
from test_dense_front_reference import _cholesky64


def inverses16(R, lo, nf):
    """the 16 x 16 inverses of the diagonal tiles of the front at rows lo .. lo + nf of R (tiles counted from the front's first row;
    the last one may be short)"""
    out = []
    for t in range(0, nf, 16):
        e = min(nf, t + 16)
        out.append(np.linalg.inv(np.triu(R[lo + t:lo + e, lo + t:lo + e])))
    return out


def explicit_inverse(Rbb, inv16):
    """X = inv(Rbb) of one block (at most 128 rows) from the inverses of its 16-blocks"""
    nb = Rbb.shape[0]
    cuts = list(range(0, nb, 16)) + [nb]
    X = np.zeros_like(Rbb)
    for h in range(len(cuts) - 1):
        hs = slice(cuts[h], cuts[h + 1])
        X[hs, hs] = inv16[h]
        for g in range(h - 1, -1, -1):
            gs = slice(cuts[g], cuts[g + 1])
            m = np.zeros((cuts[g + 1] - cuts[g], cuts[h + 1] - cuts[h]))
            for k in range(g + 1, h + 1):
                ks = slice(cuts[k], cuts[k + 1])
                m += Rbb[gs, ks] @ X[ks, hs]
            X[gs, hs] = -inv16[g] @ m
    return X


def wide_backsolve(R, lo, nf, y, inv16, drop_hop=None, skip_fold=None):
    """x of the front at rows / columns lo .. lo + nf of R with right-hand side y (d - S x_S), by 128-row hops.
    drop_hop = B: the M_B x_{B+1} term left out;  skip_fold = (B, j): block j not folded into block B"""
    blocks = wc.blocks(nf)
    x = [None] * len(blocks)
    for B in range(len(blocks) - 1, -1, -1):
        r0, nb = blocks[B]
        rows = slice(lo + r0, lo + r0 + nb)
        X = explicit_inverse(np.triu(R[rows, rows]), inv16[r0 // 16:(r0 + nb + 15) // 16])
        acc = y[r0:r0 + nb].copy()
        for j in range(len(blocks) - 1, B + 1, -1):  # the folds off the chain, from the last block down to B + 2
            if skip_fold == (B, j):
                continue
            c0, ncol = blocks[j]
            acc -= R[rows, lo + c0:lo + c0 + ncol] @ x[j]
        u = X @ acc
        if B + 1 < len(blocks):
            c0, ncol = blocks[B + 1]
            M = X @ R[rows, lo + c0:lo + c0 + ncol]
            x[B] = u if drop_hop == B else u - M @ x[B + 1]
        else:
            x[B] = u
    return np.concatenate(x)


def solve_with_wide_front(R, lo, nf, inv16=None, **defect):
    """x of the whole factor [R d] (n, n + 1): plain back-substitution of the rows behind the front, the wide hops for the front.
    (The front under test comes first in every case, so nothing lies in front of it.)"""
    n = R.shape[0]
    assert lo == 0
    x = np.zeros(n)
    for j in range(n - 1, nf - 1, -1):
        x[j] = (R[j, n] - R[j, j + 1:n] @ x[j + 1:]) / R[j, j]
    y = R[:nf, n] - R[:nf, nf:n] @ x[nf:]
    x[:nf] = wide_backsolve(R, lo, nf, y, inverses16(R, lo, nf) if inv16 is None else inv16, **defect)
    return x


@pytest.mark.parametrize("name", list(wc.CASES))
def test_wide_hop_case(name):
    c = wc.case(name)
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"]) for f in infos] == c["fronts"], infos
    nf = infos[0]["nf"]
    assert nf > 1024 and infos[0]["cls"] == 1  # the dataflow path of do_backsub
    # (a) floor and cap
    kept = []
    fl = sc.floor_of(c, wc.PASSES, dc.BLOCK, keep=kept)
    tol_rsd, tol_delta = dc.tolerances(fl, [f["n"] for f in infos])
    print(f"{name}: oracle vs reference [R S d] {fl['rsd']:.2e}, delta {fl['delta']:.2e}, residual {fl['residual']:.2e}; tolerance of delta {tol_delta:.2e}")
    assert fl["residual"] < 1e-17
    assert dc.FACTOR * fl["rsd"] <= dc.CAP and dc.FACTOR * fl["delta"] <= dc.CAP, fl
    # (b) the restatement over a float64 factor of the same matrices
    import oracle_harness as oh
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    factors = list(zip(c["graph"].factor_keys_in_graph_order(), [orc.jacobian(g) for g in range(c["graph"].size())]))
    dims = sc.var_dims(c)
    (ref0, _, _), (ref1, _, _) = kept
    fronts, n = ref0.fronts, ref0.n
    R = [_cholesky64(augmented_information(factors, dims, lam, dg, fronts)[0].astype(np.float64), n) for lam, dg in wc.PASSES]

    def margin(ref, x):
        delta = {k: x[o:o + dims[k]] for k, o in ref.off.items()}
        _, dd = sc.deviations(ref, ref.front, delta)  # (the factor itself is not under test here: the reference's own)
        return dd / tol_delta
    clean = [margin(ref, solve_with_wide_front(r, 0, nf)) for ref, r in zip((ref0, ref1), R)]
    print(f"    restatement: {clean[0]:.2e}, {clean[1]:.2e} of the tolerance")
    assert max(clean) <= 1.0, clean
    # (c) the planted defects, on the second pass (the one over a previous factor)
    nblk = len(wc.blocks(nf))
    mid = nblk // 2
    stale = inverses16(R[1], 0, nf)
    t = 8 * mid + 3  # a 16-block inside the middle 128-row block
    stale[t] = inverses16(R[0], 0, nf)[t]
    margins = [(f"M_B x_(B+1) dropped for block {mid}", margin(ref1, solve_with_wide_front(R[1], 0, nf, drop_hop=mid))),
               (f"16 x 16 inverse {t} left from the previous factor", margin(ref1, solve_with_wide_front(R[1], 0, nf, inv16=stale))),
               (f"fold of block {mid + 1} (128 columns) into block {mid - 1} skipped", margin(ref1, solve_with_wide_front(R[1], 0, nf, skip_fold=(mid - 1, mid + 1))))]
    for label, m in margins:
        print(f"    {label}: {m:.2e} x the tolerance")
    print(f"ROW {name:20s}  {fl['rsd']:.1e}  {fl['delta']:.1e}   {tol_delta:.1e}   {clean[0]:.1e}  {clean[1]:.1e}   " + " / ".join(f"{m:.1e}" for _, m in margins))
    for label, m in margins:
        assert m >= 100, (name, label, m)
