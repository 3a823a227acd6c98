"""CPU side of the LDS-front size-edge cases (tests/lds_front_cases.py), without a GPU.  Per case:

  * every front has the nf / n / parent / class / level it was built for (structure-only handle);
  * the restated dispatch (lds_front_cases.launches) gives the launch counts worked out by hand for the default form, and every
    (switch, case) pair of FORM_RUNS is one in which the switch changes the launch form the way the pair is there for;
  * the reference's residual, the float64 oracle's distance from it (the floor the GPU test scales its tolerance from), 16 x floor under
    the 1e-9 cap;
  * a clean float64 factorisation of the same matrix stays within the tolerance;
  * the comparison SEES what it is for: a float64 restatement (row-at-a-time right-looking Cholesky of the augmented matrix, back-
    substitution front by front) with ONE planted defect misses the case's own tolerance by at least 100 x.  The defects, each applied to the
    cases that have the feature:
      1. the factor at position 32 of a front's list left out of H                                  (a front with more than 32 factors)
      2. lambda D missing on one frontal diagonal entry: entry 8 where nf > 8, else the last one    (every case)
      3. a child's update entry (1, 64) -- row 1, column 64 of its update matrix -- not added      (a child with ns >= 64)
      4. rows 4..7 of one sixteen-pivot panel (the second where nf > 32) left out of the 16 x 16 diagonal tile behind it   (nf >= 17)
      5. in delta only: separator column 64 dropped from S x_S of one front                        (ns > 64)
      6. one frontal row of [R S d] left from the factorisation of pass 0 in pass 1                (every case)

Per case -- measured (floor = oracle against reference over both passes; tolerance of front 0 / of delta; the smallest planted defect's
deviation in tolerances, asserted >= 100, and which defect it was).
Smallest over all cases, per defect (cases it applies to): 1: 7.4e+09 on bin[16,122] (55); 2: 2.7e+03 on tiny_sfm (69); 3: 3.9e+07 on
bin[16,122] (9); 4: 2.0e+06 on pivots_wide[33] (50); 5: 2.3e+08 on children_wide (9); 6: 5.2e+08 on bin[96] (69).
The whole module takes 6 s:
    case                floor [R S d], delta   tolerance (front 0 / delta)   smallest defect / tolerance (which)
    bin[24]             1.1e-15  9.9e-15       3.4e-13 / 3.4e-13             2.1e+05 (2)
    bin[25]             2.2e-15  9.0e-15       3.5e-13 / 3.5e-13             3.8e+07 (2)
    bin[48]             1.1e-15  7.3e-15       6.8e-13 / 6.8e-13             4.9e+06 (2)
    bin[49]             1.4e-15  8.4e-15       6.9e-13 / 6.9e-13             3.4e+05 (2)
    bin[72]             9.7e-16  1.4e-14       1.0e-12 / 1.0e-12             9.7e+03 (2)
    bin[73]             7.2e-16  1.9e-14       1.0e-12 / 1.0e-12             6.2e+04 (2)
    bin[96]             1.3e-15  6.8e-15       1.4e-12 / 1.4e-12             9.1e+05 (2)
    bin[97]             1.2e-15  1.0e-14       1.4e-12 / 1.4e-12             2.9e+04 (2)
    bin[120]            1.0e-15  3.7e-15       1.7e-12 / 1.7e-12             4.4e+04 (2)
    bin[121]            8.8e-16  1.9e-14       1.7e-12 / 1.7e-12             4.1e+03 (2)
    bin[64,74]          6.0e-16  8.3e-15       2.0e-12 / 2.0e-12             5.4e+03 (2)
    bin[65,73]          8.4e-16  1.5e-14       2.0e-12 / 2.0e-12             8.2e+03 (2)
    bin[3,135]          8.5e-16  1.6e-14       2.0e-12 / 2.0e-12             2.2e+04 (2)
    bin[135,3]          1.2e-15  9.7e-15       2.0e-12 / 2.0e-12             2.5e+04 (2)
    bin[16,122]         6.1e-16  9.3e-15       2.0e-12 / 2.0e-12             2.3e+06 (2)
    bin_pooled          1.0e-15  1.6e-14       3.4e-13 / 1.4e-12             4.2e+04 (2)
    pivots[2]           7.7e-16  1.7e-14       2.5e-13 / 2.7e-13             1.2e+06 (2)
    pivots[3]           8.0e-16  6.6e-15       2.8e-13 / 2.8e-13             1.2e+07 (2)
    pivots[5]           2.2e-15  1.8e-14       3.0e-13 / 3.0e-13             1.0e+05 (2)
    pivots[7]           1.7e-15  1.4e-14       3.4e-13 / 3.4e-13             3.4e+07 (2)
    pivots[8]           1.3e-15  5.9e-15       3.4e-13 / 3.4e-13             6.5e+05 (2)
    pivots[9]           9.1e-16  5.3e-15       3.7e-13 / 3.7e-13             4.8e+05 (2)
    pivots[11]          1.1e-15  9.2e-15       3.8e-13 / 3.8e-13             9.1e+04 (2)
    pivots[12]          8.0e-16  1.6e-14       4.1e-13 / 4.1e-13             4.1e+05 (2)
    pivots[13]          5.1e-16  3.1e-14       4.1e-13 / 4.9e-13             3.5e+07 (2)
    pivots[15]          8.7e-16  7.8e-15       4.5e-13 / 4.5e-13             6.8e+05 (2)
    pivots[16]          1.8e-15  1.2e-14       4.5e-13 / 4.5e-13             1.3e+07 (2)
    pivots[17]          1.4e-15  1.1e-14       4.8e-13 / 4.8e-13             2.6e+07 (2)
    pivots[31]          1.3e-15  1.1e-14       6.6e-13 / 6.6e-13             2.6e+05 (2)
    pivots[32]          7.6e-16  6.8e-15       6.9e-13 / 6.9e-13             1.7e+05 (2)
    pivots[33]          1.0e-15  8.0e-15       6.9e-13 / 6.9e-13             3.0e+05 (2)
    pivots[47]          5.7e-16  5.9e-15       9.0e-13 / 9.0e-13             1.8e+06 (2)
    pivots[48]          6.0e-16  1.7e-14       9.0e-13 / 9.0e-13             5.7e+04 (2)
    pivots[49]          4.5e-16  7.0e-15       9.3e-13 / 9.3e-13             1.3e+05 (2)
    pivots_wide[31]     1.2e-15  1.9e-14       1.3e-12 / 1.3e-12             2.0e+06 (2)
    pivots_wide[32]     8.2e-16  9.8e-15       1.3e-12 / 1.3e-12             2.1e+04 (2)
    pivots_wide[33]     6.4e-16  9.5e-15       1.3e-12 / 1.3e-12             4.3e+04 (2)
    pivots_wide[47]     1.1e-15  8.9e-15       1.5e-12 / 1.5e-12             5.2e+04 (2)
    pivots_wide[48]     1.5e-15  6.0e-15       1.5e-12 / 1.5e-12             4.9e+03 (2)
    pivots_wide[49]     1.5e-15  1.1e-14       1.5e-12 / 1.5e-12             2.3e+04 (2)
    tiny[15]            1.5e-15  2.8e-14       2.1e-13 / 4.5e-13             2.6e+05 (2)
    tiny[16]            1.5e-15  1.8e-14       2.3e-13 / 2.9e-13             1.1e+05 (2)
    tiny[17]            1.2e-15  4.6e-15       2.4e-13 / 2.4e-13             8.0e+07 (2)
    tiny_tree           1.2e-15  8.9e-15       2.1e-13 / 2.3e-13             6.4e+05 (2)
    tiny_sfm            9.5e-16  2.2e-14       2.1e-13 / 3.6e-13             2.7e+03 (2)
    staging[31]         5.0e-15  3.2e-13       9.9e-14 / 5.0e-12             1.8e+05 (2)
    staging[32]         3.0e-15  1.2e-13       9.9e-14 / 1.9e-12             3.5e+05 (2)
    staging[33]         1.1e-15  8.2e-14       9.9e-14 / 1.3e-12             4.1e+05 (2)
    staging[64]         3.2e-14  5.9e-13       5.1e-13 / 9.4e-12             1.0e+05 (2)
    staging[65]         1.6e-14  2.0e-12       2.6e-13 / 3.2e-11             2.3e+04 (2)
    staging_pose3[7]    6.9e-16  5.0e-15       1.8e-13 / 1.8e-13             4.5e+05 (2)
    staging_pose3[8]    5.5e-16  5.4e-15       1.8e-13 / 1.8e-13             1.4e+05 (2)
    staging_mixed       2.7e-15  2.3e-14       9.9e-14 / 3.7e-13             1.3e+05 (2)
    staging[8,8]        2.9e-15  5.0e-15       2.4e-13 / 2.4e-13             1.2e+08 (2)
    staging[9,8]        1.1e-15  1.2e-14       2.5e-13 / 2.5e-13             1.6e+06 (2)
    children[1]         1.6e-15  7.8e-15       9.9e-14 / 3.1e-13             1.9e+05 (2)
    children[2]         1.6e-15  3.4e-15       9.9e-14 / 3.1e-13             4.6e+05 (2)
    children[3]         7.6e-16  1.1e-14       9.9e-14 / 3.1e-13             2.6e+05 (2)
    children[4]         3.7e-15  4.7e-15       9.9e-14 / 3.1e-13             3.2e+05 (2)
    children[5]         7.8e-16  5.7e-15       9.9e-14 / 3.1e-13             3.6e+05 (2)
    children_wide       8.1e-16  1.5e-14       9.4e-13 / 2.0e-12             1.0e+05 (2)
    backsub[63,15]      4.5e-16  8.1e-15       1.1e-12 / 1.1e-12             2.8e+04 (2)
    backsub[128,8]      5.8e-16  4.7e-15       1.9e-12 / 1.9e-12             4.1e+04 (2)
    backsub[129,6]      1.1e-15  1.5e-14       1.9e-12 / 1.9e-12             1.7e+04 (2)
    backsub[14,124]     5.1e-16  6.4e-15       2.0e-12 / 2.0e-12             1.4e+06 (2)
    backsub[15,123]     5.9e-16  8.0e-15       2.0e-12 / 2.0e-12             5.5e+03 (2)
    backsub_mixed       2.1e-15  4.2e-15       3.5e-13 / 3.5e-13             5.1e+07 (2)
    deep_chain          5.0e-16  4.2e-15       1.8e-13 / 1.8e-13             4.4e+05 (2)
    fused_level         1.8e-15  1.4e-14       3.7e-12 / 3.7e-12             1.6e+04 (2)
"""
import numpy as np
import pytest

import lds_front_cases as lc
import schur_cases as sc
from dense_reference import FactorView, augmented_information
from gtsam_personal_amd import LevenbergMarquardtOptimizer

# the default form's launches per solve, by hand from the dispatch: (lds_front, backsub_lds).  Two-level cases: one launch per level, both
# ways (a level's bins are pooled into its top bin); single fronts one; tiny_tree three levels; deep_chain thirteen levels in ONE merged
# launch each way; fused_level without the switch two levels (its medium front is the dense path's business)
_SINGLE = tuple(f"staging[{k}]" for k in lc.STAGING_COUNTS) + ("staging_pose3[7]", "staging_pose3[8]", "staging_mixed")
DEFAULT_LAUNCHES = {name: (1, 1) if name in _SINGLE or name == "deep_chain" else (3, 3) if name == "tiny_tree" else (2, 2) for name in lc.CASES}


def _infos(c):
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)
    return [opt.front_info(i) for i in range(opt.num_fronts())]


@pytest.mark.parametrize("name", list(lc.CASES))
def test_fronts_and_launch_counts(name):
    c = lc.case(name)
    infos = _infos(c)
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"], level=f["level"]) for f in infos] == c["fronts"], infos
    got = lc.launches(c["fronts"])
    medium = 1 if name == "fused_level" else 0  # its medium front: one panel and one syrk event of the batched path
    assert (got["lds_front"], got["backsub_lds"], got["panel"], got["syrk"]) == DEFAULT_LAUNCHES[name] + (medium, medium), got


def test_class_edge():
    """(17,122) is one column too wide for LDS: n = 140, class 1"""
    c = lc.tree_case(1, lc.pair(17, 122))
    assert c["fronts"][0] == dict(nf=17, n=140, parent=1, cls=1, level=0)
    f = _infos(c)[0]
    assert (f["nf"], f["n"], f["cls"]) == (17, 140, 1)


@pytest.mark.parametrize("switch,name", [(sw, nm) for sw, names in lc.FORM_RUNS for nm in names], ids=lambda v: v if isinstance(v, str) else "=".join(v))
def test_form_runs_change_the_form(switch, name):
    """the pair is worth its GPU time: under the switch the case's launches are the form the pair is listed for"""
    fronts = lc.case(name)["fronts"]
    levels = 1 + max(f["level"] for f in fronts)
    got = lc.launches(fronts, **lc.FORM_ARGUMENT[switch])
    if switch == ("LMGPU_MERGE_ELIM", "1"):  # ONE merged launch over all levels
        segs = lc.elim_segments(fronts)
        assert segs and (segs[0][0], segs[0][1]) == (0, levels - 1) and got["lds_front"] == 1, (segs, got)
        widest = max(f["n"] for f in fronts)
        assert segs[0][2] == (64 if widest <= 24 else 256 if widest <= 72 else 1024)
        if segs[0][2] == 1024:  # a sixteen-wave segment has no four-wave level
            assert all(max(f["n"] for f in fronts if f["level"] == l) > 72 for l in range(levels))
    elif switch == ("LMGPU_MERGE_ELIM", "0"):
        assert lc.launches(fronts)["lds_front"] == 1 and got["lds_front"] == levels
    elif switch == ("LMGPU_MERGE_BACKSUB", "1"):
        assert got["backsub_lds"] == 1 and levels >= 2
    elif switch == ("LMGPU_MERGE_BACKSUB", "0"):
        assert lc.launches(fronts)["backsub_lds"] == 1 and got["backsub_lds"] == levels
    elif switch == ("LMGPU_NO_WIDE16", "1"):  # a launch that takes sixteen waves by default
        assert any(f["n"] > 72 and f["cls"] == 0 for f in fronts) and got == lc.launches(fronts)
    elif switch == ("LMGPU_FUSE_LEVELS", "1"):
        assert got == dict(lds_front=1, backsub_lds=2, panel=1, syrk=0)
    else:
        assert switch == ("LMGPU_NO_LEAFPACK", "1") and got == lc.launches(fronts)


def test_edges_are_where_the_cases_put_them():
    """the sizes the docstring of lds_front_cases claims, from the built cases"""
    def f0(name):
        return lc.case(name)["fronts"][0]
    for n in lc.BIN_PAIRS:
        assert f0(f"bin[{n}]")["n"] == n
    assert all(f0(f"bin[{a},{b}]")["n"] == 139 for a, b in lc.LIMIT_PAIRS)
    assert {f0(f"pivots[{nf}]")["n"] - nf for nf in lc.PIVOT_NF} == {16, 17}
    assert [f0(f"tiny[{n}]")["n"] for n in lc.TINY_PAIRS] == [15, 16, 17]
    tt = lc.case("tiny_tree")["fronts"]
    assert max(f["n"] for f in tt) == 16 and sorted(sum(1 for g in tt if g["parent"] == i) for i in range(len(tt))) == [0, 0, 0, 0, 1, 2, 3]
    assert [lc.case(f"staging[{k}]")["graph"].size() for k in lc.STAGING_COUNTS] == list(lc.STAGING_COUNTS)
    assert 2 * 42 + 7 * 78 <= lc.LDSF_JCAP < 2 * 42 + 8 * 78
    assert sorted(f["n"] - f["nf"] for f in lc.case("children_wide")["fronts"][:5]) == [64, 65, 66, 128, 129]
    assert [f0(f"backsub[{a},{b}]")["nf"] * f0(f"backsub[{a},{b}]")["n"] for a, b in ((14, 124), (15, 123))] == [1946, 2085]
    assert lc.backsub_kernel(lc.case("backsub_mixed")["fronts"], 0) == "wide" and lc.backsub_kernel(lc.case("children[5]")["fronts"], 0) == "small"
    assert lc.backsub_kernel(lc.case("bin[24]")["fronts"], 0) == "small" and lc.backsub_kernel(lc.case("bin[25]")["fronts"], 0) == "wide"
    fl = lc.case("fused_level")["fronts"]
    assert sorted((f["cls"], f["nf"]) for f in fl if f["level"] == 0) == [(0, 13), (1, 192)]


# ------------------------------------------------------------------------------------------------ a float64 factor with a defect
def _cholesky64(H, n, skip=None):
    """[R d] (n, n + 1) of the float64 augmented matrix H, right-looking, a row at a time.  skip = (rows, row indices, column indices):
    the rank-1 updates of those pivot rows leave out the entries (row indices x column indices) of the trailing matrix"""
    W = np.array(H, dtype=np.float64)
    for j in range(n):
        W[j, j:] /= np.sqrt(W[j, j])
        U = np.multiply.outer(W[j, j + 1:], W[j, j + 1:])
        if skip is not None and j in skip[0]:
            U[np.ix_(np.asarray(skip[1]) - j - 1, np.asarray(skip[2]) - j - 1)] = 0
        W[j + 1:, j + 1:] -= U
    return np.triu(W)[:n]


def _columns(ref, dims, i):
    """global columns of front i's keys (frontal scalars first) and the rhs column; its number of frontal scalars"""
    keys, nfk = ref.fronts[i]
    cols = np.concatenate([np.arange(ref.off[k], ref.off[k] + dims[k]) for k in keys] + [[ref.n]])
    return cols, sum(dims[k] for k in keys[:nfk])


def _margin(ref, view, fronts_rsd_tol, delta_tol):
    """the largest deviation / tolerance of a factor view against the reference, over the fronts and delta"""
    per_front, dd = sc.deviations(ref, view.front, view.delta())
    return max(max(d / t for d, t in zip(per_front, fronts_rsd_tol)), dd / delta_tol)


def _measure(name):
    c = lc.case(name)
    widths = [f["n"] for f in c["fronts"]]
    kept = []
    fl = sc.floor_of(c, lc.PASSES, lc.BLOCK, keep=kept)
    tol_rsd, tol_delta = lc.tolerances(fl, widths)
    assert fl["residual"] < 1e-17
    assert lc.FACTOR * fl["rsd"] <= lc.CAP and lc.FACTOR * fl["delta"] <= lc.CAP, fl
    import oracle_harness as oh
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    factors = list(zip(c["graph"].factor_keys_in_graph_order(), [orc.jacobian(g) for g in range(c["graph"].size())]))
    dims = sc.var_dims(c)
    (ref0, _, _), (ref1, _, _) = kept
    fronts, n = ref0.fronts, ref0.n
    H = [augmented_information(factors, dims, lam, dg, fronts)[0].astype(np.float64) for lam, dg in lc.PASSES]

    def view(R):
        return FactorView(R, ref0.off, dims, fronts)

    def margin0(R):
        return _margin(ref0, view(R), tol_rsd, tol_delta)
    R0, R1 = _cholesky64(H[0], n), _cholesky64(H[1], n)
    clean = [margin0(R0), _margin(ref1, view(R1), tol_rsd, tol_delta)]
    assert max(clean) <= 1.0, clean
    cols = [_columns(ref0, dims, i) for i in range(len(fronts))]
    lds = [i for i, f in enumerate(c["fronts"]) if f["cls"] == 0]
    margins = {}
    # 1. the factor at position 32 of a front's list
    first = {}  # front -> its factors, in graph order: a factor belongs to the front of its first-eliminated variable
    front_of = {k: i for i, (keys, nfk) in enumerate(fronts) for k in keys[:nfk]}
    for g, (keys, _) in enumerate(factors):
        first.setdefault(front_of[min(keys, key=lambda k: ref0.off[k])], []).append(g)
    i = next((i for i in lds if len(first.get(i, ())) > lc.LDSF_MAXB), None)
    if i is not None:
        g = first[i][lc.LDSF_MAXB]
        Hd = augmented_information(factors[:g] + factors[g + 1:], dims, lc.PASSES[0][0], False, fronts)[0].astype(np.float64)
        margins[1] = margin0(_cholesky64(Hd, n))
    # 2. lambda D missing on one frontal diagonal entry
    i = next((i for i in lds if cols[i][1] > 8), lds[0])
    j = cols[i][0][min(8, cols[i][1] - 1)]
    Hd = H[0].copy()
    Hd[j, j] -= lc.PASSES[0][0]
    margins[2] = margin0(_cholesky64(Hd, n))
    # 3. a child's update entry (1, 64) not added
    i = next((i for i in lds if c["fronts"][i]["parent"] >= 0 and len(cols[i][0]) - cols[i][1] >= 65), None)
    if i is not None:
        cc, nf = cols[i]
        gi, gj = sorted((cc[nf + 1], cc[nf + 64]))
        margins[3] = margin0(_cholesky64(H[0], n, skip=(set(cc[:nf]), [gi], [gj])))
    # 4. rows 4..7 of a sixteen-pivot panel left out of the diagonal tile behind it
    i = next((i for i in lds if cols[i][1] >= 17), None)
    if i is not None:
        cc, nf = cols[i]
        p = 1 if nf > 32 else 0
        tile = cc[16 * (p + 1):min(16 * (p + 2), nf)]
        margins[4] = margin0(_cholesky64(H[0], n, skip=(set(cc[16 * p + 4:16 * p + 8]), tile, tile)))
    # 5. delta only: separator column 64 dropped from S x_S of one front
    i = next((i for i in lds if len(cols[i][0]) - 1 - cols[i][1] > 64), None)
    if i is not None:
        cc, nf = cols[i]
        Rd = R0.copy()
        Rd[np.ix_(cc[:nf], [cc[nf + 64]])] = 0  # (only the back-substitution reads the defective copy)
        v = view(R0)
        v._x = view(Rd)._x
        margins[5] = _margin(ref0, v, tol_rsd, tol_delta)
    # 6. one frontal row left from the previous factorisation
    cc, nf = cols[lds[0]]
    Rd = R1.copy()
    Rd[cc[min(8, nf - 1)]] = R0[cc[min(8, nf - 1)]]
    margins[6] = _margin(ref1, view(Rd), tol_rsd, tol_delta)
    return fl, tol_rsd, tol_delta, clean, margins


@pytest.mark.parametrize("name", list(lc.CASES))
def test_lds_front_case(name):
    fl, tol_rsd, tol_delta, clean, margins = _measure(name)
    print(f"{name}: residual {fl['residual']:.2e}; the float64 factor without a defect: {clean[0]:.2e}, {clean[1]:.2e} of the tolerance; defects "
          + ", ".join(f"{k}: {m:.2e}" for k, m in margins.items()))
    k = min(margins, key=margins.get)
    print(f"ROW {name:18s} {fl['rsd']:.1e}  {fl['delta']:.1e}   {tol_rsd[0]:.1e} / {tol_delta:.1e}   {margins[k]:.1e} ({k})")
    assert {2, 6} <= set(margins)
    for k, m in margins.items():
        assert m >= 100, (name, k, m)


def test_every_defect_is_planted_somewhere():
    """each of the six defects has at least one case with the feature (the per-case test only applies those that fit)"""
    def has(name):
        fr = lc.case(name)["fronts"]
        return dict(d3=any(f["parent"] >= 0 and f["n"] - f["nf"] >= 65 and f["cls"] == 0 for f in fr), d4=any(f["nf"] >= 17 and f["cls"] == 0 for f in fr),
                    d5=any(f["n"] - f["nf"] - 1 > 64 and f["cls"] == 0 for f in fr))
    feats = [has(n) for n in lc.CASES]
    assert all(any(f[k] for f in feats) for k in ("d3", "d4", "d5"))
    assert lc.case("staging[33]")["graph"].size() > lc.LDSF_MAXB


@pytest.mark.parametrize("name", [nm for nm, _ in lc.MARGINAL_RUNS])
def test_marginal_floor(name):
    """the oracle's marginal covariances against the block of (R^T R)^-1 of the reference at lambda = 0: 16 x that under the cap"""
    import oracle_harness as oh
    c = lc.case(name)
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    jac = [orc.jacobian(g) for g in range(c["graph"].size())]
    assert orc.solve(0.0, False)[0] == 0
    ref = sc.reference(c, jac, [(keys, nfk) for keys, nfk, _, _ in orc.cliques()], 0.0, False, lc.BLOCK)
    assert ref.residual < 1e-17
    for key in lc.marginal_keys(c):
        want = lc.covariance_block(ref, key)
        dev = lc.block_deviation(orc.marginal_covariance(key, want.shape[0]), want)
        print(f"{name} key {key}: oracle marginal covariance against the reference block {dev:.2e}")
        assert np.allclose(np.asarray(want, dtype=float), np.asarray(want, dtype=float).T, rtol=1e-12, atol=0) and lc.FACTOR * dev <= lc.CAP
