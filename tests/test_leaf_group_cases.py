"""CPU side of the lane-group leaf kernel (lds_front_group_kernel, csrc/kernels_leaf.hpp): that the cases of tests/leaf_group_cases.py
have the structure they claim, that the library's structure-only query (lmgpu_leaf_group_launches, on a device = -1 handle) agrees with
the eligibility rule restated there, and that the comparison the GPU test makes (tests/test_gpu_leaf_group_edges.py: every front's
[R S d] against the dense extended-precision reference, tolerance max(16 x oracle floor, 64 n 2.2e-16)) has teeth for the mistakes such
a kernel can make.

The planted mistakes act on a float64 elimination of ONE leaf from the oracle's Jacobians (the arithmetic the kernel does: frontal
block and rhs summed over the factors, damping, Cholesky of the nf x nf block, a solve per separator block, the corner), compared like
a device result with the reference's [R S d] of that leaf and with the corner sum_f b^T b - d^T d formed from the reference's d:
  1. one factor's contribution to the frontal block dropped (a lane left out of the row sum)
  2. damping skipped
  3. a separator block written to its neighbour's columns (two lanes' column offsets exchanged)
  4. the corner without - d^T d
at (lambda = 1e-2, diagonal damping), the second pass of the GPU test; asserted > 100 x the tolerance on every leaf the mistake can be
planted on (1: two factors or more; 3: two separator variables of one size or more).  The clean float64 elimination stays <= 1 x."""
import os
import re

import numpy as np
import pytest

import leaf_group_cases as lg
import oracle_harness as oh
import schur_cases as sc
from gtsam_personal_amd import LevenbergMarquardtOptimizer
from gtsam_personal_amd.synthetic import make_bal

FACTOR, EPS, CAP = 16, 2.2e-16, 1e-9  # the rule of tests/test_gpu_schur_edges.py
LD = np.longdouble


def test_constants_are_the_kernels():
    here = os.path.dirname(__file__)
    src = open(os.path.join(here, "..", "gtsam_personal_amd", "csrc", "kernels_leaf.hpp")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LEAFGRP_\w+) (\d+)", src, flags=re.M)}
    assert (defs["LEAFGRP_MAXNF"], defs["LEAFGRP_MAXROWS"], defs["LEAFGRP_MAXSEP"], defs["LEAFGRP_LANES"]) == (lg.MAXNF, lg.MAXROWS, lg.MAXSEP, lg.LANES)
    front = open(os.path.join(here, "..", "gtsam_personal_amd", "csrc", "kernels_front.hpp")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LDSF_\w+) (\d+)", front, flags=re.M)}
    assert (defs["LDSF_MAXB"], defs["LDSF_JCAP"]) == (lg.MAXB, lg.JCAP)


def _handle(c):
    return LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)


@pytest.mark.parametrize("name", list(lg.CASES))
def test_case_structure_and_query(name):
    c = lg.case(name)
    dims = sc.var_dims(c)
    opt = _handle(c)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    root = infos[-1]
    assert root["cls"] == 1 and root["n"] > lg.LDS_MAX_N and root["parent"] == -1, root
    gather = [lf for lf in c["leaves"] if lg.leaf_width(lf, dims) <= lg.LDS_MAX_N]
    # every such leaf is an LDS front directly under the root: a gather leaf of ONE launch
    assert len(gather) <= lg.MERGE_MAX
    lds = [f for f in infos if f["cls"] == 0]
    assert len(lds) == len(gather) and all(f["parent"] == len(infos) - 1 and f["level"] == 0 for f in lds)
    assert sorted(f["n"] for f in lds) == sorted(lg.leaf_width(lf, dims) for lf in gather)
    counts = [len(lf[2]) + len(c["unary"].get(lf[0], [])) for lf in gather]
    assert counts == lg.FACTOR_COUNTS[name]
    launches = lg.group_launches(c)
    assert launches == [(len(gather), lg.FORMS[name] or 0)]
    assert opt.leaf_group_launches() == lg.expected_group_launches(c) == (1 if lg.FORMS[name] else 0)
    assert opt.backsub_group_launches() == lg.expected_backsub_groups(infos) == lg.BACKSUB_FORMS[name]


def test_cases_cover_the_lane_rounds_and_launch_sizes():
    assert lg.FACTOR_COUNTS["sfm_counts"] == [1, 2, 9, 10, 15, 16, 17, 31, 32]
    assert {lg.LANES - 1, lg.LANES, lg.LANES + 1, lg.MAXB - 1, lg.MAXB} <= set(lg.FACTOR_COUNTS["sfm_counts"]) and lg.MAXB + 1 in lg.FACTOR_COUNTS["sfm_33"]
    sizes = {name: len(lg.FACTOR_COUNTS[name]) for name in ("sfm_n1", "sfm_n3", "sfm_n4", "sfm_n5", "sfm_counts")}
    assert sorted(sizes.values()) == [1, 3, 4, 5, 9]  # leaves per launch: four to a wave
    # C4's first point: camera factors and a 3-row unary prior
    c = lg.case("sfm_n3")
    assert any(len(lf[2]) >= 2 and c["unary"][lf[0]] == [3] for lf in c["leaves"])
    # the twice-seen point and what makes it ineligible
    c = lg.case("sfm_twice")
    dims = sc.var_dims(c)
    assert [lg.eligible(lf, c["unary"].get(lf[0], []), dims) for lf in c["leaves"][:4]] == [1, 1, 0, 1]
    # planar: nf = 2, separator blocks of 3, two rows; the Pose2 leaves bring three rows
    c = lg.case("planar_pose")
    dims = sc.var_dims(c)
    assert {(lf[1], r, dims[k]) for lf in c["leaves"] for k, r in lf[2]} == {(2, 2, 3), (3, 3, 3)}


@pytest.mark.parametrize("n_cam,n_pt,obs", [(20, 300, 6), (24, 700, 6)])
def test_query_on_make_bal_with_its_prior_leaf(n_cam, n_pt, obs):
    """synthetic.make_bal: every point seen by `obs` distinct cameras, a 3-row prior on the first point; up to 512 points one launch,
    beyond that one per occupied size bin (all points but the first are n = 4 + 9 obs wide, the first as well: the prior adds none)"""
    graph, initial, _, ordering = make_bal(n_cam=n_cam, n_pt=n_pt, obs_per_point=obs, seed=5)
    opt = LevenbergMarquardtOptimizer(graph, initial, ordering, device=-1)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert infos[-1]["cls"] == 1 and infos[-1]["n"] == 9 * n_cam + 1, infos[-1]
    assert sum(f["cls"] == 0 for f in infos) == n_pt and {f["n"] for f in infos[:-1]} == {4 + 9 * obs}
    assert opt.leaf_group_launches() == 1
    assert opt.backsub_group_launches() == lg.expected_backsub_groups(infos) == (1, 0)


@pytest.mark.parametrize("name", list(lg.CASES))
def test_reference_residual_and_oracle_floor(name):
    fl = lg.oracle_floor(name)
    print(f"{name}: reference residual {fl['residual']:.2e}; oracle vs reference [R S d] {fl['rsd']:.2e}, delta {fl['delta']:.2e}")
    assert fl["residual"] < 1e-17
    assert FACTOR * fl["rsd"] <= CAP and FACTOR * fl["delta"] <= CAP


# ------------------------------------------------------------------------------------------------ planted mistakes
def _eliminate_leaf(keys, dims, factors, lam, diagonal, defect=None):
    """float64 elimination of the leaf front `keys` (frontal key first) from its factors [(keys, Ab)]: ([R S d], corner)"""
    off, n = {}, 0
    for k in keys:
        off[k] = n
        n += dims[k]
    nf = dims[keys[0]]
    H = np.zeros((n + 1, n + 1))
    for q, (fkeys, Ab) in enumerate(factors):
        cols = np.concatenate([np.arange(off[k], off[k] + dims[k]) for k in fkeys] + [[n]])
        G = Ab.T @ Ab
        if defect == "drop_factor" and q == len(factors) - 1:
            fr = cols < nf
            G[np.ix_(fr, fr)] = 0.0
        H[np.ix_(cols, cols)] += G
    if defect != "no_damping":
        d = np.diagonal(H)[:nf].copy()
        H[np.arange(nf), np.arange(nf)] += lam * (np.clip(d, 1e-6, 1e32) if diagonal else np.ones(nf))
    Lc = np.linalg.cholesky(H[:nf, :nf])
    X = np.hstack([Lc.T, np.linalg.solve(Lc, H[:nf, nf:])])
    corner = H[n, n] - (0.0 if defect == "corner" else X[:, n] @ X[:, n])
    if defect == "shift_block":
        a, b = [k for k in keys[1:]][:2]
        X[:, off[a]:off[a] + dims[a]], X[:, off[b]:off[b] + dims[b]] = X[:, off[b]:off[b] + dims[b]].copy(), X[:, off[a]:off[a] + dims[a]].copy()
    return X, corner


@pytest.mark.parametrize("name", [n for n in lg.CASES if lg.FORMS[n]])
def test_planted_mistakes_miss_the_tolerance_by_a_wide_factor(name):
    c, fl = lg.case(name), lg.oracle_floor(name)
    dims = sc.var_dims(c)
    lam, diagonal = lg.PASSES[1]
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    jac = [orc.jacobian(g) for g in range(c["graph"].size())]
    rc, _, _, _ = orc.solve(lam, diagonal)
    assert rc == 0
    fronts = [(keys, nfk) for keys, nfk, _, _ in orc.cliques()]
    ref = sc.reference(c, jac, fronts, lam, diagonal)
    fk = c["graph"].factor_keys_in_graph_order()
    margins = {"drop_factor": [], "no_damping": [], "shift_block": [], "corner": []}
    clean = []
    for i, (keys, nfk) in enumerate(fronts[:-1]):
        n = sum(dims[k] for k in keys) + 1
        if nfk != 1 or n > lg.LDS_MAX_N:
            continue
        factors = [(fk[g], jac[g]) for g in range(len(fk)) if keys[0] in fk[g]]
        want = ref.front(i)
        d = want[:, -1]
        corner_ref = sum((LD(1) * Ab[:, -1].astype(LD)) @ Ab[:, -1].astype(LD) for _, Ab in factors) - d @ d
        tol = max(FACTOR * fl["rsd"], 64 * n * EPS)

        def dev(defect):
            try:
                X, corner = _eliminate_leaf(keys, dims, factors, lam, diagonal, defect)
            except np.linalg.LinAlgError:  # (the once-seen point without damping: a pivot <= 0, which the device reports as a failed front)
                return np.inf
            return max(float(np.abs(X.astype(LD) - want).max() / np.abs(want).max()), float(abs(LD(corner) - corner_ref) / abs(corner_ref))) / tol

        clean.append(dev(None))
        margins["no_damping"].append(dev("no_damping"))
        margins["corner"].append(dev("corner"))
        if len(factors) >= 2:
            margins["drop_factor"].append(dev("drop_factor"))
        seps = keys[1:]
        if len(seps) >= 2 and dims[seps[0]] == dims[seps[1]]:
            margins["shift_block"].append(dev("shift_block"))
    print(f"{name}: clean float64 leaf elimination / tolerance: largest {max(clean):.2e}")
    assert max(clean) <= 1.0, clean
    for what, m in margins.items():
        assert m, (name, what)
        print(f"{name}: {what}: deviation / tolerance over {len(m)} leaves: least {min(m):.2e}, largest {max(m):.2e}")
        assert min(m) > 100, (what, m)
