"""CPU side of the Schur-assembly edge cases (tests/schur_cases.py): the dense extended-precision reference against itself and
against a known answer, the float64 oracle against the reference (the floors the GPU test scales its tolerance from), and --
without a GPU, through a structure-only handle -- that every case takes the branch it was built for, with the list lengths
counted here from the case's own visibility table."""
import itertools

import numpy as np
import pytest

import oracle_harness as oh
import schur_cases as sc
from dense_reference import DenseReference
from gtsam_personal_amd import LevenbergMarquardtOptimizer
from gtsam_personal_amd.graph import C, X
from gtsam_personal_amd.graph import L as Lm

FLOOR_BOUND = 1e-10  # a condition on the inputs: a case that misses it is badly conditioned and gets repaired, not excused


@pytest.mark.parametrize("name", list(sc.CASES))
def test_reference_residual_and_oracle_floor(name):
    fl = sc.oracle_floor(name)
    print(f"{name}: reference residual {fl['residual']:.2e}; oracle vs reference [R S d] {fl['rsd']:.2e}, delta {fl['delta']:.2e}; "
          + "; ".join(f"lambda {lam:g} {'diag' if dg else 'id'}: {r:.1e} / {d:.1e}" for lam, dg, r, d in fl["detail"]))
    assert fl["residual"] < 1e-17
    assert fl["rsd"] < FLOOR_BOUND and fl["delta"] < FLOOR_BOUND


def test_reference_reproduces_small_example_delta():
    """tests/smallExample.h:270-289 (createGaussianFactorGraph) and createCorrectDelta (:248-256), as test_oracle_golden has them"""
    I2 = np.eye(2)
    x1, x2, l1 = X(1), X(2), Lm(1)
    fac = [([x1], np.hstack([10 * I2, -1.0 * np.ones((2, 1))])),
           ([x1, x2], np.hstack([-10 * I2, 10 * I2, np.array([[2.0], [-1.0]])])),
           ([x1, l1], np.hstack([-5 * I2, 5 * I2, np.array([[0.0], [1.0]])])),
           ([x2, l1], np.hstack([-5 * I2, 5 * I2, np.array([[-1.0], [1.5]])]))]
    expect = {l1: (-0.1, 0.1), x1: (-0.1, -0.1), x2: (0.1, -0.2)}
    for order in itertools.permutations([x1, x2, l1]):
        ref = DenseReference(fac, {x1: 2, x2: 2, l1: 2}, 0.0, False, [(list(order[i:]), 1) for i in range(3)])
        assert ref.residual < 1e-17
        for k, e in expect.items():
            assert np.allclose(ref.delta()[k].astype(float), e, atol=1e-9), (order, k)
        R = ref.front(0)
        assert R.shape == (2, 7) and abs(float(R[1, 0])) == 0.0 and float(R[0, 0]) > 0


def test_oracle_comparison_notices_a_changed_leaf_factor():
    """the comparison has teeth: one entry of one leaf factor off by 1e-8 relative lifts the oracle's deviation far above the floor.
    (Swapping two ROWS of a factor must not: [A b]^T [A b] does not depend on the row order.)"""
    c = sc.case("dims_2_3")
    fl = sc.oracle_floor("dims_2_3")
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    jac = [orc.jacobian(g) for g in range(c["graph"].size())]
    rc, delta, _, _ = orc.solve(1e-3, False)
    cl = orc.cliques()
    fronts = [(keys, nfk) for keys, nfk, _, _ in cl]
    leaf_key = c["leaves"][2][0]  # the landmark seen by five poses
    g = next(i for i, keys in enumerate(c["graph"].factor_keys_in_graph_order()) if leaf_key in keys)

    def worst(j):
        per_front, dd = sc.deviations(sc.reference(c, j, fronts, 1e-3, False), lambda i: cl[i][2], delta)
        return max(per_front), dd
    swapped = [a.copy() for a in jac]
    swapped[g][[0, 1]] = swapped[g][[1, 0]]
    r, d = worst(swapped)
    assert r <= fl["rsd"] and d <= fl["delta"]
    bent = [a.copy() for a in jac]
    bent[g][0, 0] *= 1.0 + 1e-8
    r, d = worst(bent)
    assert r > 1e-10 and r > 100 * fl["rsd"], (r, fl)


# ------------------------------------------------------------------------------------------------ structure, without a GPU
def _structure(name):
    c = sc.case(name)
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)
    fronts = []
    for i in range(opt.num_fronts()):
        keys, _ = opt.front(i, numeric=False)
        fronts.append(dict(opt.front_info(i), keys=keys))
    dims = sc.var_dims(c)
    front_of = {k: i for i, f in enumerate(fronts) for k in f["keys"][:f["n_frontal_keys"]]}
    position = {k: i for i, k in enumerate(c["ordering"])}
    return c, fronts, dims, front_of, position


@pytest.mark.parametrize("name", list(sc.CASES))
def test_every_leaf_and_root_has_its_intended_front(name):
    """every leaf of the visibility table is a front of its own (no merge into the root), with the class, n, nf, parent and level it
    was built for; every other variable is frontal in a class-1 root with n = nf + 1 (level 1 when it has leaves)"""
    c, fronts, dims, front_of, _ = _structure(name)
    leaf_keys = set()
    for leaf in c["leaves"]:
        key, nf, links = leaf
        leaf_keys.add(key)
        f = fronts[front_of[key]]
        n = sc.leaf_n(leaf, dims)
        assert f["n_frontal_keys"] == 1 and (f["nf"], f["n"]) == (nf, n), (key, f)
        assert f["cls"] == (0 if n <= sc.LDS_MAX_N else 1) and f["level"] == 0
        assert f["parent"] == front_of[links[0][0]] and set(f["keys"][1:]) == {k for k, _ in links}
    roots = [f for f in fronts if f["keys"][0] not in leaf_keys]
    assert len(roots) + len(c["leaves"]) == len(fronts)
    for i, f in enumerate(fronts):
        if f["keys"][0] in leaf_keys:
            continue
        has_children = any(g["parent"] == i for g in fronts)
        assert f["cls"] == 1 and f["parent"] == -1 and f["level"] == int(has_children) and f["n"] == f["nf"] + 1 and f["n"] > sc.LDS_MAX_N
        assert f["n_keys"] == f["n_frontal_keys"]
    n_hbm = sum(f["cls"] == 1 for f in fronts)
    assert n_hbm == dict(leaf_degrees=3, many_hbm_fronts=5).get(name, 1)


def _lists(name):
    c, fronts, dims, front_of, position = _structure(name)
    pairs, factors = sc.gather_lists(c["leaves"], dims, position)
    return c, fronts, dims, front_of, pairs, factors


def test_lists_reaches_every_list_length_boundary():
    c, fronts, dims, front_of, pairs, factors = _lists("lists")
    off = {k: v for k, v in pairs.items() if k[0] != k[1] and k[1] != sc.RHS}
    assert sorted(len(v) for v in off.values()) == sorted(sc.LIST_LENGTHS)  # 1..5: count mod 4; 32 | 33: one wave | four; 256 | 257: a second batch
    assert {k: len(v) for k, v in off.items()} == {(C(0), C(k)): n for k, n in enumerate(sc.LIST_LENGTHS, start=1)}
    # diagonal and rhs lists = points per camera
    assert len(pairs[(C(0), C(0))]) == len(pairs[(C(0), sc.RHS)]) == sum(sc.LIST_LENGTHS) == 1333
    for k, n in enumerate(sc.LIST_LENGTHS, start=1):
        assert len(pairs[(C(k), C(k))]) == len(pairs[(C(k), sc.RHS)]) == n
    assert len(factors[C(0)]) == 1333
    # four waves with a short list: count 33 -> chunks of 9, 9, 9, 6; count 5 on one wave -> groups of 4 + 1
    assert [len(g) for g in sc.groups_of_four(5)] == [4, 1]
    assert [sum(len(g) for g in sc.groups_of_four(33)[i:i + 3]) for i in (0, 3, 6)] == [9, 9, 9]
    # write mode: the root's children are all gather leaves, one HBM front, and 120 of the 136 camera pairs have no list at all
    assert sum(f["cls"] == 1 for f in fronts) == 1 and all(sc.leaf_n(lf, dims) <= sc.LDS_MAX_N for lf in c["leaves"])
    assert 17 * 16 // 2 - len(off) == 120
    # the longest list is not a contiguous run of leaves: its S blocks interleave with every other list's in the pool
    idx = [j for j, vis in enumerate(c["visibility"]) if vis == (0, 16)]
    assert len(idx) == 260 and idx[-1] - idx[0] > 4 * 260


def test_leaf_degrees_reaches_the_leaf_class_edge():
    c, fronts, dims, front_of, pairs, factors = _lists("leaf_degrees")
    by_degree = {}
    for leaf in c["leaves"]:
        by_degree.setdefault(len(leaf[2]), []).append(fronts[front_of[leaf[0]]])
    assert sorted(by_degree) == [1, 2, 14, 15, 16] and all(len(v) >= 2 for v in by_degree.values())
    assert all((f["cls"], f["n"]) == (0, 139) for f in by_degree[15])  # the LDS maximum
    assert all((f["cls"], f["nf"], f["n"]) == (1, 3, 148) for f in by_degree[16])  # a three-row panel, an update matrix
    root = len(fronts) - 1
    assert all(f["parent"] == root for v in by_degree.values() for f in v)  # the root receives both kinds of child: add mode
    assert len(pairs[(C(0), C(0))]) == 7 and (C(0), C(1)) in pairs  # camera 0: one pair point, the 14- and the 15-camera points


def test_wide_leaves_mixes_nf_inside_a_group_of_four():
    c, fronts, dims, front_of, pairs, factors = _lists("wide_leaves")
    kinds = set()
    for nfs in pairs.values():
        for g in sc.groups_of_four(len(nfs)):
            if len(g) == 4:
                kinds.add(tuple(sorted({nfs[i] for i in g})))
    assert {(3,), (6,), (3, 6)} <= kinds
    assert [pairs[(X(0), X(0))][i] for i in range(14)] == [6, 6, 6, 6, 3, 3, 3, 3, 6, 3, 6, 3, 6, 3]
    assert len(pairs[(X(0), X(0))]) % 4 == 2
    rows = factors[X(0)]
    assert rows[:4] == [6, 6, 6, 6] and rows[4:8] == [2, 2, 2, 2] and set(rows[8:12]) == {2, 6}  # the factor kernel's split on rows <= 4


def test_vec9_has_three_operand_passes():
    c, fronts, dims, front_of, pairs, factors = _lists("vec9")
    assert all(nf == 9 for v in pairs.values() for nf in v) and all(r == 9 for v in factors.values() for r in v)  # k0 = 0, 4, 8
    assert len(pairs[(X(0), X(0))]) == 7 and {len(lf[2]) for lf in c["leaves"]} == {1, 2, 3}
    (j, pos), = sc.VEC9_ZERO_PRECISION
    g = next(i for i, keys in enumerate(c["graph"].factor_keys_in_graph_order()) if set(keys) == {c["leaves"][j][0], c["leaves"][j][2][pos][0]})
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    assert orc.jacobian(g).shape == (9, 19) and not orc.jacobian(g).any()  # the precision-0 factor: nine rows of zeros


def test_dims_2_3_has_blocks_of_two_three_and_one():
    c, fronts, dims, front_of, pairs, factors = _lists("dims_2_3")
    ns = {(f["nf"], f["n"]) for f in fronts[:-1]}
    assert {(2, 6), (2, 9), (2, 18), (3, 7), (3, 10), (3, 13)} == ns  # n = 6: a landmark seen once
    assert {dims[k] for k in c["ordering"]} == {2, 3}
    mixed = [v for v in pairs.values() if {2, 3} <= set(v)]
    assert mixed and any(set(v) == {2, 3} for v in factors.values())


def test_factor_counts_are_one_to_seventeen():
    c, fronts, dims, front_of, pairs, factors = _lists("factor_counts")
    assert [len(factors[C(k)]) for k in range(17)] == list(range(1, 18))  # 16 waves: empty ranges, one entry each, one wave with two
    assert sum(f["cls"] == 1 for f in fronts) == 1


def test_many_hbm_fronts_has_a_gather_only_root_among_five():
    c, fronts, dims, front_of, pairs, factors = _lists("many_hbm_fronts")
    hbm = [i for i, f in enumerate(fronts) if f["cls"] == 1]
    assert len(hbm) == 5  # more than four: no write mode even where the children are all gather leaves
    first = front_of[c["roots"][0][0]]
    children = [f for f in fronts if f["parent"] == first]
    assert len(children) == 3 and all(f["cls"] == 0 and f["level"] == 0 for f in children)
    assert sum(1 for i in hbm if not any(f["parent"] == i for f in fronts)) == 3  # three bare clusters
