"""ISAM2's marginals of many variables, cross-covariances and joint marginals (csrc/kernels_isam2_marginals.hpp: isam2_marginal_cross_kernel;
csrc/isam2_marginals.hpp) against the longdouble walk restatement (isam2_joint_restatement.py) and
isam2_walk_reference.marginal_covariance, both computed on the DEVICE's own tree, ISAM2.cliques(): elimination is not part of the
comparison and oracle/_ref is not read (the cases' natural_order).  The cases are those of isam2_walk_cases.py: dimensions 2, 3 and 6, paths
of 1 .. 349 cliques, LDS cliques either side of a 32-row block and of the wave width, the last LDS clique, a wide clique with its offsets
in the pool, 257 children, 65 trees.  test_isam2_joint_reference.py holds the restatement against the dense inverse on the oracle's trees.

Tolerance: max(16 x floor, 64 n eps) relative to the largest entry of the block, n the widest clique; floor = the float64 walk restatement
against the longdouble one.  Bitwise claims (a block's bits depend on its pair and the tree alone) are asserted on the uint64 views.

Measured on an MI355X (floor / device deviation; the tolerance is the smallest over the case's blocks):

  case            marginals (check 1)   cross, all ordered pairs (check 2)   tolerance
  lone            5.8e-17 / 5.8e-17     5.8e-17 / 5.8e-17                    4.2e-14
  pair[32,8]      1.9e-16 / 2.3e-16     3.5e-16 / 3.0e-16                    5.6e-13
  pair[33,8]      6.6e-16 / 2.6e-16     6.6e-16 / 5.3e-16                    5.8e-13
  pair[63,3]      2.2e-16 / 2.8e-16     3.5e-16 / 3.7e-16                    9.3e-13
  pair[64,75]     2.9e-16 / 3.9e-16     7.5e-16 / 5.7e-16                    2.0e-12
  pair[65,73]     1.8e-16 / 5.7e-16     4.1e-16 / 5.7e-16                    1.9e-12
  pair[128,8]     3.3e-16 / 5.9e-16     3.3e-16 / 6.2e-16                    1.9e-12
  pair[129,6]     1.9e-16 / 3.4e-16     5.3e-16 / 4.7e-16                    1.9e-12
  pair[3,135]     1.0e-15 / 3.0e-16     1.5e-15 / 1.1e-15                    1.9e-12
  wide_tree       3.9e-16 / 4.9e-16     1.2e-15 / 1.0e-15                    4.5e-12
  children[1]     1.7e-16 / 5.0e-17     1.7e-16 / 6.8e-17                    8.4e-14
  children[257]   1.3e-16 / 1.6e-16     2.4e-16 / 5.4e-16                    8.4e-14
  forest[1]       7.7e-17 / 1.9e-16     2.5e-16 / 2.5e-16                    8.4e-14
  forest[65]      1.6e-16 / 1.5e-16     1.6e-16 / 1.5e-16                    8.4e-14
  chain[350]      8.2e-16 / 2.0e-16     6.9e-15 / 9.5e-15                    8.4e-14
  pose3           9.9e-17 / 1.8e-16     5.4e-16 / 4.6e-16                    1.7e-13
  forest[65], pairs inside one tree (check 4): 1.7e-16 / 4.3e-16, tolerance 8.4e-14; across trees: exact zeros
  decay[40] (check 7): before the update 3.0e-15 / 6.3e-15, after it 4.7e-15 / 7.9e-15; a leaf marginalized 5.8e-15 / 6.4e-15; one more
  pose 2.1e-16 / 1.5e-16; that pose gone again 5.8e-15 / 6.4e-15; tolerance 8.4e-14
Everything else the module asserts is bitwise.
"""
import ctypes as ct

import numpy as np
import pytest

from gtsam_personal_amd import ISAM2, ISAM2GaussNewtonParams, ISAM2Params, NonlinearFactorGraph, Values, _lib, noiseModel
from gtsam_personal_amd._lib import LmgpuError

import isam2_joint_restatement as ij
import isam2_walk_cases as wc
import isam2_walk_reference as wr

pytestmark = pytest.mark.gpu

CASES = ["lone", "pair[32,8]", "pair[33,8]", "pair[63,3]", "pair[64,75]", "pair[65,73]", "pair[128,8]", "pair[129,6]", "pair[3,135]",
         "wide_tree", "children[1]", "children[257]", "forest[1]", "forest[65]", "chain[350]", "pose3"]
U64 = ct.POINTER(ct.c_uint64)
SENTINEL = 7.25


def make(threshold):
    return ISAM2(ISAM2Params(ISAM2GaussNewtonParams(threshold), 0.0, 0, False), ccolamd=wc.natural_order, device=0)


def built(name, upto=None):
    """a fresh solver after the case's updates, the case, the restatement's view of the device's tree"""
    c, isam = wc.case(name), make(0.0)
    for _ in wc.replay(c, isam, upto=upto):
        pass
    return isam, c, wr.Tree(isam.cliques(), wc.dims_of(c))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _u(keys):
    return np.asarray([int(k) for k in keys], dtype=np.uint64)


def raw_marginals(isam, keys, dims, out=None):
    """-> (status, blocks in request order); duplicates stay duplicates (the dict of ISAM2.marginalCovariances would fold them)"""
    d = [dims[int(k)] for k in keys]
    off = np.concatenate([[0], np.cumsum([x * x for x in d])]).astype(int)
    out = np.full(max(int(off[-1]), 1), SENTINEL) if out is None else out
    kk = _u(keys)
    rc = isam.lib.lmgpu_isam2_marginal_covariances(isam._h, len(kk), kk.ctypes.data_as(U64), out.ctypes.data_as(_lib._D))
    return rc, [out[off[q]:off[q + 1]].reshape(d[q], d[q]).copy() for q in range(len(d))]


def raw_cross(isam, pairs, dims, out=None):
    shape = [(dims[int(i)], dims[int(j)]) for i, j in pairs]
    off = np.concatenate([[0], np.cumsum([r * c for r, c in shape])]).astype(int)
    out = np.full(max(int(off[-1]), 1), SENTINEL) if out is None else out
    ki, kj = _u([i for i, _ in pairs]), _u([j for _, j in pairs])
    rc = isam.lib.lmgpu_isam2_cross_covariances(isam._h, len(pairs), ki.ctypes.data_as(U64), kj.ctypes.data_as(U64), out.ctypes.data_as(_lib._D))
    return rc, [out[off[q]:off[q + 1]].reshape(shape[q]).copy() for q in range(len(pairs))]


def raw_joint(isam, sets, dims, begin=None, out=None):
    begin = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32) if begin is None else np.asarray(begin, dtype=np.int32)
    D = [sum(dims[int(k)] for k in s) for s in sets]
    off = np.concatenate([[0], np.cumsum([x * x for x in D])]).astype(int)
    out = np.full(max(int(off[-1]), 1), SENTINEL) if out is None else out
    flat = _u([k for s in sets for k in s])
    rc = isam.lib.lmgpu_isam2_joint_marginal_covariances(isam._h, len(sets), begin.ctypes.data_as(_lib._I), flat.ctypes.data_as(U64),
                                                         out.ctypes.data_as(_lib._D))
    return rc, [out[off[q]:off[q + 1]].reshape(D[q], D[q]).copy() for q in range(len(sets))]


def all_pairs(keys):
    return [(i, j) for j in keys for i in keys]


def record(test, name, floor, dev, tol):
    print(f"measured {test} {name}: floor {floor:.1e} dev {dev:.1e} tol {tol:.1e}")


def held(got, ref, ref64, widest, what):
    """the recipe: -> (floor, deviation, tolerance), asserted"""
    floor = wr.deviation(ref64, ref)
    tol, dev = wr.tolerance(floor, widest), wr.deviation(got, ref)
    assert wr.FACTOR * floor <= wr.CAP, (what, floor)
    assert dev <= tol, (what, dev, tol)
    return floor, dev, tol


def check_cross_against_restatement(isam, tree, pairs, name, test):
    rc, blocks = raw_cross(isam, pairs, tree.dims)
    assert rc == _lib.LMGPU_OK
    worst = (0.0, 0.0, np.inf)
    for (i, j), got in zip(pairs, blocks):
        f, d, t = held(got, ij.cross_covariance(tree, i, j), ij.cross_covariance(tree, i, j, np.float64), tree.widest(), (i, j))
        worst = (max(worst[0], f), max(worst[1], d), min(worst[2], t))
    record(test, name, *worst)
    return blocks


# ------------------------------------------------------------------------------------------------ 1. marginals
@pytest.mark.parametrize("name", CASES)
def test_marginals(name):
    isam, c, tree = built(name)
    keys = list(c["marginals"]) + [c["marginals"][0]]  # one duplicate
    rc, blocks = raw_marginals(isam, keys, tree.dims)
    assert rc == _lib.LMGPU_OK
    rc, again = raw_marginals(isam, keys, tree.dims)
    assert rc == _lib.LMGPU_OK
    Rp = wr.global_R(tree)
    worst = (0.0, 0.0, np.inf)
    for q, (k, got) in enumerate(zip(keys, blocks)):
        ref = wr.marginal_covariance(tree, k, R_pos=Rp)
        f, d, t = held(got, ref, ij.cross_covariance(tree, k, k, np.float64), tree.widest(), k)
        worst = (max(worst[0], f), max(worst[1], d), min(worst[2], t))
        assert np.array_equal(got, got.T), k
        assert same_bits(got, again[q]), k
        rc, alone = raw_marginals(isam, [k], tree.dims)
        assert rc == _lib.LMGPU_OK and same_bits(got, alone[0]), k
        old = np.asarray(isam.marginalCovariance(k))  # the single-key entry keeps its own route: other sums, not bitwise
        assert wr.deviation(old, ref) <= t and wr.deviation(got, old) <= t, (k, wr.deviation(got, old), t)
    assert same_bits(blocks[0], blocks[-1])  # the duplicate
    record("marginals", name, *worst)
    isam.close()


# ------------------------------------------------------------------------------------------------ 2. cross, 3. joint
@pytest.mark.parametrize("name", CASES)
def test_cross_and_joint(name):
    isam, c, tree = built(name)
    keys = list(dict.fromkeys(c["marginals"]))  # (a clique of one variable lists it as its first and its last: a joint set takes a key once)
    pairs = all_pairs(keys)
    assert len(pairs) <= 36
    blocks = dict(zip(pairs, check_cross_against_restatement(isam, tree, pairs, name, "cross")))
    rc, marg = raw_marginals(isam, keys, tree.dims)
    assert rc == _lib.LMGPU_OK
    for k, m in zip(keys, marg):
        assert same_bits(blocks[(k, k)], m), k
    # reordered, the sources interleaved (sorted by target), a few pairs twice
    shuffled = sorted(pairs, reverse=True) + pairs[:3]
    rc, got = raw_cross(isam, shuffled, tree.dims)
    assert rc == _lib.LMGPU_OK
    for pr, g in zip(shuffled, got):
        assert same_bits(g, blocks[pr]), pr
    # one joint set of all marginal keys: symmetric to the bit, every block the cross block under the source rule
    rc, (M,) = raw_joint(isam, [keys], tree.dims)
    assert rc == _lib.LMGPU_OK and np.array_equal(M, M.T)
    off = np.concatenate([[0], np.cumsum([tree.dims[k] for k in keys])]).astype(int)
    for a, ka in enumerate(keys):
        for b, kb in enumerate(keys):
            src_a = a == b or ij.source_is_first(tree, ka, kb)
            want = blocks[(kb, ka)].T if src_a else blocks[(ka, kb)]
            assert same_bits(M[off[a]:off[a + 1], off[b]:off[b + 1]], want), (ka, kb)
    isam.close()


# ------------------------------------------------------------------------------------------------ 4. forest
def test_forest_pairs_across_and_inside_trees():
    isam, c, tree = built("forest[65]")
    first, last = c["marginals"]
    rc, (ab, ba) = raw_cross(isam, [(first, last), (last, first)], tree.dims)
    assert rc == _lib.LMGPU_OK and not ab.any() and not ba.any() and not np.signbit(ab).any()
    assert isam.marginals_junction(first, last) == (0, None) and ij.junction(tree, first, last) is None
    inside = [(1, 3), (3, 1), (2, 4), (4, 1)]  # the first tree: (1 | 2), (2 | 3), (3 4)
    check_cross_against_restatement(isam, tree, inside, "forest[65]", "forest")
    rc, (M,) = raw_joint(isam, [[1, last, 4]], tree.dims)
    assert rc == _lib.LMGPU_OK and np.array_equal(M, M.T) and not M[0:3, 3:6].any() and not M[3:6, 6:9].any() and M[0:3, 6:9].any()
    isam.close()


# ------------------------------------------------------------------------------------------------ 5. structure taps
@pytest.mark.parametrize("name", ["wide_tree", "children[257]", "pair[32,8]", "forest[65]", "pose3"])
def test_structure_taps(name):
    isam, c, tree = built(name)
    keys = list(c["marginals"]) + ([3] if name.startswith("forest") else [])
    for i in keys:
        assert isam.marginals_path(i) == ij.path(tree, i), i
        for j in keys:
            want = ij.junction(tree, i, j)
            assert isam.marginals_junction(i, j) == ((1, want) if want is not None else (0, None)), (i, j)
    if name == "wide_tree":
        tail0, z, mid0, mid1, root0, root1 = c["marginals"]
        assert isam.marginals_junction(tail0, mid1) == (1, mid0) == isam.marginals_junction(mid1, tail0)  # in the wide clique, i below j and j below i
        assert isam.marginals_junction(mid0, mid1) == (1, mid0)  # both frontal in one clique
        assert isam.marginals_junction(z, root1) == (1, root0) and len(isam.marginals_path(tail0)) == 33
    if name == "children[257]":
        p0, p1, x0 = c["marginals"]
        assert isam.marginals_junction(p0, p1) == (1, x0) and isam.marginals_path(p0) == [p0, x0]  # siblings under the root
    assert isam.marginals_path(10 ** 9) is None and isam.marginals_junction(keys[0], 10 ** 9) == (-1, None)
    isam.close()


# ------------------------------------------------------------------------------------------------ 6. placement and chunking
def test_lds_and_scratch_placement_give_the_same_bits():
    """lds_doubles = 512: the vectors of chain[350]'s long paths (3 columns x 1050 positions) go to scratch, pair[32,8]'s (43 positions)
    stay in LDS"""
    for name, in_scratch in (("chain[350]", True), ("pair[32,8]", False)):
        isam, c, tree = built(name)
        keys = list(c["marginals"])
        pairs = all_pairs(keys)
        _, m0 = raw_marginals(isam, keys, tree.dims)
        _, x0 = raw_cross(isam, pairs, tree.dims)
        s0 = isam.marginals_stats()
        assert s0["vars_scratch"] == 0 and s0["cross_scratch"] == 0 and s0["vars_lds"] == len(keys)
        isam.set_marginals_params(lds_doubles=512)
        rc, m1 = raw_marginals(isam, keys, tree.dims)
        assert rc == _lib.LMGPU_OK
        rc, x1 = raw_cross(isam, pairs, tree.dims)
        assert rc == _lib.LMGPU_OK
        s1 = isam.marginals_stats()
        assert s1["lds_capacity"] == 512
        assert (s1["vars_scratch"] > 0 and s1["cross_scratch"] > 0) == in_scratch
        if in_scratch:  # the root's own short path still fits the window: both placements in one launch
            assert s1["vars_lds"] > s0["vars_lds"] and s1["launches"] == s0["launches"] + 1
        assert all(same_bits(a, b) for a, b in zip(m0, m1)) and all(same_bits(a, b) for a, b in zip(x0, x1))
        isam.close()


def test_chunks_by_the_scratch_budget_and_a_budget_below_one_vector():
    isam, c, tree = built("chain[350]")
    keys = sorted(tree.keys)[:6]  # paths of 349 .. 344 cliques: 3325 .. 3277 doubles each, 26 600 bytes the longest
    _, m0 = raw_marginals(isam, keys, tree.dims)
    pairs = [(k, keys[0]) for k in keys] + [(keys[0], k) for k in keys]
    _, x0 = raw_cross(isam, pairs, tree.dims)
    isam.set_marginals_params(scratch_bytes=56000, lds_doubles=512)  # two vectors per chunk
    s0 = isam.marginals_stats()
    rc, m1 = raw_marginals(isam, keys, tree.dims)
    s1 = isam.marginals_stats()
    assert rc == _lib.LMGPU_OK and s1["chunks"] - s0["chunks"] == 3 == s1["launches"] - s0["launches"] and s1["vars_scratch"] - s0["vars_scratch"] == 6
    rc, x1 = raw_cross(isam, pairs, tree.dims)
    s2 = isam.marginals_stats()
    assert rc == _lib.LMGPU_OK and s2["cross_chunks"] - s1["cross_chunks"] >= 3
    assert all(same_bits(a, b) for a, b in zip(m0, m1)) and all(same_bits(a, b) for a, b in zip(x0, x1))
    # a budget below one vector: refused before anything is written, whatever else the request holds
    isam.set_marginals_params(scratch_bytes=1000)
    root = max(tree.keys)
    out = np.full(9 * 7, SENTINEL)
    rc, _ = raw_marginals(isam, [root] + keys, tree.dims, out=out)
    assert rc == _lib.LMGPU_INVALID and (out == SENTINEL).all() and b"scratch" in isam.lib.lmgpu_isam2_last_error(isam._h)
    rc, _ = raw_cross(isam, [(root, root)] + pairs, tree.dims, out=np.full(9 * 13, SENTINEL))
    assert rc == _lib.LMGPU_INVALID
    rc, (m,) = raw_marginals(isam, [root], tree.dims)  # (its vector fits LDS: the handle answers)
    assert rc == _lib.LMGPU_OK and np.isfinite(m).all()
    isam.close()


@pytest.mark.parametrize("name", ["chain[350]", "wide_tree", "pair[33,8]"])
def test_targets_per_workgroup_gives_the_same_bits(name):
    isam, c, tree = built(name)
    pairs = all_pairs(list(c["marginals"]))
    _, x0 = raw_cross(isam, pairs, tree.dims)
    walks = []
    for cap in (1, 2, 16):
        isam.set_marginals_params(targets_per_workgroup=cap)
        before = isam.marginals_stats()
        rc, x1 = raw_cross(isam, pairs, tree.dims)
        after = isam.marginals_stats()
        assert rc == _lib.LMGPU_OK and after["cross_cap"] == cap and after["cross_launches"] == before["cross_launches"] + 1
        assert after["cross_targets"] - before["cross_targets"] == len(pairs)
        walks.append(after["cross_walks"] - before["cross_walks"])
        assert all(same_bits(a, b) for a, b in zip(x0, x1)), cap
    n = len(c["marginals"])
    assert walks == [n * n, n * ((n + 1) // 2), n]  # pairs with one source share its walk, `cap` of them per workgroup
    isam.close()


# ------------------------------------------------------------------------------------------------ 7. the tree moves
def test_answers_follow_the_tree_through_an_update():
    """decay[40]: a request, the update that re-eliminates the top (a prior on the last pose), the request again -- the second answers are
    those of the NEW tree (position tables kept from the first request would give the old ones)"""
    isam, c, tree0 = built("decay[40]", upto=1)
    keys = list(c["marginals"])
    pairs = all_pairs(keys)
    before = check_cross_against_restatement(isam, tree0, pairs, "decay[40] update 0", "moves")
    g, v, _ = c["updates"][1]
    isam.update(g, v)
    tree1 = wr.Tree(isam.cliques(), wc.dims_of(c))
    after = check_cross_against_restatement(isam, tree1, pairs, "decay[40] update 1", "moves")
    moved = pairs.index((keys[-1], keys[-1]))  # the pose the new prior sits on (what lies beyond the tight anchor barely feels it)
    assert wr.deviation(after[moved], before[moved]) > 0.1
    rc, marg = raw_marginals(isam, keys, tree1.dims)
    assert rc == _lib.LMGPU_OK and all(same_bits(m, after[pairs.index((k, k))]) for k, m in zip(keys, marg))
    isam.close()


def test_gone_keys_are_refused_and_the_live_ones_still_match():
    isam, c, tree = built("decay[40]")
    dims = dict(tree.dims)
    first, last = min(tree.keys), max(tree.keys)
    # ---- a marginalized leaf (the chain's first pose); its neighbour becomes a fixed variable and stays in the tree
    isam.marginalizeLeaves([first])
    assert isam.getFixedVariables() == [first + 1]
    del dims[first]
    tree = wr.Tree(isam.cliques(), dims)
    for call in (lambda o: raw_marginals(isam, [last, first], tree.dims | {first: 3}, out=o),
                 lambda o: raw_cross(isam, [(last, last), (first, last)], tree.dims | {first: 3}, out=o),
                 lambda o: raw_cross(isam, [(last, last), (last, first)], tree.dims | {first: 3}, out=o),
                 lambda o: raw_joint(isam, [[last, first]], tree.dims | {first: 3}, out=o)):
        out = np.full(36, SENTINEL)
        rc, _ = call(out)
        assert rc == _lib.LMGPU_INVALID and (out == SENTINEL).all() and b"not a variable of the Bayes tree" in isam.lib.lmgpu_isam2_last_error(isam._h)
    assert isam.marginals_path(first) is None
    live = [first + 1, c["marginals"][1], last]
    check_cross_against_restatement(isam, tree, all_pairs(live), "decay[40] marginalized", "gone")
    # ---- a variable that leaves with its last factor
    new = last + 1
    g, v = NonlinearFactorGraph(), Values()
    v.insert_pose2(new, 0.5, 0.5, 0.1)
    g.add_BetweenFactorPose2(last, new, [1.0, 0.0, 0.0], noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    isam.update(g, v)
    dims[new] = 3
    tree = wr.Tree(isam.cliques(), dims)
    check_cross_against_restatement(isam, tree, all_pairs([new, last]), "decay[40] one more pose", "gone")
    isam.update(removeFactorIndices=[isam.num_factors() - 1])
    assert isam.unusedKeys() == [new]
    out = np.full(9, SENTINEL)
    rc, _ = raw_marginals(isam, [new], {new: 3}, out=out)
    assert rc == _lib.LMGPU_INVALID and (out == SENTINEL).all()
    with pytest.raises(LmgpuError, match="not a variable of the Bayes tree"):
        isam.marginalCovariances([last, new])
    del dims[new]
    tree = wr.Tree(isam.cliques(), dims)
    check_cross_against_restatement(isam, tree, all_pairs(live), "decay[40] the pose gone again", "gone")
    isam.close()


# ------------------------------------------------------------------------------------------------ 8. launch count
def test_one_launch_per_call_that_fits_one_chunk():
    isam, c, tree = built("wide_tree")
    keys = list(c["marginals"])
    s = [isam.marginals_stats()]
    raw_marginals(isam, keys, tree.dims)
    s.append(isam.marginals_stats())
    raw_cross(isam, all_pairs(keys), tree.dims)
    s.append(isam.marginals_stats())
    raw_joint(isam, [keys, keys[:2]], tree.dims)
    s.append(isam.marginals_stats())
    assert [x["launches"] for x in s] == [0, 1, 1, 1] and [x["chunks"] for x in s] == [0, 1, 1, 1]
    assert [x["cross_launches"] for x in s] == [0, 0, 1, 2] and [x["cross_chunks"] for x in s] == [0, 0, 1, 2]
    assert s[-1]["factorizations"] == 0 and s[1]["vars_lds"] == len(keys) and s[1]["longest_path"] == 33
    assert s[2]["cross_targets"] == 36 and s[3]["cross_targets"] == 36 + 21 + 3  # a joint computes every block once
    isam.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_write_nothing_and_leave_the_handle_usable():
    isam, c, tree = built("pose3")
    keys = list(c["marginals"])
    lib, h = isam.lib, isam._h
    out = np.full(36 * 9, SENTINEL)
    D, K = out.ctypes.data_as(_lib._D), _u(keys).ctypes.data_as(U64)
    msg = lambda: lib.lmgpu_isam2_last_error(h)
    rc, _ = raw_joint(isam, [[keys[0], keys[1], keys[0]]], tree.dims, out=out)
    assert rc == _lib.LMGPU_INVALID and b"twice" in msg()
    rc, _ = raw_joint(isam, [keys[:2], keys[2:]], tree.dims, begin=[0, 2, 1], out=out)
    assert rc == _lib.LMGPU_INVALID and b"decreases" in msg()
    rc, _ = raw_joint(isam, [keys[:2]], tree.dims, begin=[-1, 1], out=out)
    assert rc == _lib.LMGPU_INVALID
    assert lib.lmgpu_isam2_marginal_covariances(h, 3, K, None) == _lib.LMGPU_INVALID
    assert lib.lmgpu_isam2_marginal_covariances(h, 3, None, D) == _lib.LMGPU_INVALID
    assert lib.lmgpu_isam2_marginal_covariances(h, -1, K, D) == _lib.LMGPU_INVALID and b"n < 0" in msg()
    assert lib.lmgpu_isam2_cross_covariances(h, 3, K, K, None) == _lib.LMGPU_INVALID
    assert lib.lmgpu_isam2_cross_covariances(h, 3, K, None, D) == _lib.LMGPU_INVALID
    assert lib.lmgpu_isam2_cross_covariances(h, -3, K, K, D) == _lib.LMGPU_INVALID
    begin = np.array([0, 3], dtype=np.int32).ctypes.data_as(_lib._I)
    assert lib.lmgpu_isam2_joint_marginal_covariances(h, 1, begin, K, None) == _lib.LMGPU_INVALID
    assert lib.lmgpu_isam2_joint_marginal_covariances(h, 1, None, K, D) == _lib.LMGPU_INVALID
    assert lib.lmgpu_isam2_joint_marginal_covariances(h, -1, begin, K, D) == _lib.LMGPU_INVALID
    rc, _ = raw_marginals(isam, [keys[0], 99], tree.dims | {99: 6}, out=out)  # a key never added
    assert rc == _lib.LMGPU_INVALID and b"key 99" in msg()
    assert (out == SENTINEL).all()
    st = isam.marginals_stats()
    assert st["launches"] == 0 and st["cross_launches"] == 0
    assert lib.lmgpu_isam2_marginal_covariances(h, 0, None, None) == _lib.LMGPU_OK
    check_cross_against_restatement(isam, tree, all_pairs(keys), "pose3 after the refusals", "refusals")
    isam.close()


# ------------------------------------------------------------------------------------------------ 10. the Python mirror
def test_python_api_shapes():
    isam, c, tree = built("pair[32,8]")  # (poses and landmarks: blocks of 3 and of 2)
    keys = list(c["marginals"])
    every = isam.marginalCovariances()
    assert sorted(every) == tree.keys and all(every[k].shape == (tree.dims[k], tree.dims[k]) for k in tree.keys)
    assert {2, 3} == {m.shape[0] for m in every.values()}
    some = isam.marginalCovariances(keys + keys[:1])
    assert list(some) == keys and all(same_bits(some[k], every[k]) for k in keys)
    pairs = all_pairs(keys[:3])
    cross = isam.crossCovariances(pairs)
    assert list(cross) == pairs and all(cross[(i, j)].shape == (tree.dims[i], tree.dims[j]) for i, j in pairs)
    assert all(same_bits(cross[(k, k)], every[k]) for k in keys[:3])
    joints = isam.jointMarginalCovariances([keys, keys[1::-1]])
    assert [j.keys for j in joints] == [sorted(keys), sorted(keys[:2])]
    D = sum(tree.dims[k] for k in keys)
    assert joints[0].fullMatrix().shape == (D, D) and np.array_equal(joints[0].fullMatrix(), joints[0].fullMatrix().T)
    one = isam.jointMarginalCovariance(keys[:2])
    assert same_bits(one.fullMatrix(), joints[1].fullMatrix())
    a, b = sorted(keys[:2])
    assert same_bits(one.at(a, b), cross[(a, b)] if ij.source_is_first(tree, b, a) else cross[(b, a)].T)
    assert same_bits(np.asarray(one.at(a, a)), every[a])
    assert isam.marginalCovariance(keys[0]).shape == every[keys[0]].shape  # unchanged entry
    st = isam.marginals_stats()
    assert st["launches"] == 2 and st["cross_launches"] == 3 and st["factorizations"] == 0
    with pytest.raises(LmgpuError):
        isam.crossCovariances([(keys[0], 10 ** 6)])
    isam.close()
