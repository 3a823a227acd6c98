"""Cross-covariances and joint marginals without a device: the long-double restatement of the cross walk
(tests/joint_marginals_restatement.py) against the dense inverse on Bayes trees built in numpy, the order rule of a source's targets,
and the junction tap and the refusals of the new calls on structure-only (device = -1) handles of tests/marginals_path_cases.py."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import joint_marginals_restatement as jr
import marginals_path_cases as cases
import marginals_path_restatement as mr
from gtsam_personal_amd import LevenbergMarquardtOptimizer, LevenbergMarquardtParams, _lib
from test_marginals_path_reference import TREES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, tree = [(frontal slots, parent, separator slots)] children first, dims per slot)
MORE_TREES = [
    # two sibling leaves of different frontal size under one parent: from the short leaf the branch to the other is longer than the
    # source's own path, from the long one shorter
    ("siblings_unequal", [([0], 2, [2]), ([1, 3], 2, [2]), ([2], 3, [4]), ([4], -1, [])], [2, 6, 3, 9, 3]),
    # the junction of the two subtrees is the root
    ("junction_root", [([0], 1, [1]), ([1], 4, [4]), ([2], 3, [3]), ([3], 4, [4, 5]), ([4, 5], -1, [])], [3, 2, 6, 3, 3, 1]),
    # i's front an ancestor of j's and the reverse (all ordered pairs are run), with separators that skip a level
    ("ancestors", [([0], 1, [1, 3]), ([1], 2, [2, 3]), ([2], 3, [3]), ([3], -1, [])], [3, 6, 2, 9]),
    ("forest_deep", [([0], 1, [1]), ([1], 2, [2]), ([2], -1, []), ([3], 5, [5]), ([4], 5, [5]), ([5, 6], -1, [])], [3, 3, 2, 6, 1, 3, 2]),
    # three levels of branching: junctions at three depths from one source
    ("comb", [([0], 1, [1]), ([1], 3, [3]), ([2], 3, [3]), ([3], 5, [5]), ([4], 5, [5]), ([5], 7, [7]), ([6], 7, [7]), ([7], -1, [])],
     [3, 2, 6, 3, 5, 3, 9, 2]),
]
ALL_TREES = list(TREES) + MORE_TREES


def _rel(got, want, sii, sjj):
    return float(np.linalg.norm((got - want).astype(np.float64)) /
                 np.sqrt(np.linalg.norm(sii.astype(np.float64)) * np.linalg.norm(sjj.astype(np.float64))))


@pytest.mark.parametrize("name,tree,dims", ALL_TREES, ids=[t[0] for t in ALL_TREES])
def test_cross_restatement_equals_dense_inverse(name, tree, dims):
    """every ordered pair (i, j) of every tree, j the source, at the bound test_marginals_path_reference.py holds path_marginal to"""
    cliques, info, off = mr.random_bayes_tree(tree, dims, seed=len(name))
    sigma = mr.inverse_ld(info)
    blk = lambda a, b: sigma[off[a]:off[a + 1], off[b]:off[b + 1]]
    for j in range(len(dims)):
        for i in range(len(dims)):
            got = jr.cross_covariance(cliques, dims, i, j)
            assert got.shape == (dims[i], dims[j])
            rel = _rel(got, blk(i, j), blk(i, i), blk(j, j))
            assert rel <= 1e-12, (name, i, j, rel)
            if jr.junction(cliques, i, j) is None:
                assert (got == 0).all() and np.abs(blk(i, j).astype(np.float64)).max() <= 1e-15 * float(np.abs(sigma).max())


@pytest.mark.parametrize("name,tree,dims", ALL_TREES, ids=[t[0] for t in ALL_TREES])
def test_all_targets_of_a_source_in_one_walk(name, tree, dims):
    """one walk of the source, every variable a target, deepest junction first: the same blocks as one walk per pair, to the bit (the
    descent of a branch reads the shared part and zeros only)"""
    cliques, _, _ = mr.random_bayes_tree(tree, dims, seed=len(name))
    for j in range(len(dims)):
        targets = jr.order_targets(cliques, dims, j, list(range(len(dims))))
        for t, got in zip(targets, jr.cross_blocks(cliques, dims, j, targets)):
            assert np.array_equal(got, jr.cross_covariance(cliques, dims, t, j)), (name, t, j)


def test_block_of_a_variable_with_itself_is_the_path_marginal():
    """(i, i) with i its own source is the path walk's block, symmetrised alike (the two restatements sum in different orders: a few
    long-double roundings apart)"""
    for name, tree, dims in ALL_TREES:
        cliques, _, _ = mr.random_bayes_tree(tree, dims, seed=3)
        for s in range(len(dims)):
            got, want = jr.cross_covariance(cliques, dims, s, s), mr.path_marginal(cliques, dims, s)
            assert np.array_equal(got, got.T)
            assert float(np.abs(got - want).max()) <= 1e-16 * float(np.abs(want).max()), (name, s)


def _comb():
    name, tree, dims = MORE_TREES[-1]
    return mr.random_bayes_tree(tree, dims, seed=11) + (dims,)


def test_targets_in_ascending_junction_depth_fail_the_order_assert():
    """source 0 (the deepest leaf of the comb); target 6 meets it at the root, target 4 one level down, target 2 two levels down.  Root
    junction first: the descent to 6 zeroes everything below the root, which the junctions of 4 and 2 lie in."""
    cliques, _, _, dims = _comb()
    with pytest.raises(AssertionError, match="targets out of order"):
        jr.cross_blocks(cliques, dims, 0, [6, 4, 2])


def test_targets_deepest_junction_first_pass():
    cliques, info, off, dims = _comb()
    sigma = mr.inverse_ld(info)
    order = jr.order_targets(cliques, dims, 0, [6, 4, 2])
    assert order == [2, 4, 6]
    for t, got in zip(order, jr.cross_blocks(cliques, dims, 0, order)):
        want = sigma[off[t]:off[t + 1], off[0]:off[1]]
        assert _rel(got, want, sigma[off[t]:off[t + 1], off[t]:off[t + 1]], sigma[off[0]:off[1], off[0]:off[1]]) <= 1e-12, t


def test_joint_restatement_is_symmetric_and_equals_dense_inverse():
    for name, tree, dims in ALL_TREES:
        cliques, info, off = mr.random_bayes_tree(tree, dims, seed=5)
        sigma = mr.inverse_ld(info)
        slots = list(range(len(dims)))[::-1]
        M = jr.joint_marginal(cliques, dims, slots)
        assert np.array_equal(M, M.T)
        idx = np.concatenate([np.arange(off[s], off[s + 1]) for s in slots])
        want = sigma[np.ix_(idx, idx)]
        assert float(np.abs((M - want).astype(np.float64)).max()) <= 1e-12 * float(np.abs(want.astype(np.float64)).max()), name


# ---------------------------------------------------------------- structure-only handles
def _structure_handle(builder, **kw):
    graph, values, ordering = builder()
    return LevenbergMarquardtOptimizer(graph, values, ordering, LevenbergMarquardtParams(), device=-1, **kw), ordering


def _path(opt, slot):
    buf = np.zeros(4096, dtype=np.int32)
    n = opt.lib.lmgpu_marginals_path(opt._h, slot, buf.ctypes.data_as(ct.POINTER(ct.c_int32)), len(buf))
    assert 0 < n <= len(buf)
    return buf[:n].tolist()


@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_junction_is_the_deepest_common_front_of_the_two_paths(name):
    opt, ordering = _structure_handle(cases.SMALL[name])
    n = len(ordering)
    paths = [_path(opt, s) for s in range(n)]
    across = 0
    for a in range(n):
        for b in range(n):
            on_b = set(paths[b])
            want = next((f for f in paths[a] if f in on_b), -1)
            assert opt.lib.lmgpu_marginals_junction(opt._h, a, b) == want, (name, a, b)
            across += want < 0
    assert (across > 0) == (name == "forest")
    for a, b in ((-1, 0), (0, -1), (n, 0), (0, n)):
        assert opt.lib.lmgpu_marginals_junction(opt._h, a, b) == -1
    opt.close()


def _ip(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_int32))


def _dp(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


def _cross(opt, out):
    one = np.zeros(1, dtype=np.int32)
    return opt.lib.lmgpu_marginal_cross_covariances(opt._h, 1, _ip(one), _ip(one), _dp(out))


def _joint(opt, out, slots=(0, 1)):
    sl = np.array(slots, dtype=np.int32)
    begin = np.array([0, len(sl)], dtype=np.int32)
    return opt.lib.lmgpu_joint_marginal_covariances(opt._h, 1, _ip(begin), _ip(sl), _dp(out))


def test_structural_refusals_come_first_on_structure_handles():
    """a handle finalized under PCG and a two-rank handle refuse the new calls with marg_refused's messages before anything else is
    looked at -- even an out-of-range slot -- and nothing is written; the junction tap of a PCG structure (no fronts) answers -1"""
    from gtsam_personal_amd import BlockJacobiPreconditionerParameters, PCGSolverParameters
    g, v, o = cases.SMALL["chain"]()
    pcg = LevenbergMarquardtParams()
    pcg.linearSolverType, pcg.iterativeParams = "ITERATIVE", PCGSolverParameters(BlockJacobiPreconditionerParameters())
    for opt, msg in ((LevenbergMarquardtOptimizer(g, v, o, pcg, device=-1), b"finalized under PCG"),
                     (LevenbergMarquardtOptimizer(g, v, o, LevenbergMarquardtParams(), device=-1, world_size=2), b"one GPU")):
        out = np.full(36, 7.0)
        assert _cross(opt, out) == _lib.LMGPU_INVALID and msg in opt.lib.lmgpu_last_error(opt._h) and (out == 7.0).all()
        assert _joint(opt, out) == _lib.LMGPU_INVALID and msg in opt.lib.lmgpu_last_error(opt._h) and (out == 7.0).all()
        assert _joint(opt, out, (0, 99)) == _lib.LMGPU_INVALID and msg in opt.lib.lmgpu_last_error(opt._h)
        if msg.startswith(b"finalized"):
            assert opt.lib.lmgpu_marginals_junction(opt._h, 0, 1) == -1
        opt.close()


def test_structure_handle_checks_arguments_then_refuses_compute():
    """on a device = -1 handle: an out-of-range slot and a slot twice in a set are LMGPU_INVALID with their message, an empty request is
    LMGPU_OK, a well-formed one is refused for want of a device; nothing is written, no cross counter moves, the cap switch is kept"""
    opt, ordering = _structure_handle(cases.SMALL["chain"])
    n = len(ordering)
    out = np.full(36, 7.0)
    bad = np.array([n], dtype=np.int32)
    ok = np.zeros(1, dtype=np.int32)
    assert opt.lib.lmgpu_marginal_cross_covariances(opt._h, 1, _ip(bad), _ip(ok), _dp(out)) == _lib.LMGPU_INVALID
    assert b"out of range" in opt.lib.lmgpu_last_error(opt._h)
    assert opt.lib.lmgpu_marginal_cross_covariances(opt._h, 1, _ip(ok), _ip(bad), _dp(out)) == _lib.LMGPU_INVALID
    assert _joint(opt, out, (0, n)) == _lib.LMGPU_INVALID and b"out of range" in opt.lib.lmgpu_last_error(opt._h)
    assert _joint(opt, out, (1, 0, 1)) == _lib.LMGPU_INVALID and b"twice" in opt.lib.lmgpu_last_error(opt._h)
    assert opt.lib.lmgpu_marginal_cross_covariances(opt._h, 0, None, None, None) == _lib.LMGPU_OK
    assert opt.lib.lmgpu_joint_marginal_covariances(opt._h, 0, None, None, None) == _lib.LMGPU_OK
    assert opt.lib.lmgpu_marginal_cross_covariances(opt._h, -1, None, None, None) == _lib.LMGPU_INVALID
    assert _cross(opt, out) != _lib.LMGPU_OK
    assert _joint(opt, out) != _lib.LMGPU_OK
    assert (out == 7.0).all()
    assert opt.lib.lmgpu_set_marginals_cross_cap(opt._h, -1) == _lib.LMGPU_INVALID
    assert opt.lib.lmgpu_set_marginals_cross_cap(opt._h, 3) == _lib.LMGPU_OK
    st = _lib.lmgpu_marginals_stats()
    assert opt.lib.lmgpu_get_marginals_stats(opt._h, ct.byref(st)) == _lib.LMGPU_OK
    assert (st.cross_launches, st.cross_chunks, st.cross_walks, st.cross_targets, st.cross_lds, st.cross_scratch, st.longest_union) == (0,) * 7
    assert st.cross_cap == 3
    assert opt.lib.lmgpu_set_marginals_cross_cap(opt._h, 0) == _lib.LMGPU_OK
    assert opt.lib.lmgpu_get_marginals_stats(opt._h, ct.byref(st)) == _lib.LMGPU_OK and st.cross_cap > 3
    opt.close()


NEW_SYMBOLS = ("lmgpu_marginal_cross_covariances", "lmgpu_joint_marginal_covariances", "lmgpu_marginals_junction", "lmgpu_set_marginals_cross_cap")


def test_new_symbols_are_declared():
    """in the header, in the ctypes table and in the integration guide; the library exports them; the old joint entry point stays"""
    header = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
        assert name in guide, name
        assert getattr(lib, name) is not None
    m = re.search(r"typedef struct lmgpu_marginals_stats \{(.*?)\} lmgpu_marginals_stats;", header, re.S)
    fields = [f.strip() for part in m.group(1).split(";") for f in re.sub(r"\b(int64_t|int32_t)\b", "", part).split(",") if f.strip()]
    assert fields == [f for f, _ in _lib.lmgpu_marginals_stats._fields_]
    assert {"cross_launches", "cross_walks", "cross_targets", "longest_union", "cross_cap"} <= set(fields)
    assert "lmgpu_marginal_covariance" in _lib.SYMBOLS and "lmgpu_joint_marginal_covariance" in _lib.SYMBOLS
