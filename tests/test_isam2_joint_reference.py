"""ISAM2's many-marginals / cross-covariance / joint-marginal route without a device.

  * the walk restatement (isam2_joint_restatement.py) on the CPU oracle's trees of the walk cases (isam2_walk_cases.py, the cases' own
    ordering: no oracle/_ref) against the blocks of the inverse of R^T R assembled by isam2_walk_reference.global_R: deviation <=
    tolerance(floor, widest) = max(16 x floor, 64 n eps), the floor being the float64 dense inverse against the longdouble one;
    cross(i, i) against wr.marginal_covariance; joints exactly symmetric; exact zeros and no junction across two trees
  * the pin to the reference, tests/testGaussianISAM2.cpp:977-986 extended to pairs: on the slam-like sequence the blocks from the
    ISAM2 tree equal the batch restatement (joint_marginals_restatement.py, itself pinned to testMarginals.cpp) on the same factors at the
    linearization point, within assert_equal's default 1e-9 absolute
  * the new symbols: declared in lmgpu.h, exported, in _lib.SYMBOLS; the frozen enum counts; the refusals and the
    structure taps of a handle without a device
test_gpu_isam2_marginals.py holds the device to the same restatement on the device's own tree."""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest

import isam2_joint_restatement as ij
import isam2_walk_cases as wc
import isam2_walk_reference as wr
import joint_marginals_restatement as jr
import oracle_harness as oh
from gtsam_personal_amd import Ordering, _lib
from gtsam_personal_amd import graph as G
from gtsam_personal_amd.graph import VAR_DIM
from isam2_examples import slamlike_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble

CASES = ["lone", "pair[32,8]", "pair[33,8]", "pair[63,3]", "pair[64,75]", "pair[65,73]", "pair[128,8]", "pair[129,6]", "pair[3,135]",
         "wide_tree", "children[1]", "children[257]", "forest[1]", "forest[65]", "chain[350]", "pose3"]


@functools.lru_cache(maxsize=None)
def oracle_tree(name):
    c, orc = wc.case(name), oh.OracleISAM2(0.0, 0, False, 0.0, ccolamd=wc.natural_order)
    for _ in wc.replay(c, orc):
        pass
    return wr.Tree(orc.cliques(), wc.dims_of(c))


def request_keys(name, tree):
    """the case's marginal keys; in the forest also a second key of the first tree (a pair inside one tree) -- read-only"""
    keys = list(wc.case(name)["marginals"])
    if name.startswith("forest"):
        keys.insert(1, 3)
    return [int(k) for k in keys]


def dense_columns(tree, R_pos, key, dtype):
    """Sigma[:, key] in the positions of R, by two triangular solves with the assembled global R (all columns of the key at once)"""
    R, pos = R_pos
    n, d, o = tree.n, tree.dims[key], tree.off[key]
    Y = np.zeros((n, d), dtype=dtype)
    Y[pos[o:o + d], np.arange(d)] = 1
    for i in range(n):
        Y[i] = (Y[i] - R[:i, i] @ Y[:i]) / R[i, i]
    X = np.zeros((n, d), dtype=dtype)
    for i in range(n - 1, -1, -1):
        X[i] = (Y[i] - R[i, i + 1:] @ X[i + 1:]) / R[i, i]
    return X


@pytest.mark.parametrize("name", CASES)
def test_walk_restatement_equals_the_inverse_of_the_assembled_R(name):
    tree = oracle_tree(name)
    keys = request_keys(name, tree)
    Rp, Rp64 = wr.global_R(tree), wr.global_R(tree, np.float64)
    inv64 = np.linalg.inv(Rp64[0].T @ Rp64[0])
    at = lambda k: Rp[1][tree.off[k]:tree.off[k] + tree.dims[k]]
    worst = dict(floor=0.0, dev=0.0, dev64=0.0)
    for j in keys:
        cols = dense_columns(tree, Rp, j, LD)
        for i in keys:
            ref = cols[at(i)]
            floor = wr.deviation(inv64[np.ix_(at(i), at(j))], ref)
            tol = wr.tolerance(floor, tree.widest())
            assert wr.FACTOR * floor <= wr.CAP, (i, j, floor)
            got, got64 = ij.cross_covariance(tree, i, j), ij.cross_covariance(tree, i, j, np.float64)
            assert got.shape == (tree.dims[i], tree.dims[j]) and got.dtype == LD and got64.dtype == np.float64
            if i == j:  # symmetrised alike on both sides
                ref = 0.5 * (ref + ref.T)
                assert np.array_equal(got, got.T)
                assert wr.deviation(got, wr.marginal_covariance(tree, i, R_pos=Rp)) <= tol, i
            dev, dev64 = wr.deviation(got, ref), wr.deviation(got64, ref)
            assert dev <= tol and dev64 <= tol, (i, j, dev, dev64, tol)
            if ij.junction(tree, i, j) is None:
                assert not got.any() and not got64.any() and not np.asarray(ref, dtype=np.float64).any(), (i, j)
            worst = dict(floor=max(worst["floor"], floor), dev=max(worst["dev"], dev), dev64=max(worst["dev64"], dev64))
    print(f"measured restatement {name}: floor {worst['floor']:.1e} walk {worst['dev']:.1e} float64 walk {worst['dev64']:.1e}")


@pytest.mark.parametrize("name", CASES)
def test_joint_restatement_is_symmetric_and_made_of_the_source_rule_blocks(name):
    tree = oracle_tree(name)
    keys = sorted(request_keys(name, tree))
    for dtype in (LD, np.float64):
        M = ij.joint_covariance(tree, keys, dtype)
        assert np.array_equal(M, M.T)
        off = np.concatenate([[0], np.cumsum([tree.dims[k] for k in keys])]).astype(int)
        for a, ka in enumerate(keys):
            for b, kb in enumerate(keys):
                src_a = a == b or ij.source_is_first(tree, ka, kb)
                want = ij.cross_covariance(tree, kb, ka, dtype).T if src_a else ij.cross_covariance(tree, ka, kb, dtype)
                assert np.array_equal(M[off[a]:off[a + 1], off[b]:off[b + 1]], want), (ka, kb)


def test_two_trees_of_a_forest():
    tree = oracle_tree("forest[65]")
    last = wc.case("forest[65]")["marginals"][-1]
    assert ij.junction(tree, 1, last) is None and ij.junction(tree, last, 1) is None
    assert not ij.cross_covariance(tree, 1, last).any() and not ij.cross_covariance(tree, last, 1, np.float64).any()
    assert ij.junction(tree, 1, 3) == 3 and ij.junction(tree, 1, 2) == 2  # inside the first tree: (1 | 2), (2 | 3), (3 4)
    assert ij.path(tree, 1) == [1, 2, 3] and ij.path(tree, 4) == [3]
    assert ij.cross_covariance(tree, 1, 3).any()


def test_paths_and_junctions_follow_the_cases_construction():
    """i an ancestor of j, j an ancestor of i, both frontal in one clique, siblings under the root, the junction in a wide clique"""
    tree, c = oracle_tree("wide_tree"), wc.case("wide_tree")
    tail0, z, mid0, mid1, root0, root1 = c["marginals"]
    assert ij.path(tree, tail0)[-3:] == [z, mid0, root0] and len(ij.path(tree, tail0)) == 33
    assert ij.junction(tree, tail0, mid1) == mid0 == ij.junction(tree, mid1, tail0)  # in the wide clique (65, 258), either way round
    assert ij.junction(tree, mid0, mid1) == mid0 and ij.junction(tree, root0, root1) == root0  # both frontal in one clique
    assert ij.junction(tree, z, root1) == root0
    tree, c = oracle_tree("children[257]"), wc.case("children[257]")
    p0, p1, x0 = c["marginals"]
    assert ij.path(tree, p0) == [p0, x0] and ij.junction(tree, p0, p1) == x0  # siblings under the root
    assert ij.path_scalars(tree, p0) == 8 and ij.path_scalars(tree, x0) == 6
    assert ij.source_is_first(tree, x0, p0) and not ij.source_is_first(tree, p0, x0) and ij.source_is_first(tree, p0, p1)  # (a tie: the smaller key)


# ------------------------------------------------------------------------------------------------ the pin to the reference
def _merge(steps):
    graph, init = G.NonlinearFactorGraph(), G.Values()
    for g, v in steps:
        graph.push_back(g)
        for k in v.keys():
            init.insert(k, v.type(k), v.at(k))
    return graph, init


def test_slamlike_blocks_equal_the_batch_restatement_at_the_linearization_point():
    """TEST(ISAM2, marginalCovariance), tests/testGaussianISAM2.cpp:977-986, extended to pairs: Marginals(isam.getFactorsUnsafe(),
    isam.getLinearizationPoint()) is the batch elimination of the same factors, read by the batch restatement"""
    steps = slamlike_steps()
    isam = oh.OracleISAM2(0.0, 0, False, 0.001, ccolamd=wc.natural_order)  # createSlamlikeISAM2's parameters
    for g, v in steps:
        isam.update(g, v)
    lin = isam.getLinearizationPoint()
    dims = {int(k): VAR_DIM[lin.type(k)] for k in lin.keys()}
    tree = wr.Tree(isam.cliques(), dims)
    fullgraph, _ = _merge(steps)
    batch = oh.OracleProblem(fullgraph, lin, Ordering.Natural(fullgraph))
    batch.linearize()
    assert batch.solve(0.0)[0] == 0
    bcliques = [(keys, nfk, parent, rsd) for keys, nfk, rsd, parent in batch.cliques()]
    keys = (5, 0, 11, 100, 101)
    for j in keys:
        for i in keys:
            expected = jr.cross_covariance(bcliques, dims, i, j)
            actual = ij.cross_covariance(tree, i, j)
            assert actual.shape == expected.shape and float(np.max(np.abs(actual - expected))) <= 1e-9, (i, j)
    expected = jr.joint_marginal(bcliques, dims, sorted(keys))
    assert float(np.max(np.abs(ij.joint_covariance(tree, sorted(keys)) - expected))) <= 1e-9


# ------------------------------------------------------------------------------------------------ the C ABI without a device
NEW_SYMBOLS = ("lmgpu_isam2_marginal_covariances", "lmgpu_isam2_cross_covariances", "lmgpu_isam2_joint_marginal_covariances",
               "lmgpu_isam2_marginals_path", "lmgpu_isam2_marginals_junction", "lmgpu_isam2_set_marginals_params",
               "lmgpu_isam2_get_marginals_stats")


def test_new_symbols_are_declared():
    """in the header, in the ctypes table and in the integration guide; the library exports them; the single-key entry stays"""
    header = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
        assert name in guide, name
        assert getattr(lib, name) is not None
    assert "lmgpu_isam2_marginal_covariance" in _lib.SYMBOLS and "linearization point" in header.lower()


def test_frozen_enum_counts():
    header = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    val = lambda name: int(re.search(r"\b%s = (\d+)" % name, header).group(1))
    assert val("LMGPU_NUM_FACTOR_TYPES") == len(G.FACTOR_ARITY) == 14 and val("LMGPU_NUM_VAR_TYPES") == len(G.VAR_DIM) == 7


def _u64(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_uint64))


def test_refusals_on_a_handle_without_a_device():
    """argument checks answer LMGPU_INVALID, an empty request LMGPU_OK, a well-formed one LMGPU_HIP_ERROR for want of a device; the
    structure taps refuse a key that is in no tree; nothing is written and no counter moves"""
    lib = _lib.load()
    cb = _lib.CCOLAMD_FN(lambda *a: 0)
    prm = _lib.lmgpu_isam2_params(0.1, 10, 1, 0.001)
    cfg = _lib.lmgpu_config(-1, 0, 1, 0)
    h = ct.c_void_p()
    assert lib.lmgpu_isam2_create(ct.byref(cfg), ct.byref(prm), ct.cast(cb, ct.c_void_p), None, ct.byref(h)) == _lib.LMGPU_HIP_ERROR and h
    out = np.full(81, 7.0)
    D = out.ctypes.data_as(_lib._D)
    k = np.array([1, 2, 1], dtype=np.uint64)
    I = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(_lib._I)
    try:
        assert lib.lmgpu_isam2_marginal_covariances(h, 0, None, None) == _lib.LMGPU_OK
        assert lib.lmgpu_isam2_cross_covariances(h, 0, None, None, None) == _lib.LMGPU_OK
        assert lib.lmgpu_isam2_joint_marginal_covariances(h, 0, None, None, None) == _lib.LMGPU_OK
        assert lib.lmgpu_isam2_marginal_covariances(h, -1, _u64(k), D) == _lib.LMGPU_INVALID
        assert b"n < 0" in lib.lmgpu_isam2_last_error(h)
        assert lib.lmgpu_isam2_marginal_covariances(h, 1, None, D) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_marginal_covariances(h, 1, _u64(k), None) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_cross_covariances(h, -1, _u64(k), _u64(k), D) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_cross_covariances(h, 1, _u64(k), None, D) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_cross_covariances(h, 1, _u64(k), _u64(k), None) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_joint_marginal_covariances(h, -1, I([0, 2]), _u64(k), D) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_joint_marginal_covariances(h, 1, I([0, 2]), _u64(k), None) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_joint_marginal_covariances(h, 1, I([0, 3]), _u64(k), D) == _lib.LMGPU_INVALID
        assert b"twice" in lib.lmgpu_isam2_last_error(h)
        assert lib.lmgpu_isam2_joint_marginal_covariances(h, 2, I([0, 2, 1]), _u64(k), D) == _lib.LMGPU_INVALID
        assert b"decreases" in lib.lmgpu_isam2_last_error(h)
        assert lib.lmgpu_isam2_joint_marginal_covariances(h, 1, I([-1, 1]), _u64(k), D) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_marginal_covariances(h, 1, _u64(k), D) == _lib.LMGPU_HIP_ERROR
        assert lib.lmgpu_isam2_cross_covariances(h, 1, _u64(k), _u64(k), D) == _lib.LMGPU_HIP_ERROR
        assert lib.lmgpu_isam2_joint_marginal_covariances(h, 1, I([0, 2]), _u64(k), D) == _lib.LMGPU_HIP_ERROR
        assert (out == 7.0).all()
        path = np.full(4, 9, dtype=np.uint64)
        assert lib.lmgpu_isam2_marginals_path(h, 1, _u64(path), 4) == -1 and (path == 9).all()
        assert lib.lmgpu_isam2_marginals_junction(h, 1, 2, _u64(path)) == -1 and (path == 9).all()
        assert lib.lmgpu_isam2_set_marginals_params(h, -1, 0, 0) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_set_marginals_params(h, 0, -1, 0) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_set_marginals_params(h, 0, 1 << 20, 0) == _lib.LMGPU_INVALID
        assert lib.lmgpu_isam2_set_marginals_params(h, 0, 0, -1) == _lib.LMGPU_INVALID
        st = _lib.lmgpu_marginals_stats()
        assert lib.lmgpu_isam2_get_marginals_stats(h, ct.byref(st)) == _lib.LMGPU_OK
        defaults = (st.scratch_bytes, st.lds_capacity, st.cross_cap)
        assert defaults == (64 << 20, 6144, 16)
        assert lib.lmgpu_isam2_set_marginals_params(h, 1 << 20, 0, 3) == _lib.LMGPU_OK  # 0 keeps
        assert lib.lmgpu_isam2_get_marginals_stats(h, ct.byref(st)) == _lib.LMGPU_OK
        assert (st.scratch_bytes, st.lds_capacity, st.cross_cap) == (1 << 20, 6144, 3)
        assert (st.launches, st.chunks, st.factorizations, st.vars_lds, st.vars_scratch, st.cross_launches, st.cross_chunks, st.cross_walks,
                st.cross_targets) == (0,) * 9
    finally:
        lib.lmgpu_isam2_destroy(h)
