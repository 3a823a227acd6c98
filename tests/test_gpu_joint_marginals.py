"""Cross-covariances and joint marginals from the one factorization (lmgpu_marginal_cross_covariances, lmgpu_joint_marginal_covariances,
csrc/kernels_marginals.hpp marginal_cross_kernel) on the device.  Every block is held against
  (a) the long-double restatement of the cross walk (tests/joint_marginals_restatement.py) on the device's own fronts (lmgpu_get_front),
      over the union of the two paths;
  (b) the refined long-double dense inverse of A^T A from linear_graph().
Error of a block: ||got - ref||_F / sqrt(||ref_ii||_F ||ref_jj||_F) (never the block's own norm: a cross block can be near zero).
Bound: section 17's rule, min(max(4 e_old, 1e-13), 1e-6), e_old the same measure of lmgpu_joint_marginal_covariance's block on a second
handle.  Every comparison prints (e_old, e_new, bound)."""
import ctypes as ct

import numpy as np
import pytest

import joint_marginals_cases as jc
import joint_marginals_restatement as jr
import marginals_path_cases as cases
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, LevenbergMarquardtOptimizer, LevenbergMarquardtParams, Marginals, Ordering,
                                PCGSolverParameters, _lib)
from gtsam_personal_amd.synthetic import make_bal
from test_gpu_marginals_path import _dense_columns_ld, _information_ld
from test_oracle_golden import PLANAR_SLAM_JOINT_L2_X1_X3, _odometry_example, _planar_slam_example

pytestmark = pytest.mark.gpu
LD = np.longdouble
_I = ct.POINTER(ct.c_int32)
_D = ct.POINTER(ct.c_double)
# targets per workgroup forced in most tests: all targets of a source behind ONE walk of its path (the built-in rule spreads a small
# request one target per workgroup, which would leave the target loop untested)
SHARED = 64


def _fn(a):
    return float(np.linalg.norm(np.asarray(a, dtype=LD).astype(np.float64)))


def _err(got, ref, ref_ii, ref_jj):
    return _fn(np.asarray(got, dtype=LD) - ref) / np.sqrt(_fn(ref_ii) * _fn(ref_jj))


def _dim(o, k):
    return int(o._xoff[o._slot[int(k)] + 1] - o._xoff[o._slot[int(k)]])


def _path(o, key):
    buf = np.zeros(o.num_fronts() + 1, dtype=np.int32)
    n = o.lib.lmgpu_marginals_path(o._h, o._slot[int(key)], buf.ctypes.data_as(_I), len(buf))
    assert 1 <= n <= o.num_fronts()
    return [int(f) for f in buf[:n]]


def _union_cliques(o, ki, kj, cache):
    """the fronts on the two paths, read from the device, as the restatement's clique list (variables named by key)"""
    fronts = []
    for f in _path(o, ki) + _path(o, kj):
        if f not in fronts:
            fronts.append(f)
    for f in fronts:
        if f not in cache:
            cache[f] = (o.front_info(f), o.front(f))
    index = {f: q for q, f in enumerate(fronts)}
    return [(cache[f][1][0], cache[f][0]["n_frontal_keys"], index.get(cache[f][0]["parent"], -1), cache[f][1][1]) for f in fronts]


class _Refs:
    """the two references of a case, computed once: (b)'s columns for the keys asked about, (a)'s fronts as they are read"""

    def __init__(self, m, keys):
        self.o = m._opt
        self.keys = [int(k) for k in dict.fromkeys(int(k) for k in keys)]
        o = self.o
        self.dims = {int(k): _dim(o, k) for k in o._slot}
        self.rows = {k: np.arange(o._xoff[o._slot[k]], o._xoff[o._slot[k] + 1]) for k in self.keys}
        cols = np.concatenate([self.rows[k] for k in self.keys])
        self.X = _dense_columns_ld(_information_ld(o), cols)
        off = np.concatenate([[0], np.cumsum([self.dims[k] for k in self.keys])]).astype(int)
        self.col = {k: np.arange(off[q], off[q + 1]) for q, k in enumerate(self.keys)}
        self.cache = {}

    def b(self, ki, kj):
        blk = self.X[np.ix_(self.rows[int(ki)], self.col[int(kj)])]
        return 0.5 * (blk + blk.T) if int(ki) == int(kj) else blk

    def a(self, ki, kj):
        return jr.cross_covariance(_union_cliques(self.o, ki, kj, self.cache), self.dims, int(ki), int(kj))


def _set_cap(m, cap):
    assert m._opt.lib.lmgpu_set_marginals_cross_cap(m._opt._h, cap) == _lib.LMGPU_OK


def _old_block(old, ki, kj):
    ki, kj = int(ki), int(kj)
    return old.jointMarginalCovariance([ki] if ki == kj else [ki, kj]).at(ki, kj)


def _check_pairs(name, graph, values, ordering, pairs, lds_doubles=0):
    """the cross route of a fresh handle for `pairs` against (a) and (b) under the bound the old route sets; returns (Marginals, blocks)"""
    m, old = Marginals(graph, values, ordering), Marginals(graph, values, ordering)
    if lds_doubles:
        assert m._opt.lib.lmgpu_set_marginals_params(m._opt._h, 0, lds_doubles) == _lib.LMGPU_OK
    _set_cap(m, SHARED)
    pairs = [(int(a), int(b)) for a, b in pairs]
    got = m.crossCovariances(pairs)
    refs = _Refs(m, [k for pr in pairs for k in pr])
    worst = (0.0, 0.0, 0.0)
    for ki, kj in pairs:
        assert got[(ki, kj)].shape == (refs.dims[ki], refs.dims[kj])
        cov_old = _old_block(old, ki, kj)
        ref_ii, ref_jj = refs.b(ki, ki), refs.b(kj, kj)
        for tag, ref in (("a", refs.a(ki, kj)), ("b", refs.b(ki, kj))):
            e_old, e_new = _err(cov_old, ref, ref_ii, ref_jj), _err(got[(ki, kj)], ref, ref_ii, ref_jj)
            bound = min(max(4.0 * e_old, 1e-13), 1e-6)
            print(f"  {name} pair ({ki}, {kj}) ({tag}): old route {e_old:.3g}, cross route {e_new:.3g}, bound {bound:.3g}")
            if e_new > worst[1]:
                worst = (e_old, e_new, bound)
            assert e_new <= bound, (name, ki, kj, tag, e_old, e_new, bound)
    print(f"  {name} WORST: old route {worst[0]:.3g}, cross route {worst[1]:.3g}, bound {worst[2]:.3g}")
    old.close()
    return m, got


def _junction(m, ki, kj):
    o = m._opt
    return o.lib.lmgpu_marginals_junction(o._h, o._slot[int(ki)], o._slot[int(kj)])


def _front_of(m, k):
    return _path(m._opt, k)[0]


def _stats(m):
    return m.marginalsStats()


# ---------------------------------------------------------------- shapes
def test_single_variable_pair_with_itself():
    g, v, o = cases.single_variable()
    m, got = _check_pairs("single", g, v, o, [(7, 7)])
    assert np.array_equal(got[(7, 7)], m.marginalCovariances([7])[7])
    m.close()


def test_odometry_all_ordered_pairs():
    g, v = _odometry_example()
    m, got = _check_pairs("odometry", g, v, Ordering([1, 2, 3]), [(a, b) for a in (1, 2, 3) for b in (1, 2, 3)])
    for a in (1, 2, 3):
        for b in (1, 2, 3):
            assert np.allclose(got[(a, b)], got[(b, a)].T, rtol=0, atol=1e-12)
    m.close()


def test_planar_slam_joint_at_the_reference_tolerance_and_mixed_dimensions():
    """tests/testMarginals.cpp:128-176 at the reference's 1e-6 through Marginals(path_solves=True); source dimension 2 with target
    dimension 3 and the reverse"""
    g, soln, keys = _planar_slam_example()
    x1, x2, x3, l1, l2 = keys
    for ordering in ([l1, l2, x1, x2, x3], list(keys)):
        mp = Marginals(g, soln, Ordering(ordering), path_solves=True)
        joint = mp.jointMarginalCovariance([x1, l2, x3])
        assert joint.keys == [l2, x1, x3] and joint.dims == [2, 3, 3]
        full = joint.fullMatrix()
        assert np.array_equal(full, full.T)
        assert np.allclose(full, PLANAR_SLAM_JOINT_L2_X1_X3, rtol=0, atol=1e-6)
        assert np.allclose(joint(l2, l2), PLANAR_SLAM_JOINT_L2_X1_X3[0:2, 0:2], atol=1e-6)
        assert np.allclose(joint(x1, l2), PLANAR_SLAM_JOINT_L2_X1_X3[2:5, 0:2], atol=1e-6)
        assert np.allclose(joint(x3, x1), PLANAR_SLAM_JOINT_L2_X1_X3[5:8, 2:5], atol=1e-6)
        joint2 = mp.jointMarginalCovariance([l2, x1])
        assert np.allclose(joint2.fullMatrix(), PLANAR_SLAM_JOINT_L2_X1_X3[0:5, 0:5], atol=1e-6)
        assert np.allclose(mp.jointMarginalInformation([l2, x1]).fullMatrix() @ joint2.fullMatrix(), np.eye(5), atol=1e-9)
        st = _stats(mp)
        assert st["factorizations"] == 1 and st["cross_launches"] == 3
        mp.close()
        m, got = _check_pairs("planar_slam", g, soln, Ordering(ordering), [(x1, l2), (l2, x1), (l1, l2), (x3, l1), (l1, x3), (x2, x2)])
        assert got[(x1, l2)].shape == (3, 2) and got[(l2, x1)].shape == (2, 3)
        m.close()


def test_both_variables_frontal_in_one_front():
    g, v, o = cases.dense_clique(4)
    m, _ = _check_pairs("dense_clique", g, v, o, [(o[0], o[3]), (o[3], o[0]), (o[1], o[2]), (o[2], o[2])])
    assert m._opt.num_fronts() == 1 and _junction(m, o[0], o[3]) == 0
    m.close()


def test_target_above_the_source_and_source_above_the_target():
    """pose2_chain: ends and middle, both orders; i's front an ancestor of j's (a read) and the reverse (the branch is the rest of i's path)"""
    g, v, o = cases.pose2_chain(5)
    m, _ = _check_pairs("chain", g, v, o, [(1, 5), (5, 1), (1, 3), (3, 1), (3, 5), (5, 3)])
    assert _junction(m, 1, 5) == _front_of(m, 5) and _junction(m, 1, 3) == _front_of(m, 3) != _front_of(m, 1)
    m.close()


def test_sibling_leaves_under_the_poses():
    g, v, o = cases.projection()
    m, _ = _check_pairs("projection", g, v, o, [(0, 1), (1, 0), (3, 6), (0, 100), (100, 0), (101, 102), (2, 2)])
    assert _junction(m, 0, 1) not in (_front_of(m, 0), _front_of(m, 1))
    m.close()


def test_branching_tree_three_junction_depths():
    g, v, o = jc.pose2_comb()
    m, _ = _check_pairs("comb", g, v, o, [(a, b) for a in range(1, 8) for b in (1, 4, 7, 6)])
    assert len({_junction(m, 1, 2), _junction(m, 1, 7), _junction(m, 1, 4)}) == 3
    m.close()


def test_forest_pair_across_components_is_exact_zero_and_joint_is_block_diagonal():
    g, v, o = cases.forest()
    m, got = _check_pairs("forest", g, v, o, [(1, 2), (12, 11), (4, 4)])
    assert _junction(m, 1, 11) == -1
    before = _stats(m)
    across = m.crossCovariances([(1, 11), (13, 4), (2, 1)])
    assert (across[(1, 11)] == 0).all() and (across[(13, 4)] == 0).all() and across[(1, 11)].shape == (3, 3)
    assert np.array_equal(across[(2, 1)], m.crossCovariances([(2, 1)])[(2, 1)]) and np.abs(across[(2, 1)]).max() > 0
    assert _stats(m)["cross_targets"] - before["cross_targets"] == 4
    full = m.jointMarginalCovariances([[1, 3, 11, 13]])[0].fullMatrix()
    assert (full[:6, 6:] == 0).all() and (full[6:, :6] == 0).all() and np.array_equal(full, full.T)
    refs = _Refs(m, [1, 3, 11, 13])
    for a in (1, 3, 11, 13):
        assert np.array_equal(full[refs.col[a]][:, refs.col[a]], m.marginalCovariances([a])[a])
    m.close()


def test_three_variable_factors_meet_the_bound_where_the_old_route_does_not():
    """calibrated_sfm: GeneralSFMFactor2 ties pose, point and calibration.  The cross route is held to the bound against both references;
    the old route's distance from them (3 % at the time of writing: zero_rhs_kernel clears the wrong column) is printed beside it."""
    g, v, o = cases.calibrated_sfm()
    m, _ = _check_pairs("calibrated_sfm", g, v, o, [(0, 500), (500, 0), (100, 500), (0, 100), (100, 3), (2, 4), (101, 102), (500, 500)])
    m.close()


def test_nine_columns():
    g, v, o = cases.vec9_chain()
    m, _ = _check_pairs("vec9", g, v, o, [(0, 3), (3, 0), (1, 2), (2, 2)])
    m.close()


def test_junction_is_a_270_column_hbm_root():
    """30 BAL cameras: camera-camera (one front, columns on both sides of the block-of-32 boundaries), camera-point, point-camera and
    point-point pairs, all meeting at the root"""
    g, v, _, o = make_bal(n_cam=30, n_pt=200, obs_per_point=6, seed=9)
    keys = list(o)
    cam, pt = keys[200:], keys[:200]
    m, _ = _check_pairs("bal30", g, v, o, [(cam[0], cam[29]), (cam[3], cam[4]), (cam[28], cam[7]), (cam[2], pt[0]), (pt[0], cam[2]),
                                           (pt[199], cam[17]), (pt[5], pt[150]), (pt[150], pt[5])])
    root = m._opt.front_info(m._opt.num_fronts() - 1)
    assert root["nf"] == 270 and root["cls"] == 1
    assert _junction(m, pt[5], pt[150]) == _junction(m, cam[0], pt[0]) == m._opt.num_fronts() - 1
    m.close()


def test_register_lds_and_hbm_fronts_on_one_union_of_paths():
    g, v, o, leaf = cases.sphere_head_with_leaf()
    ks = sorted(int(x) for x in o if int(x) != leaf)
    m, _ = _check_pairs("sphere_head_leaf", g, v, o, [(leaf, ks[150]), (ks[150], leaf), (0, ks[150])])
    st = _stats(m)
    assert st["cross_scratch"] >= 1 and st["cross_launches"] == 1
    m.close()


# ---------------------------------------------------------------- placement, chunks, order, split: the same bits
def _comb_need(source_len, target_len, source_depth, branch, dp=3):
    return max(source_len, target_len) * dp + (source_depth + 1 + branch + 1) // 2


def test_lds_window_edge_reached_by_the_branch():
    """pose2_comb: source 4 (path of 9 scalars, two fronts), target 1 (15 scalars, three fronts below the root): the work vector is as long
    as the TARGET's path.  The window exactly at the need, then one double below: LDS, then scratch, the same bits."""
    g, v, o = jc.pose2_comb()
    need = _comb_need(9, 15, 1, 3)
    res = []
    for lds, want_scratch in ((need, 0), (need - 1, 1)):
        m = Marginals(g, v, o)
        assert m._opt.lib.lmgpu_set_marginals_params(m._opt._h, 0, lds) == _lib.LMGPU_OK
        res.append(m.crossCovariances([(1, 4)])[(1, 4)])
        st = _stats(m)
        assert (st["cross_scratch"], st["cross_lds"]) == (want_scratch, 1 - want_scratch), (lds, st)
        # the source alone needs less: 9 scalars
        alone = m.crossCovariances([(4, 4)])
        assert _stats(m)["cross_lds"] - st["cross_lds"] == 1 and np.array_equal(alone[(4, 4)], m.marginalCovariances([4])[4])
        m.close()
    assert np.array_equal(res[0], res[1]) and np.abs(res[0]).max() > 0


def test_small_scratch_budget_cuts_the_pairs_into_chunks():
    g, v, o = jc.pose2_comb()
    pairs = [(a, b) for b in range(1, 8) for a in range(1, 8)]
    ref = Marginals(g, v, o)
    _set_cap(ref, SHARED)
    want = ref.crossCovariances(pairs)
    assert _stats(ref)["cross_chunks"] == 1 and _stats(ref)["cross_walks"] == 7
    m = Marginals(g, v, o)
    _set_cap(m, SHARED)
    assert m._opt.lib.lmgpu_set_marginals_params(m._opt._h, 2 * _comb_need(15, 15, 3, 3) * 8, 8) == _lib.LMGPU_OK  # all in scratch, two vectors at most
    got = m.crossCovariances(pairs)
    st = _stats(m)
    assert st["cross_lds"] == 0 and st["cross_scratch"] == 7 and 4 <= st["cross_chunks"] == st["cross_launches"] <= 7 and st["factorizations"] == 1
    for pr in pairs:
        assert np.array_equal(got[pr], want[pr]), pr
    assert m._opt.lib.lmgpu_set_marginals_params(m._opt._h, 40 * 8, 8) == _lib.LMGPU_OK
    with pytest.raises(_lib.LmgpuError, match="scratch"):
        m.crossCovariances([(1, 4)])
    m.close()
    ref.close()


def test_order_of_targets_and_the_rest_of_the_request_do_not_change_a_block():
    """source 1 with target 7 (junction: the front of 3) and target 4 (junction: the root), in both orders, alone, and inside all pairs"""
    g, v, o = jc.pose2_comb()
    m = Marginals(g, v, o)
    _set_cap(m, SHARED)
    alone7, alone4 = m.crossCovariances([(7, 1)])[(7, 1)], m.crossCovariances([(4, 1)])[(4, 1)]
    for pairs in ([(7, 1), (4, 1)], [(4, 1), (7, 1)], [(4, 1), (3, 6), (7, 1), (1, 1), (5, 1)], [(a, b) for a in range(1, 8) for b in range(1, 8)]):
        got = m.crossCovariances(pairs)
        assert np.array_equal(got[(7, 1)], alone7) and np.array_equal(got[(4, 1)], alone4), pairs
    assert np.abs(alone7).max() > 0 and np.abs(alone4).max() > 0 and not np.array_equal(alone7, alone4)
    # duplicates are served
    o_ = m._opt
    si = np.array([o_._slot[4], o_._slot[7], o_._slot[4]], dtype=np.int32)
    sj = np.array([o_._slot[1]] * 3, dtype=np.int32)
    out = np.zeros(27)
    assert o_.lib.lmgpu_marginal_cross_covariances(o_._h, 3, si.ctypes.data_as(_I), sj.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_OK
    blocks = out.reshape(3, 3, 3)
    assert np.array_equal(blocks[0], alone4) and np.array_equal(blocks[1], alone7) and np.array_equal(blocks[2], alone4)
    m.close()


def test_targets_of_one_source_split_over_workgroups():
    g, v, o = cases.projection()
    keys = [int(k) for k in o]
    pairs = [(k, 100) for k in keys] + [(k, 3) for k in keys]
    m = Marginals(g, v, o)
    default_cap = _stats(m)["cross_cap"]
    _set_cap(m, SHARED)
    want = m.crossCovariances(pairs)
    base = _stats(m)
    assert base["cross_walks"] == 2 and base["cross_targets"] == len(pairs) and base["cross_cap"] == 64
    for cap, walks in ((1, len(pairs)), (3, 2 * ((len(keys) + 2) // 3))):
        _set_cap(m, cap)
        before = _stats(m)
        got = m.crossCovariances(pairs)
        st = _stats(m)
        assert st["cross_cap"] == cap and st["cross_walks"] - before["cross_walks"] == walks and st["cross_launches"] - before["cross_launches"] == 1
        for pr in pairs:
            assert np.array_equal(got[pr], want[pr]), (cap, pr)
    _set_cap(m, 0)  # the built-in rule: a small request is spread, one target per workgroup
    before = _stats(m)
    got = m.crossCovariances(pairs)
    assert _stats(m)["cross_cap"] == default_cap and _stats(m)["cross_walks"] - before["cross_walks"] == len(pairs)
    for pr in pairs:
        assert np.array_equal(got[pr], want[pr]), pr
    m.close()


def test_diagonal_blocks_are_the_path_walks_and_joints_are_symmetric():
    for name, builder in (("comb", jc.pose2_comb), ("projection", cases.projection), ("vec9", cases.vec9_chain), ("sfm", cases.calibrated_sfm)):
        g, v, o = builder()
        keys = [int(k) for k in o]
        m = Marginals(g, v, o)
        _set_cap(m, SHARED)
        single = m.marginalCovariances(keys)
        diag = m.crossCovariances([(k, k) for k in keys])
        for k in keys:
            assert np.array_equal(diag[(k, k)], single[k]), (name, k)
        sets = [keys, keys[::-1][:3], [keys[0], keys[-1]], [keys[1]]]
        joints = m.jointMarginalCovariances(sets)
        cross = m.crossCovariances([(a, b) for a in keys for b in keys])
        for ks, jm in zip(sets, joints):
            full = jm.fullMatrix()
            assert jm.keys == sorted(ks) and np.array_equal(full, full.T), name
            for a in ks:
                assert np.array_equal(jm.at(a, a), single[a])
                for b in ks:
                    if a != b:  # computed once, from one of the two as the source, and mirrored
                        assert np.array_equal(jm.at(a, b), cross[(a, b)]) or np.array_equal(jm.at(a, b), cross[(b, a)].T), (name, a, b)
        assert _stats(m)["factorizations"] == 1
        m.close()


# ---------------------------------------------------------------- failures, staleness, refusals, counters
def test_gauge_freedom_reports_indeterminate_with_a_failed_slot():
    g, v, o = cases.gauge_freedom()
    m = Marginals(g, v, o, path_solves=True)
    h = m._opt
    with pytest.raises(_lib.IndeterminantLinearSystemException):
        m.crossCovariances([(1, 2)])
    assert h.lib.lmgpu_last_failed_slot(h._h) in (0, 1)
    with pytest.raises(_lib.IndeterminantLinearSystemException):
        m.jointMarginalCovariance([1, 2])
    slots = np.array([0, 1], dtype=np.int32)
    begin = np.array([0, 2], dtype=np.int32)
    out = np.zeros(36)
    assert h.lib.lmgpu_joint_marginal_covariances(h._h, 1, begin.ctypes.data_as(_I), slots.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_INDETERMINATE
    assert h.lib.lmgpu_last_failed_slot(h._h) in (0, 1)
    m.close()


def test_stale_factorization_is_rebuilt_after_set_values():
    g, v, o = jc.pose2_comb()
    m = Marginals(g, v, o)
    h = m._opt
    first = m.crossCovariances([(7, 1), (4, 1)])
    m.jointMarginalCovariances([[1, 4]])
    assert _stats(m)["factorizations"] == 1
    rng = np.random.default_rng(4)
    h.retract(rng.normal(0, 0.05, h._ntot))
    moved = h.values()
    h.set_values(moved)
    second = m.crossCovariances([(7, 1), (4, 1)])
    assert _stats(m)["factorizations"] == 2
    fresh = Marginals(g, moved, o)
    want = fresh.crossCovariances([(7, 1), (4, 1)])
    for pr in want:
        assert np.array_equal(second[pr], want[pr]) and not np.array_equal(first[pr], second[pr]), pr
    m.close()
    fresh.close()


def test_the_refusals():
    """smart factors and a handle finalized under PCG: marg_refused's messages, nothing written; an out-of-range slot and a slot twice in
    a set: LMGPU_INVALID before anything is written; an empty request: LMGPU_OK and no counter moves"""
    import smart_cases as sc
    g, v, o = cases.pose2_chain(4)
    pcg = LevenbergMarquardtParams()
    pcg.linearSolverType, pcg.iterativeParams = "ITERATIVE", PCGSolverParameters(BlockJacobiPreconditionerParameters())
    sg, sv, so, _ = sc.package(sc.ring_scene([3, 4, 2], seed=3))
    one, begin, two = np.zeros(1, dtype=np.int32), np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    for h, msg in ((LevenbergMarquardtOptimizer(sg, sv, so, LevenbergMarquardtParams()), b"smart projection factors"),
                   (LevenbergMarquardtOptimizer(g, v, o, pcg), b"finalized under PCG")):
        out = np.full(144, 7.0)
        assert h.lib.lmgpu_marginal_cross_covariances(h._h, 1, one.ctypes.data_as(_I), one.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_INVALID
        assert msg in h.lib.lmgpu_last_error(h._h), h.lib.lmgpu_last_error(h._h)
        assert h.lib.lmgpu_joint_marginal_covariances(h._h, 1, begin.ctypes.data_as(_I), two.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_INVALID
        assert msg in h.lib.lmgpu_last_error(h._h) and (out == 7.0).all()
        h.close()
    m = Marginals(g, v, o)
    h = m._opt
    m.crossCovariances([(1, 2)])
    before = _stats(m)
    for bad in (4, -1):
        si, sj = np.array([0, bad, 1], dtype=np.int32), np.array([1, 0, 2], dtype=np.int32)
        out = np.full(27, 7.0)
        for a, b in ((si, sj), (sj, si)):
            assert h.lib.lmgpu_marginal_cross_covariances(h._h, 3, a.ctypes.data_as(_I), b.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_INVALID
            assert (out == 7.0).all() and b"out of range" in h.lib.lmgpu_last_error(h._h)
        sets, sb = np.array([0, 1, bad], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32)
        out = np.full(81, 7.0)
        assert h.lib.lmgpu_joint_marginal_covariances(h._h, 2, sb.ctypes.data_as(_I), sets.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_INVALID
        assert (out == 7.0).all() and b"out of range" in h.lib.lmgpu_last_error(h._h)
    with pytest.raises(_lib.LmgpuError, match="twice"):
        m.jointMarginalCovariances([[1, 2], [3, 2, 3]])
    assert h.lib.lmgpu_marginal_cross_covariances(h._h, 0, None, None, None) == _lib.LMGPU_OK
    assert h.lib.lmgpu_joint_marginal_covariances(h._h, 0, None, None, None) == _lib.LMGPU_OK
    assert m.crossCovariances([]) == {} and m.jointMarginalCovariances([]) == []
    assert _stats(m) == before
    m.close()


def test_stats_counters_move_as_documented():
    g, v, o = jc.pose2_comb()
    m = Marginals(g, v, o)
    _set_cap(m, SHARED)
    st0 = _stats(m)
    assert all(st0[f] == 0 for f in ("cross_launches", "cross_chunks", "cross_walks", "cross_targets", "cross_lds", "cross_scratch", "longest_union"))
    m.crossCovariances([(7, 1), (4, 1), (2, 4)])  # two sources; source 1 (4 fronts) + the branch to 7 (1) or to 4 (1); source 4 (2) + the branch to 2 (2)
    st = _stats(m)
    assert (st["cross_launches"], st["cross_chunks"], st["cross_walks"], st["cross_targets"], st["cross_lds"], st["cross_scratch"]) == (1, 1, 2, 3, 2, 0)
    assert st["longest_union"] == 5 and st["factorizations"] == 1
    assert (st["launches"], st["chunks"], st["vars_lds"], st["vars_scratch"], st["longest_path"]) == (0, 0, 0, 0, 0)  # the single-variable counters stay
    m.jointMarginalCovariances([[1, 4]])  # (1, 1), (4, 4) and one cross block from 4, the shorter path
    st2 = _stats(m)
    assert st2["cross_walks"] - st["cross_walks"] == 2 and st2["cross_targets"] - st["cross_targets"] == 3 and st2["cross_launches"] - st["cross_launches"] == 1
    m.close()
