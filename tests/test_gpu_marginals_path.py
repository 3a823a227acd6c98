"""Marginal covariances along each variable's path to the root (lmgpu_marginal_covariances, csrc/kernels_marginals.hpp)
on the device, every case three ways:
  (a) the long-double restatement of the walk (tests/marginals_path_restatement.py) on the device's own fronts (lmgpu_get_front);
  (b) the long-double dense inverse of the information matrix assembled from lmgpu_get_jacobians;
  (c) where the repository holds them, the reference's known answers at the reference's tolerances.
Bound for (a) and (b): not fixed in advance.  The existing per-column route (lmgpu_marginal_covariance, on a second handle) is measured
against the same long-double answer as a relative Frobenius norm; the path route may deviate at most 4 x that (the same conditioning, a
different summation order), with a floor of 1e-13, and never more than the project's 1e-6.  Every comparison prints its pair."""
import ctypes as ct

import numpy as np
import pytest

import marginals_path_cases as cases
import marginals_path_restatement as mr
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, LevenbergMarquardtOptimizer, LevenbergMarquardtParams, Marginals, Ordering,
                                PCGSolverParameters, _lib)
from gtsam_personal_amd.synthetic import make_bal
from test_oracle_golden import ODOMETRY_EXACT, PLANAR_SLAM_EXPECTED, _odometry_example, _planar_slam_example

pytestmark = pytest.mark.gpu
LD = np.longdouble
_I = ct.POINTER(ct.c_int32)
_D = ct.POINTER(ct.c_double)


def _relf(got, want):
    want = np.asarray(want, dtype=LD)
    return float(np.linalg.norm((np.asarray(got, dtype=LD) - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))


def _information_ld(opt):
    """A^T A of the linearization on the device, long double, scalars in slot order"""
    N = int(opt._xoff[-1])
    info = np.zeros((N, N), dtype=LD)
    lg = opt.linear_graph()
    for i in range(lg.size()):
        f = lg.at(i)
        if f is None:
            continue
        cols = np.concatenate([np.arange(opt._xoff[opt._slot[int(k)]], opt._xoff[opt._slot[int(k)] + 1]) for k in f.keys()])
        A = f.jacobian()[0].astype(LD)
        info[np.ix_(cols, cols)] += A.T @ A
    return info


def _dense_columns_ld(info, cols):
    """columns `cols` of info^-1 in long double: the float64 inverse, refined against the long-double residual"""
    N = info.shape[0]
    inv = np.linalg.inv(info.astype(np.float64))
    E = np.zeros((N, len(cols)), dtype=LD)
    E[cols, np.arange(len(cols))] = 1
    X = inv[:, cols].astype(LD)
    eps = float(np.finfo(LD).eps)
    for _ in range(6):
        X = X + (inv @ (E - info @ X).astype(np.float64)).astype(LD)
    # converged to what long double can resolve: the residual against the rounding of the products that form it
    floor = float(np.max(np.abs(info) @ np.abs(X)))
    assert float(np.max(np.abs(E - info @ X))) <= 64 * eps * floor, "the refinement of the dense inverse did not converge"
    return X


def _path_cliques(opt, key, cache):
    """the fronts of the key's path, read from the device, as the restatement's clique list (variables named by key)"""
    buf = np.zeros(opt.num_fronts() + 1, dtype=np.int32)
    n = opt.lib.lmgpu_marginals_path(opt._h, opt._slot[int(key)], buf.ctypes.data_as(_I), len(buf))
    assert 1 <= n <= opt.num_fronts()
    out = []
    for q in range(n):
        f = int(buf[q])
        if f not in cache:
            cache[f] = (opt.front_info(f), opt.front(f))
        fi, (keys, rsd) = cache[f]
        assert fi["parent"] == (int(buf[q + 1]) if q + 1 < n else -1)
        out.append((keys, fi["n_frontal_keys"], q + 1 if q + 1 < n else -1, rsd))
    return out


def _stats(m):
    return m.marginalsStats()


def _set_params(m, scratch_bytes=0, lds_doubles=0):
    assert m._opt.lib.lmgpu_set_marginals_params(m._opt._h, scratch_bytes, lds_doubles) == _lib.LMGPU_OK


def _three_ways(name, graph, values, ordering, keys, known=None, lds_doubles=0, request=None):
    """the path route of a fresh handle for `request` (default: all variables) against (a), (b) and the old route's distance from them,
    for `keys`; returns (Marginals of the path route, its answers)"""
    m, old = Marginals(graph, values, ordering), Marginals(graph, values, ordering)
    if lds_doubles:
        _set_params(m, lds_doubles=lds_doubles)
    got = m.marginalCovariances(request)
    o = m._opt
    dims = {int(k): int(o._xoff[o._slot[int(k)] + 1] - o._xoff[o._slot[int(k)]]) for k in ordering}
    info = _information_ld(o)
    cols = np.concatenate([np.arange(o._xoff[o._slot[int(k)]], o._xoff[o._slot[int(k)] + 1]) for k in keys])
    X = _dense_columns_ld(info, cols)
    cache, c0 = {}, 0
    for k in keys:
        k, d = int(k), dims[int(k)]
        s0 = int(o._xoff[o._slot[k]])
        ref_b = X[s0:s0 + d, c0:c0 + d]
        ref_b = 0.5 * (ref_b + ref_b.T)
        c0 += d
        ref_a = mr.path_marginal(_path_cliques(o, k, cache), dims, k)
        cov_old = old.marginalCovariance(k)
        assert got[k].shape == (d, d) and np.array_equal(got[k], got[k].T)
        for tag, ref in (("a", ref_a), ("b", ref_b)):
            e_old, e_new = _relf(cov_old, ref), _relf(got[k], ref)
            bound = min(max(4.0 * e_old, 1e-13), 1e-6)
            print(f"  {name} key {k} ({tag}): per-column route {e_old:.3g}, path route {e_new:.3g}, bound {bound:.3g}")
            assert e_new <= bound, (name, k, tag, e_old, e_new)
        if known is not None:
            assert np.allclose(got[k], np.array(known[k]), rtol=1e-9, atol=1e-8), (name, k)
    old.close()
    return m, got


def _path_len(m, key):
    return m._opt.lib.lmgpu_marginals_path(m._opt._h, m._opt._slot[int(key)], None, 0)


# ---------------------------------------------------------------- shapes
def test_single_variable_graph():
    g, v, o = cases.single_variable()
    m, _ = _three_ways("single", g, v, o, list(o))
    assert _path_len(m, o[0]) == 1
    m.close()


def test_root_variable_and_known_answers_odometry():
    """the odometry example: the last variable is frontal in the root (path length 1); the reference's printed / exact covariances"""
    g, v = _odometry_example()
    for ordering in ([1, 2, 3], [3, 1, 2]):
        m, got = _three_ways("odometry", g, v, Ordering(ordering), [1, 2, 3])
        assert _path_len(m, ordering[-1]) == 1
        for k in (1, 2, 3):
            assert np.allclose(got[k], np.array(ODOMETRY_EXACT[k]), rtol=1e-9, atol=1e-12), (k, got[k])
        m.close()


def test_planar_slam_known_answers_mixed_pose2_point2():
    """tests/testMarginals.cpp:40-126 at the reference's 1e-8; Pose2 + Point2 (3 / 2)"""
    g, soln, keys = _planar_slam_example()
    for ordering in ([keys[3], keys[4], keys[0], keys[1], keys[2]], list(keys)):
        m, got = _three_ways("planar_slam", g, soln, Ordering(ordering), keys)
        for k, expected in zip(keys, PLANAR_SLAM_EXPECTED):
            assert np.allclose(got[k], np.array(expected), rtol=0, atol=1e-8), (k, got[k])
        infos = m.marginalInformations(keys[:2])
        for k in keys[:2]:
            assert np.allclose(infos[k] @ got[k], np.eye(got[k].shape[0]), atol=1e-9)
        m.close()


def test_forest_of_two_components():
    g, v, o = cases.forest()
    m, _ = _three_ways("forest", g, v, o, list(o))
    assert len({int(_path_root(m, k)) for k in o}) == 2
    m.close()


def _path_root(m, key):
    buf = np.zeros(m._opt.num_fronts(), dtype=np.int32)
    n = m._opt.lib.lmgpu_marginals_path(m._opt._h, m._opt._slot[int(key)], buf.ctypes.data_as(_I), len(buf))
    return buf[n - 1]


def test_front_with_four_frontal_variables():
    g, v, o = cases.dense_clique(4)
    m, _ = _three_ways("dense_clique", g, v, o, [o[0], o[1], o[2], o[3]])
    assert m._opt.num_fronts() == 1 and m._opt.front_info(0)["n_frontal_keys"] == 4  # first, middle ones and last of one front
    m.close()


@pytest.mark.parametrize("name", ["projection", "calibrated_sfm", "vec9", "loop"])
def test_mixed_dimensions(name):
    """Pose3 + Point3 projection (6 / 3); Cal3_S2 (5) above poses and points; VEC9; a Pose2 loop"""
    g, v, o = cases.SMALL[name]()
    m, _ = _three_ways(name, g, v, o, list(o))
    m.close()


def test_bal_cameras_and_points_group_packed_leaves():
    """BAL cameras and points (9 / 3): group-packed gather leaves under the cameras' root"""
    g, v, _, o = make_bal(n_cam=20, n_pt=100, obs_per_point=4, seed=3)
    keys = list(o)
    m, _ = _three_ways("bal20", g, v, o, [keys[0], keys[31], keys[99], keys[100], keys[107], keys[-1]])
    assert m._opt.leaf_group_launches() > 0 and m._opt.front_info(m._opt.num_fronts() - 1)["cls"] == 1
    m.close()


def test_dense_root_wider_than_one_panel_and_the_handle_afterwards():
    """30 cameras: a 270-column root, wider than one 256-column panel; afterwards a plain linearize + solve works on the handle"""
    g, v, _, o = make_bal(n_cam=30, n_pt=200, obs_per_point=6, seed=9)
    keys = list(o)
    m, got = _three_ways("bal30", g, v, o, [keys[0], keys[199], keys[200], keys[229]])
    h = m._opt
    root = h.front_info(h.num_fronts() - 1)
    assert root["nf"] == 270 and root["parent"] == -1 and root["cls"] == 1
    ref = Marginals(g, v, o)._opt
    for x in (h, ref):
        x.linearize()
    (_, d, e0, e1), (_, dr, r0, r1) = h.solve(1e-3), ref.solve(1e-3)
    assert np.linalg.norm(d - dr) <= 1e-9 * np.linalg.norm(dr) and abs(e1 - r1) <= 1e-9 * max(1.0, abs(r1)) and abs(e0 - r0) <= 1e-9 * abs(r0)
    again = m.marginalCovariances([keys[200]])[keys[200]]  # (stale after the solve: factored again, the same bits)
    assert np.array_equal(again, got[keys[200]]) and _stats(m)["factorizations"] == 2
    m.close()
    ref.close()


def _path_classes(probe, info, key):
    buf = np.zeros(len(info), dtype=np.int32)
    n = probe.lib.lmgpu_marginals_path(probe._h, probe._slot[int(key)], buf.ctypes.data_as(_I), len(buf))
    fr = [info[f] for f in buf[:n]]
    return (any(f["cls"] == 0 and f["n"] <= 16 for f in fr), any(f["cls"] == 0 and f["n"] > 16 for f in fr), any(f["cls"] == 1 for f in fr))


def test_one_path_through_register_lds_and_hbm_fronts():
    """sphere2500's first 300 poses in natural order.  Its smallest front has 19 columns, so the path of pose 0 crosses LDS and HBM
    fronts only; with one more pose hung on pose 0 and eliminated first (a 13-column front) one path crosses a front of at most 16
    columns, wider LDS fronts and HBM fronts.  Both graphs are held to the three-way comparison."""
    g, v, o = cases.sphere_head_natural()
    probe = LevenbergMarquardtOptimizer(g, v, o, LevenbergMarquardtParams(), device=-1)
    info = [probe.front_info(f) for f in range(probe.num_fronts())]
    assert _path_classes(probe, info, 0) == (False, True, True)
    probe.close()
    ks = sorted(int(x) for x in o)
    m, _ = _three_ways("sphere_head", g, v, o, [0, ks[57], ks[150], ks[-1]])
    st = _stats(m)
    assert st["launches"] == st["chunks"] == 1 and st["vars_lds"] + st["vars_scratch"] == len(ks)
    m.close()
    g, v, o, leaf = cases.sphere_head_with_leaf()
    probe = LevenbergMarquardtOptimizer(g, v, o, LevenbergMarquardtParams(), device=-1)
    info = [probe.front_info(f) for f in range(probe.num_fronts())]
    assert _path_classes(probe, info, leaf) == (True, True, True)
    probe.close()
    m, _ = _three_ways("sphere_head_leaf", g, v, o, [leaf, 0, ks[150]])
    m.close()


def test_pose3_chain_either_side_of_the_lds_capacity():
    """a Pose3 chain in natural order: the path of pose 0 runs through every clique.  N from the capacity the stats report: just below it
    every vector stays in LDS, just above it pose 0's goes to scratch"""
    g, v, o = cases.pose3_chain(4)
    probe = Marginals(g, v, o)
    cap = _stats(probe)["lds_capacity"]
    probe.close()
    n_lo, n_hi = cap // 37, cap // 36 + 4  # work vector of pose 0: 6 N scalars x 6 columns + the path's front ids (N / 2 doubles at most)
    assert 8 <= n_lo < n_hi <= 600
    g, v, o = cases.pose3_chain(n_lo)
    m, _ = _three_ways("chain_lds", g, v, o, [0, n_lo // 2, n_lo - 1])
    st = _stats(m)
    assert st["vars_scratch"] == 0 and st["vars_lds"] == n_lo and st["longest_path"] == _path_len(m, 0) >= n_lo - 1
    m.close()
    g, v, o = cases.pose3_chain(n_hi)
    m, _ = _three_ways("chain_scratch", g, v, o, [0, 1, n_hi // 2, n_hi - 1])
    st = _stats(m)
    assert st["vars_scratch"] >= 1 and st["vars_lds"] >= 1 and st["vars_scratch"] + st["vars_lds"] == n_hi and st["launches"] == 1
    m.close()


def _need_of_pose0(g, v, o):
    """doubles of pose 0's work vector in a 12-pose chain: its 72 path scalars x 6 columns + the ids of its path's fronts, two per double"""
    probe = LevenbergMarquardtOptimizer(g, v, o, LevenbergMarquardtParams(), device=-1)
    n = probe.lib.lmgpu_marginals_path(probe._h, 0, None, 0)
    probe.close()
    return 6 * 12 * 6 + (n + 1) // 2


def test_lds_window_edge_is_exact():
    """the LDS window set to exactly what pose 0 of a 12-pose chain needs, then one double less: LDS, then scratch, the same bits"""
    g, v, o = cases.pose3_chain(12)
    need = _need_of_pose0(g, v, o)
    res = []
    for lds, want_scratch in ((need, 0), (need - 1, 1)):
        m = Marginals(g, v, o)
        _set_params(m, lds_doubles=lds)
        res.append(m.marginalCovariances([0])[0])
        st = _stats(m)
        assert (st["vars_scratch"], st["vars_lds"]) == (want_scratch, 1 - want_scratch), (lds, st)
        m.close()
    assert np.array_equal(res[0], res[1])


def test_small_scratch_budget_cuts_a_request_into_chunks():
    """every vector in scratch (an LDS window of 8 doubles) and a budget of three of pose 0's vectors: seven requests of it take three
    chunks, the last one partial; all variables under that budget equal the default handle's bits; one vector over the budget is refused"""
    g, v, o = cases.pose3_chain(12)
    need = _need_of_pose0(g, v, o)
    m, got = _three_ways("chunks", g, v, o, [0, 5, 11], lds_doubles=8)
    base = _stats(m)
    assert base["vars_lds"] == 0 and base["vars_scratch"] == 12 and base["chunks"] == 1
    _set_params(m, scratch_bytes=3 * need * 8)
    out = np.zeros(7 * 36)
    slots = np.zeros(7, dtype=np.int32)
    assert m._opt.lib.lmgpu_marginal_covariances(m._opt._h, 7, slots.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_OK
    st = _stats(m)
    assert st["chunks"] - base["chunks"] == 3 and st["launches"] - base["launches"] == 3 and st["factorizations"] == 1
    for q in range(7):
        assert np.array_equal(out[36 * q:36 * q + 36].reshape(6, 6), got[0])
    everything = m.marginalCovariances()
    ref = Marginals(g, v, o)
    want = ref.marginalCovariances()
    assert _stats(m)["chunks"] - st["chunks"] >= 3
    for k in o:
        assert np.array_equal(everything[k], want[k]), k
    _set_params(m, scratch_bytes=need * 8 - 8)
    with pytest.raises(_lib.LmgpuError, match="scratch"):
        m.marginalCovariances([0])
    m.close()
    ref.close()


def test_duplicates_empty_and_out_of_range_requests():
    g, v, o = cases.pose2_chain(5)
    m = Marginals(g, v, o)
    h = m._opt
    one = m.marginalCovariances([3])[3]
    slots = np.array([2, 2, 0, 2], dtype=np.int32)
    out = np.zeros(4 * 9)
    assert h.lib.lmgpu_marginal_covariances(h._h, 4, slots.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_OK
    blocks = out.reshape(4, 3, 3)
    assert np.array_equal(blocks[0], one) and np.array_equal(blocks[1], one) and np.array_equal(blocks[3], one)
    assert np.array_equal(blocks[2], m.marginalCovariances([1])[1])
    before = _stats(m)
    assert h.lib.lmgpu_marginal_covariances(h._h, 0, None, None) == _lib.LMGPU_OK
    assert m.marginalCovariances([]) == {}
    assert _stats(m) == before
    for bad in (5, -1):
        slots = np.array([0, bad, 1], dtype=np.int32)
        out = np.full(27, 7.0)
        assert h.lib.lmgpu_marginal_covariances(h._h, 3, slots.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_INVALID
        assert (out == 7.0).all() and b"out of range" in h.lib.lmgpu_last_error(h._h)
    assert _stats(m) == before
    m.close()


def test_gauge_freedom_reports_indeterminate():
    g, v, o = cases.gauge_freedom()
    m = Marginals(g, v, o, path_solves=True)
    with pytest.raises(_lib.IndeterminantLinearSystemException):
        m.marginalCovariances()
    with pytest.raises(_lib.IndeterminantLinearSystemException):
        m.marginalCovariance(2)
    m.close()


def test_stale_factorization_is_rebuilt():
    """query, retract a step, query again: the second answer is bitwise that of a fresh handle at the same values; two factorizations"""
    g, v, o = cases.pose3_chain(9)
    m = Marginals(g, v, o)
    h = m._opt
    first = m.marginalCovariances()
    assert _stats(m)["factorizations"] == 1
    m.marginalCovariances([0, 3])
    assert _stats(m)["factorizations"] == 1  # (still valid: nothing moved)
    rng = np.random.default_rng(2)
    h.retract(rng.normal(0, 0.05, h._ntot))
    second = m.marginalCovariances()
    assert _stats(m)["factorizations"] == 2
    fresh = Marginals(g, h.values(), o)
    want = fresh.marginalCovariances()
    for k in o:
        assert np.array_equal(second[k], want[k]), k
    assert any(not np.array_equal(first[k], second[k]) for k in o)
    # the other ways a factorization goes stale: set_values, linearize, solve, the per-column route
    for touch in (lambda: h.set_values(h.values()), h.linearize, lambda: (h.linearize(), h.solve(0.5)), lambda: m.marginalCovariance(0)):
        n = _stats(m)["factorizations"]
        touch()
        again = m.marginalCovariances([4])[4]
        assert _stats(m)["factorizations"] == n + 1 and np.array_equal(again, want[4])
    m.close()
    fresh.close()


def test_robust_noise_graph():
    g, v, o = cases.SMALL["robust"]()
    m, _ = _three_ways("robust", g, v, o, list(o))
    m.close()


def test_the_three_refusals():
    """smart factors, a handle finalized under PCG, world_size > 1: LMGPU_INVALID with one message each, nothing written"""
    import smart_cases as sc
    g, v, o = cases.pose2_chain(4)
    pcg = LevenbergMarquardtParams()
    pcg.linearSolverType, pcg.iterativeParams = "ITERATIVE", PCGSolverParameters(BlockJacobiPreconditionerParameters())
    sg, sv, so, _ = sc.package(sc.ring_scene([3, 4, 2], seed=3))
    handles = [(LevenbergMarquardtOptimizer(sg, sv, so, LevenbergMarquardtParams()), b"smart projection factors"),
               (LevenbergMarquardtOptimizer(g, v, o, pcg), b"finalized under PCG"),
               (LevenbergMarquardtOptimizer(g, v, o, LevenbergMarquardtParams(), world_size=2, finalize_only=True), b"one GPU")]
    for h, msg in handles:
        out = np.full(81, 7.0)
        slots = np.zeros(1, dtype=np.int32)
        assert h.lib.lmgpu_marginal_covariances(h._h, 1, slots.ctypes.data_as(_I), out.ctypes.data_as(_D)) == _lib.LMGPU_INVALID
        assert msg in h.lib.lmgpu_last_error(h._h), h.lib.lmgpu_last_error(h._h)
        assert h.lib.lmgpu_marginals_factor(h._h) == _lib.LMGPU_INVALID and msg in h.lib.lmgpu_last_error(h._h)
        assert (out == 7.0).all()
        h.close()


def test_alone_inside_all_and_twice_are_the_same_bits():
    g, v, o = cases.sphere_head_natural()
    ks = sorted(int(x) for x in o)
    m = Marginals(g, v, o)
    everything = m.marginalCovariances()
    for k in (ks[0], ks[123], ks[-1]):
        alone = m.marginalCovariances([k])[k]
        twice = m.marginalCovariances([k])[k]
        mixed = m.marginalCovariances([ks[7], k, ks[200]])[k]
        assert np.array_equal(alone, everything[k]) and np.array_equal(twice, alone) and np.array_equal(mixed, alone), k
    assert _stats(m)["factorizations"] == 1
    # path_solves: marginalCovariance / marginalInformation answer from the same factorization
    mp = Marginals(g, v, o, path_solves=True)
    assert np.array_equal(mp.marginalCovariance(ks[123]), everything[ks[123]])
    assert np.allclose(mp.marginalInformation(ks[123]) @ everything[ks[123]], np.eye(6), atol=1e-9)
    assert _stats(mp)["factorizations"] == 1
    m.close()
    mp.close()
