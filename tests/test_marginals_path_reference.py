"""The marginal path walk without a device: the long-double restatement (tests/marginals_path_restatement.py) against
the dense inverse on Bayes trees built in numpy from random SPD information matrices with prescribed elimination trees, and the host
tables of finalize -- paths and path offsets -- on structure-only (device = -1) handles of the shapes of tests/marginals_path_cases.py."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import marginals_path_cases as cases
import marginals_path_restatement as mr
from gtsam_personal_amd import LevenbergMarquardtOptimizer, LevenbergMarquardtParams, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, tree = [(frontal slots, parent, separator slots)] children first, dims per slot)
TREES = [
    ("single", [([0], -1, [])], [3]),
    ("root_pair", [([0, 1], -1, [])], [3, 2]),
    ("chain", [([0], 1, [1]), ([1], 2, [2]), ([2], 3, [3]), ([3], -1, [])], [3, 3, 3, 3]),
    ("chain_skip", [([0], 1, [1, 3]), ([1], 2, [2, 3]), ([2], 3, [3]), ([3], -1, [])], [6, 3, 6, 2]),
    ("forest", [([0], 1, [1]), ([1], -1, []), ([2], 3, [3]), ([3, 4], -1, [])], [3, 2, 3, 2, 3]),
    ("wide_frontal", [([0], 2, [2, 4]), ([1], 2, [3]), ([2, 3, 4], 3, [5]), ([5, 6], -1, [])], [2, 3, 3, 2, 6, 9, 5]),
    ("star", [([0], 4, [4]), ([1], 4, [4, 5]), ([2], 4, [5]), ([3], 4, [4]), ([4, 5], -1, [])], [3, 3, 3, 3, 9, 9]),
    ("deep_mixed", [([0], 1, [1, 2]), ([1], 2, [2, 4]), ([2, 3], 3, [4, 5]), ([4], 4, [5]), ([5], -1, [])], [9, 5, 3, 2, 6, 3]),
]


@pytest.mark.parametrize("name,tree,dims", TREES, ids=[t[0] for t in TREES])
def test_restatement_equals_dense_inverse(name, tree, dims):
    cliques, info, off = mr.random_bayes_tree(tree, dims, seed=len(name))
    sigma = mr.inverse_ld(info)
    for slot in range(len(dims)):
        want = sigma[off[slot]:off[slot + 1], off[slot]:off[slot + 1]]
        got = mr.path_marginal(cliques, dims, slot)
        rel = float(np.linalg.norm((got - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
        assert rel <= 1e-12, (name, slot, rel)


@pytest.mark.parametrize("name,tree,dims", TREES, ids=[t[0] for t in TREES])
def test_restatement_offsets_invariant(name, tree, dims):
    """the compact work vector: a root starts at 0, a child behind its parent's frontals, and every separator scalar lies inside the
    frontal range of an ancestor"""
    cliques, _, _ = mr.random_bayes_tree(tree, dims, seed=1)
    poff, spos = mr.path_offsets(cliques, dims)
    nf = [sum(dims[s] for s in sl[:nfv]) for sl, nfv, _, _ in cliques]
    for c, (_, _, par, _) in enumerate(cliques):
        assert poff[c] == (0 if par < 0 else poff[par] + nf[par])
        ranges = []
        a = par
        while a >= 0:
            ranges.append((poff[a], poff[a] + nf[a]))
            a = cliques[a][2]
        for p in spos[c]:
            assert any(lo <= p < hi for lo, hi in ranges), (name, c, p)
            assert p < poff[c]


def _structure_handle(builder):
    graph, values, ordering = builder()
    return LevenbergMarquardtOptimizer(graph, values, ordering, LevenbergMarquardtParams(), device=-1), ordering


@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_paths_equal_parent_chain_on_structure_handles(name):
    """lmgpu_marginals_path on a device = -1 handle = the parent chain read through lmgpu_front_info, from the front that lists the slot
    among its frontal variables"""
    opt, ordering = _structure_handle(cases.SMALL[name])
    nfr = opt.num_fronts()
    frontal_in = {}
    for f in range(nfr):
        fi = opt.front_info(f)
        keys, _ = opt.front(f, numeric=False)
        for k in keys[:fi["n_frontal_keys"]]:
            frontal_in[k] = f
    assert sorted(frontal_in) == sorted(int(k) for k in ordering)
    for k in ordering:
        slot = opt._slot[int(k)]
        want, f = [], frontal_in[int(k)]
        while f >= 0:
            want.append(f)
            f = opt.front_info(f)["parent"]
        buf = np.full(len(want) + 2, -7, dtype=np.int32)
        n = opt.lib.lmgpu_marginals_path(opt._h, slot, buf.ctypes.data_as(ct.POINTER(ct.c_int32)), len(buf))
        assert n == len(want) and buf[:n].tolist() == want and (buf[n:] == -7).all(), (name, k)
        # a short buffer: the length is still returned, nothing is written past cap
        small = np.full(2, -7, dtype=np.int32)
        assert opt.lib.lmgpu_marginals_path(opt._h, slot, small.ctypes.data_as(ct.POINTER(ct.c_int32)), 1) == n
        assert small[0] == want[0] and small[1] == -7
    assert opt.lib.lmgpu_marginals_path(opt._h, len(ordering), None, 0) == -1
    assert opt.lib.lmgpu_marginals_path(opt._h, -1, None, 0) == -1
    opt.close()


@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_path_offset_invariant_on_structure_handles(name):
    """finalize's tables: poff[root] = 0, poff[child] = poff[parent] + nf[parent]; every separator scalar of a front maps into the frontal
    range of an ancestor, and exactly to the scalar the restatement's tables name"""
    opt, ordering = _structure_handle(cases.SMALL[name])
    nfr = opt.num_fronts()
    info = [opt.front_info(f) for f in range(nfr)]
    dims = {opt._slot[int(k)]: int(opt._xoff[opt._slot[int(k)] + 1] - opt._xoff[opt._slot[int(k)]]) for k in ordering}
    cliques = []
    for f in range(nfr):
        keys, _ = opt.front(f, numeric=False)
        cliques.append(([opt._slot[k] for k in keys], info[f]["n_frontal_keys"], info[f]["parent"], None))
    want_poff, want_spos = mr.path_offsets(cliques, dims)
    for f in range(nfr):
        ns = info[f]["n"] - info[f]["nf"] - 1
        poff = ct.c_int32(-1)
        spos = np.full(ns + 1, -7, dtype=np.int32)
        got = opt.lib.lmgpu_marginals_front_offsets(opt._h, f, ct.byref(poff), spos.ctypes.data_as(ct.POINTER(ct.c_int32)), ns)
        assert got == ns and spos[ns] == -7
        par = info[f]["parent"]
        assert poff.value == want_poff[f] == (0 if par < 0 else want_poff[par] + info[par]["nf"])
        assert spos[:ns].tolist() == want_spos[f], (name, f)
        for p in spos[:ns]:
            a, ok = par, False
            while a >= 0 and not ok:
                ok = want_poff[a] <= p < want_poff[a] + info[a]["nf"]
                a = info[a]["parent"]
            assert ok, (name, f, int(p))
    assert opt.lib.lmgpu_marginals_front_offsets(opt._h, nfr, None, None, 0) == -1
    opt.close()


def test_structure_handle_refuses_compute_and_counts_nothing():
    """a device = -1 handle answers the structure calls only; the parameters are kept and the statistics start at zero"""
    opt, ordering = _structure_handle(cases.SMALL["chain"])
    out = np.zeros(9)
    slots = np.zeros(1, dtype=np.int32)
    rc = opt.lib.lmgpu_marginal_covariances(opt._h, 1, slots.ctypes.data_as(ct.POINTER(ct.c_int32)), out.ctypes.data_as(ct.POINTER(ct.c_double)))
    assert rc != _lib.LMGPU_OK and (out == 0).all()
    assert opt.lib.lmgpu_marginals_factor(opt._h) != _lib.LMGPU_OK
    assert opt.lib.lmgpu_set_marginals_params(opt._h, 1 << 20, 512) == _lib.LMGPU_OK
    assert opt.lib.lmgpu_set_marginals_params(opt._h, -1, 0) == _lib.LMGPU_INVALID
    assert opt.lib.lmgpu_set_marginals_params(opt._h, 0, 1 << 20) == _lib.LMGPU_INVALID
    st = _lib.lmgpu_marginals_stats()
    assert opt.lib.lmgpu_get_marginals_stats(opt._h, ct.byref(st)) == _lib.LMGPU_OK
    assert (st.launches, st.chunks, st.factorizations, st.vars_lds, st.vars_scratch, st.longest_path) == (0, 0, 0, 0, 0, 0)
    assert st.scratch_bytes == 1 << 20 and st.lds_capacity == 512
    opt.close()


NEW_SYMBOLS = ("lmgpu_marginals_factor", "lmgpu_marginal_covariances", "lmgpu_marginals_path", "lmgpu_marginals_front_offsets",
               "lmgpu_set_marginals_params", "lmgpu_get_marginals_stats")


def test_new_symbols_are_declared():
    """in the header, in the ctypes table and in the integration guide; the library exports them"""
    header = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
        assert name in guide, name
        assert getattr(lib, name) is not None
    # the stats struct of the binding has the header's fields, in order
    m = re.search(r"typedef struct lmgpu_marginals_stats \{(.*?)\} lmgpu_marginals_stats;", header, re.S)
    fields = [f.strip() for part in m.group(1).split(";") for f in re.sub(r"\b(int64_t|int32_t)\b", "", part).split(",") if f.strip()]
    assert fields == [f for f, _ in _lib.lmgpu_marginals_stats._fields_]
    # the old entry points are still there
    assert "lmgpu_marginal_covariance" in _lib.SYMBOLS and "lmgpu_joint_marginal_covariance" in _lib.SYMBOLS


def test_structural_refusals_come_first_on_structure_handles():
    """a handle finalized under PCG and a two-rank handle refuse with their own message before anything else is looked at; the path taps
    of a PCG structure (no fronts) answer -1"""
    from gtsam_personal_amd import BlockJacobiPreconditionerParameters, PCGSolverParameters
    g, v, o = cases.SMALL["chain"]()
    pcg = LevenbergMarquardtParams()
    pcg.linearSolverType, pcg.iterativeParams = "ITERATIVE", PCGSolverParameters(BlockJacobiPreconditionerParameters())
    for opt, msg in ((LevenbergMarquardtOptimizer(g, v, o, pcg, device=-1), b"finalized under PCG"),
                     (LevenbergMarquardtOptimizer(g, v, o, LevenbergMarquardtParams(), device=-1, world_size=2), b"one GPU")):
        out = np.full(9, 7.0)
        slots = np.zeros(1, dtype=np.int32)
        rc = opt.lib.lmgpu_marginal_covariances(opt._h, 1, slots.ctypes.data_as(ct.POINTER(ct.c_int32)), out.ctypes.data_as(ct.POINTER(ct.c_double)))
        assert rc == _lib.LMGPU_INVALID and msg in opt.lib.lmgpu_last_error(opt._h) and (out == 7.0).all()
        assert opt.lib.lmgpu_marginals_factor(opt._h) == _lib.LMGPU_INVALID and msg in opt.lib.lmgpu_last_error(opt._h)
        if msg.startswith(b"finalized"):
            assert opt.lib.lmgpu_marginals_path(opt._h, 0, None, 0) == -1
            assert opt.lib.lmgpu_marginals_front_offsets(opt._h, 0, None, None, 0) == -1
        opt.close()
