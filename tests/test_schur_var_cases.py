"""CPU side of the per-variable Schur walk (schur_var_kernel): that the case of tests/schur_var_cases.py puts a list length one below,
at and one above every boundary the walk has -- counted here from the case's own visibility table -- and that the comparison the GPU
test makes (tests/test_gpu_schur_var_edges.py: the root's [R S d] against the dense extended-precision reference, tolerance
max(16 x oracle floor, 64 n 2.2e-16)) has teeth for the three mistakes such a kernel can make.

The planted mistakes act on the root's assembled matrix U = R^T R (R = the reference's own root factor, extended precision), which is
then factored in float64 and compared like a device result:
  1. the S_v^T d column of one variable dropped             U[v, rhs] += sum_l S_v^T d
  2. the leaf part of one variable not negated              U[v, v | rhs] += 2 sum_l S_v^T [S_v d]
  3. two factors paired across a change of row count        U[v, v | rhs] -= a_3^T [a_3 b_3]: the 3-row factor next to a 2-row one
     (dims_2_3: the only mixed lists)                       in v's list loses its third row to the two k-slots a pair member gets
Measured margins (deviation / tolerance; clean float64 factor: <= 1): see the printed lines; asserted > 100 each."""
import numpy as np
import pytest

import oracle_harness as oh
import schur_cases as sc
import schur_var_cases as svc
from gtsam_personal_amd import LevenbergMarquardtOptimizer
from gtsam_personal_amd.graph import C

FACTOR, EPS, CAP = 16, 2.2e-16, 1e-9  # the rule of tests/test_gpu_schur_edges.py
LAM = 1e-3


def test_constants_are_the_kernels():
    """tests/schur_var_cases.py restates the kernel's constants: its list lengths only sit at boundaries while the two agree"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "gtsam_personal_amd", "csrc", "kernels_schur.hpp")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (SCHUR_V\w+) (\d+)", src, flags=re.M)}
    assert (defs["SCHUR_VU"], defs["SCHUR_VAR_SHORT"], defs["SCHUR_VAR_WAVES"]) == (svc.VU, svc.SHORT, svc.WAVES), defs
    assert "base += 64" in src and svc.FETCH == 64


def _lists(c):
    dims = sc.var_dims(c)
    position = {k: i for i, k in enumerate(c["ordering"])}
    return sc.gather_lists(c["leaves"], dims, position)


def test_var_lists_reaches_every_boundary_of_the_walk():
    c = svc.case()
    pairs, factors = _lists(c)
    want = dict(enumerate(svc.VAR_LENGTHS, start=1))
    want.update({16: 504, 17: 512, 18: 513})
    want[0] = sum(svc.VAR_LENGTHS) + 513
    assert want[0] == 807 == len(c["leaves"])
    for k in range(svc.N_CAM):  # leaf entries of camera k = the leaves that see it; factor entries = their factors on it: equally many
        assert len(pairs[(C(k), C(k))]) == len(pairs[(C(k), sc.RHS)]) == len(factors[C(k)]) == want[k], k
        assert set(pairs[(C(k), C(k))]) == {3} and set(factors[C(k)]) == {2}  # nf = 3: one MFMA per leaf; 2-row factors: pairs
    lengths = set(want.values())
    # the threshold between the two launch shapes
    assert {svc.SHORT - 1, svc.SHORT, svc.SHORT + 1} <= lengths
    assert svc.waves_of(32, 32) == 1 and svc.waves_of(33, 33) == svc.WAVES and svc.waves_of(807, 807) == svc.WAVES
    # entries in flight per round, on the one-wave shape (chunk = the whole list): 8 leaf entries, 16 factor entries
    assert {7, 8, 9, 15, 16, 17} <= lengths
    assert [svc.rounds(n, False) for n in (7, 8, 9)] == [[7], [8], [8, 1]]
    assert [svc.rounds(n, True) for n in (15, 16, 17)] == [[15], [16], [16, 1]]
    # pairing of the 2-row factors: odd and even counts, a single one
    assert {1, 2, 3} <= lengths and [svc.rounds(n, True) for n in (1, 2, 3)] == [[1], [2], [3]]
    # the per-wave chunk of the eight-wave shape: an empty last wave, a short last wave, full waves; factor chunks are even
    assert {33, 39, 40, 41} <= lengths
    assert svc.chunks(33, 8, False) == [5, 5, 5, 5, 5, 5, 3, 0] and svc.chunks(33, 8, True) == [6, 6, 6, 6, 6, 3, 0, 0]
    assert svc.chunks(39, 8, False) == [5] * 7 + [4] and svc.chunks(40, 8, False) == [5] * 8 and svc.chunks(41, 8, False) == [6] * 6 + [5, 0]
    assert svc.chunks(39, 8, True) == [6] * 6 + [3, 0] and svc.chunks(40, 8, True) == [6] * 6 + [4, 0] and svc.chunks(41, 8, True) == [6] * 6 + [5, 0]
    # the 64-entry fetch inside a wave's chunk: chunks of 63, 64 and 65 leaf entries; factor chunks of 64 (full and short last) and 66
    assert svc.chunks(504, 8, False) == [63] * 8 and svc.chunks(512, 8, False) == [64] * 8 and svc.chunks(513, 8, False) == [65] * 7 + [58]
    assert svc.chunks(504, 8, True) == [64] * 7 + [56] and svc.chunks(512, 8, True) == [64] * 8 and svc.chunks(513, 8, True) == [66] * 7 + [51]
    assert svc.rounds(63, False) == [8] * 7 + [7] and svc.rounds(64, False) == [8] * 8 and svc.rounds(65, False) == [8] * 8 + [1]
    assert svc.rounds(64, True) == [16] * 4 and svc.rounds(66, True) == [16] * 4 + [2]
    assert svc.chunks(807, 8, False) == [101] * 7 + [100] and svc.rounds(101, False) == [8] * 8 + [8] * 4 + [5]  # camera 0: a second fetch
    # off-diagonal lists stay pair blocks: camera 0 with each, and the three long ones among the nested cameras
    off = {k: len(v) for k, v in pairs.items() if k[0] != k[1] and k[1] != sc.RHS}
    assert off == {**{(C(0), C(k)): want[k] for k in range(1, svc.N_CAM)}, (C(16), C(17)): 504, (C(16), C(18)): 504, (C(17), C(18)): 512}
    # the lists interleave in the pool: the points of camera 16 are not a contiguous run of leaves
    idx = [j for j, vis in enumerate(c["visibility"]) if 16 in vis]
    assert len(idx) == 504 and idx[-1] - idx[0] > 700


def test_var_lists_structure_one_write_mode_root():
    c = svc.case()
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=-1)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert len(infos) == 808 and sum(f["cls"] == 1 for f in infos) == 1
    root = infos[-1]
    assert (root["cls"], root["nf"], root["n"], root["parent"]) == (1, 9 * svc.N_CAM, 9 * svc.N_CAM + 1, -1)
    dims = sc.var_dims(c)
    assert all(f["cls"] == 0 and f["parent"] == len(infos) - 1 for f in infos[:-1])  # all children are gather leaves: write mode
    assert max(sc.leaf_n(lf, dims) for lf in c["leaves"]) == 3 + 4 * 9 + 1


def test_var_lists_reference_residual_and_oracle_floor():
    fl = svc.oracle_floor()
    print(f"{svc.NAME}: reference residual {fl['residual']:.2e}; oracle vs reference [R S d] {fl['rsd']:.2e}, delta {fl['delta']:.2e}")
    assert fl["residual"] < 1e-17
    assert FACTOR * fl["rsd"] <= CAP and FACTOR * fl["delta"] <= CAP


# ------------------------------------------------------------------------------------------------ planted mistakes
class _Root:
    """the reference's root front of a case at (LAM, identity damping): R (extended precision), U = R^T R, the leaves' [R S d]"""

    def __init__(self, c):
        orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
        orc.linearize()
        self.jac = [orc.jacobian(g) for g in range(c["graph"].size())]
        rc, _, _, _ = orc.solve(LAM, False)
        assert rc == 0
        self.fronts = [(keys, nfk) for keys, nfk, _, _ in orc.cliques()]
        self.dims = sc.var_dims(c)
        self.ref = sc.reference(c, self.jac, self.fronts, LAM, False)
        self.keys, nfk = self.fronts[-1]
        assert nfk == len(self.keys)  # the root: every key frontal
        self.R = self.ref.front(len(self.fronts) - 1)
        self.n = self.R.shape[0]
        assert self.R.shape == (self.n, self.n + 1)
        self.U = self.R.T @ self.R
        self.col, o = {}, 0
        for k in self.keys:
            self.col[k] = np.arange(o, o + self.dims[k])
            o += self.dims[k]

    def leaf_blocks(self, v):
        """(S_v, d) of every leaf front that sees v, from the reference"""
        for i, (keys, nfk) in enumerate(self.fronts[:-1]):
            if v in keys[nfk:]:
                X = self.ref.front(i)
                o = sum(self.dims[k] for k in keys[:keys.index(v)])
                yield X[:, o:o + self.dims[v]], X[:, -1]

    def deviation(self, U):
        """a float64 Cholesky of U's leading block (+ the rhs column), compared with the reference's root like a device result"""
        n = self.n
        H = np.triu(U.astype(np.float64))
        H = H + np.triu(H, 1).T
        Lc = np.linalg.cholesky(H[:n, :n])
        Rd = np.hstack([Lc.T, np.linalg.solve(Lc, H[:n, n])[:, None]])
        return float(np.abs(Rd.astype(np.longdouble) - self.R).max() / np.abs(self.R).max())


def _add(U, rows, cols, block):
    U[np.ix_(rows, cols)] += block
    if rows is cols:
        return
    U[np.ix_(cols, rows)] += block.T


def test_planted_mistakes_miss_the_tolerance_by_a_wide_factor():
    c, fl = svc.case(), svc.oracle_floor()
    root = _Root(c)
    n = root.n
    tol = max(FACTOR * fl["rsd"], 64 * (n + 1) * EPS)
    clean = root.deviation(root.U)
    print(f"{svc.NAME}: clean float64 factor of the root {clean:.2e}, tolerance {tol:.2e}")
    assert clean <= tol
    rhs = np.array([n])
    margins = {1: [], 2: []}
    for k in range(svc.N_CAM):  # every camera in turn: list lengths 1 .. 807
        v = C(k)
        SS = sum(S.T @ S for S, _ in root.leaf_blocks(v))
        Sd = sum(S.T @ d for S, d in root.leaf_blocks(v))[:, None]
        U1 = root.U.copy()
        _add(U1, root.col[v], rhs, Sd)
        margins[1].append(root.deviation(U1) / tol)
        U2 = root.U.copy()
        U2[np.ix_(root.col[v], root.col[v])] += 2 * SS
        _add(U2, root.col[v], rhs, 2 * Sd)
        margins[2].append(root.deviation(U2) / tol)
    for m, what in ((1, "S_v^T d dropped"), (2, "leaf part not negated")):
        print(f"{svc.NAME}: {what}: deviation / tolerance over the cameras: least {min(margins[m]):.2e}, largest {max(margins[m]):.2e}")
        assert min(margins[m]) > 100, (m, margins[m])


def test_planted_pairing_across_a_change_of_row_count_misses_the_tolerance():
    name = "dims_2_3"
    c, fl = sc.case(name), sc.oracle_floor(name)
    root = _Root(c)
    n = root.n
    tol = max(FACTOR * fl["rsd"], 64 * (n + 1) * EPS)
    clean = root.deviation(root.U)
    assert clean <= tol, (clean, tol)
    _, factors = _lists(c)
    fk = c["graph"].factor_keys_in_graph_order()
    margins = []
    for v, rows in factors.items():
        leaves_of_v = [lf for lf in c["leaves"] if any(k == v for k, _ in lf[2])]
        assert [r for lf in leaves_of_v for k, r in lf[2] if k == v] == rows
        for q in range(len(rows) - 1):
            if {rows[q], rows[q + 1]} != {2, 3}:
                continue
            leaf_key = leaves_of_v[q if rows[q] == 3 else q + 1][0]  # the 3-row member of the would-be pair
            g, = [i for i, keys in enumerate(fk) if set(keys) == {leaf_key, v}]
            Ab = root.jac[g]
            assert Ab.shape[0] == 3
            o = sum(root.dims[k] for k in fk[g][:list(fk[g]).index(v)])
            a3 = Ab[2, o:o + root.dims[v]].astype(np.longdouble)[:, None]
            b3 = np.longdouble(Ab[2, -1])
            Ud = root.U.copy()
            Ud[np.ix_(root.col[v], root.col[v])] -= a3 @ a3.T
            _add(Ud, root.col[v], np.array([n]), -a3 * b3)
            margins.append(root.deviation(Ud) / tol)
    assert margins, "dims_2_3 has no list in which a 2-row and a 3-row factor are neighbours"
    print(f"{name}: third row lost to a pair, {len(margins)} places: deviation / tolerance least {min(margins):.2e}, largest {max(margins):.2e} "
          f"(clean {clean:.2e}, tolerance {tol:.2e})")
    assert min(margins) > 100, margins
