"""front_tail_kernel (the end of a dense front in one workgroup: update with the last full panel on the matrix cores, partial Cholesky
of the last nft < 64 frontal columns in registers, the update matrix behind them, the four 16 x 16 inverses) at its shape edges, on
dense fronts whose schedule ends in a DENSE_TAIL record.

Shapes.  m = n - r0 is the width of the block the kernel owns (last partial panel + separator + right-hand side, <= 48), nft = nf - r0
its frontal columns, `panels` the finished 256-row panels in front of it (1: panel_dataflow_kernel, then the tail; 2: a fused step
between them; 4: a chained launch of three steps between them).  The fronts come from tests/dense_front_cases.py (hub ordering), not
from the Cal3Bundler / Pose3 residue classes of tests/leaf_group_cases.py: Pose2 = 3 and Point2 = 2 columns reach EVERY width,
nf = 3 a + 2 b with b <= 2, so m = 16, 32 and 48 need no second separator variable.  The kernel sees scalars only.
  root[panels, m]      a root, n = nf + 1, nf = 256 panels + m - 1, so nft = m - 1:
                       panels = 1 and 2: m = 2, 6, 16, 17, 18, 32, 33, 34, 41, 48
                       panels = 4: m = 2, 3, 4, 6, 17, 18, 34 (nft = 1, 2, 3, 5, 16, 17, 33)
  sep[panels, nft, ns] a front with ns separator scalars under an LDS root, n = nf + ns + 1, nf = 256 panels + nft, m = nft + ns + 1:
                       panels = 1: nft = 1 (the pivot-exponent test reads the previous diagonal from A), 2, 3, 4, 5 (the four-pivot
                       group boundary: the group that straddles nft treats 3, 2, 1, 0, 3 rows as unit pivots), 13, 16, 17 (the 16-row
                       strip boundary), 20, 31, 33 (two strips), with m = 8, 48, 17, 33, 17, 41, 34, 32, 33, 48, 41, 48 (ns >= 6: the
                       parent needs two poses); panels = 2: nft = 3, m = 16; panels = 4: (nft, ns) = (1, 6), (3, 12), (5, 35),
                       (17, 15), (33, 14)
Which (variable type, count) gives which width: composition(name) = dense_front_cases.split_width of the frontal and the separator
width, (Pose2, a) + (Point2, b) with 3 a + 2 b = width and b = (0, 2, 1)[width % 3].  Frontal part: panels = 1: m = 2: (85, 1);
6: (87, 0); 16: (89, 2); 17: (90, 1); 18: (91, 0); 32: (95, 1); 33: (96, 0); 34: (95, 2); 41: (98, 1); 48: (101, 0).  panels = 2:
(171, 0), (171, 2), (175, 1), (176, 0), (175, 2), (181, 0), (180, 2), (181, 1), (184, 0), (185, 2).  panels = 4, roots: (341, 1), (342, 0),
(341, 2), (343, 0), (346, 1), (347, 0), (351, 2).  Separators: ns = 6: (2, 0); 9: (3, 0); 12: (4, 0); 14: (4, 1); 15: (5, 0); 20: (6, 1);
27: (9, 0); 29: (9, 1); 35: (11, 1); 46: (14, 2).

Every case: the planner's records (lmgpu_selftest_dense_schedule) end in DENSE_TAIL -- and those of m = 49 do not --, the fronts are
the intended ones (front_info), and then what tests/test_gpu_dense_front_edges.py does, at ITS tolerance (max(16 x the
oracle-vs-reference floor, 64 n 2.2e-16) per front, n the widest front for delta): two passes (lambda = 1e-6 identity, then 1e-2
diagonal over the previous R), every front's [R S d] and delta against the blocked extended-precision reference built from the device's
Jacobians, the oracle comparison of _check_solve alongside, the same solve again bitwise equal with the expected launch counters.  Then
the same case on the test library under LMGPU_TAIL_SCALAR=1 (front_tail_scalar_kernel, the previous form): against the reference at the
same tolerance, and against the default form at the same tolerance.

The inverses.  Only a front of nf > BSS_MAX_NF = 1024 rows is back-substituted by the kernel that multiplies with the inv16 blocks the
tail leaves (hbm_backsolve_wide_kernel; do_backsub in csrc/lmgpu.hip); the fronts with one or two panels take
hbm_backsolve_blocks_kernel, which inverts its own diagonal blocks, so their delta says nothing about the identity tile of
potrf48_partial_wave and its masks.  The panels = 4 cases are there for that: nft on both sides of the four-pivot and the 16-row
boundaries, roots and fronts with a separator; their delta is the check of the inverses.  The launch counters do not tell the two
back-substitutions apart, so the test asserts the condition do_backsub decides by (nf > 1024, one dense front).  A reference of
1 058 columns takes 2.5 s, so these cases take the first pass only (the floor is then measured on that pass alone, which can only
tighten the tolerance); its repeated solve, bitwise equal, runs over the inv16 blocks the first one left.

Two failure cases: a root whose last variable is a pose whose only factor (to the hub) has sigma = 1e200, so that its diagonal block
is exactly zero, is indeterminate at lambda = 0 with the same failed slot in both forms (and the oracle's verdict); a NaN prior
measurement on the last variable (its Jacobian is finite, its right-hand side NaN): in both forms R and S of the root stay finite, d
of the tail's rows is NaN, and the back-substitution reports the NaN as an indeterminate system with the same failed slot, like the
reference and the oracle.

Measured on an MI355X (deviation from the reference = max|X - X_ref| / max|X_ref| over the fronts, relative 2-norm for delta; worst of
the two passes; last figure but one: delta of the default form against the scalar form).  Every repeated solve was bitwise equal and
every launch count the expected one; both failure cases gave the same outcome in both forms (indeterminate, same slot):
                     default form          scalar form           default vs   tolerance
    case             [R S d]  delta        [R S d]  delta        scalar       (front 0 / delta)
    root[1,2]        1.3e-15  5.4e-15   1.3e-15  5.4e-15   4.9e-17   3.6e-12 / 3.6e-12
    root[1,6]        1.5e-15  7.7e-15   1.5e-15  8.0e-15   8.4e-14   3.7e-12 / 3.7e-12
    root[1,16]       1.7e-15  1.4e-14   1.7e-15  1.4e-14   1.0e-13   3.8e-12 / 3.8e-12
    root[1,17]       1.5e-15  1.4e-14   1.5e-15  1.4e-14   9.0e-14   3.8e-12 / 3.8e-12
    root[1,18]       8.1e-16  1.3e-14   8.1e-16  1.2e-14   1.3e-13   3.9e-12 / 3.9e-12
    root[1,32]       2.5e-15  1.9e-14   2.5e-15  1.9e-14   8.0e-14   4.1e-12 / 4.1e-12
    root[1,33]       1.5e-15  2.0e-14   1.7e-15  2.0e-14   1.1e-13   4.1e-12 / 4.1e-12
    root[1,34]       1.1e-15  1.8e-14   1.1e-15  1.8e-14   4.4e-14   4.1e-12 / 4.1e-12
    root[1,41]       6.6e-16  1.9e-14   6.6e-16  2.0e-14   1.5e-13   4.2e-12 / 4.2e-12
    root[1,48]       5.2e-16  2.8e-14   5.2e-16  2.8e-14   6.9e-14   4.3e-12 / 4.3e-12
    root[2,2]        8.4e-16  1.3e-14   8.4e-16  1.3e-14   1.3e-14   7.2e-12 / 7.2e-12
    root[2,6]        8.5e-16  1.3e-14   8.5e-16  1.3e-14   5.3e-14   7.3e-12 / 7.3e-12
    root[2,16]       2.9e-15  3.1e-14   2.9e-15  3.1e-14   5.9e-14   7.4e-12 / 7.4e-12
    root[2,17]       1.4e-15  1.4e-14   1.4e-15  1.5e-14   8.8e-14   7.5e-12 / 7.5e-12
    root[2,18]       1.6e-15  2.3e-14   1.6e-15  2.3e-14   6.9e-14   7.5e-12 / 7.5e-12
    root[2,32]       1.6e-15  2.5e-14   1.6e-15  2.5e-14   1.0e-13   7.7e-12 / 7.7e-12
    root[2,33]       1.1e-15  3.5e-14   1.1e-15  3.5e-14   4.3e-14   7.7e-12 / 7.7e-12
    root[2,34]       7.7e-16  7.4e-15   7.7e-16  7.0e-15   5.2e-14   7.7e-12 / 7.7e-12
    root[2,41]       2.1e-15  1.6e-14   2.1e-15  1.6e-14   6.8e-14   7.8e-12 / 7.8e-12
    root[2,48]       2.4e-15  2.1e-14   2.4e-15  2.2e-14   8.5e-14   7.9e-12 / 7.9e-12
    root[4,2]        7.4e-16  1.6e-14   7.4e-16  1.6e-14   9.9e-17   1.4e-11 / 1.4e-11
    root[4,3]        7.0e-16  7.1e-15   7.0e-16  7.1e-15   8.5e-17   1.5e-11 / 1.5e-11
    root[4,4]        1.9e-15  7.0e-15   1.9e-15  7.0e-15   7.6e-17   1.5e-11 / 1.5e-11
    root[4,6]        2.6e-15  1.6e-14   2.6e-15  1.6e-14   1.4e-16   1.5e-11 / 1.5e-11
    root[4,17]       1.9e-15  7.0e-15   1.9e-15  6.9e-15   2.8e-16   1.5e-11 / 1.5e-11
    root[4,18]       1.2e-15  1.2e-14   1.2e-15  1.2e-14   3.2e-16   1.5e-11 / 1.5e-11
    root[4,34]       3.5e-16  1.6e-14   3.5e-16  1.6e-14   2.9e-16   1.5e-11 / 1.5e-11
    sep[1,1,6]       7.1e-16  1.5e-14   7.1e-16  1.5e-14   1.7e-14   3.7e-12 / 3.7e-12
    sep[1,1,46]      1.1e-15  1.5e-14   1.1e-15  1.5e-14   9.8e-14   4.3e-12 / 4.3e-12
    sep[1,2,14]      6.2e-16  2.1e-14   6.1e-16  2.1e-14   2.9e-14   3.8e-12 / 3.8e-12
    sep[1,3,29]      8.6e-16  1.3e-14   8.6e-16  1.3e-14   5.5e-14   4.1e-12 / 4.1e-12
    sep[1,4,12]      8.0e-16  1.0e-14   8.0e-16  8.0e-15   1.5e-13   3.8e-12 / 3.8e-12
    sep[1,5,35]      8.6e-16  3.5e-14   8.6e-16  3.5e-14   6.4e-14   4.2e-12 / 4.2e-12
    sep[1,13,20]     9.1e-16  2.4e-14   9.1e-16  2.3e-14   4.3e-14   4.1e-12 / 4.1e-12
    sep[1,16,15]     1.5e-15  2.6e-14   1.5e-15  2.7e-14   4.9e-14   4.1e-12 / 4.1e-12
    sep[1,17,15]     1.6e-15  1.6e-14   1.6e-15  1.7e-14   7.5e-14   4.1e-12 / 4.1e-12
    sep[1,20,27]     7.4e-16  9.5e-15   7.4e-16  9.6e-15   7.1e-14   4.3e-12 / 4.3e-12
    sep[1,31,9]      1.5e-15  3.1e-14   1.5e-15  3.2e-14   7.7e-14   4.2e-12 / 4.2e-12
    sep[1,33,14]     1.9e-15  6.7e-15   1.9e-15  6.9e-15   1.2e-13   4.3e-12 / 4.3e-12
    sep[2,3,12]      1.2e-15  1.1e-14   1.2e-15  1.2e-14   5.2e-14   7.4e-12 / 7.4e-12
    sep[4,1,6]       1.2e-15  1.3e-14   1.2e-15  1.3e-14   1.2e-16   1.5e-11 / 1.5e-11
    sep[4,3,12]      2.1e-15  1.0e-14   2.1e-15  1.0e-14   2.4e-16   1.5e-11 / 1.5e-11
    sep[4,5,35]      1.8e-15  1.8e-14   1.8e-15  1.8e-14   3.0e-16   1.5e-11 / 1.5e-11
    sep[4,17,15]     1.9e-15  2.1e-14   1.9e-15  2.1e-14   4.5e-16   1.5e-11 / 1.5e-11
    sep[4,33,14]     2.2e-15  6.9e-15   2.2e-15  6.9e-15   2.1e-16   1.5e-11 / 1.5e-11
The module takes 80 s, most of it the references of the twelve fronts of more than 1024 rows (4 - 5 s each).
"""
import ctypes as ct
import functools
import hashlib

import numpy as np
import pytest

import dense_front_cases as dc
import schur_cases as sc
from gtsam_personal_amd import _lib
from gtsam_personal_amd.graph import X
from test_gpu_parity import _check_linearize, _check_solve, _pair

pytestmark = pytest.mark.gpu

DENSE_TAIL = 6  # dense_schedule.hpp: DenseKind
BSS_MAX_NF = 1024  # kernels_dense.hpp: a dense front of more rows is back-substituted by hbm_backsolve_wide_kernel, which reads inv16
WIDTHS = (2, 6, 16, 17, 18, 32, 33, 34, 41, 48)
ROOTS = [(1, m) for m in WIDTHS] + [(2, m) for m in WIDTHS]
SEPS = [(1, 1, 6), (1, 1, 46), (1, 2, 14), (1, 3, 29), (1, 4, 12), (1, 5, 35), (1, 13, 20), (1, 16, 15), (1, 17, 15), (1, 20, 27),
        (1, 31, 9), (1, 33, 14), (2, 3, 12)]
# four finished panels: nf = 1024 + nft > BSS_MAX_NF, the back-substitution multiplies with the tail's inv16 blocks
WIDE_ROOTS = [(4, m) for m in (2, 3, 4, 6, 17, 18, 34)]  # nft = 1, 2, 3, 5, 16, 17, 33
WIDE_SEPS = [(4, 1, 6), (4, 3, 12), (4, 5, 35), (4, 17, 15), (4, 33, 14)]
NAMES = [f"root[{p},{m}]" for p, m in ROOTS + WIDE_ROOTS] + [f"sep[{p},{nft},{ns}]" for p, nft, ns in SEPS + WIDE_SEPS]


@functools.lru_cache(maxsize=None)
def case(name):
    kind, args = name.split("[")
    args = [int(a) for a in args.rstrip("]").split(",")]
    seed = 900 + NAMES.index(name)
    if kind == "root":
        panels, m = args
        nf = 256 * panels + m - 1
        c = dc.root_case(nf, seed, None)
    else:
        panels, nft, ns = args
        c = dc.separator_case(256 * panels + nft, ns, seed, None)
    c["launches"] = dc.per_front_launches(c["fronts"])
    c["launches"]["panel_work"] = True
    c["passes"] = dc.PASSES if panels < 4 else dc.PASSES[:1]  # (a reference of 1 058 columns takes 2.5 s: the wide cases take one pass)
    return c


def composition(name):
    """(variable type, count) of the dense front of a case: its frontal part and, for a sep case, its separator"""
    kind, args = name.split("[")
    args = [int(a) for a in args.rstrip("]").split(",")]
    nf = 256 * args[0] + (args[1] - 1 if kind == "root" else args[1])
    fp, fq = dc.split_width(nf)
    out = {"frontal": (("Pose2", fp), ("Point2", fq))}
    if kind == "sep":
        sp, sq = dc.split_width(args[2])
        out["separator"] = (("Pose2", sp), ("Point2", sq))
    return out


def schedule(n, nf):
    cap = 4096
    buf = (ct.c_int32 * (4 * cap))()
    count = _lib.load().lmgpu_selftest_dense_schedule(n, nf, 0, 0, cap, buf)
    assert count > 0
    return [tuple(buf[4 * k:4 * k + 4]) for k in range(count)]


def test_m_49_is_not_a_tail():
    assert schedule(256 + 49, 256 + 48)[-1][0] != DENSE_TAIL
    assert schedule(256 + 48, 256 + 47)[-1][0] == DENSE_TAIL


_refs = {}


def _reference(key, c, jac, fronts, lam, diagonal):
    """once per linearization: the default and the scalar form of a case see the same Jacobians"""
    digest = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in jac)).hexdigest()
    if (key, digest) not in _refs:
        _refs[(key, digest)] = sc.reference(c, jac, fronts, lam, diagonal, block=dc.BLOCK)
    return _refs[(key, digest)]


def _solve_passes(name, c, fl, check_counts):
    """the two passes of test_gpu_dense_front_edges._run; returns [(rsd per front, packed delta by key)] per pass"""
    opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"]) for f in infos] == c["fronts"], infos
    fronts = [(opt.front(i, numeric=False)[0], infos[i]["n_frontal_keys"]) for i in range(len(infos))]
    tol_rsd, tol_d = dc.tolerances(fl, [f["n"] for f in infos])
    out = []
    for p, (lam, diagonal) in enumerate(c["passes"]):
        _check_linearize(opt, orc, c["graph"])
        lin = opt.linear_graph()
        jac = [lin.at(g).augmentedJacobian() for g in range(c["graph"].size())]
        ref = _reference((name.split(" ")[0], p), c, jac, fronts, lam, diagonal)
        assert ref.residual < 1e-17
        dk = _check_solve(opt, orc, lam, diagonal)
        rsd = [opt.front(i)[1] for i in range(len(infos))]
        per_front, dd = sc.deviations(ref, lambda i: rsd[i], dk)
        print(f"{name} pass {p}: [R S d] " + ", ".join(f"{d:.2e}" for d in per_front) + " (tolerance "
              + ", ".join(f"{t:.2e}" for t in tol_rsd) + f"), delta {dd:.2e} (tolerance {tol_d:.2e})")
        for i, dev in enumerate(per_front):
            assert dev <= tol_rsd[i], (name, p, i, infos[i], dev)
        assert dd <= tol_d, (name, p, dd)
        opt.set_kernel_timing(1)  # the same solve again, counted: bitwise
        dk2, _, _, _ = opt.solve(lam, diagonal)
        kt = opt.kernel_times()
        opt.set_kernel_timing(False)
        assert all(np.array_equal(dk[k], dk2[k]) for k in dk)
        assert all(np.array_equal(rsd[i], opt.front(i)[1]) for i in range(len(infos)))
        if check_counts:
            seen = dict(panel=kt["panel"]["launches"], syrk=kt["syrk"]["launches"], chain=kt["chain"]["launches"], panel_work=kt["panel"]["work"] > 0)
            assert seen == c["launches"], (name, seen, c["launches"])
        assert kt["backsub_hbm"]["launches"] >= 1
        out.append((rsd, dk))
        if p == 0 and len(c["passes"]) > 1:
            opt.retract()
            orc.retract({k: dk[k] for k in dk})
    opt.close()
    return out, (tol_rsd, tol_d)


@pytest.mark.parametrize("name", NAMES)
def test_tail_against_reference_and_scalar_form(request, monkeypatch, name):
    c = case(name)
    dense = [f for f in c["fronts"] if f["cls"] == 1]
    assert len(dense) == 1
    n, nf = dense[0]["n"], dense[0]["nf"]
    records = schedule(n, nf)
    assert records[-1][0] == DENSE_TAIL, records
    r0 = 256 * (records[-1][1] + 1)
    assert 2 <= n - r0 <= 48 and 1 <= nf - r0 < n - r0
    # the back-substitution that consumes the tail's inv16 blocks: hbm_backsolve_wide_kernel, taken by do_backsub for a front of
    # nf > BSS_MAX_NF whose factorisation was the last to write inv16 (the only dense front of the case); smaller fronts take
    # hbm_backsolve_blocks_kernel, which inverts its own diagonal blocks.  The launch counters do not tell the two apart.
    assert (nf > BSS_MAX_NF) == name.split("[")[1].startswith("4,"), (name, nf)
    fl = sc.floor_of(c, c["passes"], dc.BLOCK)  # (one pass for most wide cases: the floor, and with it the tolerance, can only get smaller)
    assert dc.FACTOR * fl["rsd"] <= dc.CAP and dc.FACTOR * fl["delta"] <= dc.CAP, fl
    default, (tol_rsd, tol_d) = _solve_passes(name, c, fl, True)
    request.getfixturevalue("dev_switches")
    monkeypatch.setenv("LMGPU_TAIL_SCALAR", "1")
    scalar, _ = _solve_passes(name + " scalar", c, fl, True)
    for p in range(len(c["passes"])):
        for i, (a, b) in enumerate(zip(default[p][0], scalar[p][0])):
            dev = float(np.abs(a - b).max() / np.abs(b).max())
            assert dev <= tol_rsd[i], (name, p, i, dev)
        a = np.concatenate([default[p][1][k] for k in sorted(default[p][1])])
        b = np.concatenate([scalar[p][1][k] for k in sorted(scalar[p][1])])
        dd = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print(f"{name} pass {p}: default against scalar form, delta {dd:.2e}")
        assert dd <= tol_d, (name, p, dd)


def _tail_graph(extra):
    """a root of nf = 257 + 3 (m = 5, nft = 4) whose last variable is a pose made by `extra(builder, key, keys of the front)`"""
    b = dc._Builder(990)
    keys = b.hub_front(0, 257)
    last = X(50000)
    t = np.array([3.0, -2.0, 0.4])
    b.truth[last] = t
    b.initial.insert_pose2(last, *t)
    extra(b, last, keys)
    return b.graph, b.initial, dc.Ordering(keys + [last])


def _outcome(graph, initial, ordering, lam):
    """(status, failed slot, packed delta or None, [R S d] of the root) of one solve, and the oracle"""
    opt, orc, _ = _pair(graph, initial, ordering)
    ri = opt.num_fronts() - 1
    root = opt.front_info(ri)
    assert (root["nf"], root["n"], root["cls"]) == (260, 261, 1), root
    opt.linearize()
    try:
        _, packed, _, _ = opt.solve(lam)
        out = ("ok", None, packed)
    except _lib.IndeterminantLinearSystemException as e:
        out = ("indeterminate", e.args, None)
    out += (opt.front(ri)[1],)
    opt.close()
    return out, orc


def test_underdetermined_variable_in_the_tail(request, monkeypatch):
    def extra(b, last, keys):  # its only factor carries no information: sigma = 1e200, the squares of the whitened Jacobian underflow to 0
        b.graph.add_BetweenFactorPose2(keys[0], last, [0.5, 0.5, 0.1], dc.noiseModel.Diagonal.Sigmas([1e200, 1e200, 1e200]))
    graph, initial, ordering = _tail_graph(extra)
    assert schedule(261, 260)[-1][0] == DENSE_TAIL
    default, orc = _outcome(graph, initial, ordering, 0.0)
    orc.linearize()
    assert orc.solve(0.0)[0] == 1
    assert default[0] == "indeterminate", default[:2]
    request.getfixturevalue("dev_switches")
    monkeypatch.setenv("LMGPU_TAIL_SCALAR", "1")
    scalar, _ = _outcome(graph, initial, ordering, 0.0)
    assert scalar[:2] == default[:2], (scalar[:2], default[:2])


def test_nan_measurement_passes_through_the_tail(request, monkeypatch):
    def extra(b, last, keys):
        b.link(keys[0], last, force=True)
        b.graph.add_PriorFactorPose2(last, [float("nan"), -2.0, 0.4], b.prior)
    graph, initial, ordering = _tail_graph(extra)
    default, orc = _outcome(graph, initial, ordering, 1e-3)
    request.getfixturevalue("dev_switches")
    monkeypatch.setenv("LMGPU_TAIL_SCALAR", "1")
    scalar, _ = _outcome(graph, initial, ordering, 1e-3)
    print("NaN case:", default[:2], scalar[:2])
    for form in (default, scalar):
        # the factorisation takes the NaN through: no pivot is NaN or <= 0, R and S of the root are finite, the NaN sits in d
        rsd = form[3]
        assert np.isfinite(rsd[:, :-1]).all()
        assert np.isfinite(rsd[:256, -1]).all() and np.isnan(rsd[256:, -1]).any()
        # ... and the back-substitution reports the NaN it meets in x, as the reference does (linearAlgorithms-inst.h:99)
        assert form[0] == "indeterminate", form[:2]
    assert scalar[:2] == default[:2], (scalar[:2], default[:2])
    orc.linearize()
    assert orc.solve(1e-3)[0] == 1
