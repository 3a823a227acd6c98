"""Small seeded graphs that put the dense (HBM-class) front's factorisation and back-substitution at their panel boundaries: outer
panels of 256 rows, 64-column block columns, dataflow panels against the two-launch form, the tail kernel, fused steps and chained
runs, the quadrant update against the 128-tile update, the batched medium path, and the three back-substitution forms.

A dense front of prescribed width from few factors: a hub Pose2 that is eliminated FIRST and is adjacent to every other variable
makes all the rest one clique, and the clique-merge rule collapses the chain of fronts into one.  Poses (3) and Point2 landmarks (2)
reach every width, nf = 3 a + 2 b, and are shuffled behind the hub so that blocks of 2 and 3 straddle the tile edges.  Every
non-hub variable also gets DEGREE factors to random other variables of the front (between / bearing-range), which makes the front
numerically dense instead of block-diagonal plus rank 3; every pose has a prior.  test_dense_front_reference.py decides whether that is
dense enough (an injected defect has to show).

A case is a dict in the shape of schur_cases: graph, initial, ordering; plus
  fronts    the intended fronts in front order: dict(nf, n, parent, cls)   (asserted from a structure-only handle, no GPU)
  switches  environment the case runs under in its default comparison (one_panel: LMGPU_NO_MED)
  launches  per solve, from reading the planner (csrc/dense_schedule.hpp: dense_front_schedule) and the level loop of do_eliminate in
            csrc/lmgpu.hip: dict(panel, syrk, chain[, panel_work]) = launch counters of kernel_times(); panel_work False = the batched
            medium path (its launches carry no flop count)

The cases (nf = frontal scalars of the front under test; a root has n = nf + 1):
  medium_batch         one graph, seven components with a dense front of nf = 63, 64, 65, 128, 193, 255, 256, all on level 0:
                       med_*_kernel over unequal sizes in one batch
  one_panel[nf]        the same seven sizes, one graph each, under LMGPU_NO_MED: the per-front path with one panel -- dataflow panel
                       (64, 128, 256) or diag_potrf + panel_trsm (63, 65, 193, 255), then one quadrant update
  tail[nf]             257, 303 (m = n - 256 = 2, 48: front_tail_kernel, 48 the last it accepts), 304 (m = 49: refused), 319 (last panel
                       of 63 rows: unfused update + two-launch panel), 320 (64 rows: fused step_kernel), 321 (65 rows)
  chain[nf]            576 (chained run of 2 steps), 768 (run of 2, then a 1-column quadrant update), 771 (run of 2, then the tail
                       kernel), 832 (run of 3: a merged pair and a single step), 900 (run of 2, unfused step, two-launch panel of 132
                       rows), 1088 (run of 4; nf > 1024: hbm_backsolve_dataflow2_kernel instead of hbm_backsolve_blocks_kernel)
  beyond_1024          1290: with LMGPU_NO_FUSE the first update has m = 1035 > 1024 (syrk_mfma_kernel); by default a run of 4, then
                       the tail kernel (last panel of 10 rows)
  separator[nf,ns]     a NON-root dense front A (hub ordering) below root B: (192, 70), (300, 138), (96, 600), (1030, 66)

Departures from the plan the cases were drawn up from, each from reading the dispatch:
  * medium_batch / one_panel with nf = 63, 64, 65, 128: a ROOT of that size has n <= 139 and is an LDS front, which none of the dense
    kernels sees.  These four are non-root fronts instead, with a separator of 78 scalars (n = nf + 79 > 139) under an LDS root of
    81; the quadrant update behind their one panel then has 79 columns, not 1.  193, 255 and 256 are roots as planned.
  * separator: the parent B is the ns separator scalars PLUS one pose that A does not touch.  Without it A's separator equals the
    root's whole key set and the merge rule folds A into the root (one front, no separator).  So the roots have nf = ns + 3:
    73 and 69 (LDS roots), 141 (n = 142: the smallest HBM root there is room for; taken by the medium path), 603 (per-front HBM root:
    fused step, unfused step, two-launch panel of 91 rows).
  * separator (192, 70) and (96, 600) have nf <= 256 and no gather leaves, so A itself takes the batched medium path (med_syrk over
    71 / 604 columns); the GPU test runs both under LMGPU_NO_MED as well, which is where the per-front panel and update kernels meet a
    wide separator part.  (300, 138) and (1030, 66) take the per-front path by default.
  * beyond_1024 has six panels, not five (1290 = 5 x 256 + 10).
  * the launch counters cannot tell a dataflow panel from diag_potrf + panel_trsm (one counted event either way); which of the two a
    size takes is `rows % 64 == 0`, asserted on the planner's records (test_dense_schedule.py).
"""
import functools

import numpy as np

from gtsam_personal_amd import NonlinearFactorGraph, Ordering, Values, noiseModel
from gtsam_personal_amd.graph import L, X

from schur_cases import _rel2

DEGREE = 6
MEDIUM_SIZES = (63, 64, 65, 128, 193, 255, 256)
TAIL_SIZES = (257, 303, 304, 319, 320, 321)
CHAIN_SIZES = (576, 768, 771, 832, 900, 1088)
SEPARATOR_SIZES = ((192, 70), (300, 138), (96, 600), (1030, 66))
LDS_MAX_N = 139
# (lambda, diagonal damping) of the two solves every comparison makes: the second runs over the R of the first
PASSES = ((1e-6, False), (1e-2, True))


def split_width(width):
    """(poses, points) with 3 poses + 2 points = width, as few points as possible"""
    b = (0, 2, 1)[width % 3]
    assert width >= 2 * b + 3 and (width - 2 * b) % 3 == 0
    return (width - 2 * b) // 3, b


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.graph, self.initial = NonlinearFactorGraph(), Values()
        self.truth = {}  # key -> (x, y, theta) for a pose, (x, y) for a point
        # wide sigmas: information entries of 0.03 .. 30, against which the lambda = 1e-6 of the first pass is still visible in R at
        # 100 x the tolerance (test_dense_front_reference plants a missing lambda to see that)
        self.between = noiseModel.Diagonal.Sigmas([6.0, 6.0, 2.0])
        self.br = noiseModel.Diagonal.Sigmas([1.0, 4.0])
        self.prior = noiseModel.Diagonal.Sigmas([10.0, 10.0, 4.0])

    def variables(self, base, n_pose, n_point):
        """n_pose poses X(base + i) with a prior each and n_point points L(base + j), scattered over a 30 x 30 square"""
        rng = self.rng
        poses, points = [X(base + i) for i in range(n_pose)], [L(base + j) for j in range(n_point)]
        for k in poses:
            t = np.array([rng.uniform(-15, 15), rng.uniform(-15, 15), rng.uniform(-3, 3)])
            self.truth[k] = t
            self.initial.insert_pose2(k, *(t + rng.normal(0, [0.05, 0.05, 0.02])))
            self.graph.add_PriorFactorPose2(k, list(t + rng.normal(0, [0.1, 0.1, 0.05])), self.prior)
        for k in points:
            p = rng.uniform(-15, 15, 2)
            self.truth[k] = p
            self.initial.insert_point2(k, p + rng.normal(0, 0.05, 2))
        return poses, points

    def link(self, a, b, force=False):
        """one factor between two variables, at least one of them a pose; False (unless forced) when it would be a bearing at a range under 1"""
        rng, ta, tb = self.rng, self.truth[a], self.truth[b]
        if len(ta) == 2:
            a, b, ta, tb = b, a, tb, ta
        if len(tb) == 3:
            z = np.array(_rel2(ta, tb)) + rng.normal(0, [0.05, 0.05, 0.02])
            self.graph.add_BetweenFactorPose2(a, b, list(z), self.between)
            return True
        q = _rel2(ta, [tb[0], tb[1], 0.0])
        if np.hypot(q[0], q[1]) < 1.0 and not force:
            return False
        self.graph.add_BearingRangeFactor2D(a, b, np.arctan2(q[1], q[0]) + rng.normal(0, 0.02), np.hypot(q[0], q[1]) + rng.normal(0, 0.1), self.br)
        return True

    def hub_front(self, base, nf, separator=()):
        """a front of nf frontal scalars whose separator is `separator` (keys of variables made elsewhere): the hub X(base) is linked
        to every other frontal variable and every separator variable; every other frontal variable to DEGREE random variables of the
        front (a point only to poses).  Returns the frontal keys in elimination order: hub, then the rest shuffled."""
        rng = self.rng
        n_pose, n_point = split_width(nf)
        poses, points = self.variables(base, n_pose, n_point)
        hub, rest = poses[0], poses[1:] + points
        rest = [rest[i] for i in rng.permutation(len(rest))]
        everyone = rest + list(separator)
        pose_like = [k for k in everyone if len(self.truth[k]) == 3]
        for k in everyone:
            self.link(hub, k, force=True)
        for k in rest:
            made = 0
            while made < DEGREE:
                pool = everyone if len(self.truth[k]) == 3 else pose_like
                other = pool[rng.integers(len(pool))]
                if other != k and self.link(k, other):
                    made += 1
        return [hub] + rest

    def case(self, ordering, fronts, launches, switches=()):
        return dict(graph=self.graph, initial=self.initial, ordering=Ordering(ordering), fronts=fronts, launches=launches, switches=tuple(switches))


def _cls(n):
    return 0 if n <= LDS_MAX_N else 1


def _root(nf):
    return dict(nf=nf, n=nf + 1, parent=-1, cls=_cls(nf + 1))


def root_case(nf, seed, launches, switches=()):
    b = _Builder(seed)
    return b.case(b.hub_front(0, nf), [_root(nf)], launches, switches)


def _with_parent(b, base, nf, ns, first_front):
    """front A (nf frontal scalars, hub ordering) with the ns scalars of S as its separator; its parent is S plus one pose that A
    does not touch (ordered last), made one front by its own hub: the first variable of S.  Returns (ordering, the two fronts)"""
    sp, spt = split_width(ns)
    s_poses, s_points = b.variables(base + 10000, sp, spt)
    (extra,), _ = b.variables(base + 20000, 1, 0)
    sep = s_poses + s_points
    for k in sep[1:] + [extra]:  # the parent's own factors: its first variable to all the others, and a ring
        b.link(sep[0], k, force=True)
    for i, k in enumerate(s_poses):
        b.link(k, s_poses[(i + 1) % sp])
        b.link(k, extra)
    a_keys = b.hub_front(base, nf, separator=sep)
    fronts = [dict(nf=nf, n=nf + ns + 1, parent=first_front + 1, cls=_cls(nf + ns + 1)), _root(ns + 3)]
    return a_keys + sep + [extra], fronts


SMALL_NS = 78  # a front of nf <= 138 is dense-class (n > 139) only with a separator: 78 scalars under an LDS root of 81


def medium_batch_case():
    b = _Builder(500)
    order, fronts = [], []
    for i, nf in enumerate(MEDIUM_SIZES):
        if nf + 1 > LDS_MAX_N:
            order += b.hub_front(100000 * i, nf)
            fronts.append(_root(nf))
        else:
            o, f = _with_parent(b, 100000 * i, nf, SMALL_NS, len(fronts))
            order += o
            fronts += f
    return b.case(order, fronts, dict(panel=1, syrk=1, chain=0, panel_work=False))


def one_panel_case(nf, seed):
    launches = _launches(1, 1, 0)  # panel 0, then the update of the columns behind it (the rhs alone, or separator + rhs)
    if nf + 1 > LDS_MAX_N:
        return root_case(nf, seed, launches, ("LMGPU_NO_MED",))
    b = _Builder(seed)
    order, fronts = _with_parent(b, 0, nf, SMALL_NS, 0)
    return b.case(order, fronts, launches, ("LMGPU_NO_MED",))


def separator_case(nf, ns, seed, launches):
    b = _Builder(seed)
    order, fronts = _with_parent(b, 0, nf, ns, 0)
    return b.case(order, fronts, launches)


def _launches(panel, syrk, chain, panel_work=True):
    return dict(panel=panel, syrk=syrk, chain=chain, panel_work=panel_work)


def front_launches(nf, n, two_launch=False, no_fuse=False, no_chain=False, no_tail=False):
    """the launch counters one dense front on the per-front path adds per solve: the planner dense_front_schedule
    (csrc/dense_schedule.hpp) restated -- dataflow_ok, fusable, chainable, the tail condition -- with the switches LMGPU_PANEL_2L,
    LMGPU_NO_FUSE, LMGPU_NO_CHAIN, LMGPU_NO_TAIL.  test_dense_schedule.py holds the planner's records against it on the CPU, the GPU
    test the library's own counters."""
    panels = -(-nf // 256)

    def rows(i):
        return min(nf, 256 * (i + 1)) - 256 * i

    def dataflow_ok(i):
        return rows(i) % 64 == 0 and not two_launch

    def fusable(i):
        return i + 1 < panels and dataflow_ok(i + 1) and not no_fuse and n - 256 * i - rows(i) > 0

    def chainable(i):
        return fusable(i) and not no_chain and rows(i) == 256
    out = _launches(1, 0, 0)  # panel 0
    i = 0
    while i < panels:
        m = n - 256 * i - rows(i)
        if m <= 0:
            break
        if chainable(i) and chainable(i + 1):  # a run of chainable steps: one launch
            while chainable(i):
                i += 1
            out["chain"] += 1
            continue
        if not no_tail and i + 2 == panels and m <= 48 and rows(i + 1) < 64:  # front_tail_kernel
            out["panel"] += 1
            break
        out["syrk"] += 1  # a fused step, or an update on its own ...
        if not fusable(i) and i + 1 < panels:
            out["panel"] += 1  # ... with the next panel behind it
        i += 1
    return out


SWITCH_ARGUMENT = dict(LMGPU_PANEL_2L="two_launch", LMGPU_NO_FUSE="no_fuse", LMGPU_NO_CHAIN="no_chain", LMGPU_NO_TAIL="no_tail")


def per_front_launches(fronts, switch=None):
    """front_launches summed over the dense fronts of a case whose dense fronts all take the per-front path"""
    kw = {SWITCH_ARGUMENT[switch]: True} if switch in SWITCH_ARGUMENT else {}
    out = _launches(0, 0, 0)
    for f in fronts:
        if f["cls"] == 1:
            for k, v in front_launches(f["nf"], f["n"], **kw).items():
                if k != "panel_work":
                    out[k] += v
    return out


# per solve, by the planner dense_front_schedule (rows(i) = rows of outer panel i, m = columns behind it):
#   panel 0 is one `panel` event; a run of >= 2 chainable steps one `chain` event; the tail kernel one `panel` event; a fused step one
#   `syrk` launch; an unfused step one `syrk` event plus one `panel` event when a panel follows it
_TAIL_LAUNCHES = {257: _launches(2, 0, 0), 303: _launches(2, 0, 0),  # panel 0, tail kernel
                  304: _launches(2, 2, 0), 319: _launches(2, 2, 0), 321: _launches(2, 2, 0),  # update, two-launch panel, 1-column update
                  320: _launches(1, 2, 0)}  # fused step, 1-column update
_CHAIN_LAUNCHES = {576: _launches(1, 1, 1), 768: _launches(1, 1, 1), 832: _launches(1, 1, 1), 1088: _launches(1, 1, 1),  # run, 1-column update
                   771: _launches(2, 0, 1),  # run of 2, tail kernel
                   900: _launches(2, 2, 1)}  # run of 2, update, two-launch panel, 1-column update
_SEPARATOR_LAUNCHES = {(192, 70): _launches(1, 1, 0, False),  # A on the medium path; LDS root
                       (300, 138): _launches(3, 3, 0),  # A: panel, update, two-launch panel (44 rows), update; the root on the medium path
                       (96, 600): _launches(3, 4, 0),  # A on the medium path; root: panel, fused step, update, two-launch panel, update
                       (1030, 66): _launches(2, 2, 1)}  # A: panel, run of 3, update, two-launch panel (6 rows), update; LDS root

CASES = {"medium_batch": medium_batch_case}
for _i, _nf in enumerate(MEDIUM_SIZES):
    CASES[f"one_panel[{_nf}]"] = functools.partial(one_panel_case, _nf, 510 + _i)
for _i, _nf in enumerate(TAIL_SIZES):
    CASES[f"tail[{_nf}]"] = functools.partial(root_case, _nf, 520 + _i, _TAIL_LAUNCHES[_nf])
for _i, _nf in enumerate(CHAIN_SIZES):
    CASES[f"chain[{_nf}]"] = functools.partial(root_case, _nf, 530 + _i, _CHAIN_LAUNCHES[_nf])
CASES["beyond_1024"] = functools.partial(root_case, 1290, 540, _launches(2, 0, 1))  # panel 0, run of 4, tail kernel
for _i, (_nf, _ns) in enumerate(SEPARATOR_SIZES):
    CASES[f"separator[{_nf},{_ns}]"] = functools.partial(separator_case, _nf, _ns, 550 + _i, _SEPARATOR_LAUNCHES[(_nf, _ns)])

_FOUR = ("chain[832]", "chain[900]", "chain[771]", "chain[1088]")
SWITCH_RUNS = [(("LMGPU_PANEL_2L", "1"), _FOUR), (("LMGPU_NO_FUSE", "1"), _FOUR + ("beyond_1024",)), (("LMGPU_NO_CHAIN", "1"), _FOUR),
               (("LMGPU_NO_MERGE", "1"), _FOUR), (("LMGPU_CHAIN_FAR", "100"), _FOUR),
               (("LMGPU_NO_INV16_REUSE", "1"), _FOUR + ("separator[1030,66]",)),
               (("LMGPU_NO_TAIL", "1"), ("tail[257]", "tail[303]", "chain[771]")),
               (("LMGPU_NO_MED", "1"), ("separator[192,70]", "separator[96,600]"))]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---------------------------------------------------------------------------------------------------------------- comparing
BLOCK = 32  # panel rows of the blocked extended-precision reference
FACTOR, EPS, CAP = 16, 2.2e-16, 1e-9  # the recipe of test_gpu_schur_edges


@functools.lru_cache(maxsize=None)
def oracle_floor(name):
    """schur_cases.floor_of over PASSES with the blocked reference"""
    import schur_cases as sc
    return sc.floor_of(case(name), PASSES, BLOCK)


def tolerances(fl, front_widths):
    """([tolerance of front i], tolerance of delta): max(16 x floor, 64 n 2.2e-16), n = the front's width / the widest front's"""
    return ([max(FACTOR * fl["rsd"], 64 * n * EPS) for n in front_widths], max(FACTOR * fl["delta"], 64 * max(front_widths) * EPS))
