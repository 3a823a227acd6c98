"""Small seeded graphs that put the LDS-class fronts of csrc/kernels_front.hpp -- the factorisation (lds_front_tiny, lds_front_body
inside lds_front_kernel / lds_front_merged_kernel / level_fused_kernel, fill_upper_kernel) and the back-substitution (lds_backsub_kernel,
lds_backsub_wide_kernel, lds_backsub_merged_kernel) -- at their size edges: the launch bins kBinN = {24, 48, 72, 96, 120, 139}, the pivot
groups of the four-pivot, eight-pivot and sixteen-pivot forms, the one-wave register front (n <= 16), the staging batch of LDSF_MAXB = 32
factors / LDSF_JCAP = 704 doubles, the packed record (fac_count <= 32, nf <= LEAFPACK_MAXNF = 8), the 64-column chunks of the extend-add
and of S x_S, the small / wide back-solve (LDSB_SMALL_NF = 12) and ldsb_stage's batch of 2048.

A case is a dict in the shape of dense_front_cases: graph, initial, ordering, plus
  fronts   the intended fronts in front order: dict(nf, n, parent, cls, level)   (asserted from a structure-only handle, no GPU)
The launch counts are not stored per case: `launches(fronts, ...)` below restates the dispatch of csrc/lmgpu.hip (narrow-level pooling,
level_lds_class, the merged segments of finalize, the fused-level conditions, do_backsub's segments) and gives, per solve,
dict(lds_front, backsub_lds, panel); the GPU test holds kernel_times() against it.

The tree builder.  dense_front_cases._with_parent rings the separator poses, which with ONE separator pose (ns in 3..5) is a factor on
a repeated variable, and the handle refuses the graph; it is left as it is (the measured tables of the two dense-front modules depend on
its random draws).  The cases here come from `_Tree`, a subclass of dense_front_cases._Builder with its own node spec
N(nf, ns, *children): nf frontal scalars, a separator of ns scalars that is a subset of the PARENT's frontal variables, and children.  A
node is one hub front (hub_front's make: the hub pose is eliminated first and linked to every other variable of the front, every other
frontal variable gets DEGREE random links); there is no ring.  A node with children has, as its LAST frontal variable, one pose that no
child touches: a child's separator is then a strict subset of every clique of the parent's chain, and the merge rule (child separator
count == parent clique count) cannot fold the child into it.  So a parent of children whose separator has ns scalars has nf >= ns + 3.
nf = 2 is one Point2 landmark seen from every separator pose.

Not reachable, from the variable types a Pose2 / Point2 graph has (3 a + 2 b, with the hub a pose):
  * nf = 1: no variable of dimension 1.  The row-by-row Cholesky of narrow fronts is otherwise only taken by gather leaves, which
    test_gpu_schur_edges compares.
  * nf = 4: two landmarks have no factor between them and so are two fronts; with a pose hub the widths are 3, 5, 6, 7, 8, ...  The group
    edge of four is held from both sides by nf = 3, 5, 7, 8, 9.
  * c.m > blockDim and nf > blockDim in the extend-add / emission loops: a child's update width and nf are at most 139 and every launch of
    n > 48 has at least 256 threads; n <= 48 has 128 (m <= 48), n <= 24 has 64.

The cases (front A = (nf, ns) under a root R of nf = ns + 3 unless said otherwise; n = nf + ns + 1):
  bin[n]            24 (12,11) / 25 (13,11): 64 -> 128 threads, small -> wide back-solve; 48 (20,27) / 49 (20,28): 128 -> 256; 72 (30,41) / 73
                    (30,42): first bin with sixteen waves and eight pivots by default; 96 (40,55) / 97 (40,56); 120 (50,69) / 121 (50,70);
                    the limit n = 139 as bin[64,74], bin[65,73], bin[3,135], bin[135,3], bin[16,122]
  bin_pooled        (12,11), (20,27), (40,55) as three components: narrow-level pooling runs all three in the launch of bin 3
  pivots[nf]        nf = 2, 3, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48, 49 with ns = 15 or 16 alternately (n - nf = 16 / 17: the
                    rank-16 trailing update's tile edge); every root has n - nf = 1.  pivots[2] is the front whose factors are of one type
                    and added back to back (the packed record's contiguous form; the flag itself has no tap)
  pivots_wide[nf]   nf = 31, 32, 33, 47, 48, 49 with ns = 60 (n = 92 .. 110): no pivots[nf] reaches n >= 73 with n - nf <= 17, so these put the
                    sixteen-pivot panel edges into the sixteen-wave launch (and, under LMGPU_NO_WIDE16, the four-wave one at that width)
  tiny[n]           15 (8,6), 16 (9,6), 17 (10,6): one-wave register front / general body of a merged 64-thread launch
  tiny_tree         fronts of n <= 16 with 0, 1, 2 and 3 children (root 3, one child 2, one child 1, leaves 0), on three levels
  tiny_sfm          Pose3 leaf (nf 6, n 15) under a root {Point3, Cal3_S2, Pose3} (nf 14, n 15), both with the ternary GeneralSFMFactor2
  staging[k]        one front of two Pose2 with two priors and k - 2 parallel between factors, k = 31, 32, 33, 64, 65
  staging_pose3[m]  two Pose3, two priors (42 doubles each) and m betweens (78 each): m = 7 stages 630 doubles, m = 8 stages 708 > 704
  staging_mixed     a Pose2 pair and a Pose3 pair as two components, their factors added alternately (interleaved in the pool)
  staging[8,8], staging[9,8]   the packed record's frontal offsets, nf <= 8 and above
  children[k]       a root with k = 1, 2, 3, 4, 5 children (3, 3 + 3 j): the third child on is not prefetched; level sizes 1, 4, 5 (5: a ragged
                    last block of the small back-solve's four fronts per block).  0 children: every leaf
  children_wide     (3,63), (3,64), (3,65), (3,127), (3,128) under one root of nf = 138 (43 poses and 3 landmarks, of which
                    the children take 63 .. 128 scalars, plus the untouched pose): update widths m = 64, 65, 66, 128, 129
  backsub[nf,ns]    (63,15), (128,8), (129,6): the wide kernel's 64-unknown blocks; (14,124), (15,123): nf * n = 1946 / 2085, either side of
                    ldsb_stage's 2048.  nf = 13, 32, 33, 64, 65 are bin[25], pivots[32], pivots[33], bin[64,74], bin[65,73]; a root of
                    nf <= 12 (ns = 0 in the small kernel) is the root of bin[3,135] and of every pivots case
  backsub_mixed     one level with (13,11), (3,3), (3,3), (3,6): the whole level takes the wide kernel
  deep_chain        a ladder of 14 pairs of Pose2: 13 fronts of n = 13 on 13 levels; by its depth the product library takes the merged
                    elimination, the merged back-substitution and graph replay with no switch
  fused_level       dense_front_cases' separator[192,70] component (a medium front under its LDS root) beside an LDS pair (13,20): level 0
                    holds a medium front and an LDS front; run under LMGPU_FUSE_LEVELS=1

Launch forms, each compared with the REFERENCE (FORM_RUNS, one line of reasoning each).  Which case reaches which kernel:
  lds_front_kernel<false, 256>     64 threads bin[24] and every root of n <= 24; 128 threads bin[25], bin[48]; 256 threads bin[49], bin[72], pivots[31..49];
                                   256 threads at n >= 73 under LMGPU_NO_WIDE16 (bin[73..121], the five n = 139, pivots_wide, children_wide)
  lds_front_kernel<false, 1024>    bin[73] .. bin[121], the five n = 139, pivots_wide, backsub[...], children_wide, bin_pooled
  lds_front_merged_kernel<256>     deep_chain (64 threads, by default); LMGPU_MERGE_ELIM=1 on tiny*, staging[8,8], children[5] (64 threads) and on
                                   pivots[7..49], bin[25..72], backsub_mixed (256 threads: the eight-pivot body at n <= 72)
  lds_front_merged_kernel<1024>    LMGPU_MERGE_ELIM=1 on bin[64,74], bin[65,73], bin[16,122], children_wide, backsub[14,124]
  lds_front_tiny                   every front of n <= 16 in a merged launch: deep_chain (n = 13), tiny[15], tiny[16], tiny_tree, tiny_sfm (the ternary
                                   factor), the (3,3) .. (3,12) children of children[5], the roots of backsub_mixed and pivots[..] under the 256-thread merge
  fill_upper_kernel                in front of every merged elimination launch above
  level_fused_kernel<256>          fused_level under LMGPU_FUSE_LEVELS=1.  (level_fused_kernel<1024> is only taken under LMGPU_FUSE_THREADS=1024 on a
                                   level whose LDS fronts are wider than 72; no default and no form named here takes it)
  lds_backsub_kernel               every level whose fronts all have nf <= 12: the roots of the pairs with ns <= 9, children[k], tiny*, staging[k], bin[3,135]
  lds_backsub_wide_kernel          every other level: bin[25] on, pivots[13] on, backsub[...], backsub_mixed (nf = 13 beside three of nf = 3)
  lds_backsub_merged_kernel        deep_chain (by default); LMGPU_MERGE_BACKSUB=1 on children_wide, children[5], backsub_mixed, bin[25], bin[65,73],
                                   backsub[129,6], backsub[15,123], tiny_tree, pivots[2]
lds_front_kernel<true> (gather leaves) belongs to the Schur slice (test_gpu_schur_edges.py).
"""
import functools

import numpy as np

from gtsam_personal_amd import Ordering, noiseModel
from gtsam_personal_amd.graph import L, X, symbol

import dense_front_cases as dc
from dense_front_cases import CAP, DEGREE, EPS, FACTOR, LDS_MAX_N, PASSES, _Builder, split_width, tolerances  # noqa: F401  (re-exported)

K_BIN = (24, 48, 72, 96, 120, 139)
LDSF_MAXB, LDSF_JCAP, LEAFPACK_MAXNF, LDSB_SMALL_NF = 32, 704, 8, 12
DEEP_LEVELS = 12  # from this many levels on: merged elimination, merged back-substitution, graph replay, fused levels
K0 = symbol("K", 0)
K_TRUE = (50.0, 50.0, 0.0, 50.0, 50.0)


def N(nf, ns=0, *children):
    return dict(nf=nf, ns=ns, children=list(children))


def _composition(width, min_points=0):
    """(poses, points) with 3 poses + 2 points = width and at least min_points points, as few points as possible"""
    b = (0, 2, 1)[width % 3]
    while b < min_points:
        b += 3
    assert width >= 2 * b and (width - 2 * b) % 3 == 0, (width, min_points)
    return (width - 2 * b) // 3, b


class _Tree(_Builder):
    def __init__(self, seed):
        super().__init__(seed)
        self.fronts, self.bases = [], 0

    @staticmethod
    def _pick(ns, poses, points, offset):
        """ns scalars of a parent's variables; offset rotates the choice so that siblings take different subsets"""
        sp, spt = split_width(ns) if ns != 2 else (0, 1)
        assert sp <= len(poses) and spt <= len(points), (ns, len(poses), len(points))
        return [poses[(offset + i) % len(poses)] for i in range(sp)] + [points[(offset + i) % len(points)] for i in range(spt)]

    def node(self, spec, sep=()):
        """the subtree of `spec` below the separator keys `sep`; returns (ordering of the subtree, index of its front)"""
        nf, ns, children = spec["nf"], spec["ns"], spec["children"]
        sep = list(sep)
        base = 1000 * self.bases
        self.bases += 1
        if nf == 2:  # one landmark, seen from every separator pose
            assert not children and sep and all(len(self.truth[k]) == 3 for k in sep)
            _, (point,) = self.variables(base, 0, 1)
            for k in sep:
                self.link(k, point, force=True)
            return self._emit([point], nf, ns, [])
        if children:
            need = [split_width(c["ns"]) if c["ns"] != 2 else (0, 1) for c in children]
            a, b = _composition(nf - 3, max(n[1] for n in need))
            assert a >= max(1, max(n[0] for n in need)), spec
            poses, points = self.variables(base, a + 1, b)
            last = [poses.pop()]  # the pose no child touches, eliminated last
        else:
            poses, points = self.variables(base, *split_width(nf))
            last = []
        rng = self.rng
        hub, rest = poses[0], poses[1:] + points
        rest = [rest[i] for i in rng.permutation(len(rest))] + last
        everyone = rest + sep
        pose_like = [k for k in everyone if len(self.truth[k]) == 3]
        for k in everyone:  # (before the children's factors: each variable's chain to the hub is then hooked in front of the child fronts)
            self.link(hub, k, force=True)
        for k in rest:
            pool = [o for o in (everyone if len(self.truth[k]) == 3 else pose_like) if o != k]
            made = 0
            while pool and made < DEGREE:
                if self.link(k, pool[rng.integers(len(pool))]):
                    made += 1
        # the plan numbers sibling fronts by the place of their first separator variable in this front's elimination order
        place = {k: i for i, k in enumerate([hub] + rest)}
        seps = [self._pick(c["ns"], poses, points, i) for i, c in enumerate(children)]
        orders, kids = [], []
        for i in sorted(range(len(children)), key=lambda i: min(place[k] for k in seps[i])):
            o, f = self.node(children[i], seps[i])
            orders += o
            kids.append(f)
        return self._emit(orders + [hub] + rest, nf, ns, kids)

    def _emit(self, order, nf, ns, kids):
        i = len(self.fronts)
        for k in kids:
            self.fronts[k]["parent"] = i
        n = nf + ns + 1
        self.fronts.append(dict(nf=nf, n=n, parent=-1, cls=0 if n <= LDS_MAX_N else 1, level=1 + max((self.fronts[k]["level"] for k in kids), default=-1)))
        return order, i

    def done(self, order):
        return dict(graph=self.graph, initial=self.initial, ordering=Ordering(order), fronts=self.fronts)


def tree_case(seed, *specs):
    """one component per spec"""
    t = _Tree(seed)
    order = []
    for s in specs:
        order += t.node(s)[0]
    return t.done(order)


def pair(nf, ns):
    """front (nf, ns) under a root of the separator plus one pose"""
    return N(ns + 3, 0, N(nf, ns))


# ---------------------------------------------------------------------------------------------------------------- hand-made cases
def staging_case(seed, k2=0, m3=0, interleave=False):
    """k2 > 0: two Pose2 with a prior each and k2 - 2 between factors; m3 > 0: two Pose3 with a prior each and m3 between factors.  Both:
    two components; interleave alternates the two kinds factor by factor"""
    from gtsam_personal_amd.datasets import pose3_compose, rot3_expmap
    t = _Tree(seed)
    rng = t.rng
    adds2, adds3, order = [], [], []
    if k2:
        (a, b), _ = t.variables(0, 2, 0)  # (the two priors are added here)
        order += [a, b]
        for _ in range(k2 - 2):
            adds2.append(lambda a=a, b=b: t.link(a, b))
        t.fronts.append(dict(nf=6, n=7, parent=-1, cls=0, level=0))
    if m3:
        p3 = [(rot3_expmap(rng.normal(0, 0.5, 3)), rng.uniform(-5, 5, 3)) for _ in range(2)]
        keys = [X(5000), X(5001)]
        prior = noiseModel.Diagonal.Sigmas([0.5, 0.5, 0.5, 3.0, 3.0, 3.0])
        between = noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.3, 2.0, 2.0, 2.0])
        for k, (R, p) in zip(keys, p3):
            Rn, pn = pose3_compose(R, p, rot3_expmap(rng.normal(0, 0.02, 3)), rng.normal(0, 0.05, 3))
            t.initial.insert_pose3(k, Rn, pn)
            adds3.append(lambda k=k, R=R, p=p: t.graph.add_PriorFactorPose3(k, R, p, prior))
        (R0, p0), (R1, p1) = p3
        for _ in range(m3):
            dR, dp = rot3_expmap(rng.normal(0, 0.02, 3)), rng.normal(0, 0.1, 3)
            adds3.append(lambda dR=dR, dp=dp: t.graph.add_BetweenFactorPose3(keys[0], keys[1], R0.T @ R1 @ dR, R0.T @ (p1 - p0) + dp, between))
        order += keys
        t.fronts.append(dict(nf=12, n=13, parent=-1, cls=0, level=0))
    if interleave:
        for i in range(max(len(adds2), len(adds3))):
            for adds in (adds2, adds3):
                if i < len(adds):
                    adds[i]()
    else:
        for f in adds2 + adds3:
            f()
    return t.done(order)


def tiny_sfm_case(seed=740):
    """X(1) (Pose3, leaf: nf 6, separator {point, calibration}, n 15) under the root {L(0), K, X(0)} (nf 14, n 15); ordered X1, L0, K, X0 so
    that the leaf's separator is a strict subset of the root's first clique"""
    from isam2_examples import create_points, create_poses, project_cal3_s2
    from gtsam_personal_amd.datasets import pose3_compose, rot3_expmap
    t = _Tree(seed)
    rng, g, v = t.rng, t.graph, t.initial
    point, poses = create_points()[0], create_poses()[:2]
    pix = noiseModel.Isotropic.Sigma(2, 1.0)
    for i, (R, p) in enumerate(poses):
        g.add_PriorFactorPose3(X(i), R, p, noiseModel.Diagonal.Sigmas([0.1, 0.1, 0.1, 0.3, 0.3, 0.3]))
        for _ in range(3):
            g.add_GeneralSFMFactor2(project_cal3_s2(R, p, point, K_TRUE) + rng.normal(0, 0.5, 2), pix, X(i), L(0), K0)
        v.insert_pose3(X(i), *pose3_compose(R, p, rot3_expmap([-0.02, 0.03, 0.04]), np.array([0.05, -0.10, 0.20])))
    g.add_PriorFactorPoint3(L(0), point, noiseModel.Isotropic.Sigma(3, 0.1))
    g.add_PriorFactorCal3_S2(K0, K_TRUE, noiseModel.Diagonal.Sigmas([5, 5, 0.1, 5, 5]))
    v.insert_cal3_s2(K0, 52.0, 52.0, 0.0, 49.0, 49.0)
    v.insert_point3(L(0), point + np.array([-0.05, 0.04, 0.03]))
    t.fronts = [dict(nf=6, n=15, parent=1, cls=0, level=0), dict(nf=14, n=15, parent=-1, cls=0, level=1)]
    return t.done([X(1), L(0), K0, X(0)])


LADDER_PAIRS = 14


def deep_chain_case(seed=760):
    """pairs (a_i, b_i) with a_i - b_i, a_i - a_i+1, b_i - b_i+1 and a_i - b_i+1: front i = {a_i, b_i | a_i+1, b_i+1}; the last pair folds
    into front 12, the root"""
    t = _Tree(seed)
    (poses, _) = t.variables(0, 2 * LADDER_PAIRS, 0)
    a, b = poses[0::2], poses[1::2]
    for i in range(LADDER_PAIRS):
        t.link(a[i], b[i])
        if i + 1 < LADDER_PAIRS:
            t.link(a[i], a[i + 1])
            t.link(b[i], b[i + 1])
            t.link(a[i], b[i + 1])
    nfr = LADDER_PAIRS - 1
    t.fronts = [dict(nf=6, n=13, parent=i + 1, cls=0, level=i) for i in range(nfr - 1)] + [dict(nf=12, n=13, parent=-1, cls=0, level=nfr - 1)]
    return t.done(poses)


def fused_level_case(seed=770):
    """the component of dense_front_cases' separator[192,70] (made by its _with_parent, on this case's own generator) and an LDS pair"""
    t = _Tree(seed)
    order, fronts = dc._with_parent(t, 500000, 192, 70, 0)
    for f, lvl in zip(fronts, (0, 1)):
        f["level"] = lvl
    t.fronts = fronts
    t.bases = 1
    o2, _ = t.node(pair(13, 20))
    return t.done(order + o2)


BIN_PAIRS = {24: (12, 11), 25: (13, 11), 48: (20, 27), 49: (20, 28), 72: (30, 41), 73: (30, 42), 96: (40, 55), 97: (40, 56), 120: (50, 69),
             121: (50, 70)}
LIMIT_PAIRS = ((64, 74), (65, 73), (3, 135), (135, 3), (16, 122))
PIVOT_NF = (2, 3, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48, 49)
PIVOT_WIDE_NF, PIVOT_WIDE_NS = (31, 32, 33, 47, 48, 49), 60
TINY_PAIRS = {15: (8, 6), 16: (9, 6), 17: (10, 6)}
STAGING_COUNTS = (31, 32, 33, 64, 65)
BACKSUB_PAIRS = ((63, 15), (128, 8), (129, 6), (14, 124), (15, 123))
WIDE_CHILDREN = ((3, 63), (3, 64), (3, 65), (3, 127), (3, 128))

CASES = {}
for _i, (_n, (_nf, _ns)) in enumerate(BIN_PAIRS.items()):
    CASES[f"bin[{_n}]"] = functools.partial(tree_case, 600 + _i, pair(_nf, _ns))
for _i, (_nf, _ns) in enumerate(LIMIT_PAIRS):
    CASES[f"bin[{_nf},{_ns}]"] = functools.partial(tree_case, 620 + _i, pair(_nf, _ns))
CASES["bin_pooled"] = functools.partial(tree_case, 630, pair(12, 11), pair(20, 27), pair(40, 55))
for _i, _nf in enumerate(PIVOT_NF):
    CASES[f"pivots[{_nf}]"] = functools.partial(tree_case, 640 + _i, pair(_nf, 15 if _i % 2 == 0 else 16))
for _i, _nf in enumerate(PIVOT_WIDE_NF):
    CASES[f"pivots_wide[{_nf}]"] = functools.partial(tree_case, 670 + _i, pair(_nf, PIVOT_WIDE_NS))
for _i, (_n, (_nf, _ns)) in enumerate(TINY_PAIRS.items()):
    CASES[f"tiny[{_n}]"] = functools.partial(tree_case, 700 + _i, pair(_nf, _ns))
CASES["tiny_tree"] = functools.partial(tree_case, 710, N(14, 0, N(9, 6, N(8, 6), N(5, 3)), N(11, 3, N(12, 3)), N(7, 8)))
CASES["tiny_sfm"] = tiny_sfm_case
for _i, _k in enumerate(STAGING_COUNTS):
    CASES[f"staging[{_k}]"] = functools.partial(staging_case, 720 + _i, k2=_k)
CASES["staging_pose3[7]"] = functools.partial(staging_case, 730, m3=7)
CASES["staging_pose3[8]"] = functools.partial(staging_case, 731, m3=8)
CASES["staging_mixed"] = functools.partial(staging_case, 732, k2=20, m3=6, interleave=True)
CASES["staging[8,8]"] = functools.partial(tree_case, 733, pair(8, 8))
CASES["staging[9,8]"] = functools.partial(tree_case, 734, pair(9, 8))
for _k in (1, 2, 3, 4, 5):
    CASES[f"children[{_k}]"] = functools.partial(tree_case, 740 + _k, N(21, 0, *[N(3, 3 + 3 * _j) for _j in range(_k)]))
CASES["children_wide"] = functools.partial(tree_case, 750, N(138, 0, *[N(_nf, _ns) for _nf, _ns in WIDE_CHILDREN]))
for _i, (_nf, _ns) in enumerate(BACKSUB_PAIRS):
    CASES[f"backsub[{_nf},{_ns}]"] = functools.partial(tree_case, 751 + _i, pair(_nf, _ns))
CASES["backsub_mixed"] = functools.partial(tree_case, 757, N(14, 0, N(13, 11), N(3, 3), N(3, 3), N(3, 6)))
CASES["deep_chain"] = deep_chain_case
CASES["fused_level"] = fused_level_case


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---------------------------------------------------------------------------------------------------------------- the dispatch, restated
def _bin(n):
    return next(b for b, top in enumerate(K_BIN) if n <= top)


def _level_class(lds_widths, no_wide16):
    """level_lds_class: threads of the one launch that would hold the LDS fronts of a level (None: no such launch); no case has gather leaves"""
    if not lds_widths or len(lds_widths) > 160:
        return None
    top = _bin(max(lds_widths))
    return 1024 if top >= 3 and len(lds_widths) <= 256 and not no_wide16 else 64 if top == 0 else 256


def elim_segments(fronts, no_wide16=False):
    """the merged elimination segments of finalize: [(lowest level, highest level, threads)] over runs of >= 2 consecutive levels with LDS
    fronts, no dense front below the top level of the run, and sixteen-wave levels apart from four-wave ones"""
    nl = 1 + max(f["level"] for f in fronts)
    lds = [[f["n"] for f in fronts if f["level"] == l and f["cls"] == 0] for l in range(nl)]
    hbm = [any(f["level"] == l and f["cls"] == 1 for f in fronts) for l in range(nl)]
    segs, l = [], 0
    while l < nl:
        t = _level_class(lds[l], no_wide16)
        if t is None:
            l += 1
            continue
        hi = l
        while hi + 1 < nl and not hbm[hi]:
            t2 = _level_class(lds[hi + 1], no_wide16)
            if t2 is None or (t2 == 1024) != (t == 1024):
                break
            hi, t = hi + 1, max(t, t2)
        if hi > l:
            segs.append((l, hi, t))
        l = hi + 1
    return segs


def launches(fronts, merge_elim=None, merge_backsub=None, no_wide16=False, fuse_levels=None):
    """per solve: dict(lds_front, backsub_lds, panel, syrk).  `panel` / `syrk`: a level's medium fronts (dense, nf <= 256, the only dense
    fronts a case here has: fused_level) are one panel and one syrk event, or ONE panel event when the level is fused with its LDS fronts;
    the LDS fronts of a fused level have no launch of their own.  None = the library's own rule: on from
    DEEP_LEVELS levels.  One LDS launch per occupied (level, bin group) after pooling (<= 512 fronts on a level share the top bin's
    launch; no case has more, or gather leaves), or one per merged segment; one back-solve launch per level, or per run of levels with no
    dense front between them"""
    nl = 1 + max(f["level"] for f in fronts)
    deep = nl >= DEEP_LEVELS
    merge_elim, merge_backsub, fuse_levels = (deep if x is None else x for x in (merge_elim, merge_backsub, fuse_levels))
    lds = [[f["n"] for f in fronts if f["level"] == l and f["cls"] == 0] for l in range(nl)]
    hbm = [[f for f in fronts if f["level"] == l and f["cls"] == 1] for l in range(nl)]
    assert all(len(x) <= 512 for x in lds)
    segs = elim_segments(fronts, no_wide16) if merge_elim else []
    in_seg = {l for lo, hi, _ in segs for l in range(lo, hi + 1)}
    out = dict(lds_front=len(segs), backsub_lds=0, panel=0, syrk=0)
    for l in range(nl):
        medium = [f for f in hbm[l] if f["nf"] <= 256]  # (no case has gather leaves below a dense front)
        if fuse_levels and medium and l not in in_seg and _level_class(lds[l], no_wide16) is not None:
            out["panel"] += 1
            continue
        if medium:
            out["panel"] += 1
            out["syrk"] += 1
        if lds[l] and l not in in_seg:
            out["lds_front"] += 1
    if merge_backsub:
        pending = False
        for l in range(nl - 1, -1, -1):
            if hbm[l] and pending:
                out["backsub_lds"] += 1
                pending = False
            pending = pending or bool(lds[l])
            if pending and (l == 0 or hbm[l - 1]):
                out["backsub_lds"] += 1
                pending = False
    else:
        out["backsub_lds"] = sum(1 for x in lds if x)
    return out


def backsub_kernel(fronts, level):
    """'wide' when any LDS front of the level has nf > LDSB_SMALL_NF, else 'small' (run_level of do_backsub)"""
    return "wide" if max(f["nf"] for f in fronts if f["level"] == level and f["cls"] == 0) > LDSB_SMALL_NF else "small"


# ---------------------------------------------------------------------------------------------------------------- launch forms
# (switch, value) -> cases, each compared with the reference.  The default form of every case (no switch; test library only where a case
# names one) already runs lds_front_kernel<false, 256> at 64 / 128 / 256 threads (bin[24] / bin[48] / bin[49..72]), lds_front_kernel<false, 1024>
# (bin[73] on), lds_backsub_kernel (roots, children[k]), lds_backsub_wide_kernel (nf > 12) and, in deep_chain, lds_front_merged_kernel<256> at 64
# threads with lds_front_tiny, fill_upper_kernel and lds_backsub_merged_kernel.
_N73 = ("bin[73]", "bin[96]", "bin[97]", "bin[120]", "bin[121]", "bin[64,74]", "bin[65,73]", "bin[3,135]", "bin[135,3]", "bin[16,122]")
FORM_RUNS = [
    # merged elimination, 64 threads: lds_front_tiny at n = 15 / 16 and its neighbour the DATAFLOW body at 17; 0..3 children; the c2 branch
    (("LMGPU_MERGE_ELIM", "1"), ("tiny[15]", "tiny[16]", "tiny[17]", "tiny_tree", "tiny_sfm", "staging[8,8]",
                                 # 256 threads, DATAFLOW body = the eight-pivot code at n <= 72: pivot-group edges and both bin edges below 73
                                 "pivots[7]", "pivots[8]", "pivots[9]", "pivots[11]", "pivots[12]", "pivots[13]", "pivots[15]", "pivots[16]",
                                 "pivots[17]", "pivots[31]", "pivots[32]", "pivots[33]", "bin[25]", "bin[48]", "bin[49]", "bin[72]",
                                 "pivots[47]", "pivots[48]", "pivots[49]", "children[5]", "backsub_mixed",
                                 # lds_front_merged_kernel<1024> (both levels wider than 72): sixteen-pivot panels, the extend-add's 64-column chunks
                                 "bin[64,74]", "bin[65,73]", "bin[16,122]", "children_wide", "backsub[14,124]")),
    # the per-level launches where the library would merge
    (("LMGPU_MERGE_ELIM", "0"), ("deep_chain",)),
    # lds_backsub_merged_kernel away from n = 13: 64-column chunks of S x_S, the 32-row stride of y, ragged levels, ns = 0 roots
    (("LMGPU_MERGE_BACKSUB", "1"), ("children_wide", "children[5]", "backsub_mixed", "bin[25]", "bin[65,73]", "backsub[129,6]", "backsub[15,123]",
                                    "tiny_tree", "pivots[2]")),
    (("LMGPU_MERGE_BACKSUB", "0"), ("deep_chain",)),
    # lds_front_kernel<false, 256> with four waves and four pivots where sixteen waves are the default
    (("LMGPU_NO_WIDE16", "1"), _N73 + tuple(f"pivots_wide[{nf}]" for nf in PIVOT_WIDE_NF) + ("children_wide",)),
    # the general descriptor path in place of the packed record
    (("LMGPU_NO_LEAFPACK", "1"), tuple(f"staging[{k}]" for k in STAGING_COUNTS) + ("staging_pose3[7]", "staging_pose3[8]", "staging_mixed", "staging[8,8]",
                                                                                  "staging[9,8]", "tiny[15]", "tiny[16]", "tiny[17]", "tiny_tree", "tiny_sfm")),
    # level_fused_kernel<256>
    (("LMGPU_FUSE_LEVELS", "1"), ("fused_level",)),
]
# graph replay (read by both libraries): three solves, captured at the second; deep_chain replays by default, these two are shallow
GRAPH_RUNS = ("children[3]", "bin[25]")
GRAPH_PASSES = PASSES + ((1e-4, True),)  # the third solve is the second replay: its lambda has to arrive too
FORM_ARGUMENT = {("LMGPU_MERGE_ELIM", "1"): dict(merge_elim=True), ("LMGPU_MERGE_ELIM", "0"): dict(merge_elim=False),
                 ("LMGPU_MERGE_BACKSUB", "1"): dict(merge_backsub=True), ("LMGPU_MERGE_BACKSUB", "0"): dict(merge_backsub=False),
                 ("LMGPU_NO_WIDE16", "1"): dict(no_wide16=True), ("LMGPU_NO_LEAFPACK", "1"): {}, ("LMGPU_FUSE_LEVELS", "1"): dict(fuse_levels=True),
                 ("LMGPU_GRAPH", "1"): {}, ("LMGPU_GRAPH", "0"): {}}

BLOCK = dc.BLOCK


@functools.lru_cache(maxsize=None)
def oracle_floor(name, passes=PASSES):
    """schur_cases.floor_of over the passes with the blocked reference"""
    import schur_cases as sc
    return sc.floor_of(case(name), passes, BLOCK)


# ---------------------------------------------------------------------------------------------------------------- marginals (the unit right-hand side)
MARGINAL_RUNS = (("tiny[16]", ("LMGPU_MERGE_ELIM", "1")), ("bin[25]", None), ("children[3]", None))


def marginal_keys(c):
    """one variable of a leaf front (the first eliminated) and one of the root (the last)"""
    order = list(c["ordering"])
    return int(order[0]), int(order[-1])


def covariance_block(ref, key):
    """the block of (R^T R)^-1 of variable `key`, in the reference's extended precision: R^T y = e, R x = y for the variable's unit vectors"""
    R, n = ref.R[:, :ref.n], ref.n
    c0, d = ref.off[key], ref.dims[key]
    Y = np.zeros((n, d), dtype=R.dtype)
    Y[c0:c0 + d] = np.eye(d, dtype=R.dtype)
    for j in range(n):
        Y[j] = (Y[j] - R[:j, j] @ Y[:j]) / R[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - R[j, j + 1:] @ Y[j + 1:]) / R[j, j]
    return Y[c0:c0 + d]


def block_deviation(got, want):
    return float(np.abs(np.asarray(got, dtype=want.dtype) - want).max() / np.abs(want).max())


def marginal_tolerance(oracle_deviation, widest):
    return max(FACTOR * oracle_deviation, 64 * widest * EPS)
