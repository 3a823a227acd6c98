"""Small seeded update sequences that put the cliques ISAM2's tree-walk kernels see (csrc/isam2.hpp: isam2_wildfire_kernel,
isam2_marginal_kernel, the tree products of the dog leg, isam2_tree_patch_kernel, isam2_mark_kernel) on either side of the sizes at which
those kernels change behaviour.  test_isam2_walk_reference.py computes from the ORACLE's tree that every edge of EDGES is reached and that
the restatement (isam2_walk_reference.py) reproduces the oracle; test_gpu_isam2_walk_edges.py compares the device with the restatement on
the DEVICE's tree.

The ordering is the case's own: `natural_order`, a stable sort of the columns by their constraint group, given to both sides.  Columns
come in ascending key order, so a tree is shaped by numbering the variables: a block of variables that are mutually adjacent (after the
fill of its first variable) and adjacent to a block of higher keys becomes one clique (nf, ns).  The merge rule of the reference (a child
whose separator has as many variables as the parent's whole clique joins the parent) is kept away the way lds_front_cases does it: a
parent has one last variable no child touches.  Keys are plain integers.

A case: dict(updates=[(graph, values, keys of the new factors)], marginals=[keys], threshold, radii).
  update 0 holds the whole graph (a batch elimination: every clique is replaced; by default the walk hands x over by value);
  update 1 adds one prior on the LAST variable of every root: the roots are re-eliminated, every other clique is an orphan that is hung
  back, dirty by its separator, solved from LDS or memory, compared with the threshold and kept.

What the variable types allow (Pose2 = 3 scalars, Point2 = 2; a Point2 only has bearing-range factors to poses, none to another point):
  * the landmarks of a block have the block's HIGHEST keys: the first pose sees every landmark, its elimination joins them, and the chain
    pose .. pose, landmark, landmark merges into one clique.  (With the landmarks first, two of them are siblings under the first pose
    and the merge rule takes only one.)
  * a root of (2, 0) would be a landmark alone in its component, which no factor type allows; the narrowest root is one Pose2, (3, 0),
    the case `lone`.
  * a child whose separator is the WHOLE root joins the root, so the wide root above (65, 258) has one pose more: (261, 0).

variablesReeliminated, as the reference counts it (ISAM2-impl / UpdateImpl::recalculateIncremental): the frontal variables of the removed top
PLUS the observed keys, the list not made unique; from 65 % of all variables on, the update is a batch one and the count is every variable
(`expected_reeliminated`).
"""
import functools

import numpy as np

from gtsam_personal_amd import NonlinearFactorGraph, Values, noiseModel

from schur_cases import _rel2

LDS_MAX_COLS = 139  # scalar columns (n - 1) of a clique staged in LDS; more: walked from memory
WL_GROUPS = 64

# edge -> predicate over the list of cliques (nf, ns, children) of a tree the oracle built; every edge must be true for some case
EDGES = {
    "root of one variable (3, 0)": lambda cl: any(c[:2] == (3, 0) for c in cl),
    "LDS nf = 32": lambda cl: any(c[0] == 32 and sum(c[:2]) <= 139 for c in cl),
    "LDS nf = 33": lambda cl: any(c[0] == 33 and sum(c[:2]) <= 139 for c in cl),
    "LDS nf = 63": lambda cl: any(c[0] == 63 and sum(c[:2]) <= 139 for c in cl),
    "LDS nf = 64": lambda cl: any(c[0] == 64 and sum(c[:2]) <= 139 for c in cl),
    "LDS nf = 65": lambda cl: any(c[0] == 65 and sum(c[:2]) <= 139 for c in cl),
    "LDS nf = 128": lambda cl: any(c[0] == 128 and sum(c[:2]) <= 139 for c in cl),
    "LDS nf = 129": lambda cl: any(c[0] == 129 and sum(c[:2]) <= 139 for c in cl),
    "LDS (3, 135)": lambda cl: any(c[:2] == (3, 135) for c in cl),
    "LDS n - 1 = 139": lambda cl: any(sum(c[:2]) == 139 for c in cl),
    "wide n - 1 = 140": lambda cl: any(sum(c[:2]) == 140 for c in cl),
    "wide nf = 64": lambda cl: any(c[0] == 64 and sum(c[:2]) > 139 for c in cl),
    "wide nf = 65": lambda cl: any(c[0] == 65 and sum(c[:2]) > 139 for c in cl),
    "wide nf = 128": lambda cl: any(c[0] == 128 and sum(c[:2]) > 139 for c in cl),
    "wide nf = 129": lambda cl: any(c[0] == 129 and sum(c[:2]) > 139 for c in cl),
    "wide ns = 0, nf > 256": lambda cl: any(c[0] > 256 and c[1] == 0 for c in cl),
    "wide ns > 256": lambda cl: any(c[1] > 256 for c in cl),
    "wide clique between a root and a leaf": lambda cl: any(sum(c[:2]) > 139 and c[1] > 0 and c[2] > 0 for c in cl),
    "1 child": lambda cl: any(c[2] == 1 for c in cl),
    "256 children": lambda cl: any(c[2] == 256 for c in cl),
    "257 children": lambda cl: any(c[2] == 257 for c in cl),
    "1 root": lambda cl: sum(c[3] for c in cl) == 1,
    "64 roots": lambda cl: sum(c[3] for c in cl) == WL_GROUPS,
    "65 roots": lambda cl: sum(c[3] for c in cl) == WL_GROUPS + 1,
    "more than 256 cliques, count no multiple of 4": lambda cl: len(cl) > 256 and len(cl) % 4 != 0,
    "more than 1024 scalars": lambda cl: sum(c[0] for c in cl) > 1024,
}


def natural_order(n_rows, n_cols, col_ptr, row_idx, cmember):
    """constrained natural order: the columns sorted by group, each group in the order given (ascending key)"""
    return np.argsort(np.asarray(cmember[:n_cols]), kind="stable").astype(np.int32)


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.truth, self.next_key = {}, 1
        self.graph, self.values = NonlinearFactorGraph(), Values()
        self.between = noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1])
        self.br = noiseModel.Diagonal.Sigmas([0.05, 0.4])
        self.prior = noiseModel.Diagonal.Sigmas([1.0, 1.0, 0.3])

    def poses(self, n, prior=True):
        out = []
        for _ in range(n):
            k, rng = self.next_key, self.rng
            self.next_key += 1
            t = np.array([rng.uniform(-15, 15), rng.uniform(-15, 15), rng.uniform(-3, 3)])
            self.truth[k] = t
            self.values.insert_pose2(k, *(t + rng.normal(0, [0.05, 0.05, 0.02])))
            if prior:
                self.graph.add_PriorFactorPose2(k, list(t + rng.normal(0, [0.1, 0.1, 0.05])), self.prior)
            out.append(k)
        return out

    def points(self, n):
        out = []
        for _ in range(n):
            k = self.next_key
            self.next_key += 1
            p = self.rng.uniform(-15, 15, 2)
            self.truth[k] = p
            self.values.insert_point2(k, p + self.rng.normal(0, 0.05, 2))
            out.append(k)
        return out

    def link(self, a, b):
        g, rng, ta, tb = self.graph, self.rng, self.truth[a], self.truth[b]
        if len(ta) == 2:
            a, b, ta, tb = b, a, tb, ta
        if len(tb) == 3:
            g.add_BetweenFactorPose2(a, b, list(np.array(_rel2(ta, tb)) + rng.normal(0, [0.05, 0.05, 0.02])), self.between)
        else:
            q = _rel2(ta, [tb[0], tb[1], 0.0])
            g.add_BearingRangeFactor2D(a, b, np.arctan2(q[1], q[0]) + rng.normal(0, 0.02), np.hypot(q[0], q[1]) + rng.normal(0, 0.1), self.br)

    def clique(self, frontal, separator=(), degree=2):
        """factors that make `frontal` (+ `separator`) one clique under the natural order: every landmark to every pose, the first pose
        to every other pose, and `degree` random links per pose"""
        everyone = list(frontal) + list(separator)
        poses = [k for k in everyone if len(self.truth[k]) == 3]
        for k in frontal:
            if len(self.truth[k]) == 2:
                for p in poses:
                    self.link(p, k)
        fp = [k for k in frontal if len(self.truth[k]) == 3]
        for k in separator:  # (a separator landmark: the first frontal pose sees it, the fill does the rest)
            if len(self.truth[k]) == 2:
                self.link(fp[0], k)
        for p in poses:
            if p != fp[0]:
                self.link(fp[0], p)
        for k in fp[1:]:
            for _ in range(degree):
                o = poses[self.rng.integers(len(poses))]
                if o != k:
                    self.link(k, o)

    def block(self, nf):
        """variables of nf scalars: poses, then the landmarks (the highest keys)"""
        b = (0, 2, 1)[nf % 3]
        assert nf >= 2 * b + 3
        return self.poses((nf - 2 * b) // 3) + self.points(b)

    def tail(self, keys, onto):
        """links the poses `keys` (made first: lower keys than everything) into a chain that ends at `onto`; returns its cliques"""
        chain = list(keys) + [onto]
        for a, c in zip(chain[:-1], chain[1:]):
            self.link(a, c)
        return [([a], [c]) for a, c in zip(chain[:-1], chain[1:])]


def _case(b, second_keys, marginals=(), threshold=1e-5, expect=(), **extra):
    """expect: the cliques by construction, [(frontal keys, separator keys)]"""
    extra["expect"] = sorted((tuple(f), tuple(sorted(s))) for f, s in expect)
    ups = [(b.graph, b.values, sorted(b.truth))]
    g2 = NonlinearFactorGraph()
    for i, k in enumerate(second_keys):
        s = 1.0 + 0.1 * (i % 7)
        g2.add_PriorFactorPose2(k, list(b.truth[k] + s * np.array([0.8, -0.6, 0.15])), noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.02]))
    ups.append((g2, None, sorted(second_keys)))
    return dict(updates=ups, marginals=list(marginals), threshold=threshold, **extra)


def pair_case(nf, ns, seed, tail=0):
    """clique (nf, ns) under a root of the separator plus one pose, (ns + 3, 0); tail: a chain of that many poses below the clique's first
    pose (so that the root is less than 65 % of the variables and the second update is an incremental one)"""
    b = _Builder(seed)
    tail_keys = b.poses(tail, prior=False)  # (no priors: a change at its end travels the whole chain)
    fr = b.block(nf)
    sep = b.block(ns)
    last = b.poses(1)
    b.clique(fr, sep)
    b.clique(sep + last)
    # marginals: the first and the last frontal variable of the clique (a landmark when it has one), the root's first and last
    return _case(b, last, marginals=[fr[0], fr[-1], sep[0], last[0]] + tail_keys[:1], expect=[(fr, sep), (sep + last, [])] + b.tail(tail_keys, fr[0]))


def wide_tree_case(seed):
    """a chain of 30 poses (so that the root is less than 65 % of the variables) under (3, 6) under (65, 258) under the root (261, 0):
    paths to the root run through a wide clique"""
    b = _Builder(seed)
    tail = b.poses(30, prior=False)
    z = b.poses(1)
    mid = b.block(65)
    root = b.poses(87)
    b.link(z[0], mid[3])
    b.link(z[0], mid[7])
    b.clique(mid, root[:86], degree=1)
    b.clique(root, degree=1)
    return _case(b, root[-1:], marginals=[tail[0], z[0], mid[0], mid[-1], root[0], root[-1]],
                 expect=[(z, [mid[3], mid[7]]), (mid, root[:86]), (root, [])] + b.tail(tail, z[0]))


def children_case(k, seed):
    """root (6, 0) of two poses with k single-landmark children (2, 3), each seen from the first pose only"""
    b = _Builder(seed)
    pts = b.points(k)
    x = b.poses(2)
    b.link(x[0], x[1])
    for p in pts:
        b.link(x[0], p)
    return _case(b, x[-1:], marginals=[pts[0], pts[-1], x[0]], expect=[([p], [x[0]]) for p in pts] + [(x, [])])


def forest_case(k, seed):
    """k components of four poses in a chain: a root (6, 0) and two cliques (3, 3) each"""
    b = _Builder(seed)
    lasts, expect = [], []
    for _ in range(k):
        p = b.poses(4)
        for i in range(3):
            b.link(p[i], p[i + 1])
        lasts.append(p[3])
        expect += [([p[0]], [p[1]]), ([p[1]], [p[2]]), (p[2:], [])]
    return _case(b, lasts, marginals=[1, lasts[-1]], expect=expect)


def lone_case(seed):
    """one Pose2 with a prior: the single-variable root (3, 0), no separator, no child"""
    b = _Builder(seed)
    x = b.poses(1)
    # (a second prior, tight in the angle alone: the Newton step is then well over 1.5^2 times the steepest-descent step, which the blend radius needs)
    b.graph.add_PriorFactorPose2(x[0], list(b.truth[x[0]] + np.array([1.2, -0.9, 0.002])), noiseModel.Diagonal.Sigmas([1.0, 1.0, 0.01]))
    return _case(b, x, marginals=x, expect=[(x, [])])


def chain_case(n, seed, anchors=(), anchor_sigma=1e-4, priors=False, **kw):
    """n Pose2 in a chain, the prior at the first (a leaf), the root {n - 1, n} at the other end; `anchors`: poses with a tight prior,
    across which a change at the root does not travel"""
    b = _Builder(seed)
    p = []
    for i in range(n):
        p += b.poses(1, prior=priors or i == 0)
    for i in range(n - 1):
        b.link(p[i], p[i + 1])
    for a in anchors:
        k = p[a]
        b.graph.add_PriorFactorPose2(k, list(b.truth[k] + b.rng.normal(0, [0.01, 0.01, 0.005])), noiseModel.Diagonal.Sigmas([anchor_sigma] * 3))
    c = _case(b, p[-1:], marginals=[p[0], p[n // 2], p[-1]], expect=[([p[i]], [p[i + 1]]) for i in range(n - 2)] + [(p[-2:], [])], **kw)
    c["builder"] = b
    return c


def pose3_case(seed):
    """four Pose3 in a chain with a prior each: the marginal kernel at dimension 6"""
    from gtsam_personal_amd.datasets import rot3_expmap
    rng = np.random.default_rng(seed)
    g, v = NonlinearFactorGraph(), Values()
    prior = noiseModel.Diagonal.Sigmas([0.1, 0.1, 0.1, 0.5, 0.5, 0.5])
    btw = noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.05, 0.2, 0.2, 0.2])
    Rs, ts = [], []
    for k in range(1, 5):
        R, t = rot3_expmap(rng.normal(0, 0.4, 3)), rng.uniform(-5, 5, 3)
        Rs.append(R)
        ts.append(t)
        v.insert_pose3(k, rot3_expmap(rng.normal(0, 0.02, 3)) @ R, t + rng.normal(0, 0.05, 3))
        g.add_PriorFactorPose3(k, R, t, prior)
    for i in range(3):
        g.add_BetweenFactorPose3(i + 1, i + 2, Rs[i].T @ Rs[i + 1], Rs[i].T @ (ts[i + 1] - ts[i]), btw)
    g2 = NonlinearFactorGraph()
    g2.add_PriorFactorPose3(4, Rs[3], ts[3] + np.array([0.3, -0.2, 0.1]), noiseModel.Diagonal.Sigmas([0.02] * 6))
    return dict(updates=[(g, v, [1, 2, 3, 4]), (g2, None, [4])], marginals=[1, 3, 4], threshold=1e-5,
                expect=[((1,), (2,)), ((2,), (3,)), ((3, 4), ())])


def epoch_case(seed, updates=262):
    """a chain of 12 poses anchored at the sixth; then `updates` - 1 priors on the last pose, alternating about its place: every update
    re-eliminates the root alone, the change runs down to the anchor and stops there"""
    c = chain_case(12, seed, anchors=(5,), anchor_sigma=1e-5, threshold=EPOCH_THRESHOLD)
    b = c["builder"]
    first = c["updates"][0]
    ups = [first]
    last = max(b.truth)
    for i in range(updates - 1):
        g = NonlinearFactorGraph()
        s = (1.0 if i % 2 == 0 else -1.0) * (1.0 + 0.05 * (i % 5))
        g.add_PriorFactorPose2(last, list(b.truth[last] + s * np.array([0.4, -0.3, 0.08])), noiseModel.Diagonal.Sigmas([0.2, 0.2, 0.08]))
        ups.append((g, None, [last]))
    c["updates"] = ups
    return c


# thresholds of the section-5 cases: the middle (geometric) of the widest gap of the per-clique changes the oracle's run shows
# (test_isam2_walk_reference.py recomputes the gap and holds every visited clique a factor 10 away)
DECAY_THRESHOLD = 5e-5      # decay[40]: 1.3e-7 | 2.5e-2, the walk stops at the anchor
TWO_ANCHOR_THRESHOLD = 1e-11  # decay[two anchors]: 1.1e-14 | 9.0e-9 (wider than 2.9e-6 | 5.5e-2): past the first anchor, stopped by the second
EPOCH_THRESHOLD = 1e-6      # below the anchor at most 3e-9 (first update), above it at least 3e-5 (last update)

BUILDERS = {
    "lone": lambda: lone_case(11),
    "pair[32,8]": lambda: pair_case(32, 8, 12),
    "pair[33,8]": lambda: pair_case(33, 8, 13),
    "pair[63,3]": lambda: pair_case(63, 3, 14),
    "pair[64,75]": lambda: pair_case(64, 75, 15),
    "pair[65,73]": lambda: pair_case(65, 73, 16),
    "pair[128,8]": lambda: pair_case(128, 8, 17),
    "pair[129,6]": lambda: pair_case(129, 6, 18),
    "pair[3,135]": lambda: pair_case(3, 135, 19, tail=30),
    "pair[65,75]": lambda: pair_case(65, 75, 20),
    "pair[64,78]": lambda: pair_case(64, 78, 21),
    "pair[128,12]": lambda: pair_case(128, 12, 22),
    "pair[129,12]": lambda: pair_case(129, 12, 23),
    "wide_tree": lambda: wide_tree_case(24),
    "children[1]": lambda: children_case(1, 25),
    "children[256]": lambda: children_case(256, 26),
    "children[257]": lambda: children_case(257, 27),
    "forest[1]": lambda: forest_case(1, 28),
    "forest[64]": lambda: forest_case(64, 29),
    "forest[65]": lambda: forest_case(65, 30),
    "chain[350]": lambda: chain_case(350, 31),
    "pose3": lambda: pose3_case(32),
    "decay[40]": lambda: chain_case(40, 33, anchors=(19,), threshold=DECAY_THRESHOLD),
    "decay[two anchors]": lambda: chain_case(30, 34, anchors=(9, 21), threshold=TWO_ANCHOR_THRESHOLD),
}
NAMES = list(BUILDERS)
THRESHOLD_NAMES = ["decay[40]", "decay[two anchors]"]
DOGLEG_NAMES = [n for n in NAMES if n not in THRESHOLD_NAMES]

# Dog-leg radii per case, one per branch of ComputeDoglegPoint: 0.5 ||dx_u||, sqrt(||dx_u|| ||dx_n||), 2 ||dx_n|| of the FIRST update, as the
# restatement on the oracle's tree gives them (test_isam2_walk_reference.py holds them a factor 1.5 from both norms)
RADII = {
    "lone": (0.00629493, 0.0995508, 1.57434),
    "pair[32,8]": (0.0132795, 0.106371, 0.852046),
    "pair[33,8]": (0.0108949, 0.0910872, 0.761539),
    "pair[63,3]": (0.0158383, 0.122585, 0.94878),
    "pair[64,75]": (0.0147976, 0.134883, 1.22949),
    "pair[65,73]": (0.0209266, 0.160989, 1.23849),
    "pair[128,8]": (0.00863301, 0.101601, 1.19572),
    "pair[129,6]": (0.0112091, 0.114948, 1.17878),
    "pair[3,135]": (0.0162465, 0.574733, 20.3316),
    "pair[65,75]": (0.0159824, 0.143494, 1.28833),
    "pair[64,78]": (0.0202547, 0.157194, 1.21996),
    "pair[128,12]": (0.0181624, 0.14639, 1.17991),
    "pair[129,12]": (0.0253769, 0.17469, 1.20253),
    "wide_tree": (0.00644492, 0.379774, 22.3787),
    "children[1]": (0.0217934, 0.12103, 0.672147),
    "children[256]": (0.0110405, 0.344177, 10.7294),
    "children[257]": (0.00919594, 0.320917, 11.1993),
    "forest[1]": (0.0112934, 0.0744096, 0.490268),
    "forest[64]": (0.0780742, 0.591942, 4.48798),
    "forest[65]": (0.0785576, 0.595458, 4.5135),
    "chain[350]": (0.124064, 4.58226, 169.245),
    "pose3": (0.0332297, 0.103693, 0.323575),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c["name"] = name
    c["radii"] = RADII.get(name)
    return c


def dims_of(c):
    """{key: scalars} over all updates"""
    from gtsam_personal_amd.graph import VAR_DIM
    out = {}
    for _, v, _ in c["updates"]:
        if v is not None:
            for k in v.keys():
                out[int(k)] = VAR_DIM[v.type(k)]
    return out


def replaced_keys(tree, new_factor_keys):
    """relinearization off: the frontal variables of every clique on the path from a new factor's keys to its root, in the tree BEFORE
    the update (a Tree of isam2_walk_reference); None tree: the first update replaces everything"""
    where = {}
    for i, c in enumerate(tree.cliques):
        for k in c["fk"]:
            where[k] = i
    out = set()
    for k in new_factor_keys:
        i = where.get(int(k), -1)
        while i >= 0:
            out.update(tree.cliques[i]["fk"])
            i = tree.cliques[i]["parent"]
    return out


def expected_reeliminated(tree_before, new_factor_keys, n_variables):
    """-> (replaced keys, ISAM2Result.variablesReeliminated) of an update that adds factors on `new_factor_keys` (no new variables)"""
    if tree_before is None:
        return None, n_variables
    rep = replaced_keys(tree_before, new_factor_keys)
    if len(rep) >= 0.65 * n_variables:
        return set(tree_before.keys), n_variables
    return rep, len(rep) + len(set(new_factor_keys))


def expected_shape(c):
    """the case's cliques in the form of Tree.shape(): the parent holds the separator's lowest key (the first to be eliminated)"""
    first = {}
    for f, _ in c["expect"]:
        for k in f:
            first[k] = f[0]
    return sorted((f, s, first[s[0]] if s else None) for f, s in c["expect"])


def clique_table(tree):
    """[(nf, ns, children, is root)] for EDGES"""
    return [(c["nf"], c["ns"], len(tree.children.get(i, [])), 1 if c["parent"] < 0 else 0) for i, c in enumerate(tree.cliques)]


def replay(c, solver, upto=None):
    """feeds the case's updates to `solver` (ISAM2 or OracleISAM2), reading delta after each; yields per update
    dict(i, new_keys, before (delta before the update), delta, cliques, reeliminated)"""
    before = {}
    for i, (g, v, new_keys) in enumerate(c["updates"][:upto]):
        r = solver.update(g, v)
        r = r if isinstance(r, dict) else r.as_dict()
        delta = solver.getDelta()
        yield dict(i=i, new_keys=new_keys, before=before, delta=delta, reeliminated=r["variablesReeliminated"])
        before = delta


# ------------------------------------------------------------------------------------------------ checks shared by the two test modules
# `make(threshold)` / `make_dogleg(radius)` return a fresh solver: OracleISAM2 on the CPU, ISAM2 on the device, both with natural_order and
# relinearization off.  Each check asserts and returns what it measured, dict(floor, dev, tol), for the tables in the modules' docstrings.
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def walk_step(tree, prev, st, threshold, exact=True):
    """one update's delta against wildfire(): the count of re-eliminated variables, the factor 10 between every visited clique's change and
    the threshold, bitwise equality where the restatement says untouched, the tolerance where it says kept"""
    import isam2_walk_reference as wr
    rep, count = expected_reeliminated(prev, st["new_keys"], len(tree.keys))
    assert st["reeliminated"] == count, (st["i"], st["reeliminated"], count)
    rep = set(tree.keys) if rep is None else rep
    ref, info = wr.wildfire(tree, st["before"], rep, threshold)
    f64, info64 = wr.wildfire(tree, st["before"], rep, threshold, np.float64)
    got, old = tree.vec(st["delta"], np.float64), tree.vec(st["before"], np.float64)
    kept = np.zeros(tree.n, dtype=bool)
    for c, i, i64 in zip(tree.cliques, info, info64):
        assert (i["visited"], i["dirty"], i["kept"]) == (i64["visited"], i64["dirty"], i64["kept"])
        if threshold > 0 and i["dirty"] and not i["replaced"]:
            assert i["change"] >= 10 * threshold or i["change"] <= 0.1 * threshold, (st["i"], c["fk"], i["change"], threshold)
        kept[c["fx"]] = i["kept"]
    if exact:
        assert np.array_equal(_bits(got[~kept]), _bits(old[~kept])), (st["i"], "a clique the walk leaves alone was written")
    floor = wr.deviation(f64[kept], ref[kept])
    tol = wr.tolerance(floor, tree.widest())
    dev = wr.deviation(got[kept], ref[kept])
    assert wr.FACTOR * floor <= wr.CAP, (st["i"], floor)
    assert dev <= tol, (st["i"], dev, tol)
    return dict(floor=floor, dev=dev, tol=tol, visited=sum(i["visited"] for i in info), kept=sum(i["kept"] for i in info),
                changes=sorted(i["change"] for i in info if i["dirty"] and not i["replaced"]))


def check_walk(c, make, threshold, exact=True, steps=None):
    """every update of the case (or those of `steps`) through walk_step; also the tree's shape after each"""
    import isam2_walk_reference as wr
    dims, solver, prev, out = dims_of(c), make(threshold), None, []
    for st in replay(c, solver):
        if steps is not None and st["i"] not in steps and st["i"] + 1 not in steps:
            prev = None
            continue
        tree = wr.Tree(solver.cliques(), dims)
        assert tree.shape() == expected_shape(c), st["i"]
        if steps is None or st["i"] in steps:
            assert prev is not None or st["i"] == 0
            out.append(walk_step(tree, prev, st, threshold, exact))
        prev = tree
    return solver, out


def merge(stats):
    return dict(floor=max(s["floor"] for s in stats), dev=max(s["dev"] for s in stats), tol=min(s["tol"] for s in stats))


def check_marginals(c, solver, dense=False):
    """marginalCovariance of the case's keys on the solver's present tree.  The floor is the solver's own operation in float64: two
    triangular solves per column (the device), or -- dense -- the inverse of the assembled R^T R (the oracle; that one is not held to the
    symmetry of 1e-14 of the largest entry test_gpu_marginals asks of the device)"""
    import isam2_walk_reference as wr
    tree = wr.Tree(solver.cliques(), dims_of(c))
    Rp, Rp64 = wr.global_R(tree), wr.global_R(tree, np.float64)
    out, inv = [], None
    for k in c["marginals"]:
        ref = wr.marginal_covariance(tree, k, R_pos=Rp)
        if dense:
            if inv is None:
                inv = np.linalg.inv(Rp64[0].T @ Rp64[0])
            at = Rp64[1][tree.off[k]:tree.off[k] + tree.dims[k]]
            floor = wr.deviation(inv[np.ix_(at, at)], ref)
        else:
            floor = wr.deviation(wr.marginal_covariance(tree, k, np.float64, R_pos=Rp64), ref)
        got = np.asarray(solver.marginalCovariance(k))
        assert got.shape == ref.shape, (k, got.shape)
        assert dense or np.max(np.abs(got - got.T)) <= 1e-14 * np.max(np.abs(got)), k
        tol, dev = wr.tolerance(floor, tree.widest()), wr.deviation(got, ref)
        assert wr.FACTOR * floor <= wr.CAP, (k, floor)
        assert dev <= tol, (k, dev, tol)
        out.append(dict(floor=floor, dev=dev, tol=tol))
    return merge(out)


RHO_BANDS = ((0.225, 0.275), (0.675, 0.825))  # within 10 % of 0.25 / 0.75: the case is moved, not asserted


def check_dogleg(c, make_dogleg):
    """the first update under ISAM2DoglegParams(radius, 0, ONE_STEP_PER_ITERATION) at the case's three radii: getDelta() is the dog-leg point
    at that radius, the radius afterwards follows from rho, whose model part is the tree's error at 0 and at the point"""
    import isam2_walk_reference as wr
    dims, out = dims_of(c), []
    g, v, _ = c["updates"][0]
    for branch, radius in enumerate(c["radii"]):
        solver = make_dogleg(radius)
        assert solver.doglegDelta() == radius
        solver.update(g, v)
        delta = solver.getDelta()
        tree = wr.Tree(solver.cliques(), dims)
        assert tree.shape() == expected_shape(c)
        ref, f64 = wr.dogleg_point(tree, radius), wr.dogleg_point(tree, radius, np.float64)
        for norm in (ref["nu"], ref["nn"]):
            assert radius >= 1.5 * norm or radius <= norm / 1.5, (radius, ref["nu"], ref["nn"])
        assert ref["branch"] == branch == f64["branch"], (radius, ref["branch"])
        floor = wr.deviation(f64["dx_d"], ref["dx_d"])
        tol, dev = wr.tolerance(floor, tree.widest()), wr.deviation(tree.vec(delta, np.float64), ref["dx_d"])
        assert wr.FACTOR * floor <= wr.CAP, floor
        assert dev <= tol, (radius, dev, tol)
        # rho = (f(x0) - f(x0 + dx_d)) / (M(0) - M(dx_d)): the nonlinear errors are the solver's, the model's are the restatement's
        rho = (solver.error(2) - solver.error(0)) / float(ref["M0"] - ref["M1"])
        assert rho >= 0 and not any(lo <= rho <= hi for lo, hi in RHO_BANDS), (radius, rho)
        want = wr.radius_after(radius, rho, ref["nd"])
        assert abs(solver.doglegDelta() - want) <= 1e-12 * want, (radius, rho, solver.doglegDelta(), want)
        out.append(dict(floor=floor, dev=dev, tol=tol, rho=rho))
    return out
