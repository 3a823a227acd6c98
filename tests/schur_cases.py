"""Small seeded graphs that put the Schur-form front assembly (csrc/kernels_schur.hpp and the host tables built around gp_tmp /
gv_tmp in csrc/lmgpu.hip) at its list and shape boundaries.  Every case has a root that one panel (plus at most the tail) factors:
all the variety is in the gather in front of it and in the leaves below it.

A case is a dict: graph, initial, ordering, leaves.  `leaves` is the case's own visibility table, in elimination order:
(leaf key, nf, [(separator key, rows of the factor that links them)]) -- the tests count list lengths from it, not from the library.

  lists            17 cameras, 1333 points of two observations: camera 0 is co-seen with camera k by LIST_LENGTHS[k - 1] points,
                   no other pair is co-seen at all (write mode, 120 zero blocks).  Diagonal / rhs lists: camera 0 has 1333 entries,
                   camera k has LIST_LENGTHS[k - 1].  The points are shuffled, so every list interleaves with the others.
  leaf_degrees     17 cameras; points seen by 1, 2, 14, 15 (n = 139, the LDS maximum) and 16 (n = 148: an HBM front with nf = 3)
  wide_leaves      24 Pose3 + Pose3 leaves (nf = 6, 6-row factors) + Point3 landmarks (nf = 3, 2-row factors) in shared lists
  vec9             16 VEC9 + VEC9 leaves (nf = 9, 9-row factors), one leaf factor of precision 0
  dims_2_3         47 Pose2 + Point2 landmarks (nf = 2; n = 6 for one sighting) + Pose2 leaves (nf = 3, 3-row factors)
  factor_counts    17 cameras, camera k with exactly k + 1 leaf factors
  many_hbm_fronts  five dense Pose2 components (five HBM fronts), the first with gather leaves only
"""
import functools

import numpy as np

from gtsam_personal_amd import NonlinearFactorGraph, Ordering, Values, noiseModel
from gtsam_personal_amd.graph import VAR_DIM, C, L, P, X, camera_pack
from gtsam_personal_amd.synthetic import _expmap_pose, _lookat, project_bundler

LIST_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 128, 129, 256, 257, 260)
LDS_MAX_N = 139
RHS = "rhs"
K_S2 = [50.0, 50.0, 0.0, 50.0, 50.0]


def _ring(n, rng, radius=30.0):
    """n poses on a ring looking at the origin (the camera ring of synthetic.make_bal)"""
    ang = 2 * np.pi * np.arange(n) / n
    eyes = np.stack([radius * np.cos(ang), radius * np.sin(ang), rng.uniform(-3, 3, n)], axis=1)
    up = np.array([0.0, 0.0, 1.0])
    Rs, ts = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        Rs[i], ts[i] = _lookat(eyes[i], np.zeros(3), up)
    return Rs, ts


# ---------------------------------------------------------------------------------------------------------------- BAL-shaped
def covis_bal(n_cam, visibility, seed=0, cam_order=None):
    """SFM factors for an explicit list of camera sets (one per point), a weak PriorFactorCamera on every camera (the root's own
    factors), PriorFactorPoint3 on the points seen once; Schur ordering: points in list order, then the cameras in cam_order"""
    rng = np.random.default_rng(seed)
    Rs, ts = _ring(n_cam, rng)
    f = 500 + 20 * rng.uniform(-1, 1, n_cam)
    k1 = 1e-3 * rng.uniform(-1, 1, n_cam)
    k2 = 1e-4 * rng.uniform(-1, 1, n_cam)
    n_pt = len(visibility)
    pts = rng.uniform(-8, 8, (n_pt, 3))
    ci = np.array([c for vis in visibility for c in vis])
    pj = np.array([j for j, vis in enumerate(visibility) for _ in vis])
    z, depth = project_bundler(Rs[ci], ts[ci], f[ci], k1[ci], k2[ci], pts[pj])
    assert (depth > 0).all()
    z = z + rng.normal(0, 0.5, z.shape)
    graph, initial = NonlinearFactorGraph(), Values()
    cam_keys = np.array([C(i) for i in range(n_cam)], dtype=np.uint64)
    pt_keys = np.array([P(j) for j in range(n_pt)], dtype=np.uint64)
    graph.add_GeneralSFMFactor(z, noiseModel.Isotropic.Sigma(2, 1.0), cam_keys[ci], pt_keys[pj])
    for i in range(n_cam):
        graph.add_PriorFactorCamera(C(i), camera_pack(Rs[i], ts[i], f[i], k1[i], k2[i]), noiseModel.Isotropic.Sigma(9, 0.1))
    for j, vis in enumerate(visibility):
        if len(vis) == 1:
            graph.add_PriorFactorPoint3(P(j), pts[j], noiseModel.Isotropic.Sigma(3, 0.5))
    for i in range(n_cam):
        dR, dt = _expmap_pose(np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)]))
        initial.insert(C(i), 3, camera_pack(Rs[i] @ dR, ts[i] + Rs[i] @ dt, f[i], k1[i], k2[i]))
    noise_p = rng.normal(0, 0.05, (n_pt, 3))
    for j in range(n_pt):
        initial.insert_point3(P(j), pts[j] + noise_p[j])
    cam_order = list(range(n_cam)) if cam_order is None else list(cam_order)
    ordering = Ordering([P(j) for j in range(n_pt)] + [C(i) for i in cam_order])
    leaves = [(P(j), 3, [(C(c), 2) for c in vis]) for j, vis in enumerate(visibility)]
    return dict(graph=graph, initial=initial, ordering=ordering, leaves=leaves, visibility=[tuple(v) for v in visibility])


# ---------------------------------------------------------------------------------------------------------------- clusters
POSE2, POSE3, VEC9 = "Pose2", "Pose3", "VEC9"
_DIM = {POSE2: 3, POSE3: 6, VEC9: 9, "Point2": 2, "Point3": 3}


def _rel2(a, b):
    """Pose2 between: b in the frame of a (the between helper of test_gpu_parity's builders, which are closures there)"""
    c, s = np.cos(a[2]), np.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return [c * dx + s * dy, -s * dx + c * dy, np.arctan2(np.sin(b[2] - a[2]), np.cos(b[2] - a[2]))]


def _rand_rot(rng, scale=1.0):
    return _expmap_pose(np.concatenate([rng.normal(0, scale, 3), np.zeros(3)]))[0]


class _Cluster:
    """one connected component: a dense all-pairs cluster of `kind` (keys X(base + i)) and its leaves (keys L(base + j)).
    leaves: [(leaf kind, links)] in elimination order; leaf kind = the cluster's own kind, or 'Point3' (Pose3 clusters, seen through
    GenericProjectionFactor) / 'Point2' (Pose2 clusters, BearingRangeFactor2D).  A same-kind leaf j is linked by a between factor
    (leaf, cluster) when j + link position is even and (cluster, leaf) when odd, so both column positions of the factor occur.
    zero_precision: {(leaf index, link position)}: that VEC9 leaf factor gets precision 0."""

    def __init__(self, graph, initial, kind, n_cluster, leaves, rng, base=0, zero_precision=()):
        self.kind, self.n = kind, n_cluster
        ck = [X(base + i) for i in range(n_cluster)]
        lk = [L(base + j) for j in range(len(leaves))]
        self.cluster_keys, self.leaf_keys, self.leaves = ck, lk, []
        add = {POSE2: self._pose2, POSE3: self._pose3, VEC9: self._vec9}[kind]
        add(graph, initial, ck, lk, leaves, rng, set(zero_precision))

    def _record(self, key, leaf_kind, links, ck, rows):
        self.leaves.append((key, _DIM[leaf_kind], [(ck[c], rows) for c in links]))

    def _pose2(self, graph, initial, ck, lk, leaves, rng, _zp):
        n = len(ck)
        ang = 2 * np.pi * np.arange(n) / n
        truth = np.stack([10 * np.cos(ang), 10 * np.sin(ang), ang + np.pi / 2 + rng.normal(0, 0.2, n)], axis=1)
        model = noiseModel.Diagonal.Sigmas([0.3, 0.3, 0.1])
        for i in range(n):
            initial.insert_pose2(ck[i], *(truth[i] + rng.normal(0, [0.05, 0.05, 0.02])))
        for a in range(n):
            for b in range(a + 1, n):
                graph.add_BetweenFactorPose2(ck[a], ck[b], _rel2(truth[a], truth[b]), model)
        graph.add_PriorFactorPose2(ck[n - 1], list(truth[n - 1]), noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.02]))
        br = noiseModel.Diagonal.Sigmas([0.05, 0.2])
        for j, (lkind, links) in enumerate(leaves):
            if lkind == "Point2":
                p = rng.uniform(-5, 5, 2)
                initial.insert_point2(lk[j], p + rng.normal(0, 0.05, 2))
                for c in links:
                    q = _rel2(truth[c], [p[0], p[1], 0.0])
                    graph.add_BearingRangeFactor2D(ck[c], lk[j], np.arctan2(q[1], q[0]) + rng.normal(0, 0.02), np.hypot(q[0], q[1]) + rng.normal(0, 0.1), br)
                self._record(lk[j], lkind, links, ck, 2)
            else:
                t = np.array([rng.uniform(-12, 12), rng.uniform(-12, 12), rng.uniform(-3, 3)])
                initial.insert_pose2(lk[j], *(t + rng.normal(0, [0.05, 0.05, 0.02])))
                for pos, c in enumerate(links):
                    if (j + pos) % 2 == 0:
                        graph.add_BetweenFactorPose2(lk[j], ck[c], _rel2(t, truth[c]), model)
                    else:
                        graph.add_BetweenFactorPose2(ck[c], lk[j], _rel2(truth[c], t), model)
                self._record(lk[j], lkind, links, ck, 3)

    def _pose3(self, graph, initial, ck, lk, leaves, rng, _zp):
        n = len(ck)
        Rs, ts = _ring(n, rng)
        model = noiseModel.Diagonal.Sigmas([0.05, 0.05, 0.05, 0.2, 0.2, 0.2])

        def perturbed(R, t):
            dR, dt = _expmap_pose(np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)]))
            return R @ dR, t + R @ dt
        for i in range(n):
            initial.insert_pose3(ck[i], *perturbed(Rs[i], ts[i]))
        for a in range(n):
            for b in range(a + 1, n):
                graph.add_BetweenFactorPose3(ck[a], ck[b], Rs[a].T @ Rs[b], Rs[a].T @ (ts[b] - ts[a]), model)
        graph.add_PriorFactorPose3(ck[n - 1], Rs[n - 1], ts[n - 1], noiseModel.Diagonal.Sigmas([0.02, 0.02, 0.02, 0.1, 0.1, 0.1]))
        pix = noiseModel.Isotropic.Sigma(2, 1.0)
        for j, (lkind, links) in enumerate(leaves):
            if lkind == "Point3":
                p = rng.uniform(-5, 5, 3)
                initial.insert_point3(lk[j], p + rng.normal(0, 0.05, 3))
                for c in links:
                    q = Rs[c].T @ (p - ts[c])
                    assert q[2] > 0
                    z = [K_S2[0] * q[0] / q[2] + K_S2[3] + rng.normal(0, 0.5), K_S2[1] * q[1] / q[2] + K_S2[4] + rng.normal(0, 0.5)]
                    graph.add_GenericProjectionFactor(z, pix, ck[c], lk[j], K_S2)
                if len(links) == 1:
                    graph.add_PriorFactorPoint3(lk[j], p, noiseModel.Isotropic.Sigma(3, 0.5))
                self._record(lk[j], lkind, links, ck, 2)
            else:
                R, t = _rand_rot(rng), rng.uniform(-20, 20, 3)
                initial.insert_pose3(lk[j], *perturbed(R, t))
                for pos, c in enumerate(links):
                    if (j + pos) % 2 == 0:
                        graph.add_BetweenFactorPose3(lk[j], ck[c], R.T @ Rs[c], R.T @ (ts[c] - t), model)
                    else:
                        graph.add_BetweenFactorPose3(ck[c], lk[j], Rs[c].T @ R, Rs[c].T @ (t - ts[c]), model)
                self._record(lk[j], lkind, links, ck, 6)

    def _vec9(self, graph, initial, ck, lk, leaves, rng, zero_precision):
        n = len(ck)
        for i in range(n):
            initial.insert_vec9(ck[i], rng.normal(0, 1.0, 9))
        for a in range(n):
            for b in range(a + 1, n):
                graph.add_ChordalBetweenFactor(ck[a], ck[b], _rand_rot(rng), (1.0, 2.0, 0.5)[(a + b) % 3])
        graph.add_PriorFactorVec9(ck[0], rng.normal(0, 1.0, 9))
        for j, (lkind, links) in enumerate(leaves):
            assert lkind == VEC9
            initial.insert_vec9(lk[j], rng.normal(0, 1.0, 9))
            for pos, c in enumerate(links):
                prec = 0.0 if (j, pos) in zero_precision else (1.0, 4.0)[(j + pos) % 2]
                if (j + pos) % 2 == 0:
                    graph.add_ChordalBetweenFactor(lk[j], ck[c], _rand_rot(rng), prec)
                else:
                    graph.add_ChordalBetweenFactor(ck[c], lk[j], _rand_rot(rng), prec)
            self._record(lk[j], lkind, links, ck, 9)


def _components(specs, seed):
    """specs: [(kind, n_cluster, leaves, zero_precision)]; ordering: every leaf (component by component), then every cluster"""
    rng = np.random.default_rng(seed)
    graph, initial = NonlinearFactorGraph(), Values()
    comps = [_Cluster(graph, initial, kind, n, leaves, rng, base=1000 * i, zero_precision=zp) for i, (kind, n, leaves, zp) in enumerate(specs)]
    ordering = Ordering([k for c in comps for k in c.leaf_keys] + [k for c in comps for k in c.cluster_keys])
    return dict(graph=graph, initial=initial, ordering=ordering, leaves=[lf for c in comps for lf in c.leaves],
                roots=[c.cluster_keys for c in comps])


def cluster_with_leaves(kind, n_cluster, leaf_links, landmarks=(), zero_precision=(), seed=0):
    """a dense all-pairs cluster of `kind` plus leaves of the same kind, each linked to 1-3 cluster variables; ordered leaves first.
    landmarks (Pose3 only): the indices into leaf_links that are Point3 landmarks seen through GenericProjectionFactor instead"""
    leaves = [("Point3" if j in set(landmarks) else kind, tuple(links)) for j, links in enumerate(leaf_links)]
    return _components([(kind, n_cluster, leaves, zero_precision)], seed)


def pose2_point2(n_pose, sightings, pose_leaves=(), extra_components=(), seed=0):
    """a dense Pose2 cluster with Point2 landmarks seen through BearingRangeFactor2D (sightings: one pose tuple per landmark) and,
    after them, Pose2 leaves (pose_leaves: one link tuple each); extra_components: further (n_pose, sightings, pose_leaves) components
    of the same make, not connected to the first"""
    specs = [(POSE2, n, [("Point2", tuple(s)) for s in sight] + [(POSE2, tuple(s)) for s in pl], ())
             for n, sight, pl in [(n_pose, sightings, pose_leaves)] + list(extra_components)]
    return _components(specs, seed)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _case_lists():
    vis = [(0, k) for k, n in enumerate(LIST_LENGTHS, start=1) for _ in range(n)]
    perm = np.random.default_rng(101).permutation(len(vis))
    return covis_bal(17, [vis[i] for i in perm], seed=1)


def _without(*cams):
    return tuple(c for c in range(17) if c not in cams)


LEAF_DEGREES_VIS = [
    (1,), (0, 5), _without(2, 9, 16), _without(4, 16), _without(16),
    (4,), (3, 11), _without(5, 6, 7), _without(8, 12), (7, 16),
    (9,), (2, 14), _without(1, 15, 16), _without(3, 10), _without(6),
    (12,), (10, 13)]


def _case_leaf_degrees():
    return covis_bal(17, LEAF_DEGREES_VIS, seed=2)


def factor_counts_visibility():
    """camera k gets exactly k + 1 observations: camera 16 shares one point with each other camera (so the cameras form one clique
    once it is eliminated FIRST) and has one point of its own; the rest is paired largest-remaining first, then single points"""
    vis = [(k, 16) for k in range(16)] + [(16,)]
    need = {k: k for k in range(16)}
    while True:
        top = sorted((k for k in need if need[k] > 0), key=lambda k: (-need[k], k))
        if len(top) < 2:
            break
        a, b = sorted(top[:2])
        vis.append((a, b))
        need[a] -= 1
        need[b] -= 1
    for k, r in need.items():
        vis.extend([(k,)] * r)
    return vis


def _case_factor_counts():
    return covis_bal(17, factor_counts_visibility(), seed=3, cam_order=range(16, -1, -1))


WIDE_LEAVES = [  # (is landmark, links): the leaves that see pose 0 come as PPPP LLLL PLPL PL in its lists
    (0, (0,)), (0, (0, 5)), (0, (0, 7, 11)), (0, (0, 5)),
    (1, (0, 5)), (1, (0, 7)), (1, (0, 5, 11)), (1, (0, 3)),
    (0, (0, 3)), (1, (0, 3, 5)), (0, (0, 11)), (1, (0, 7, 11)),
    (0, (0, 5, 7)), (1, (0, 11)),
    (0, (3,)), (1, (2, 9, 17)), (0, (9, 17)), (1, (13, 20))]


def _case_wide_leaves():
    return cluster_with_leaves(POSE3, 24, [l for _, l in WIDE_LEAVES], landmarks=[j for j, (lm, _) in enumerate(WIDE_LEAVES) if lm], seed=4)


VEC9_LEAVES = [(0,), (0, 3), (1, 4, 9), (2,), (0, 5), (3, 7), (0, 1, 2), (0, 9), (0, 4, 12), (0,), (5, 9)]
VEC9_ZERO_PRECISION = [(4, 1)]  # leaf 4's factor to cluster variable 5


def _case_vec9():
    return cluster_with_leaves(VEC9, 16, VEC9_LEAVES, zero_precision=VEC9_ZERO_PRECISION, seed=5)


DIMS_SIGHTINGS = [(3,), (0, 10), (0, 3, 10, 20, 40), (20,), (3, 30), (1, 2, 3, 4, 5), (45,), (20, 21), (3, 10, 17, 30, 44)]
DIMS_POSE_LEAVES = [(3,), (0, 10), (3, 20, 30), (10,), (3, 40)]


def _case_dims_2_3():
    return pose2_point2(47, DIMS_SIGHTINGS, DIMS_POSE_LEAVES, seed=6)


def _case_many_hbm_fronts():
    return pose2_point2(47, [(3,), (0, 10), (3, 10, 20)], (),
                        extra_components=[(47, [(5,), (2, 30)], [(7, 9)]), (47, [], []), (47, [], []), (47, [], [])], seed=7)


CASES = dict(lists=_case_lists, leaf_degrees=_case_leaf_degrees, wide_leaves=_case_wide_leaves, vec9=_case_vec9,
             dims_2_3=_case_dims_2_3, factor_counts=_case_factor_counts, many_hbm_fronts=_case_many_hbm_fronts)
SWITCH_CASES = ("lists", "wide_leaves", "dims_2_3")
# lambda / damping-mode variants every comparison runs through (lambda = 0 is determinate in every case: all have priors)
DAMPINGS = ((0.0, False), (1e-3, False), (1e-2, True))


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---------------------------------------------------------------------------------------------------------------- counting
def leaf_n(leaf, dims):
    _, nf, links = leaf
    return nf + sum(dims[k] for k, _ in links) + 1


def gather_lists(leaves, dims, position):
    """the lists the host builds for the gather leaves (n <= 139), counted from the visibility table alone:
    pair lists {(a, b): [nf of the leaf, ...]} over the separator variables a <= b (by `position`) of every leaf plus RHS, without
    (RHS, RHS); factor lists {a: [rows of the leaf factor, ...]}.  Entries are in leaf (elimination) order."""
    pairs, factors = {}, {}
    for leaf in leaves:
        if leaf_n(leaf, dims) > LDS_MAX_N:
            continue
        _, nf, links = leaf
        sep = sorted((k for k, _ in links), key=lambda k: position[k]) + [RHS]
        for x in range(len(sep) - 1):
            for y in range(x, len(sep)):
                pairs.setdefault((sep[x], sep[y]), []).append(nf)
        for k, rows in links:
            factors.setdefault(k, []).append(rows)
    return pairs, factors


def groups_of_four(count, waves=None):
    """index groups the pairs kernel forms from a list: 1 wave up to 32 entries, else 4 waves with ceil(count / 4) entries each,
    every wave taking 64 entries at a time, four per group (the last group of a batch may be short)"""
    waves = waves or (1 if count <= 32 else 4)
    per = -(-count // waves)
    out = []
    for w in range(waves):
        b, e = min(count, w * per), min(count, (w + 1) * per)
        for base in range(b, e, 64):
            for g in range(base, min(e, base + 64), 4):
                out.append(list(range(g, min(g + 4, e, base + 64))))
    return out


# ---------------------------------------------------------------------------------------------------------------- comparing
def var_dims(c):
    return {k: VAR_DIM[c["initial"].type(k)] for k in c["ordering"]}


def reference(c, jacobians, fronts, lam, diagonal, block=0):
    """the dense extended-precision reference of case c from whitened Jacobians [Ab of factor g] and [(front keys, n frontal keys)];
    block: dense_reference's row-at-a-time form (0) or its blocked one (panel rows)"""
    from dense_reference import DenseReference
    fk = c["graph"].factor_keys_in_graph_order()
    return DenseReference(list(zip(fk, jacobians)), var_dims(c), lam, diagonal, fronts, block=block)


def deviations(ref, rsd_of_front, delta_by_key):
    """(max|X - X_ref| / max|X_ref| per front, relative 2-norm of delta - delta_ref)"""
    per_front = []
    for i in range(len(ref.fronts)):
        want = ref.front(i)
        got = np.asarray(rsd_of_front(i), dtype=np.longdouble)
        assert got.shape == want.shape, (i, got.shape, want.shape)
        per_front.append(float(np.abs(got - want).max() / np.abs(want).max()))
    dref = ref.delta()
    a = np.concatenate([np.asarray(delta_by_key[k], dtype=np.longdouble) for k in sorted(dref)])
    b = np.concatenate([dref[k] for k in sorted(dref)])
    return per_front, float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def floor_of(c, dampings, block=0, keep=None):
    """the float64 oracle against the reference built from the oracle's own Jacobians, over `dampings`: dict(rsd = largest per-front
    deviation, delta = largest delta deviation, residual = largest reference residual, detail = [(lam, diagonal, rsd, delta)]).
    keep: a list that receives (reference, oracle cliques, oracle delta) of every damping"""
    import oracle_harness as oh
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.linearize()
    jac = [orc.jacobian(g) for g in range(c["graph"].size())]
    out = dict(rsd=0.0, delta=0.0, residual=0.0, detail=[])
    for lam, diagonal in dampings:
        rc, delta, _, _ = orc.solve(lam, diagonal)
        assert rc == 0, lam
        cl = orc.cliques()
        ref = reference(c, jac, [(keys, nfk) for keys, nfk, _, _ in cl], lam, diagonal, block)
        per_front, dd = deviations(ref, lambda i: cl[i][2], delta)
        out["detail"].append((lam, diagonal, max(per_front), dd))
        out["rsd"], out["delta"], out["residual"] = max(out["rsd"], max(per_front)), max(out["delta"], dd), max(out["residual"], ref.residual)
        if keep is not None:
            keep.append((ref, cl, delta))
    return out


@functools.lru_cache(maxsize=None)
def oracle_floor(name):
    """floor_of the case `name` over DAMPINGS, with the row-at-a-time reference"""
    return floor_of(case(name), DAMPINGS)
