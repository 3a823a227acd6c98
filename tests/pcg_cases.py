"""TEST INFRASTRUCTURE: the cases of the PCG edge tests (numpy only, no device) -- graphs at the sizes where the kernels of
csrc/kernels_pcg.hpp and the queueing loop pcg_solve_enqueue change behaviour.  EDGES names every such size as a predicate over
(nvars, ntot, nfac, dimensions present, factor types present, largest degree, designed failing slots);
test_pcg_edges_reference.py::test_every_edge_is_reached asserts that some case makes each true.

The ordering is Ordering.Natural (ascending key: what the optimizer takes under ITERATIVE), so a slot is the rank of a key.

  single          one Pose2, one prior
  block[...]      Pose2 / Point2 graphs (a prior on every pose, odometry, loop closures, one bearing-range factor per point): across the
                  six, nvars, ntot and nfac each take 255, 256 and 257 (the 256-thread guards of gram, chol and forward)
  mixed           all seven variable types and all 14 bucket factor types on the 50-digit fixture of the factor-bucket tests
                  (GeneralSFMFactor2 = key position 2; the 5- and 9-row priors; the 9-row chordal factor)
  hub             one Cal3_S2 and one Pose3 shared by 257 GeneralSFMFactor2; 57 points seen twice, 143 seen once; every point has a prior
                  (one view leaves a point's depth to lambda alone, and the floor of the comparison with it)
  stride          769 Pose2 = three full blocks + 1, priors everywhere, odometry: what a grid clamped to 1, 2 or 3 blocks strides over
  partials[n]     Pose2 chains of 65 536 and 65 537 poses added as arrays: 256 / 257 and 768 / 769 block partials
  weak_chain      40 Pose2, a prior on the first only: dozens of iterations are natural
  stop[K]         a chain of K 9-vectors (a unit prior on the first, chordal between factors with rotations): the matrix is T_K (x) I_9
                  up to an orthogonal change of basis, has K distinct eigenvalues under either preconditioner and damping mode, and CG
                  started from a right-hand side on the first variable ends after exactly K iterations -- gamma_K is rounding noise,
                  many orders below gamma_(K-1), which is what a test of a stop AT k = K needs
  indeterminate[3|2]  about 600 variables; three (two) points seen by ONE projection on the optical axis of an unrotated camera, at slots
                  in three (two) different 256-blocks: exactly singular 3 x 3 blocks under Gauss-Newton"""
from __future__ import annotations

import numpy as np

import factor_bucket_cases as fb
from gtsam_personal_amd.graph import (CAL3_S2, F_BEARING_RANGE_2D, F_BETWEEN_POSE2, F_CHORDAL_BETWEEN, F_PRIOR_CAL3_S2, F_PRIOR_CAM,
                                      F_PRIOR_POINT3, F_PRIOR_POSE2, F_PRIOR_POSE3, F_PRIOR_VEC9, F_PROJECTION, F_PROJECTION_BPS, F_SFM, F_SFM2,
                                      FACTOR_ARITY, N_DIAG, N_GAUSS, N_UNIT, POINT2, POINT3, POSE2, POSE3, VAR_DIM, VEC9, NonlinearFactorGraph,
                                      Values, noiseModel)

LAMBDA = 1e-3
STRIDE_CAPS = (None, 1, 2, 3)  # grid clamps of the stride case (None: the product's 2048)
CHUNK_MAX = (1, 15, 16, 17, 31, 32, 33)
STOP_K = (3, 16, 17)
RESETS = (1, 2, 16, 17)
K_CAL = (500.0, 500.0, 0.0, 320.0, 240.0)
INDETERMINATE_SLOTS = {"indeterminate[3]": (100, 300, 550), "indeterminate[2]": (300, 550)}

EDGES = {
    "one variable": lambda s: s["nvars"] == 1,
    **{"%s = %d" % (q, v): (lambda s, q=q, v=v: s[q] == v) for q in ("nvars", "ntot", "nfac") for v in (255, 256, 257)},
    "every variable dimension (2, 3, 5, 6, 9)": lambda s: s["dims"] >= {2, 3, 5, 6, 9},
    "every variable type": lambda s: s["vtypes"] == set(range(7)),
    "all 14 bucket factor types": lambda s: s["ftypes"] == set(range(14)),
    "key position 2 (GeneralSFMFactor2)": lambda s: F_SFM2 in s["ftypes"],
    "factor rows 5 and 9": lambda s: {F_PRIOR_CAL3_S2, F_PRIOR_VEC9, F_PRIOR_CAM, F_CHORDAL_BETWEEN} <= s["ftypes"],
    "an incidence list longer than a block": lambda s: s["max_degree"] >= 257,
    "a point seen once (one projection and its prior) beside a hub": lambda s: s["max_degree"] >= 257 and s["min_degree"] == 2,
    "three full blocks + 1 variables (stride)": lambda s: s["nvars"] == 769,
    "256 r.r partials, 768 p.q partials": lambda s: s["nvars"] == 65536 and s["ntot"] == 768 * 256,
    "257 r.r partials, 769 p.q partials": lambda s: s["nvars"] == 65537 and (s["ntot"] + 255) // 256 == 769,
    "singular blocks in three 256-blocks": lambda s: len({v // 256 for v in s["failing"]}) == 3,
    "singular blocks in two 256-blocks, none in the first": lambda s: len({v // 256 for v in s["failing"]}) == 2 and min(s["failing"]) >= 256,
    "3 iterations end the solve": lambda s: s["finite_termination"] == 3,
    "16 iterations end the solve (a chunk boundary)": lambda s: s["finite_termination"] == 16,
    "17 iterations end the solve (first of a chunk)": lambda s: s["finite_termination"] == 17,
    "a chain anchored at one end": lambda s: s["name"] == "weak_chain" and s["nfac"] == s["nvars"],
}


# ---------------------------------------------------------------- Pose2 worlds
def _pose2_truth(n, rng):
    th = np.cumsum(rng.normal(0.0, 0.25, n))
    step = rng.uniform(0.8, 1.2, n)
    xy = np.cumsum(np.stack([step * np.cos(th), step * np.sin(th)], axis=1), axis=0)
    return np.concatenate([xy, th[:, None]], axis=1)


def _relative(Ti, Tj):
    """T_i^-1 T_j of (n, 3) Pose2 arrays"""
    d = Tj[:, :2] - Ti[:, :2]
    c, s = np.cos(Ti[:, 2]), np.sin(Ti[:, 2])
    th = Tj[:, 2] - Ti[:, 2]
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], np.arctan2(np.sin(th), np.cos(th))], axis=1)


PRIOR2 = noiseModel.Diagonal.Sigmas([0.3, 0.2, 0.1])
ODOM2 = noiseModel.Diagonal.Sigmas([0.2, 0.25, 0.1])
LOOP2 = noiseModel.Diagonal.Sigmas([0.4, 0.3, 0.15])
BR2 = noiseModel.Diagonal.Sigmas([0.1, 0.2])


def _pose2_graph(name, n_pose, n_point=0, n_loop=0, priors="all", seed=0):
    """poses are keys 0 .. n_pose - 1, points follow.  Measurements come from a seeded truth, the initial values are the truth moved by
    a few centimetres and hundredths of a radian, so that b is not zero"""
    rng = np.random.default_rng([seed, n_pose, n_point, n_loop])
    T = _pose2_truth(n_pose, rng)
    init = T + rng.normal(0.0, 1.0, T.shape) * np.array([0.05, 0.05, 0.02])
    graph, values = NonlinearFactorGraph(), Values()
    for k in range(n_pose):
        values.insert(k, POSE2, init[k])
    pk = np.arange(n_pose)
    who = pk if priors == "all" else pk[:1]
    graph._add(F_PRIOR_POSE2, who.reshape(-1, 1), T[who], PRIOR2)
    if n_pose > 1:
        graph._add(F_BETWEEN_POSE2, np.stack([pk[:-1], pk[1:]], axis=1), _relative(T[:-1], T[1:]), ODOM2)
    if n_loop:
        i = rng.integers(0, n_pose - 2, n_loop)
        j = np.minimum(n_pose - 1, i + 2 + rng.integers(0, 5, n_loop))
        graph._add(F_BETWEEN_POSE2, np.stack([i, j], axis=1), _relative(T[i], T[j]), LOOP2)
    for p in range(n_point):
        i = int(rng.integers(0, n_pose))
        rel = rng.uniform(1.0, 3.0) * np.array([np.cos(0.7 * p + 0.3), np.sin(0.7 * p + 0.3)])
        c, s = np.cos(T[i, 2]), np.sin(T[i, 2])
        pt = T[i, :2] + np.array([c * rel[0] - s * rel[1], s * rel[0] + c * rel[1]])
        values.insert(n_pose + p, POINT2, pt + rng.normal(0.0, 0.05, 2))
        graph._add(F_BEARING_RANGE_2D, [[i, n_pose + p]], [np.arctan2(rel[1], rel[0]), np.hypot(rel[0], rel[1])], BR2)
    return dict(name=name, graph=graph, initial=values)


# (poses, points, loop closures): nfac = poses + (poses - 1) + loops + points
BLOCKS = {
    "block[ntot255,nfac255]": (85, 0, 86),
    "block[ntot256,nfac256]": (84, 2, 87),
    "block[ntot257,nfac257]": (85, 1, 87),
    "block[nvars255]": (255, 0, 3),
    "block[nvars256]": (254, 2, 0),
    "block[nvars257]": (256, 1, 5),
}


# ---------------------------------------------------------------- cases on the factor-bucket fixture
def _mixed():
    fx = fb.load()
    c = fb.Case("pcg", "mixed", fx)
    kinds = (N_DIAG, N_GAUSS, N_UNIT)
    p2, p3, v9 = fb._Chain(c, POSE2), fb._Chain(c, POSE3), fb._Chain(c, VEC9)
    weak = []

    def noise(ft, kind=None):
        f = len(c.factors)
        return fb.noise_for(ft, f, kinds[f % 3] if kind is None else kind)
    for ch in (p2, p3, v9):
        for j in range(3):
            ch.between(j, kinds[j])
        for j in range(4):
            ch.prior(j, kinds[(j + 1) % 3])
    for j in range(3):
        lm = c.var(POINT2, fb.split_vals(F_BEARING_RANGE_2D, fx["f%d_vals" % F_BEARING_RANGE_2D][j])[1])
        c.add(F_BEARING_RANGE_2D, [p2.key(j), lm], j, noise(F_BEARING_RANGE_2D))
        for ft in (F_PROJECTION, F_PROJECTION_BPS):
            pt = c.var(POINT3, fb.split_vals(ft, fx["f%d_vals" % ft][j])[1])
            c.add(ft, [p3.key(j), pt], j, noise(ft))
            weak.append(pt)
    K = c.var(CAL3_S2, fb.split_vals(F_SFM2, fx["f%d_vals" % F_SFM2][0])[2])
    c.add(F_PRIOR_CAL3_S2, [K], 0, noise(F_PRIOR_CAL3_S2, N_GAUSS))
    for j in range(3):
        pt = c.var(POINT3, fb.split_vals(F_SFM2, fx["f%d_vals" % F_SFM2][j])[1])
        c.add(F_SFM2, [p3.key(0), pt, K], j, noise(F_SFM2))
        c.add(F_PRIOR_POINT3, [pt], j, noise(F_PRIOR_POINT3))
        cam, lp = c.own(F_SFM, j)
        c.add(F_SFM, [cam, lp], j, noise(F_SFM))
        c.add(F_PRIOR_CAM, [cam], j, noise(F_PRIOR_CAM))
        weak.append(lp)
    for i, pt in enumerate(weak):  # seen by one projection: a prior of their own (not a fixture case), or lambda alone would hold their depth
        c.graph.add_PriorFactorPoint3(pt, c.values.at(pt) + np.array([0.02, -0.03, 0.05]) * (1 + i), noiseModel.Diagonal.Sigmas([0.1, 0.2, 0.15]))
    return dict(name="mixed", graph=c.graph, initial=c.values)


def _hub():
    fx = fb.load()
    c = fb.Case("pcg", "hub", fx)
    vals = fx["f%d_vals" % F_SFM2]
    pose, K = c.var(POSE3, fb.split_vals(F_SFM2, vals[0])[0]), c.var(CAL3_S2, fb.split_vals(F_SFM2, vals[0])[2])
    c.add(F_PRIOR_POSE3, [pose], 0, fb.noise_for(F_PRIOR_POSE3, 0, N_GAUSS))
    c.add(F_PRIOR_CAL3_S2, [K], 0, fb.noise_for(F_PRIOR_CAL3_S2, 0, N_DIAG))
    pts = [(c.var(POINT3, fb.split_vals(F_SFM2, vals[j % fb.NCASE])[1]), j % fb.NCASE) for j in range(200)]
    for f in range(257):
        pt, case = pts[f // 2] if f < 114 else pts[f - 57]
        c.add(F_SFM2, [pose, pt, K], case, fb.noise_for(F_SFM2, f, (N_DIAG, N_GAUSS, N_UNIT)[f % 3]))
    for j in range(200):  # every point has a prior: one view (or the same view twice) leaves its depth to lambda alone
        c.add(F_PRIOR_POINT3, [pts[j][0]], pts[j][1], fb.noise_for(F_PRIOR_POINT3, j, N_DIAG))
    return dict(name="hub", graph=c.graph, initial=c.values)


# ---------------------------------------------------------------- a chain of 9-vectors that CG ends in exactly K iterations
def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _stop(K):
    rng = np.random.default_rng([K, 9])
    graph, values = NonlinearFactorGraph(), Values()
    for k in range(K):
        values.insert(k, VEC9, rng.normal(size=9))
    graph.add_PriorFactorVec9(0, values.at(0) + rng.uniform(0.5, 1.5, 9), noiseModel.Unit.Create(9))
    for k in range(K - 1):
        graph.add_ChordalBetweenFactor(k, k + 1, _rotation(rng), 1.0)
    return dict(name="stop[%d]" % K, graph=graph, initial=values, finite_termination=K)


# ---------------------------------------------------------------- singular point blocks under Gauss-Newton
def _indeterminate(name):
    """slot s: a failing point where designed, else a camera if s % 3 == 0, else a point seen by the two cameras around it.  Cameras are
    unrotated, one unit apart along x; a failing point lies 5 in front of its camera's centre and is seen by that camera only, so the third
    column of its Jacobian is exactly zero"""
    failing = INDETERMINATE_SLOTS[name]
    n = 600
    graph, values = NonlinearFactorGraph(), Values()
    rng = np.random.default_rng(len(failing))
    cams = [s for s in range(n) if s % 3 == 0 and s not in failing]
    pos = {s: np.array([float(i), 0.0, 0.0]) for i, s in enumerate(cams)}
    pose_noise, px = noiseModel.Diagonal.Sigmas([1e-2] * 3 + [1e-1] * 3), noiseModel.Isotropic.Sigma(2, 1.0)
    fx_, fy_, _, u0, v0 = K_CAL
    for s in cams:
        values.insert_pose3(s, np.eye(3), pos[s])
        graph.add_PriorFactorPose3(s, np.eye(3), pos[s], pose_noise)
    for s in range(n):
        if s in pos:
            continue
        a = max(c for c in cams if c < s)
        later = [c for c in cams if c > s]
        b = later[0] if later else cams[cams.index(a) - 1]
        if s in failing:
            values.insert_point3(s, pos[a] + np.array([0.0, 0.0, 5.0]))
            graph.add_GenericProjectionFactor([u0 + 2.0, v0 - 1.0], px, a, s, K_CAL)
            continue
        p = 0.5 * (pos[a] + pos[b]) + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5), rng.uniform(5.0, 7.0)])
        values.insert_point3(s, p)
        for cam in (a, b):
            q = p - pos[cam]
            z = np.array([fx_ * q[0] / q[2] + u0, fy_ * q[1] / q[2] + v0]) + rng.normal(0.0, 1.0, 2)
            graph.add_GenericProjectionFactor(z, px, cam, s, K_CAL)
    return dict(name=name, graph=graph, initial=values, failing=tuple(failing))


def _table():
    T = {"single": lambda: _pose2_graph("single", 1)}
    for nm, (npose, npt, nloop) in BLOCKS.items():
        T[nm] = lambda nm=nm, a=npose, b=npt, c=nloop: _pose2_graph(nm, a, b, c, seed=1)
    T["mixed"], T["hub"] = _mixed, _hub
    T["stride"] = lambda: _pose2_graph("stride", 769, seed=2)
    for n in (65536, 65537):
        T["partials[%d]" % n] = lambda n=n: _pose2_graph("partials[%d]" % n, n, seed=3)
    T["weak_chain"] = lambda: _pose2_graph("weak_chain", 40, priors="first", seed=4)
    for K in STOP_K:
        T["stop[%d]" % K] = lambda K=K: _stop(K)
    for nm in INDETERMINATE_SLOTS:
        T[nm] = lambda nm=nm: _indeterminate(nm)
    return T


CASES = _table()
NAMES = list(CASES)
SHAPES = ["single"] + list(BLOCKS) + ["mixed", "hub"]


def shape_ks(name):
    """the iterations a case is compared at.  `single`: BlockJacobi solves one variable exactly, the float64 gamma_1 can be exactly 0, and
    with eps 0 the loop then ends by itself -- there is no second iteration to compare"""
    return (1,) if name == "single" else (1, 2, 4)


def case(name):
    c = CASES[name]()
    assert c["name"] == name
    return c


def factor_slots(graph, ordering):
    """(graph.size(), 3) slots of every factor's keys by graph index, -1 beyond the arity"""
    keys = np.array(list(ordering), dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    out = np.full((graph.size(), 3), -1, dtype=np.int64)
    for ftype, _, gi, fk, _, _, _ in graph.buckets():
        ar = FACTOR_ARITY[ftype]
        out[gi[:, None], np.arange(ar)[None, :]] = order[np.searchsorted(keys[order], fk.reshape(-1))].reshape(-1, ar)
    return out


def layout(c):
    """(factor slots, dimension of every slot) under Ordering.Natural"""
    keys = c["initial"].keys()
    assert keys == c["graph"].keys()
    return factor_slots(c["graph"], keys), np.array([VAR_DIM[c["initial"].type(k)] for k in keys], dtype=np.int64)


def stats(c):
    """what EDGES reads"""
    slots, dims = layout(c)
    deg = np.bincount(slots[slots >= 0], minlength=len(dims))
    v = c["initial"]
    return dict(name=c["name"], nvars=len(dims), ntot=int(dims.sum()), nfac=c["graph"].size(), dims=set(dims.tolist()),
                vtypes={v.type(k) for k in v.keys()}, ftypes={b[0] for b in c["graph"].buckets()}, max_degree=int(deg.max()),
                min_degree=int(deg.min()), failing=c.get("failing", ()), finite_termination=c.get("finite_termination", 0))
