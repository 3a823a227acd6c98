"""Small seeded graphs for lds_front_group_kernel (csrc/kernels_leaf.hpp): gather leaves eliminated four to a wave, one lane per
factor, 16 lanes per leaf.  Every case hangs its leaf level under ONE HBM-class root (wider than 139 columns): 20 Cal3Bundler cameras
(181 columns; a point seen by all of them, itself an HBM front, ties them together) or 50 Pose2 (151).  A level of at most 512 gather
leaves is one launch (the host merges its size bins), so every case is one bin launch, and the number of leaves of the case is the
number of leaves of that launch.

A case is a dict: graph, initial, ordering, leaves, unary.  `leaves` is the case's own table in elimination order, in the format of
tests/schur_cases.py: (leaf key, nf, [(separator key, rows of the factor that links them)]); `unary` maps a leaf key to the rows of its
unary factors.  eligible() and group_launches() restate the host's rule (lmgpu.hip, leaf_group_form) on that table alone.

  SFM cases (a leaf = a Point3; (cameras, 3-row priors) per leaf):
    sfm_counts   9 leaves with 1, 2, 9, 10, 15, 16, 17, 31 and 32 factors: a lane group that is nearly empty, the 16th lane, the first
                 lane of the second round, the packed record's cap.  No separator variable may occur twice in a leaf and a leaf is at
                 most 139 columns wide (15 cameras), so from 16 factors on the rest are priors on the point.  The 1-factor leaf is a
                 point seen once at sigma = 50 pixels and nothing else: two rows for three unknowns, held by the damping alone, with
                 R_22 small enough for the pivot-exponent test at lambda = 1e-6.  The launch is two full waves and a wave with one group.
    sfm_n1 / sfm_n3 / sfm_n4 / sfm_n5   launches of 1, 3, 4 and 5 leaves: less than a wave, a full wave, a wave and a group.
                 sfm_n3 holds the shape of C4's first point: camera factors and one 3-row unary prior.
    sfm_twice    sfm_n4 with one point observed twice from the same camera: two lanes would own the same columns -- the bin takes
                 lds_front_kernel<true>
    sfm_33       a leaf of 33 factors (15 cameras, 18 priors): no packed record -- the bin takes lds_front_kernel<true>
    sfm_single   one point seen once at sigma = 1 and no prior: at lambda = 0 its third pivot is 0 (the failure-status test)
  Planar cases (50 Pose2; schur_cases.pose2_point2):
    planar       Point2 landmarks through BearingRangeFactor2D: nf = 2, 2-row factors, separator blocks of 3; 1 .. 5 sightings
    planar_pose  the same with three Pose2 leaves (nf = 3, 3-row between factors): the launch takes the four-row instantiation
"""
import functools

import numpy as np

import schur_cases as sc
from gtsam_personal_amd import NonlinearFactorGraph, Ordering, Values, noiseModel
from gtsam_personal_amd.graph import C, P, camera_pack
from gtsam_personal_amd.synthetic import _expmap_pose, project_bundler

# the kernel's caps (csrc/kernels_leaf.hpp, LEAFGRP_*) and the packed record's (csrc/kernels_front.hpp)
MAXNF, MAXROWS, MAXSEP, LANES = 4, 4, 9, 16
MAXB, JCAP = 32, 704
LDS_MAX_N = 139
BIN_N = (24, 48, 72, 96, 120, 139)
MERGE_MAX = 512  # a level with at most this many gather leaves is one launch
N_CAM, N_POSE = 20, 50
PASSES = ((1e-6, False), (1e-2, True))

SFM_COUNTS = [  # (cameras, priors, priors first in the graph, pixel sigma)
    ((7,), 0, False, 50.0),
    ((0, 11), 0, False, 1.0),
    (tuple(range(2, 11)), 0, False, 1.0),
    (tuple(range(5, 15)), 0, False, 1.0),
    (tuple(range(0, 15)), 0, False, 1.0),
    (tuple(range(3, 18)), 1, False, 1.0),
    ((1, 9, 19), 14, True, 1.0),
    (tuple(range(6, 20)), 17, False, 1.0),
    (tuple(range(4, 19)), 17, True, 1.0),
]
SFM_N5 = [((0, 3), 0, False, 1.0), ((1, 4, 9, 16), 1, False, 1.0), ((2, 5, 7), 0, False, 1.0), ((0, 8, 12, 13, 19), 0, False, 1.0),
          ((6, 10), 2, True, 1.0)]


def sfm_case(points, seed, twice=()):
    """20 cameras on schur_cases' ring with a weak prior each; points: [(cameras, number of 3-row priors, priors before the camera
    factors in the graph, pixel sigma)]; twice: indices of points whose first camera observes them a second time.  One more point,
    eliminated after the others, is seen by all 20 cameras: 184 columns, an HBM front of its own, which makes the cameras one clique."""
    points = list(points) + [(tuple(range(N_CAM)), 0, False, 1.0)]
    rng = np.random.default_rng(seed)
    Rs, ts = sc._ring(N_CAM, rng)
    f = 500 + 20 * rng.uniform(-1, 1, N_CAM)
    k1 = 1e-3 * rng.uniform(-1, 1, N_CAM)
    k2 = 1e-4 * rng.uniform(-1, 1, N_CAM)
    pts = rng.uniform(-8, 8, (len(points), 3))
    graph, initial = NonlinearFactorGraph(), Values()
    leaves, unary = [], {}
    for j, (cams, n_prior, first, sigma) in enumerate(points):
        cams = list(cams) + ([cams[0]] if j in twice else [])
        ci = np.array(cams)
        z, depth = project_bundler(Rs[ci], ts[ci], f[ci], k1[ci], k2[ci], np.repeat(pts[j][None], len(ci), axis=0))
        assert (depth > 0).all()
        z = z + rng.normal(0, 0.5, z.shape)

        def priors():
            for _ in range(n_prior):
                graph.add_PriorFactorPoint3(P(j), pts[j] + rng.normal(0, 0.05, 3), noiseModel.Isotropic.Sigma(3, 0.5))

        if first:
            priors()
        graph.add_GeneralSFMFactor(z, noiseModel.Isotropic.Sigma(2, sigma), np.array([C(c) for c in cams], dtype=np.uint64),
                                   np.full(len(cams), P(j), dtype=np.uint64))
        if not first:
            priors()
        leaves.append((P(j), 3, [(C(c), 2) for c in cams]))
        unary[P(j)] = [3] * n_prior
    for i in range(N_CAM):
        graph.add_PriorFactorCamera(C(i), camera_pack(Rs[i], ts[i], f[i], k1[i], k2[i]), noiseModel.Isotropic.Sigma(9, 0.1))
        dR, dt = _expmap_pose(np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)]))
        initial.insert(C(i), 3, camera_pack(Rs[i] @ dR, ts[i] + Rs[i] @ dt, f[i], k1[i], k2[i]))
    for j in range(len(points)):
        initial.insert_point3(P(j), pts[j] + rng.normal(0, 0.05, 3))
    ordering = Ordering([P(j) for j in range(len(points))] + [C(i) for i in range(N_CAM)])
    return dict(graph=graph, initial=initial, ordering=ordering, leaves=leaves, unary=unary)


PLANAR_SIGHTINGS = [(3,), (0, 10), (0, 3, 10, 20, 40), (20,), (3, 30), (1, 2, 3, 4, 5), (45,), (20, 21), (3, 10, 17, 30, 44), (7, 49)]
PLANAR_POSE_LEAVES = [(3,), (0, 10), (3, 20, 30)]


def _planar(pose_leaves):
    c = sc.pose2_point2(N_POSE, PLANAR_SIGHTINGS, pose_leaves, seed=16)
    c["unary"] = {}
    return c


CASES = dict(
    sfm_counts=lambda: sfm_case(SFM_COUNTS, seed=11),
    sfm_n1=lambda: sfm_case(SFM_N5[:1], seed=12),
    sfm_n3=lambda: sfm_case(SFM_N5[:3], seed=13),
    sfm_n4=lambda: sfm_case(SFM_N5[:4], seed=14),
    sfm_n5=lambda: sfm_case(SFM_N5, seed=15),
    sfm_twice=lambda: sfm_case(SFM_N5[:4], seed=14, twice=(2,)),
    sfm_33=lambda: sfm_case(SFM_N5[:2] + [(tuple(range(0, 15)), 18, False, 1.0)], seed=17),
    planar=lambda: _planar(()),
    planar_pose=lambda: _planar(PLANAR_POSE_LEAVES),
)
# the instantiation of lds_front_group_kernel a case's launch takes (1: <2, 9, 3>, 2: <4, 9, 4>), None: the generic kernel
FORMS = dict(sfm_counts=1, sfm_n1=1, sfm_n3=1, sfm_n4=1, sfm_n5=1, sfm_twice=None, sfm_33=None, planar=1, planar_pose=2)
FACTOR_COUNTS = dict(sfm_counts=[1, 2, 9, 10, 15, 16, 17, 31, 32], sfm_n1=[2], sfm_n3=[2, 5, 3], sfm_n4=[2, 5, 3, 5], sfm_n5=[2, 5, 3, 5, 4],
                     sfm_twice=[2, 5, 4, 5], sfm_33=[2, 5, 33], planar=[len(s) for s in PLANAR_SIGHTINGS],
                     planar_pose=[len(s) for s in PLANAR_SIGHTINGS] + [len(s) for s in PLANAR_POSE_LEAVES])


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def single_observation_case():
    """sfm_single: sfm_n3 plus a point seen once (sigma = 1) without a prior, eliminated first"""
    return sfm_case([((5,), 0, False, 1.0)] + SFM_N5[:3], seed=18)


@functools.lru_cache(maxsize=None)
def oracle_floor(name):
    """schur_cases.floor_of over this module's PASSES"""
    return sc.floor_of(case(name), PASSES)


# ---------------------------------------------------------------------------------------------------------------- the host's rule, restated
def leaf_width(leaf, dims):
    _, nf, links = leaf
    return nf + sum(dims[k] for k in {k for k, _ in links}) + 1


def eligible(leaf, unary_rows, dims):
    """0: the leaf keeps the bin on lds_front_kernel<true>; 1: fine, nf <= 3 and binary factors of at most two rows; 2: fine"""
    _, nf, links = leaf
    if nf > MAXNF or not 1 <= len(links) + len(unary_rows) <= MAXB:
        return 0
    if len({k for k, _ in links}) != len(links):  # a separator variable seen by two factors
        return 0
    if any(r > MAXROWS for _, r in links) or any(r > MAXROWS for r in unary_rows) or any(dims[k] > MAXSEP for k, _ in links):
        return 0
    staged = sum(r * (nf + dims[k] + 1) for k, r in links) + sum(r * (nf + 1) for r in unary_rows)
    if staged > JCAP:  # no single-batch packed record
        return 0
    return 2 if nf > 3 or any(r > 2 for _, r in links) else 1


def group_launches(c):
    """[(leaves of the launch, form or 0)] over the gather-leaf launches of the case's leaf level, from its table alone"""
    dims = sc.var_dims(c)
    gather = [lf for lf in c["leaves"] if leaf_width(lf, dims) <= LDS_MAX_N]
    if len(gather) <= MERGE_MAX:
        bins = [gather] if gather else []
    else:
        bins = [[lf for lf in gather if lo < leaf_width(lf, dims) <= hi] for lo, hi in zip((0,) + BIN_N[:-1], BIN_N)]
        bins = [b for b in bins if b]
    out = []
    for b in bins:
        forms = [eligible(lf, c["unary"].get(lf[0], []), dims) for lf in b]
        out.append((len(b), 0 if 0 in forms else max(forms)))
    return out


def expected_group_launches(c):
    return sum(1 for _, form in group_launches(c) if form)


# ---- the way down: which back-substitution kernel a level's plain launch takes, restated (lmgpu.hip backsub_group_form)
BACKSUB_MAXNF, BACKSUB_NARROW_NF, BACKSUB_NARROW_NS = 4, 3, 96


def expected_backsub_groups(infos):
    """(levels whose LDS fronts all have nf <= 4: lds_backsub_group_kernel; how many of them in its <4, 9> form) from front_info records"""
    levels = {}
    for f in infos:
        if f["cls"] == 0:
            nf, ns = levels.get(f["level"], (0, 0))
            levels[f["level"]] = (max(nf, f["nf"]), max(ns, f["n"] - f["nf"] - 1))
    group = [(nf, ns) for nf, ns in levels.values() if nf <= BACKSUB_MAXNF]
    return len(group), sum(1 for nf, ns in group if nf > BACKSUB_NARROW_NF or ns > BACKSUB_NARROW_NS)


# what the cases are meant to reach: sfm_counts has a leaf of 15 cameras (135 separator columns): the <4, 9> form; the others <3, 6>
BACKSUB_FORMS = dict(sfm_counts=(1, 1), sfm_n1=(1, 0), sfm_n3=(1, 0), sfm_n4=(1, 0), sfm_n5=(1, 0), sfm_twice=(1, 0), sfm_33=(1, 1), planar=(1, 0),
                     planar_pose=(1, 0))

