"""One more case beside tests/schur_cases.py, for schur_var_kernel (csrc/kernels_schur.hpp): the per-variable walk that builds a
separator variable's (v, v) and (v, rhs) blocks from its leaf entries and its factor entries.

  var_lists        19 cameras, 807 points.  Camera k = 1..15 is co-seen with camera 0 by VAR_LENGTHS[k - 1] points of two
                   observations; cameras 16, 17, 18 share nested points with camera 0 -- 504 points seen by (0, 16, 17, 18), 8 more by
                   (0, 17, 18), 1 more by (0, 18) -- so their lists have 504, 512 and 513 entries at the cost of 513 points.
                   Every camera's leaf list and factor list have the same length (one 2-row factor per sighting): camera 0 has 807.
                   The points are shuffled.  (16, 17), (16, 18) and (17, 18) keep long OFF-diagonal pair lists (504, 504, 512).

The constants below restate the kernel's (SCHUR_VU, SCHUR_VAR_SHORT, SCHUR_VAR_WAVES, the 64-entry fetch); chunks() and rounds() are
the walk's index arithmetic, so that a test can count from the visibility table which boundaries a list length reaches.
"""
import functools

import numpy as np

import schur_cases as sc

VU = 8            # MFMAs in flight per wave and round: 8 leaf entries, or 16 factor entries (two 2-row factors per MFMA)
FETCH = 64        # entry records fetched at a time
SHORT = 32        # at most this many leaf entries and at most this many factor entries: the one-wave launch
WAVES = 8         # waves per variable in the other launch
VAR_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 39, 40, 41)
NESTED = ((504, (0, 16, 17, 18)), (8, (0, 17, 18)), (1, (0, 18)))
N_CAM = 19


def _case_var_lists():
    vis = [(0, k) for k, n in enumerate(VAR_LENGTHS, start=1) for _ in range(n)] + [cams for n, cams in NESTED for _ in range(n)]
    perm = np.random.default_rng(202).permutation(len(vis))
    return sc.covis_bal(N_CAM, [vis[i] for i in perm], seed=8)


NAME = "var_lists"


@functools.lru_cache(maxsize=None)
def case():
    return _case_var_lists()


@functools.lru_cache(maxsize=None)
def oracle_floor():
    """schur_cases.oracle_floor's method: the float64 oracle against the row-at-a-time reference over DAMPINGS"""
    return sc.floor_of(case(), sc.DAMPINGS)


def waves_of(n_leaf, n_factor):
    return 1 if n_leaf <= SHORT and n_factor <= SHORT else WAVES


def chunks(count, waves, factor):
    """entries per wave: contiguous chunks of ceil(count / waves), rounded up to even for a factor list"""
    per = -(-count // waves)
    if factor:
        per += per & 1
    return [max(0, min(count, (w + 1) * per) - min(count, w * per)) for w in range(waves)]


def rounds(chunk, factor):
    """entries per round of one wave's chunk: fetches of 64, rounds of 8 leaf entries / 16 factor entries inside a fetch"""
    per_round = VU * (2 if factor else 1)
    out = []
    for base in range(0, chunk, FETCH):
        cnt = min(FETCH, chunk - base)
        out.extend(min(per_round, cnt - e) for e in range(0, cnt, per_round))
    return out
