"""Dense fronts that put the root back-substitution's 128-row hops (hbm_backsolve_wide_kernel, csrc/kernels_dense.hpp) at their block
edges.  The fronts are the hub fronts of tests/dense_front_cases.py (same builder, same densities, same two passes); only the widths
are new.  A front of nf > 1024 frontal scalars whose 16 x 16 inverses are still its own takes one workgroup per 128-row block B; a
128-row block is eight 16-blocks of one 256-row panel of the factorisation.

  root[1025]            nine blocks, the last of 1 row
  root[1151]            the last block has 127 rows
  root[1152]            nine whole blocks
  root[1153]            ten blocks, the last of 1 row; the last 256-row panel is partial
  root[1280]            ten whole blocks, whole panels
  separator[1153,66]    the same partial block in a NON-root front (right-hand side from ywork, behind hbm_rhs_init_kernel), under an LDS
                        root of 69

Launch counters per solve: dense_front_cases.front_launches (the planner restated), as for the cases of that module.
"""
import functools

import dense_front_cases as dc

HOP = 128  # rows of a block of the wide form
ROOT_SIZES = (1025, 1151, 1152, 1153, 1280)
SEPARATOR = (1153, 66)
PASSES = dc.PASSES
SWITCH_HOP64 = "LMGPU_BACKSOLVE_HOP64"  # test library: the 64-row form (hbm_backsolve_dataflow2_kernel) in its place


def _root(nf, seed):
    launches = dict(dc.front_launches(nf, nf + 1))
    return dc.root_case(nf, seed, launches)


def _separator(nf, ns, seed):
    b = dc._Builder(seed)
    order, fronts = dc._with_parent(b, 0, nf, ns, 0)
    return b.case(order, fronts, dc.per_front_launches(fronts))


CASES = {f"root[{nf}]": functools.partial(_root, nf, 600 + i) for i, nf in enumerate(ROOT_SIZES)}
CASES[f"separator[{SEPARATOR[0]},{SEPARATOR[1]}]"] = functools.partial(_separator, SEPARATOR[0], SEPARATOR[1], 610)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle_floor(name):
    """schur_cases.floor_of over the two passes with the blocked reference, as dense_front_cases.oracle_floor"""
    import schur_cases as sc
    return sc.floor_of(case(name), PASSES, dc.BLOCK)


def blocks(nf):
    """[(first row, rows)] of the 128-row blocks of a front of nf frontal scalars"""
    return [(r, min(HOP, nf - r)) for r in range(0, nf, HOP)]
