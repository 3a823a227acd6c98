"""The launch tables of finalize (csrc/launch_tables.hpp) through their digests (lmgpu_debug_table_digest, test library), on structure-only
handles: no GPU.  tests/tools/table_digest.py holds a whole tree against another with the same records; here: the digest is a function
of the problem, and a device = -1 handle now holds the tables that used to be built behind the device check -- the packed leaf records,
the block back-substitution table, the medium fronts and the fused levels' task lists.

The three cases and what each must hold, from its fronts:
  fused_level (lds_front_cases, LMGPU_FUSE_LEVELS=1)  a medium front (nf 192) and an LDS front on level 0: packs, bsd, med_fronts, level_tasks
  lists (schur_cases)                                  gather leaves under one dense root: packs, bsd; the root takes the Schur gather, so
                                                       it is no medium front and med_fronts is empty
  medium_batch (dense_front_cases)                     several medium fronts on one level: packs, bsd, med_fronts
"""
import os
import sys

import pytest

import dense_front_cases as dc
import lds_front_cases as lc
import schur_cases as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import table_digest as td  # noqa: E402

CASES = {"fused_level": (lc, ("LMGPU_FUSE_LEVELS", "1")), "lists": (sc, None), "medium_batch": (dc, None)}
LATE_TABLES = {"fused_level": ("packs", "bsd", "med_fronts", "level_tasks"), "lists": ("packs", "bsd"), "medium_batch": ("packs", "bsd", "med_fronts")}


def digest_of(name, device=-1):
    module, switch = CASES[name]
    c = module.case(name)
    return td.digest(c["graph"], c["initial"], c["ordering"], device=device, switch=switch)


@pytest.mark.parametrize("name", list(CASES))
def test_digest_is_a_function_of_the_problem(name):
    a, b = digest_of(name), digest_of(name)
    assert a == b
    names = [t for t, _, _ in a]
    assert len(set(names)) == len(names), names
    for other in CASES:
        if other != name:
            assert {t: h for t, _, h in digest_of(other)} != {t: h for t, _, h in a}


@pytest.mark.parametrize("name", list(CASES))
def test_structure_only_handle_holds_the_late_tables(name):
    counts = {t: n for t, n, _ in digest_of(name)}
    print(name, counts)
    for table in LATE_TABLES[name]:
        assert counts[table] > 0, (name, table)
    for table in ("bs_parent", "bs_pos", "small", "levels.packs", "levels.backsub", "levels.med", "levels.fuse", "flags", "bsd_runs"):
        assert table in counts, table
