"""Digests of the launch tables lmgpu_finalize_structure builds (lmgpu_debug_table_digest, test library), one line per
(problem, configuration, table), sorted:

    <problem> <configuration> <table> <entries> <fnv1a>

Two trees whose lines are equal build the same tables; that is how a change to the finalize path is held against its parent (run this file
in both, compare the outputs).  Structure-only handles by default, so it needs no GPU; --device N builds device handles, stopped after
finalize (no communicator, no values, no solve).

    python tests/tools/table_digest.py [--device N] [--problems SUBSTRING] > tables.txt
"""
import argparse
import ctypes as ct
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, LevenbergMarquardtOptimizer, LevenbergMarquardtParams,  # noqa: E402
                                PCGSolverParameters, _lib)

# the switches that change tables (read by the test library when the handle is created or finalized)
SWITCHES = [("LMGPU_SCHUR_SPLIT_DIAG", "1"), ("LMGPU_NO_LEAFPACK", "1"), ("LMGPU_NO_LEAF_GROUPS", "1"), ("LMGPU_NO_MED", "1"),
            ("LMGPU_FUSE_LEVELS", "0"), ("LMGPU_FUSE_LEVELS", "1"), ("LMGPU_MERGE_ELIM", "0"), ("LMGPU_MERGE_ELIM", "1"),
            ("LMGPU_MERGE_BACKSUB", "0"), ("LMGPU_MERGE_BACKSUB", "1"), ("LMGPU_NO_WIDE16", "1")]
# name -> (constructor keywords, switch, PCG selected before finalize)
CONFIGS = {"world1": ({}, None, False)}
for _w in (2, 4):
    for _r in range(_w):
        CONFIGS[f"world{_w}.rank{_r}"] = (dict(world_size=_w, rank=_r), None, False)
CONFIGS["split_root"] = (dict(split_root=True), None, False)
CONFIGS["pcg"] = ({}, None, True)
for _sw in SWITCHES:
    CONFIGS["=".join(_sw)] = ({}, _sw, False)


def problems():
    """name -> function returning (graph, initial, ordering)"""
    import backsolve_wide_cases as bw
    import bt_products_cases as bt
    import dense_front_cases as dc
    import lds_front_cases as lc
    import leaf_group_cases as lg
    import schur_cases as sc
    import schur_var_cases as sv
    from gtsam_personal_amd.synthetic import make_bal

    def of_case(get):
        return lambda: (lambda c: (c["graph"], c["initial"], c["ordering"]))(get())

    out = {}
    for mod, tag in ((dc, "dense"), (lc, "lds"), (sc, "schur"), (lg, "leaf_group"), (bt, "bt"), (bw, "backsolve_wide")):
        for name in mod.CASES:
            out[f"{tag}:{name}"] = of_case(lambda mod=mod, name=name: mod.case(name))
    out["schur_var:" + sv.NAME] = of_case(sv.case)
    for n_cam, n_pt, seed in ((64, 800, 7), (20, 300, 5), (24, 700, 5)):  # smoke(), tests/test_leaf_group_cases.py
        def bal(n_cam=n_cam, n_pt=n_pt, seed=seed):
            graph, initial, _, ordering = make_bal(n_cam=n_cam, n_pt=n_pt, obs_per_point=6, seed=seed)
            return graph, initial, ordering
        out[f"make_bal:{n_cam}x{n_pt}"] = bal
    return out


def digest(graph, initial, ordering, device=-1, switch=None, pcg=False, **kw):
    """[(table, entries, fnv1a)] of one handle, in the library's order"""
    _lib.use_test_library(True)
    params = LevenbergMarquardtParams()
    if pcg:
        params.linearSolverType, params.iterativeParams = "ITERATIVE", PCGSolverParameters(BlockJacobiPreconditionerParameters())
    if switch:
        os.environ[switch[0]] = switch[1]
    try:
        opt = LevenbergMarquardtOptimizer(graph, initial, ordering, params, device=device, finalize_only=True, **kw)
    finally:
        if switch:
            del os.environ[switch[0]]
        _lib.use_test_library(False)
    n = opt.lib.lmgpu_debug_table_digest(opt._h, 0, None, None, None)
    names, counts, hashes = ct.create_string_buffer(32 * n), (ct.c_uint64 * n)(), (ct.c_uint64 * n)()
    assert opt.lib.lmgpu_debug_table_digest(opt._h, n, names, counts, hashes) == n
    opt.close()
    return [(names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode(), counts[i], hashes[i]) for i in range(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", type=int, default=-1)
    ap.add_argument("--problems", default="", help="only the problems whose name contains this")
    args = ap.parse_args()
    lines = []
    for pname, make in problems().items():
        if args.problems not in pname:
            continue
        graph, initial, ordering = make()
        for cname, (kw, switch, pcg) in CONFIGS.items():
            try:
                for table, count, h in digest(graph, initial, ordering, args.device, switch, pcg, **kw):
                    lines.append(f"{pname} {cname} {table} {count} {h:016x}")
            except _lib.LmgpuError as e:  # a configuration the library refuses for this graph: the refusal is the line
                lines.append(f"{pname} {cname} refused: {e}")
    print("\n".join(sorted(lines)))


if __name__ == "__main__":
    main()
