"""Device handles against structure-only ones, and the solve-time fill tables outside the enqueue path.

  * lmgpu_finalize_structure builds the same launch tables whether or not a device is bound: the digests (lmgpu_debug_table_digest) of a
    device handle equal those of a device = -1 handle of the same problem, table by table.  Finalize only, nothing is launched.
  * The clears and sentinel fills of a solve (ensure_fill_tables) are allocated before anything is queued: on lds_front_cases' fused_level
    under LMGPU_FUSE_LEVELS=1, one LM iteration behind an eager solve gives the same error whether the iteration's solve is replayed from
    a graph captured at that point (LMGPU_GRAPH=1) or queued eagerly (LMGPU_GRAPH=0).  An allocation or a synchronous copy inside
    do_eliminate / do_backsub would break the capture.  Tolerance: the one test_gpu_lds_front_edges.py holds this case's delta to
    (lds_front_cases.tolerances over the case's oracle floor: max(16 x floor, 64 n eps), 3.7e-12), relative to the error.
"""
import pytest

import lds_front_cases as lc
from gtsam_personal_amd import LevenbergMarquardtOptimizer
from test_table_digest import CASES, digest_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_device_handle_builds_the_tables_of_a_structure_only_handle(name):
    host, device = digest_of(name), digest_of(name, device=0)
    assert [t for t, _, _ in host] == [t for t, _, _ in device]
    for h, d in zip(host, device):
        assert h == d, (name, h, d)


def _error_after_one_iteration(c):
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"])
    opt.linearize()
    opt.solve(opt.lambda_())  # the eager solve: builds the dense schedules and the fill tables
    opt.iterate()             # LMGPU_GRAPH=1: its solve is captured here and replayed
    e = opt.error()
    opt.close()
    return e


def test_fused_level_iteration_under_graph_capture(monkeypatch, dev_switches):
    c = lc.case("fused_level")
    widths = [f["n"] for f in c["fronts"]]
    _, tol = lc.tolerances(lc.oracle_floor("fused_level"), widths)
    monkeypatch.setenv("LMGPU_FUSE_LEVELS", "1")
    monkeypatch.setenv("LMGPU_GRAPH", "0")
    eager = _error_after_one_iteration(c)
    monkeypatch.setenv("LMGPU_GRAPH", "1")
    replayed = _error_after_one_iteration(c)
    print(f"fused_level: error after one iteration, eager {eager:.17g}, replayed {replayed:.17g}, tolerance {tol:.2e}")
    assert abs(replayed - eager) <= tol * abs(eager)
