"""The resident form of chain_kernel: a chained launch starts min(tasks, workgroups the device holds at once) workgroups, and each
draws tickets in a loop until the list is exhausted (kernels_step.hpp).  The loop changes no arithmetic, no hand-off and no ticket
order, so everything here is BITWISE.

The product runs one workgroup per task (the resident form measured slower); the test library compiles
the loop.  There LMGPU_CHAIN_ONE_TASK=1 is the product's form (the same kernel, left behind its first task), and LMGPU_CHAIN_GRID=<n>
selects the resident form with a grid of n workgroups:
  0        the form's own grid ("default" below): min(tasks, resident workgroups)
  1        one workgroup does every task, in list order (no two workgroups are ever resident together)
  2        the smallest grid with a hand-off between two workgroups
  7        not a multiple of the XCD count
  513      one more than two workgroups per compute unit: the last one starts when another has ended

Cases (tests/dense_front_cases.py; root[2311] as in test_gpu_chain_writethrough.py):
  chain[576]    a run of two steps: the smallest hand-off between steps
  chain[1088]   a run of four: merged depth-512 pairs
  beyond_1024   1290 columns, a run of four
  root[2311]    a run of eight steps, then the tail kernel: a far tile row idles and then delivers pairs

Per case, once (shared by the tests): the ONE-TASK form at the initial linearization with both passes of dc.PASSES, then -- after a retract
by the first delta -- the second pass at the new linearization.
  test 1  every grid repeats pass 0, retract, pass 1: delta and every front's [R S d] np.array_equal, the launch counters of the case
          (chain = 1) in both solves
  test 2  root[2311] through _check_solve against the oracle at its 1e-6, once
  test 3  twenty solves on ONE handle, alternating the two lambdas (the matrix changes between solves: a flag, a ticket counter or an
          LDS line left from the solve before would show), each bitwise the one-task result for its lambda
No test provokes a hand-off timeout: a solve whose spin ran out raises in solve()."""
import contextlib
import functools
import os

import numpy as np
import pytest

import dense_front_cases as dc
from gtsam_personal_amd import LevenbergMarquardtOptimizer, LevenbergMarquardtParams
from test_gpu_parity import _check_solve, _pair

pytestmark = pytest.mark.gpu

ROOT_2311 = "root[2311]"
NAMES = ("chain[576]", "chain[1088]", "beyond_1024", ROOT_2311)
GRIDS = (None, 1, 2, 7, 513)
SWITCHES = ("LMGPU_CHAIN_ONE_TASK", "LMGPU_CHAIN_GRID", "LMGPU_CHAIN_FENCED_TILES", "LMGPU_CHAIN_PREREAD")


@functools.lru_cache(maxsize=None)
def _case(name):
    if name != ROOT_2311:
        return dc.case(name)
    launches = dict(dc.front_launches(2311, 2312))  # panel 0, ONE chained launch of eight steps, the tail kernel
    assert launches == dict(panel=2, syrk=0, chain=1, panel_work=True), launches
    return dc.root_case(2311, 560, launches)


@contextlib.contextmanager
def _form(**switches):
    """the switches are read once, when the handle is made: set for the construction only"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update({k: str(v) for k, v in switches.items()})
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _optimizer(c, **switches):
    with _form(**switches):
        return LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], LevenbergMarquardtParams(), device=0)


def _resident(c, grid):
    return _optimizer(c, LMGPU_CHAIN_GRID=0 if grid is None else grid)


def _solve(opt, c, lam, diagonal):
    """(packed delta, [R S d] per front), with the launch counters of the case; raises when the solve ends with the hand-off-timeout status"""
    opt.set_kernel_timing(1)  # (resets the launch counters)
    _, d, _, _ = opt.solve(lam, diagonal)
    kt = opt.kernel_times()
    seen = dict(panel=kt["panel"]["launches"], syrk=kt["syrk"]["launches"], chain=kt["chain"]["launches"], panel_work=kt["panel"]["work"] > 0)
    assert seen == c["launches"] and seen["chain"] == 1, seen
    return d.copy(), [opt.front(i)[1] for i in range(opt.num_fronts())]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and len(got[1]) == len(want[1]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))


@functools.lru_cache(maxsize=None)
def _one_task(name):
    """the one-task form: dict(first = both passes at the initial linearization, second = pass 1 after the retract by pass 0's delta)"""
    c = _case(name)
    opt = _optimizer(c, LMGPU_CHAIN_ONE_TASK=1)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"]) for f in infos] == c["fronts"], infos
    opt.linearize()
    first = [_solve(opt, c, lam, diagonal) for lam, diagonal in dc.PASSES]
    opt.retract(first[0][0])
    opt.linearize()
    second = _solve(opt, c, *dc.PASSES[1])
    opt.close()
    assert not _same(first[1], second)  # the retract moved the linearization point
    return dict(first=first, second=second)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_resident_workgroups_and_one_task_per_workgroup_agree_bitwise(dev_switches, name, grid):
    c, ref = _case(name), _one_task(name)
    opt = _resident(c, grid)
    opt.linearize()
    got = _solve(opt, c, *dc.PASSES[0])
    assert _same(got, ref["first"][0]), (name, grid)
    opt.retract(got[0])
    opt.linearize()
    assert _same(_solve(opt, c, *dc.PASSES[1]), ref["second"]), (name, grid)
    opt.close()


def test_root_2311_against_the_oracle(dev_switches):
    c = _case(ROOT_2311)
    with _form(LMGPU_CHAIN_GRID=0):
        opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    opt.linearize()
    orc.linearize()
    _check_solve(opt, orc, *dc.PASSES[0])
    opt.close()


@pytest.mark.parametrize("grid", (None, 7))
def test_twenty_solves_on_one_handle_leave_nothing_behind(dev_switches, grid):
    name = "chain[1088]"
    c, ref = _case(name), _one_task(name)
    opt = _resident(c, grid)
    opt.linearize()
    for k in range(20):
        assert _same(_solve(opt, c, *dc.PASSES[k & 1]), ref["first"][k & 1]), (grid, k)
    opt.close()
