"""The tile roles of a fused / chained step (head quadrants, head 128-tiles, update tiles of a step that a later step of the same launch
continues) hand their C tile over WRITE-THROUGH: agent-scope relaxed atomic stores, every storing wave drains, workgroup barrier, one
lane adds to the flag -- no release fence (kernels_potrf.hpp: pdf_publish_wt; kernels_dense.hpp: store_c).  The consumers are unchanged.
The change moves bytes differently and computes nothing differently, so everything here is BITWISE.

The test library keeps the form this replaced (plain stores + release fence) under LMGPU_CHAIN_FENCED_TILES, and under
LMGPU_CHAIN_PREREAD a consumer that plain-loads the first row of every 16-row group of its C tile BEFORE it waits for the hand-off:
its CU's L1 then holds the bytes of before the hand-off, and a consumer load that was not behind the acquire would compute with them
(cdna_hip_programming.md Guideline 16, pitfall 3: a hand-off checked on cold lines only can pass and still be wrong).

Cases (tests/dense_front_cases.py, and one built here):
  chain[576]    a run of two steps: the smallest at which a tile of one step hands over to a tile of the next
  chain[1088]   a run of four: merged depth-512 pairs
  beyond_1024   1290 columns, a run of four: a tile that lives through three hand-offs
  root[2311]    nine full panels + a remainder of 7 rows, a run of eight steps, then the tail kernel: the smallest at which a far tile
                row idles and then delivers pairs to head tiles

Per case, once (shared by the tests): the FENCED form at the initial linearization with both passes of dc.PASSES (lambda = 1e-6 identity
damping, lambda = 1e-2 diagonal damping), then -- after a retract by the first delta -- the second pass at the new linearization.
  test 1  the default form repeats pass 0, retract, pass 1: delta and every front's [R S d] np.array_equal; root[2311] also goes through
          _check_solve against the oracle at its 1e-6, once
  test 2  default form + LMGPU_CHAIN_PREREAD: twenty solves at the initial linearization, alternating the two lambdas (the matrix
          changes between solves, a line left from the solve before would show), each bitwise the fenced result for its lambda, each
          with the launch counters of the case
  test 3  is part of both: a solve whose hand-off spin ran out (status[1] != 0) returns LMGPU_HIP_ERROR, and solve() raises
"""
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
FORM_SWITCHES = ("LMGPU_CHAIN_FENCED_TILES", "LMGPU_CHAIN_PREREAD")


@functools.lru_cache(maxsize=None)
def _case(name):
    if name != ROOT_2311:
        return dc.case(name)
    launches = dict(dc.front_launches(2311, 2312))  # panel 0, ONE chained launch of eight steps, the tail kernel
    assert launches == dict(panel=2, syrk=0, chain=1, panel_work=True), launches
    return dc.root_case(2311, 560, launches)


@contextlib.contextmanager
def _form(*switches):
    """the switches are read once, when the handle is made: set for the construction only"""
    saved = {k: os.environ.pop(k, None) for k in FORM_SWITCHES}
    os.environ.update({k: "1" for k in switches})
    try:
        yield
    finally:
        for k in FORM_SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _optimizer(c, *switches):
    with _form(*switches):
        return LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], LevenbergMarquardtParams(), device=0)


def _solve(opt, lam, diagonal):
    """(packed delta, [R S d] per front); raises when the solve ends with the hand-off-timeout status (status[1] != 0)"""
    _, d, _, _ = opt.solve(lam, diagonal)
    return d.copy(), [opt.front(i)[1] for i in range(opt.num_fronts())]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and len(got[1]) == len(want[1]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))


@functools.lru_cache(maxsize=None)
def _fenced(name):
    """the fenced form: dict(first = both passes at the initial linearization, second = pass 1 after the retract by pass 0's delta)"""
    c = _case(name)
    opt = _optimizer(c, "LMGPU_CHAIN_FENCED_TILES")
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    assert [dict(nf=f["nf"], n=f["n"], parent=f["parent"], cls=f["cls"]) for f in infos] == c["fronts"], infos
    opt.linearize()
    first = [_solve(opt, lam, diagonal) for lam, diagonal in dc.PASSES]
    opt.retract(first[0][0])
    opt.linearize()
    second = _solve(opt, *dc.PASSES[1])
    opt.close()
    assert not _same(first[1], second)  # the retract moved the linearization point
    return dict(first=first, second=second)


@pytest.mark.parametrize("name", NAMES)
def test_write_through_and_fenced_tiles_agree_bitwise(dev_switches, name):
    c, ref = _case(name), _fenced(name)
    opt = _optimizer(c)
    opt.linearize()
    got = _solve(opt, *dc.PASSES[0])
    assert _same(got, ref["first"][0]), name
    opt.retract(got[0])
    opt.linearize()
    assert _same(_solve(opt, *dc.PASSES[1]), ref["second"]), name
    opt.close()


def test_root_2311_against_the_oracle(dev_switches):
    c = _case(ROOT_2311)
    with _form():
        opt, orc, _ = _pair(c["graph"], c["initial"], c["ordering"])
    opt.linearize()
    orc.linearize()
    _check_solve(opt, orc, *dc.PASSES[0])
    opt.close()


@pytest.mark.parametrize("name", NAMES)
def test_consumer_with_warm_lines_reads_fresh_bytes(dev_switches, name):
    c, ref = _case(name), _fenced(name)
    opt = _optimizer(c, "LMGPU_CHAIN_PREREAD")
    opt.linearize()
    for k in range(20):
        opt.set_kernel_timing(1)  # (resets the launch counters)
        got = _solve(opt, *dc.PASSES[k & 1])
        kt = opt.kernel_times()
        assert _same(got, ref["first"][k & 1]), (name, k)
        seen = dict(panel=kt["panel"]["launches"], syrk=kt["syrk"]["launches"], chain=kt["chain"]["launches"], panel_work=kt["panel"]["work"] > 0)
        assert seen == c["launches"], (name, k, seen)
    opt.close()
