"""CPU test: the ticket order of every chained launch, with the parameters the PRODUCT runs, is a topological order of the waits.

chain_kernel's workgroups draw tickets in a loop (kernels_step.hpp).  Its progress argument -- the holder of the lowest unfinished
ticket waits for nothing -- rests on the list the product builds: far rows from 50 % of the front, update tiles as merged pairs of
steps, 60 % of a block's update tasks in front of its row-panel workgroups (struct DevSwitches: chain_far_pct, chain_merge,
chain_split_pct).  test_dense_schedule.py checks the plain order (far_pct = 100) only.

lmgpu_selftest_chain_schedule takes the three parameters in one integer: far_pct + 1000 (merged pairs) + 100000 x (split_pct + 1)."""
import pytest

from gtsam_personal_amd import _lib
from test_dense_schedule import CHAIN, CHAIN_SHAPES, SINGLE, SPLIT_EVENTS, schedule

PRODUCT_ORDER = 50 + 1000 + 100000 * 61


@pytest.mark.parametrize("mode", [SINGLE, SPLIT_EVENTS])
def test_product_ticket_order_is_a_topological_order_of_the_waits(mode):
    lib = _lib.load()
    assert len(CHAIN_SHAPES) == 8
    checked = 0
    for n, nf in CHAIN_SHAPES:
        for kind, i0, nsteps, _ in schedule(n, nf, mode):
            if kind == CHAIN:
                assert lib.lmgpu_selftest_chain_schedule(n, nf, i0, nsteps, PRODUCT_ORDER) == 0, (n, nf, i0, nsteps)
                checked += 1
    assert checked >= (8 if mode == SINGLE else 20)
