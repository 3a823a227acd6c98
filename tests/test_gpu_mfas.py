"""MFAS on the device against the numpy restatement (tests/mfas_restatement.py): orderings (integers) and outlier weights (doubles,
bitwise) EQUAL, with the node state in LDS and, through the test library's LMGPU_MFAS_GLOBAL switch, in global scratch."""
import os

import numpy as np
import pytest

import mfas_cases as c
import mfas_restatement as mr
from gtsam_personal_amd import MFAS

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["lds", "global"])
def form(request, dev_switches):
    if request.param == "global":
        os.environ["LMGPU_MFAS_GLOBAL"] = "1"
    yield request.param
    os.environ.pop("LMGPU_MFAS_GLOBAL", None)


_want = {}


def want(name, case):
    """the restatement's answer, computed once per case and shared by both forms"""
    if name not in _want:
        _want[name] = mr.mfas_directions(case["keys"], case.get("measured"), case.get("directions"), case.get("weights"))
    return _want[name]


def check(name, case, form):
    orders, w, total, stats = MFAS.outlier_weights(case["keys"], case.get("measured"), case.get("directions"), case.get("weights"))
    assert stats["global_state"] == (1 if form == "global" else 0) and stats["n_nodes"] == len(np.unique(case["keys"]))
    worders, ww, wtotal = want(name, case)
    assert orders.shape == worders.shape and np.array_equal(orders, worders), name
    assert np.array_equal(w.view(np.uint64), ww.view(np.uint64)), name  # bitwise
    assert np.array_equal(total.view(np.uint64), wtotal.view(np.uint64)), name
    return orders, w, total


def test_reference_example(form):
    orders, w, _ = check("reference", c.reference_example(), form)
    assert [int(k) for k in orders[0]] == c.REF_ORDER1 and [int(k) for k in orders[1]] == c.REF_ORDER2
    assert not w[0].any() and list(w[1]) == [0, 0, 0, 0, 0, 0.5]
    m = MFAS(edgeWeights=dict(zip(c.REF_EDGES, c.REF_WEIGHTS2)))
    assert m.computeOrdering() == c.REF_ORDER2 and m.computeOutlierWeights()[(3, 0)] == 0.5


@pytest.mark.parametrize("n", [64, 65, 257])
def test_chains(n, form):
    orders, w, _ = check(f"chain{n}", c.chain(n), form)
    assert [int(k) for k in orders[0]] == [7 * i + 3 for i in range(n)] and not w.any()


@pytest.mark.parametrize("equal", [False, True])
def test_cycles(equal, form):
    _, w, _ = check(f"cycle{equal}", c.cycle(67, equal), form)
    assert np.count_nonzero(w) == 1  # one feedback arc


@pytest.mark.parametrize("D", [1, 2, 48])
@pytest.mark.parametrize("V", [63, 64, 65, 255, 256, 257, 300])
def test_random_graphs(V, D, form):
    _, w, total = check(f"random{V}x{D}", c.random_graph(V, D, seed=1000 + V), form)
    assert w.any() and total.any()


def test_sign_and_zero_weights(form):
    orders, w, _ = check("signs", c.sign_cases(), form)
    assert [int(k) for k in orders[0]] == [10, 30, 20, 40] and [int(k) for k in orders[2]] == [10, 20, 30, 40] and not w.any()


def test_sum_against_a_fixed_order_sum(form):
    case = c.random_graph(129, 48, seed=77)
    _, w, total = check("sum129", case, form)
    ref = np.zeros(len(case["keys"]))
    for d in range(48):
        ref = ref + w[d]
    assert np.array_equal(total.view(np.uint64), ref.view(np.uint64))


def test_lds_request_above_the_default_limit(form):
    """3 300 nodes: 66 016 B of node state, above the 64 KiB a launch may ask for without the function attribute (3 276 nodes)"""
    case = c.random_graph(3300, 1, seed=9)
    _, w, _ = check("random3300x1", case, form)
    assert 3300 * 20 + 16 > 64 * 1024 and w.any()
