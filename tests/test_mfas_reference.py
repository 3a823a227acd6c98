"""CPU tests of MFAS: the numpy restatement (tests/mfas_restatement.py) against both known answers of gtsam/sfm/tests/testMFAS.cpp, the
library's tie rule, and the refusals of lmgpu_mfas_outlier_weights, which are decided on the host before any device is touched.  No GPU."""
import numpy as np
import pytest

import mfas_cases as c
import mfas_restatement as mr
from gtsam_personal_amd import MFAS, _lib


def test_ordering_weights2():
    """testMFAS.cpp:47-72: ordering {0, 1, 3, 2}; only the edge between 3 and 0 has an outlier weight, 0.5"""
    order, w = mr.mfas(c.REF_EDGES, c.REF_WEIGHTS2)
    assert order == c.REF_ORDER2
    for e, edge in enumerate(c.REF_EDGES):
        assert abs(w[e] - (0.5 if edge in ((3, 0), (0, 3)) else 0.0)) <= 1e-6


def test_ordering_weights1():
    """testMFAS.cpp:77-97: ordering {3, 0, 1, 2}, every outlier weight 0"""
    order, w = mr.mfas(c.REF_EDGES, c.REF_WEIGHTS1)
    assert order == c.REF_ORDER1
    assert np.abs(w).max() <= 1e-6


def test_tie_rule_lowest_key():
    """several roots: the lowest key first (the reference's unordered_map walk leaves it open); equal heuristics: the lowest key as well"""
    order, _ = mr.mfas([(5, 9), (2, 9), (7, 9)], [1.0, 1.0, 1.0])
    assert order == [2, 5, 7, 9]
    cyc = c.cycle(5, equal=True)
    order, w = mr.mfas(cyc["keys"], cyc["weights"][0])
    assert order == [0, 1, 2, 3, 4]  # 0 by the tie, then each removal leaves one root
    assert list(w) == [0, 0, 0, 0, 1.0]  # the closing edge 4 -> 0 is the feedback arc
    # without a root the largest (out + 1) / (in + 1) goes first, whatever its key
    order, _ = mr.mfas([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0)], [1.0, 1.0, 1.0, 5.0, 1.0])
    assert order[0] == 2  # heuristics: node 0: 2 / 3, node 1: 1, node 2: 7 / 2, node 3: 2 / 6


def test_sign_and_zero_weights():
    s = c.sign_cases()
    orders, w, total = mr.mfas_directions(s["keys"], weights=s["weights"])
    assert [int(k) for k in orders[0]] == [10, 30, 20, 40]  # 20 -> 30 written with -2 runs 30 -> 20
    assert [int(k) for k in orders[1]] == [20, 30, 10, 40]  # every sign flipped: 20 is the only root, then 30, then 10
    assert [int(k) for k in orders[2]] == [10, 20, 30, 40]  # all zero: every node is a root, ascending keys
    assert not w.any() and not total.any()


def test_sum_is_in_direction_order():
    g = c.random_graph(65, 48, seed=1)
    _, w, total = mr.mfas_directions(g["keys"], g["measured"], g["directions"])
    ref = np.zeros(len(g["keys"]))
    for d in range(48):
        ref += w[d]
    assert np.array_equal(total, ref) and (w >= 0).all() and w.any()


def test_weights_are_uncontracted_dot_products():
    g = c.random_graph(63, 2, seed=2)
    w = mr.edge_weights(g["measured"], g["directions"][1])
    m, d = g["measured"], g["directions"][1]
    assert np.array_equal(w, (m[:, 0] * d[0] + m[:, 1] * d[1]) + m[:, 2] * d[2])


@pytest.mark.parametrize("keys,msg", [([(1, 2), (3, 4), (1, 2)], "given twice"), ([(1, 2), (2, 1)], "given twice"), ([(1, 2), (3, 3)], "to itself")])
def test_duplicate_pairs_and_self_edges_are_refused(keys, msg):
    """the reference keeps its weights in a map keyed by the ordered pair: (a, b) twice overwrites, (a, b) with (b, a) makes absWeightOfEdge
    read only one of the two.  Restatement and library refuse both, the library before it looks for a device."""
    w = np.ones((1, len(keys)))
    with pytest.raises(ValueError, match=msg):
        mr.mfas(keys, w[0])
    with pytest.raises(ValueError, match=msg):
        MFAS.outlier_weights(np.array(keys, dtype=np.uint64), edgeWeights=w, device=-1)
    if len(set(keys)) == len(keys):  # the mirror's MFAS(edgeWeights) takes a dict, which cannot hold an ordered pair twice
        with pytest.raises(ValueError, match=msg):
            MFAS(edgeWeights={k: 1.0 for k in keys}, device=-1).computeOrdering()


def test_other_refusals_and_capacity():
    lib = _lib.load()
    assert lib.lmgpu_mfas_lds_node_capacity() == (120 * 1024) // 20
    keys = np.array([(1, 2), (2, 3)], dtype=np.uint64)
    with pytest.raises(ValueError, match="non-finite"):
        MFAS.outlier_weights(keys, edgeWeights=np.array([[1.0, np.nan]]), device=-1)
    with pytest.raises(_lib.LmgpuError, match="no device"):  # a valid input reaches the device check
        MFAS.outlier_weights(keys, edgeWeights=np.array([[1.0, 1.0]]), device=-1)


def test_dot_product_keeps_contraction_off():
    """__dmul_rn / __dadd_rn are plain * and + in the HIP headers, so what keeps the weight's three products and two sums from being fused
    into FMAs is the pragma at the head of mfas_dot_rn; the bitwise GPU tests see a fused build, this pins the source without a device"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gtsam_personal_amd", "csrc", "kernels_mfas.hpp")).read()
    body = re.search(r"double mfas_dot_rn\([^)]*\)\s*\{(.*?)\n\}", src, re.S).group(1)
    assert body.lstrip().startswith("#pragma clang fp contract(off)")
    assert "mfas_dot_rn(A.meas" in src and "fma" not in body
