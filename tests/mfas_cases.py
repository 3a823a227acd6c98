"""TEST INFRASTRUCTURE: the inputs of the MFAS tests (CPU: restatement against the reference's known answers; GPU: device against
restatement).  A case is dict(keys (E, 2), and either weights (D, E) or measured (E, 3) with directions (D, 3))."""
import numpy as np

# gtsam/sfm/tests/testMFAS.cpp:25-32: the 1dSfM paper's example without node 4; the edge 3 -> 0 is the outlier
REF_EDGES = [(3, 2), (0, 1), (3, 1), (1, 2), (0, 2), (3, 0)]
REF_WEIGHTS1 = [2, 1.5, 0.5, 0.25, 1, 0.75]       # bad direction: the outlier is accepted
REF_WEIGHTS2 = [0.5, 0.75, -0.25, 0.75, 1, 0.5]   # good direction: the outlier is rejected
REF_ORDER1, REF_ORDER2 = [3, 0, 1, 2], [0, 1, 3, 2]


def reference_example():
    return dict(keys=np.array(REF_EDGES, dtype=np.uint64), weights=np.array([REF_WEIGHTS1, REF_WEIGHTS2], dtype=float))


def chain(n):
    """0 -> 1 -> ... -> n-1 with distinct weights, every other edge written backwards with a negative weight; keys spread out"""
    keys, w = [], []
    for i in range(n - 1):
        a, b = 7 * i + 3, 7 * (i + 1) + 3
        if i % 2:
            keys.append((b, a))
            w.append(-(1.0 + 0.01 * i))
        else:
            keys.append((a, b))
            w.append(1.0 + 0.01 * i)
    return dict(keys=np.array(keys, dtype=np.uint64), weights=np.array([w], dtype=float))


def cycle(n, equal):
    """a directed cycle: no root at the start, the heuristic picks; equal weights make every node tie (the lowest key goes first)"""
    keys = [(i, (i + 1) % n) for i in range(n)]
    w = [1.0] * n if equal else [1.0 + 0.125 * ((5 * i) % n) for i in range(n)]
    return dict(keys=np.array(keys, dtype=np.uint64), weights=np.array([w], dtype=float))


def random_graph(V, D, seed, per_node=6):
    """about per_node edges per node between distinct unordered pairs, unit measured directions with outliers, D unit projection
    directions; node keys are not contiguous"""
    rng = np.random.RandomState(seed)
    pos = rng.uniform(-10, 10, (V, 3))
    node_keys = np.sort(rng.choice(10 * V, V, replace=False)).astype(np.uint64)
    pairs = set()
    for i in range(V):  # connected: a ring, then random chords
        pairs.add((min(i, (i + 1) % V), max(i, (i + 1) % V)))
    want = (per_node * V) // 2
    while len(pairs) < want:
        a, b = rng.randint(0, V, 2)
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    pairs = sorted(pairs)
    order = rng.permutation(len(pairs))
    keys, meas = [], []
    for e in order:
        a, b = pairs[e]
        if rng.rand() < 0.5:
            a, b = b, a
        d = pos[b] - pos[a]
        if rng.rand() < 0.1:
            d = rng.uniform(-1, 1, 3)  # an outlier direction
        keys.append((node_keys[a], node_keys[b]))
        meas.append(d / np.linalg.norm(d))
    dirs = rng.normal(size=(D, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return dict(keys=np.array(keys, dtype=np.uint64), measured=np.array(meas), directions=dirs)


def sign_cases():
    """a negative weight flips its edge; a zero weight runs first -> second and leaves both sums alone (its head is still a root)"""
    keys = np.array([(10, 20), (20, 30), (10, 30), (30, 40)], dtype=np.uint64)
    return dict(keys=keys, weights=np.array([[1.0, -2.0, 0.5, 0.0], [-1.0, 2.0, -0.5, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=float))
