"""numpy restatement of the reference's MFAS (gtsam/sfm/MFAS.cpp:36-171), sequential: the checker of lmgpu_mfas_outlier_weights.
  graphFromEdges           :36-60    edge first -> second for weight >= 0, else second -> first; in / out sums accumulated in edge order
  selectNextNodeInOrdering :63-82    a node with inWeightSum < 1e-8, else the largest (out + 1) / (in + 1)
  removeNodeFromGraph      :94-112   one subtraction at each neighbour still in the graph
  computeOutlierWeights    :141-171  |w| where the destination precedes the source in the ordering
The reference walks an unordered_map, so its choice among several roots (and among equal heuristics) is unspecified; the library's rule,
restated here, is the LOWEST KEY.  It keeps its weights in a std::map keyed by the ordered pair, so a pair given twice overwrites and
(a, b) with (b, a) makes absWeightOfEdge read only one of the two: the library refuses an unordered pair given twice, and so does this.
Weights from directions: x dx + y dy + z dz, every product and sum rounded once (numpy float64 scalars do exactly that)."""
import numpy as np


def edge_weights(measured, direction):
    m, d = np.asarray(measured, dtype=np.float64).reshape(-1, 3), np.asarray(direction, dtype=np.float64).reshape(3)
    return np.array([np.float64(np.float64(z[0] * d[0]) + np.float64(z[1] * d[1])) + np.float64(z[2] * d[2]) for z in m])


def check_pairs(keys):
    seen = set()
    for a, b in keys:
        a, b = int(a), int(b)
        if a == b:
            raise ValueError("an edge from a node to itself")
        if (min(a, b), max(a, b)) in seen:
            raise ValueError("an unordered pair of nodes is given twice")
        seen.add((min(a, b), max(a, b)))


def mfas(keys, weights):
    """keys: E pairs; weights: E signed doubles -> (ordering [keys], outlier weights [E])"""
    check_pairs(keys)
    keys = [(int(a), int(b)) for a, b in keys]
    w = [float(x) for x in weights]
    nodes = sorted({k for e in keys for k in e})
    inw, outw = {k: 0.0 for k in nodes}, {k: 0.0 for k in nodes}
    adj = {k: [] for k in nodes}  # (neighbour, edge, neighbour is the source)
    for e, (a, b) in enumerate(keys):
        src, dst = (a, b) if w[e] >= 0 else (b, a)
        inw[dst] += abs(w[e])
        outw[src] += abs(w[e])
        adj[dst].append((src, e, True))
        adj[src].append((dst, e, False))
    alive, pos, ordering = set(nodes), {}, []
    while alive:
        choice = None
        for k in sorted(alive):
            if inw[k] < 1e-8:
                choice = k
                break
        if choice is None:
            best = None
            for k in sorted(alive):
                h = (outw[k] + 1) / (inw[k] + 1)
                if best is None or h > best:
                    best, choice = h, k
        for nb, e, nb_is_source in adj[choice]:
            if nb not in alive:
                continue
            if nb_is_source:
                outw[nb] -= abs(w[e])
            else:
                inw[nb] -= abs(w[e])
        alive.remove(choice)
        pos[choice] = len(ordering)
        ordering.append(choice)
    out = np.zeros(len(keys))
    for e, (a, b) in enumerate(keys):
        src, dst = (b, a) if w[e] < 0 else (a, b)
        out[e] = abs(w[e]) if pos[dst] < pos[src] else 0.0
    return ordering, out


def mfas_directions(keys, measured=None, directions=None, weights=None):
    """the batched form: -> (orderings (D, V), weights (D, E), per-edge sum in direction order (E,))"""
    if weights is None:
        weights = np.array([edge_weights(measured, d) for d in np.asarray(directions, dtype=np.float64).reshape(-1, 3)])
    weights = np.asarray(weights, dtype=np.float64).reshape(-1, len(keys))
    orders, outs = [], []
    for wrow in weights:
        o, x = mfas(keys, wrow)
        orders.append(o)
        outs.append(x)
    outs = np.array(outs)
    total = np.zeros(len(keys))
    for row in outs:  # in direction order, one addition each
        total = total + row
    return np.array(orders, dtype=np.uint64), outs, total
