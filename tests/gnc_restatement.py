"""TEST INFRASTRUCTURE: plain-Python restatement of the reference's graduated non-convexity outer loop, the checker of the GNC feature.
It shares no code with the library: every outer iteration builds a NEW weighted NonlinearFactorGraph (new noise models) and hands it to
the frozen CPU oracle (oracle_harness.OracleProblem), exactly the way the reference rebuilds its graph.

Which reference lines each function restates (gtsam/nonlinear/GncOptimizer.h unless stated otherwise):
  chi2inv                      Chi2inv :38-40 (MATLAB's chi2inv; own series + bisection)
  default_thresholds           setInlierCostThresholdsAtProbability :130-137
  strip_robust                 the constructor's removal of noiseModel::Robust :63-73
  weighted_graph               makeWeightedGraph :396-416 (Gaussian::Information(w * information), stated per noise kind:
                               DIAG inverse sigmas * sqrt(w), UNIT -> DIAG of sqrt(w), GAUSS R * sqrt(w))
  factor_errors                nfg_[k]->error(values) :283, :297, :442, :452 = 0.5 ||b||^2 of the oracle's whitened jacobian(k) on the
                               UNWEIGHTED graph
  initial_weights              initializeWeightsFromKnownInliersAndOutliers :174-180
  initialize_mu                initializeMu :272-314
  update_mu                    updateMu :317-329
  check_mu / check_cost / check_weights / check_convergence     :332-393
  calculate_weights            calculateWeights :419-469
  gnc_optimize                 optimize :183-269 (GncParams.h:66-81 for the parameters)
gnc_optimize also reports, per outer iteration, how far each of the three convergence tests was from flipping (`margins`), so that a
test comparing the discrete outcome (number of outer iterations, stop reason) can assert that its input is not on an edge."""
from __future__ import annotations

import math

import numpy as np

import oracle_harness as oh
from gtsam_personal_amd.graph import FACTOR_ROWS, N_DIAG, N_GAUSS, N_ISO, N_UNIT, NoiseModel, NonlinearFactorGraph

GM, TLS = 0, 1
STOP = ("maxIterations", "cost", "weights", "mu", "mu <= 0 at initialisation", "nothing unknown")


def _gamma_p(a, x):
    """regularised lower incomplete gamma function by its power series"""
    if x <= 0:
        return 0.0
    term = 1.0 / a
    s = term
    n = 0
    while abs(term) > 1e-18 * abs(s) and n < 100000:
        n += 1
        term *= x / (a + n)
        s += term
    return s * math.exp(-x + a * math.log(x) - math.lgamma(a))


def chi2inv(alpha, dofs):
    lo, hi = 0.0, max(1.0, float(dofs))
    while _gamma_p(0.5 * dofs, 0.5 * hi) < alpha:
        hi *= 2
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _gamma_p(0.5 * dofs, 0.5 * mid) < alpha:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def records(graph):
    """[(ftype, keys, meas, model) | None] over the graph index"""
    rec = [None] * graph.size()
    for ftype, _, gi, keys, meas, _, models in graph.buckets():
        for i, g in enumerate(gi.tolist()):
            rec[g] = (ftype, keys[i], meas[i], models[i])
    return rec


def default_thresholds(graph, alpha=0.99):
    return np.array([1.0 if r is None else 0.5 * chi2inv(alpha, FACTOR_ROWS[r[0]]) for r in records(graph)])


def _rebuild(graph, model_of):
    """a new graph with model_of(index, model) in place of every noise model; empty slots are dropped (the oracle has none).
    Returns (graph, index map: new position -> graph index)"""
    out, index = NonlinearFactorGraph(), []
    for g, r in enumerate(records(graph)):
        if r is None:
            continue
        ftype, keys, meas, model = r
        out._add(ftype, [keys], [meas], model_of(g, model))
        index.append(g)
    return out, index


def strip_robust(graph):
    return _rebuild(graph, lambda g, m: NoiseModel(m.dim, m.kind, m.data))


def weighted_graph(graph, w):
    def model_of(g, m):
        sw = math.sqrt(w[g])
        if m.kind == N_GAUSS:
            return NoiseModel(m.dim, N_GAUSS, m.data * sw)
        with np.errstate(divide="ignore"):
            return NoiseModel(m.dim, N_DIAG, 1.0 / (m.invsigmas() * sw))  # the oracle takes sigmas
    return _rebuild(graph, model_of)


def factor_errors(graph, values, ordering):
    """unweighted r_k over the graph index (0 for an empty slot)"""
    g2, index = strip_robust(graph)
    orc = oh.OracleProblem(g2, values, ordering)
    orc.linearize()
    r = np.zeros(graph.size())
    for i, g in enumerate(index):
        b = orc.jacobian(i)[:, -1]
        r[g] = 0.5 * float(b @ b)
    return r


def initial_weights(n, known_out):
    w = np.ones(n)
    w[list(known_out)] = 0.0
    return w


def initialize_mu(r, barc, loss, exists=None):
    ks = range(len(r)) if exists is None else [k for k in range(len(r)) if exists[k]]
    if loss == GM:
        mu = 0.0
        for k in ks:
            mu = max(mu, 2 * r[k] / barc[k])
        return mu
    mu = math.inf
    for k in ks:
        if 2 * r[k] - barc[k] > 0:
            mu = min(mu, barc[k] / (2 * r[k] - barc[k]))
    if 0 <= mu < 1e-6:
        mu = 1e-6
    return mu if (mu > 0 and not math.isinf(mu)) else -1.0


def update_mu(mu, loss, mu_step):
    return max(1.0, mu / mu_step) if loss == GM else mu * mu_step


def check_mu(mu, loss):
    return loss == GM and abs(mu - 1.0) < 1e-9


def check_cost(cost, prev_cost, tol):
    return abs(cost - prev_cost) / max(prev_cost, 1e-7) < tol


def _round(w):
    return np.sign(w) * np.floor(np.abs(w) + 0.5)


def check_weights(w, loss, tol):
    if loss != TLS:
        return False
    return not bool((np.abs(w - _round(w)) > tol).any())


def check_convergence(mu, w, cost, prev_cost, loss, cost_tol, weights_tol):
    return check_cost(cost, prev_cost, cost_tol) or check_weights(w, loss, weights_tol) or check_mu(mu, loss)


def calculate_weights(r, barc, mu, loss, known_in=(), known_out=(), exists=None):
    n = len(r)
    w = initial_weights(n, known_out)
    known = set(known_in) | set(known_out)
    for k in range(n):
        if k in known or (exists is not None and not exists[k]):
            continue
        if loss == GM:
            w[k] = ((mu * barc[k]) / (r[k] + mu * barc[k])) ** 2
        else:
            upper, lower = (mu + 1) / mu * barc[k], mu / (mu + 1) * barc[k]
            with np.errstate(divide="ignore"):
                w[k] = float(np.sqrt(np.float64(barc[k] * mu * (mu + 1)) / np.float64(r[k])) - mu)
            if r[k] >= upper or w[k] < 0:
                w[k] = 0.0
            elif r[k] <= lower or w[k] > 1:
                w[k] = 1.0
    return w


def _base_optimize(graph, w, initial, ordering, base, base_params):
    """BaseOptimizer(makeWeightedGraph(w), state_, params).optimize(); returns (values dict, final error, iterations)"""
    gw, _ = weighted_graph(graph, w)
    orc = oh.OracleProblem(gw, initial, ordering)
    orc.lm_init(base_params)
    if base == "GN":
        orc.gn_optimize(base_params)
    else:
        orc.lm_optimize(base_params)
    st = orc.lm_state()
    return orc.values(), st["error"], st["iterations"]


def _values_like(initial, vals):
    out = initial.copy()
    for k, v in vals.items():
        out.update(k, v)
    return out


def gnc_optimize(graph, initial, ordering, base, base_params, loss=TLS, max_iterations=100, mu_step=1.4, cost_tol=1e-5, weights_tol=1e-4,
                 known_in=(), known_out=(), barc=None, weights=None):
    """returns dict(values, weights, mu, cost, prev_cost, iterations, stop, trace=[(mu, cost, wdev)], margins=[(cost, weights, mu)],
    base_iterations_total).  A margin is the relative distance of a convergence test's quantity from its threshold."""
    n = graph.size()
    rec = records(graph)
    exists = [r is not None for r in rec]
    barc = default_thresholds(graph) if barc is None else np.asarray(barc, dtype=float)
    w = initial_weights(n, known_out) if weights is None else np.asarray(weights, dtype=float).copy()
    vals, err, its = _base_optimize(graph, w, initial, ordering, base, base_params)
    total_its = its
    mu = initialize_mu(factor_errors(graph, initial, ordering), barc, loss, exists)
    prev_cost, cost = err, 0.0
    out = dict(trace=[], margins=[])
    n_unknown = n - (len(known_in) + len(known_out))
    if mu <= 0 or n_unknown == 0:
        out.update(values=vals, weights=w, mu=mu, cost=cost, prev_cost=prev_cost, iterations=0, stop=4 if mu <= 0 else 5,
                   base_iterations_total=total_its)
        return out
    stop, it = 0, 0
    for it in range(max_iterations + 1):
        if it == max_iterations:
            break
        r = factor_errors(graph, _values_like(initial, vals), ordering)
        w = calculate_weights(r, barc, mu, loss, known_in, known_out, exists)
        vals, cost, its = _base_optimize(graph, w, initial, ordering, base, base_params)
        total_its += its
        wdev = float(np.abs(w - _round(w)).max())
        out["trace"].append((mu, cost, wdev))
        rel = abs(cost - prev_cost) / max(prev_cost, 1e-7)
        out["margins"].append((abs(rel - cost_tol) / cost_tol, abs(wdev - weights_tol) / weights_tol if loss == TLS else math.inf,
                               abs(abs(mu - 1.0) - 1e-9) / 1e-9 if loss == GM else math.inf))
        if check_cost(cost, prev_cost, cost_tol):
            stop = 1
            break
        if check_weights(w, loss, weights_tol):
            stop = 2
            break
        if check_mu(mu, loss):
            stop = 3
            break
        mu = update_mu(mu, loss, mu_step)
        prev_cost = cost
    out.update(values=vals, weights=w, mu=mu, cost=cost, prev_cost=prev_cost, iterations=it, stop=stop, base_iterations_total=total_its)
    return out
