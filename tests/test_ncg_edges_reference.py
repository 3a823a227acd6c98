"""The nonlinear conjugate gradient edge cases (tests/ncg_edge_cases.py) and their reference (tests/ncg_reference.py, the control rule
of tests/ncg_restatement.py), without a GPU.  This is the half of the pin that needs no device: it fixes the cases, the reference, the
tolerance of every comparison of tests/test_gpu_ncg_edges.py and the proof that each comparison sees what it is for.

The cases:
  * every predicate of ncg_edge_cases.EDGES is true for some case.
The reference on its own:
  * line_search, now ls_begin and a loop of ls_step, returns the bits the unsplit loop returned (a copy of it is kept below);
  * ls_step_planted without a defect is ls_step, bit for bit, on every control case.
What the device test relies on:
  * the tolerance of every vector comparison: floor = largest distance of the float64 runs (unpermuted and three seeded permutations of
    every sum) from the long-double run, tolerance = 16 x floor; 16 x floor < 1e-9 is asserted for every case (the cancellation cases'
    own floors are printed: with the per-element difference they stay at a few ulps too);
  * the r of prior[40], [41], [84], [85]: found again by the scan, the count unchanged under (1 +- eps) on every error, eps 1e-12 and
    1e-9, and the same count from the restatement over the CPU oracle on the graph itself;
  * the ascent direction and the all-zero direction never meet the exit test within NCG_MAX_TRIALS evaluations;
  * every planted defect is seen: a vector defect misses the tolerance of some case built for it by at least MARGIN; a control defect
    changes some record of some control case.
Measured: DESIGN section 14 (printed here as TABLE / DEFECT lines)."""
import math

import numpy as np
import pytest

import ncg_cases as nc
import ncg_edge_cases as ec
import ncg_reference as ref
import ncg_restatement as nr

MARGIN = 1e3


# ---------------------------------------------------------------- the cases
def test_every_edge_is_reached():
    vs = [ec.vector_stats(n) for n in ec.VECTOR_NAMES]
    cs = [ec.control_case(n) for n in ec.CONTROL_NAMES]
    qs = [ec.prior_trials(r)[1] for r in ec.RATIOS.values()]
    missing = [e for e, p in ec.VECTOR_EDGES.items() if not any(p(s) for s in vs)]
    missing += [e for e, p in ec.CONTROL_EDGES.items() if not any(p(c) for c in cs)]
    missing += [e for e, p in ec.QUEUE_EDGES.items() if not any(p(q) for q in qs)]
    assert not missing, missing
    assert ec.EDGES == {"vector": ec.VECTOR_EDGES, "control": ec.CONTROL_EDGES, "queue": ec.QUEUE_EDGES}


# ---------------------------------------------------------------- the split of line_search
def _line_search_unsplit(system, currentValues, gradient, stats=None):
    """lineSearch (.h:135-181) as tests/ncg_restatement.py had it before ls_begin / ls_step were cut out of it"""
    g = float(np.linalg.norm(gradient))
    phi = 0.5 * (1.0 + math.sqrt(5.0))
    resphi = 2.0 - phi
    tau = nr.TAU
    minStep = nr._div(-1.0, g)
    maxStep = 0.0
    newStep = minStep + (maxStep - minStep) / (phi + 1.0)
    newValues = system.advance(currentValues, newStep, gradient)
    newError = system.error(newValues)
    trials = 1
    while True:
        flag = (maxStep - newStep > newStep - minStep)
        testStep = newStep + resphi * (maxStep - newStep) if flag else newStep - resphi * (newStep - minStep)
        if (maxStep - minStep) < tau * (abs(testStep) + abs(newStep)):
            if stats is not None:
                stats["trials"] = trials
                stats["bracket"] = (minStep, maxStep)
            return 0.5 * (minStep + maxStep)
        testValues = system.advance(currentValues, testStep, gradient)
        testError = system.error(testValues)
        trials += 1
        if testError >= newError:
            if flag:
                maxStep = testStep
            else:
                minStep = testStep
        else:
            if flag:
                minStep = newStep
            else:
                maxStep = newStep
            newStep = testStep
            newError = testError


def _both(system, x, g):
    a, b = {}, {}
    return (nr.line_search(system(), x, g, a), a), (_line_search_unsplit(system(), x, g, b), b)


@pytest.mark.parametrize("a,x0,c", [(1.0, 0.7, 0.0), (4.0, 3.5, 3.0), (250.0, -1.0, -0.25), (1e3, 10.9, 10.0), (3.0, 1e-7, 0.0)])
def test_split_line_search_is_bit_identical_on_quadratics(a, x0, c):
    s = nr.Quadratic1D(a, c)
    new, old = _both(lambda: s, x0, s.gradient(x0))
    assert new == old


@pytest.mark.parametrize("trials", sorted(ec.RATIOS))
def test_split_line_search_is_bit_identical_on_the_prior(trials):
    x = np.array([ec.RATIOS[trials], 0.0, 0.0])
    for perturb in (None, 1e-12):
        mk = lambda: ec.PriorPoint3System(None if perturb is None else (perturb, np.random.default_rng(1)))  # noqa: E731
        new, old = _both(mk, x, x.copy())
        assert new == old and new[1]["trials"] == trials


@pytest.mark.parametrize("name", ["five_pose", "bal_small"])
def test_split_line_search_is_bit_identical_on_graphs(name):
    graph, initial = nc.problem(name)
    g = nr.OracleSystem(graph).gradient(initial)
    for seed in (None, 1):
        mk = lambda: nr.OracleSystem(graph, perturb=None if seed is None else np.random.default_rng(seed), eps=1e-12)  # noqa: E731
        new, old = _both(mk, initial, g)
        assert new == old
    assert new[0] == nc.restated_line_search(name)[0] or seed is not None


@pytest.mark.parametrize("name", ec.CONTROL_NAMES)
def test_planted_copy_without_a_defect_is_the_rule(name):
    c = ec.control_case(name)
    again = ref.run_control(c["rec0"], c["errors"], c["final"], lambda r, e: ref.ls_step_planted(r, e, None))
    assert len(again) == len(c["records"]) == len(c["errors"])
    assert all(ref.same_bits(a, b) for a, b in zip(again, c["records"]))
    k = c["done_at"]
    if k is not None:  # past done the record stays, trials included; the final error joins it
        for r in c["records"][k:k + ec.EXTRA]:
            assert ref.same_bits(r, c["records"][k - 1]) and r["trials"] == k
        assert c["records"][-1]["error"] == c["errors"][-1] and c["records"][-1]["trials"] == k
    print("TABLE control %-12s evaluations to done %s, records %d, alpha %r" % (name, k, len(again), c["records"][-1]["alpha"]))


# ---------------------------------------------------------------- floors and tolerances of the vector cases
@pytest.mark.parametrize("name", ec.VECTOR_NAMES)
def test_floors_and_tolerances(name):
    """16 x floor stays below 1e-9 for every quantity of every case that is not a cancellation case; the cancellation cases carry their
    own floor (printed; asserted against the recorded one like the others).  The recorded figures are two-digit roundings."""
    worst = dict.fromkeys(ref.QUANTITIES, 0.0)
    for (m, a), mid in zip(ec.METHODS, ec.METHOD_IDS):
        r, fl = ec.vector_reference(name, m, a)
        plain = ref.direction(m, *(ec.vector_case(name)[k] for k in ("g", "gp", "s")), dtype=np.float64, alias=a)
        miss = ref.misses(plain, r, fl)
        assert max(miss.values()) <= 1.0 / ref.FLOOR_FACTOR + 1e-12, (name, mid, miss)  # a float64 run lies within the floor itself
        if fl["noise"] is not None:
            print("TABLE vector %-16s %-9s direction below %.1e |g|: bounded, not compared" % (name, mid, ref.NOISE))
        for q in ref.QUANTITIES:
            if fl["noise"] is None or q not in ref.NOISE_QUANTITIES:
                worst[q] = max(worst[q], fl[q])
    print("TABLE vector %-16s floors %s" % (name, " ".join("%s %.1e" % (q, worst[q]) for q in ref.QUANTITIES)))
    for q in ref.QUANTITIES:
        assert math.isfinite(worst[q])
        if ec.vector_case(name)["kind"] != "cancel":
            assert ref.FLOOR_FACTOR * worst[q] < ref.CAP, (name, q, worst[q])
        rec = ec.FLOORS[name][q]
        assert (worst[q] == 0.0 and rec == 0.0) or rec / 1.06 <= worst[q] <= rec * 1.06, (name, q, worst[q], rec)


# ---------------------------------------------------------------- the queueing cases
@pytest.mark.parametrize("trials", sorted(ec.RATIOS))
def test_ratios_are_found_again_and_robust(trials):
    r = ec.RATIOS[trials]
    assert ec.find_ratio(trials) == r
    alpha, n = ec.prior_trials(r)
    assert n == trials and abs(alpha + 1.0) <= 2 * nr.TAU * (1 + 2 * nr.TAU)
    for eps in ec.PERTURB_EPS:
        for seed in ec.PERTURB_SEEDS:
            a, n = ec.prior_trials(r, (eps, np.random.default_rng(seed)))
            assert n == trials and abs(a - alpha) <= nc.BRACKET_RTOL * abs(alpha), (trials, eps, seed, n, a)
    # the same count from the restatement over the CPU oracle on the graph the device gets
    graph, initial = ec.prior_problem(trials)
    s, st = nr.OracleSystem(graph), {}
    a = nr.line_search(s, initial, s.gradient(initial), st)
    print("TABLE queue prior[%d] r %.2e alpha %.17g trials %d (oracle: alpha %.17g trials %d)" % (trials, r, alpha, trials, a, st["trials"]))
    assert st["trials"] == trials and abs(a - alpha) <= nc.BRACKET_RTOL * abs(alpha)


def _search(error_at, dnorm, limit=nr.MAX_TRIALS):
    rec, errors = nr.ls_begin(dnorm), []
    while not rec["done"] and rec["trials"] < limit:
        errors.append(error_at(rec["step"]))
        rec = nr.ls_step(rec, errors[-1])
    return rec, errors


def test_the_ascent_direction_ends_by_ties_in_the_third_queue():
    """five_pose along -gradient: the minimiser of the bracket is step 0, and in exact arithmetic the exit test is never met (maxStep stays
    0, |testStep| + |newStep| < 2 |minStep|).  In float64 it IS met: once |step| |direction| falls below the spacing of the values the
    retract returns the initial values but for their last bits, every error is error(initial) but for ITS last bits, some testError >=
    newError moves maxStep off 0 and the bracket closes around that step.  Measured: done after 102 evaluations, alpha -4.1e-19 -- in
    the third queue of the device (85 .. 128), so the device reports a finished search after three waits, not the error return."""
    graph, initial = nc.problem("five_pose")
    s = nr.OracleSystem(graph)
    d = -s.gradient(initial)
    e0 = s.error(initial)
    rec, errors = _search(lambda step: s.error(s.advance(initial, step, d)), float(np.linalg.norm(d)))
    print("TABLE queue ascent: done %d after %d evaluations, alpha %.3g, bracket [%g, %g]" % (rec["done"], rec["trials"], rec["alpha"], rec["minStep"], rec["maxStep"]))
    assert rec["done"] and ec.ASCENT_TRIALS[0] < rec["trials"] <= ec.ASCENT_TRIALS[1]
    ulp = float(np.finfo(np.float64).eps) * e0
    assert errors[0] > e0 and all(abs(e - e0) <= 4 * ulp for e in errors[-8:])  # ascent; at the end the errors are error(initial) to the last bits
    assert rec["maxStep"] < 0.0 and abs(rec["alpha"]) * rec["dnorm"] < 1e-15


def test_a_minimiser_at_zero_and_a_zero_direction_never_end():
    """origin: PriorFactorPoint3 at the origin, the point AT the origin, direction (1, 0, 0): error = step^2 / 2 is resolved down to the
    underflow, its minimiser is step 0 exactly, maxStep stays 0 and the exit test is never met.  zero: ls_begin(0) and NaN errors."""
    s = ec.PriorPoint3System()
    x, d = np.zeros(3), np.array([1.0, 0.0, 0.0])
    for what, (rec, errors) in (("origin", _search(lambda step: s.error(s.advance(x, step, d)), 1.0)),
                                ("zero direction", _search(lambda step: math.nan, 0.0))):
        print("TABLE queue %s: after %d evaluations bracket [%g, %g]" % (what, rec["trials"], rec["minStep"], rec["maxStep"]))
        assert not rec["done"] and rec["trials"] == nr.MAX_TRIALS
        if what == "origin":
            assert rec["maxStep"] == 0.0 and rec["minStep"] < 0.0 and errors[-1] > 0.0
    assert math.isnan(rec["step"]) and rec["dnorm"] == 0.0  # the zero direction: every step is NaN


# ---------------------------------------------------------------- planted defects
VECTOR_DEFECT_RUNS = {
    "stride_ignored": [("tail[65537]", 0), ("tail[131073]", 1), ("plain[65537]", 2), ("tail[131073]", -1)],
    "npart_minus_1": [("lastpart[65536]", 0), ("lastpart[65537]", 1), ("lastpart[131073]", 3), ("plain[257]", 2), ("lastpart[65536]", -1)],
    "pr_gg": [("plain[257]", 1), ("plain[65537]", 1)],
    "sd_sign": [("plain[257]", 2), ("plain[257]", 3)],
    "no_max0": [("negquot_prhs", 1), ("negquot_prhs", 2), ("negquot_dy", 3)],
    "nan_kept": [("allzero_g", 1), ("allzero_g", 3), ("sd0_gd0", 2)],
    "dir_g_beta_g": [("plain[257]", 0), ("plain[131073]", 1)],
}


@pytest.mark.parametrize("defect", ref.VECTOR_DEFECTS)
def test_planted_vector_defect_is_seen(defect):
    seen = []
    for name, m in VECTOR_DEFECT_RUNS[defect]:
        c = ec.vector_case(name)
        r, fl = ec.vector_reference(name, m, 0)
        bad = ref.direction(m, c["g"], c["gp"], c["s"], np.float64, defect=defect)
        miss = ref.misses(bad, r, fl)
        q = max(miss, key=miss.get)
        seen.append(miss[q])
        print("DEFECT %-16s %-16s %-3s worst %-8s miss / tolerance %.1e" % (defect, name, ec.METHOD_IDS[ec.METHODS.index((m, 0))], q, miss[q]))
    assert min(seen) >= MARGIN, (defect, seen)  # every run built for it, not only some


@pytest.mark.parametrize("defect", ref.CONTROL_DEFECTS)
def test_planted_control_defect_is_seen(defect):
    where = []
    for name in ec.CONTROL_NAMES:
        c = ec.control_case(name)
        bad = ref.run_control(c["rec0"], c["errors"], c["final"], lambda r, e: ref.ls_step_planted(r, e, defect))
        first = next((i for i, (a, b) in enumerate(zip(bad, c["records"])) if not ref.same_bits(a, b)), None)
        if first is not None:
            where.append("%s@%d" % (name, first))
    print("DEFECT %-16s records differ in %d of %d cases: %s" % (defect, len(where), len(ec.CONTROL_NAMES), " ".join(where)))
    assert where, defect
    if defect == "gt":
        assert {w.split("@")[0] for w in where} >= {"tie[flag 0]", "tie[flag 1]", "constant"}
