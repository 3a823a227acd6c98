"""TEST INFRASTRUCTURE: the cases of the nonlinear conjugate gradient edge tests (numpy only, no device) -- inputs at the sizes and values
where the kernels of csrc/kernels_ncg.hpp and the queueing of csrc/ncg.hpp change behaviour.  EDGES names every such place as a
predicate over a case's statistics; test_ncg_edges_reference.py::test_every_edge_is_reached asserts that some case makes each true.

Vector cases (g = currentGradient, gp = prevGradient, s = direction; each runs with METHODS: the four beta formulas, and
ncg_set_direction_kernel with a separate source and with src == dir):
  plain[n]          seeded, all four betas positive; n = 1, 255, 256, 257 (1 and 2 block partials), 65 535, 65 536 (256 full partials),
                    65 537 (the first strided element, in block 0), 131 073 (a third pass for one thread)
  tail[n]           plain[n] with the elements at index >= 65 536 multiplied by 1e3 (65 537: its one such element by 1e4): they carry most
                    of every sum
  lastpart[n]       plain[n] with the elements of the last block partial (block 255) multiplied by 1e3
  negquot_prhs      g.(g - gp) < 0 and s.(g - gp) < 0: Polak-Ribiere and Hestenes-Stiefel clamp to 0
  negquot_dy        s.(g - gp) > 0: Dai-Yuan clamps to 0
  pp0               gp = 0: Fletcher-Reeves and Polak-Ribiere divide g.g > 0 by 0 and give +inf (max(0, inf) = inf, as in the reference);
                    s has zeros, so the new direction holds infinities and NaNs (inf * 0)
  allzero_g         g = gp = 0: every quotient is 0 / 0; Fletcher-Reeves keeps the NaN, the three clamped formulas give 0
  sd0               small integers with s orthogonal to g - gp pair by pair: s.(g - gp) = 0 exactly, the quotients are -inf -> 0
  sd0_gd0           the same with g orthogonal to g - gp too: Hestenes-Stiefel's 0 / -0 is NaN -> 0
  cancel[n]         gp = g (1 + 1e-9 u): g.(g - gp) is nine digits below g.g; only the per-element difference keeps it
  zero              g = gp = s = 0: the direction into ls_begin is all zero (dnorm 0, minStep -inf, newStep NaN)

Control cases (an error sequence fed to the control rule from ls_begin(dnorm); built in closed loop with the restatement, then replayed
open loop; every one runs EXTRA evaluations past `done` and ends with the final-error kernel):
  quad[r]           error = (step * dnorm + r)^2, minimiser ratio r = 1e-3, 0.1 (dnorm 3.7), 0.5, 1.0 and 2 (outside the bracket)
  tie[flag f]       quad[0.3] with testError == newError at every third evaluation whose flag is f
  constant          every error 1.0 (every comparison is a tie)
  nan_first, nan_mid  quad[0.5] with a NaN as the first error / as the fourth
  zero_dir          ls_begin(0): the bracket [-inf, 0], NaN steps, NaN errors; never done

Queueing cases (graphs): prior[trials] = one PriorFactorPoint3 at the origin, unit sigma, the point at (r, 0, 0): error = r^2 (1 + alpha)^2 / 2
along the gradient, minimiser ratio r.  RATIOS holds values of r found by scanning (find_ratio) at which the search takes exactly 40, 41,
84 and 85 evaluations, unchanged when every error is multiplied by (1 +- eps), eps = 1e-12 and 1e-9, seeds 1..3.
  ascent            five_pose along -gradient.  In exact arithmetic its search never ends; in float64 it ends by ties once the steps fall
                    below the spacing of the values (the restatement: evaluation 102), inside the third queue: ASCENT_TRIALS
  origin            the prior's point AT the origin, direction (1, 0, 0): error = step^2 / 2, the minimiser at step 0 is resolved down to
                    the underflow and the search does not end -- the error return after NCG_MAX_TRIALS evaluations
  zero              five_pose along an all-zero direction (NaN steps, NaN errors): the same error return
Gradient cases: GRADIENT_CASES of tests/pcg_cases.py."""
from __future__ import annotations

import functools
import math

import numpy as np

import ncg_reference as ref
import ncg_restatement as nr

SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 131073)
METHODS = ((-1, 0), (-1, 1), (0, 0), (1, 0), (2, 0), (3, 0))  # (method, alias)
METHOD_IDS = ("set-src", "set-alias", "FR", "PR", "HS", "DY")
REDUCE_SIZES = (1, 255, 256, 257, 65536, 65537, 131073)
EXTRA = 3                        # evaluations past `done`
PERTURB_EPS = (1e-12, 1e-9)
PERTURB_SEEDS = (1, 2, 3)
GRADIENT_CASES = ("block[ntot255,nfac255]", "block[ntot256,nfac256]", "block[ntot257,nfac257]", "mixed", "hub")

# r of prior[trials], found by find_ratio (test_ncg_edges_reference.py::test_ratios_are_robust finds and checks them again)
RATIOS = {40: 5.7e-4, 41: 3.5e-4, 84: 3.6e-13, 85: 2.2e-13}
# the evaluations of the ascent search lie strictly between these: the third queue (the restatement takes 102; where exactly the retract
# stops resolving the step depends on its rounding, so the device's count is held to the queue, not to the number)
ASCENT_TRIALS = (84, 128)

# ---- measured on the CPU, on the reference alone (test_ncg_edges_reference.py::test_floors_and_tolerances measures them again): per case
# the largest floor over METHODS of every quantity = largest relative distance of the float64 runs (unpermuted and three seeded
# permutations of every sum) from the long-double run.  The tolerance of a device comparison is 16 x the floor of ITS (case, method,
# quantity), measured in the test's process; it is never above 16 x the figure here.
FLOORS = {
    "plain[1]": {"gg": 1.1e-16, "gd": 1.1e-16, "pp": 1.1e-16, "sd": 1.1e-16, "beta": 1.1e-16, "dir": 1.7e-16, "dnorm": 1.7e-16, "minStep": 2.0e-16, "newStep": 2.6e-16},
    "plain[255]": {"gg": 1.1e-16, "gd": 1.8e-16, "pp": 1.1e-16, "sd": 1.1e-16, "beta": 2.3e-16, "dir": 1.8e-16, "dnorm": 1.3e-16, "minStep": 1.6e-16, "newStep": 1.4e-16},
    "plain[256]": {"gg": 1.1e-16, "gd": 1.1e-16, "pp": 1.1e-16, "sd": 2.1e-16, "beta": 3.0e-16, "dir": 2.8e-16, "dnorm": 1.1e-16, "minStep": 1.5e-16, "newStep": 1.4e-16},
    "plain[257]": {"gg": 1.1e-16, "gd": 1.1e-16, "pp": 1.5e-16, "sd": 1.1e-16, "beta": 2.8e-16, "dir": 1.6e-16, "dnorm": 1.1e-16, "minStep": 1.5e-16, "newStep": 2.8e-16},
    "plain[65535]": {"gg": 1.1e-16, "gd": 1.5e-16, "pp": 1.7e-16, "sd": 1.1e-16, "beta": 2.8e-16, "dir": 2.2e-16, "dnorm": 1.3e-16, "minStep": 1.8e-16, "newStep": 2.0e-16},
    "plain[65536]": {"gg": 1.6e-16, "gd": 2.4e-16, "pp": 1.1e-16, "sd": 1.1e-16, "beta": 4.0e-16, "dir": 2.2e-16, "dnorm": 1.7e-16, "minStep": 2.5e-16, "newStep": 3.1e-16},
    "plain[65537]": {"gg": 1.1e-16, "gd": 1.8e-16, "pp": 1.9e-16, "sd": 1.3e-16, "beta": 2.2e-16, "dir": 1.6e-16, "dnorm": 1.6e-16, "minStep": 1.4e-16, "newStep": 1.4e-16},
    "plain[131073]": {"gg": 1.6e-16, "gd": 1.9e-16, "pp": 1.8e-16, "sd": 2.4e-16, "beta": 3.2e-16, "dir": 1.8e-16, "dnorm": 2.0e-16, "minStep": 1.9e-16, "newStep": 2.0e-16},
    "tail[65537]": {"gg": 1.5e-16, "gd": 5.2e-16, "pp": 2.0e-16, "sd": 3.2e-16, "beta": 8.8e-16, "dir": 2.1e-14, "dnorm": 1.4e-15, "minStep": 1.4e-15, "newStep": 1.3e-15},
    "tail[131073]": {"gg": 1.1e-16, "gd": 2.8e-16, "pp": 1.7e-16, "sd": 2.4e-16, "beta": 4.0e-16, "dir": 3.9e-16, "dnorm": 3.1e-16, "minStep": 3.1e-16, "newStep": 3.6e-16},
    "lastpart[65536]": {"gg": 1.1e-16, "gd": 1.7e-16, "pp": 1.9e-16, "sd": 1.3e-16, "beta": 3.1e-16, "dir": 2.6e-16, "dnorm": 1.9e-16, "minStep": 2.1e-16, "newStep": 2.1e-16},
    "lastpart[65537]": {"gg": 2.1e-16, "gd": 2.1e-16, "pp": 1.6e-16, "sd": 1.1e-16, "beta": 3.8e-16, "dir": 2.5e-16, "dnorm": 1.4e-16, "minStep": 2.1e-16, "newStep": 3.1e-16},
    "lastpart[131073]": {"gg": 2.1e-16, "gd": 1.4e-16, "pp": 1.8e-16, "sd": 2.6e-16, "beta": 4.8e-16, "dir": 4.7e-16, "dnorm": 1.2e-16, "minStep": 1.5e-16, "newStep": 2.5e-16},
    "negquot_prhs": {"gg": 1.7e-16, "gd": 1.1e-16, "pp": 1.1e-16, "sd": 1.1e-16, "beta": 2.1e-16, "dir": 1.2e-16, "dnorm": 1.5e-16, "minStep": 1.6e-16, "newStep": 2.6e-16},
    "negquot_dy": {"gg": 1.7e-16, "gd": 1.1e-16, "pp": 1.1e-16, "sd": 1.1e-16, "beta": 2.1e-16, "dir": 5.5e-16, "dnorm": 1.5e-16, "minStep": 1.8e-16, "newStep": 1.6e-16},
    "pp0": {"gg": 1.7e-16, "gd": 1.7e-16, "pp": 0.0, "sd": 1.7e-16, "beta": 2.0e-16, "dir": 2.3e-16, "dnorm": 1.5e-16, "minStep": 1.6e-16, "newStep": 1.3e-16},
    "allzero_g": {"gg": 0.0, "gd": 0.0, "pp": 0.0, "sd": 0.0, "beta": 0.0, "dir": 0.0, "dnorm": 1.1e-16, "minStep": 1.1e-16, "newStep": 1.1e-16},
    "zero": {"gg": 0.0, "gd": 0.0, "pp": 0.0, "sd": 0.0, "beta": 0.0, "dir": 0.0, "dnorm": 0.0, "minStep": 0.0, "newStep": 0.0},
    "sd0": {"gg": 0.0, "gd": 0.0, "pp": 0.0, "sd": 0.0, "beta": 1.1e-16, "dir": 1.1e-16, "dnorm": 1.1e-16, "minStep": 1.1e-16, "newStep": 1.1e-16},
    "sd0_gd0": {"gg": 0.0, "gd": 0.0, "pp": 0.0, "sd": 0.0, "beta": 1.1e-16, "dir": 1.1e-16, "dnorm": 1.1e-16, "minStep": 1.1e-16, "newStep": 1.1e-16},
    "cancel[257]": {"gg": 1.7e-16, "gd": 2.1e-16, "pp": 1.1e-16, "sd": 3.8e-16, "beta": 2.6e-16, "dir": 1.8e-16, "dnorm": 1.6e-16, "minStep": 1.8e-16, "newStep": 2.0e-16},
    "cancel[65537]": {"gg": 2.7e-16, "gd": 4.3e-16, "pp": 1.7e-16, "sd": 9.1e-16, "beta": 5.8e-16, "dir": 1.3e-16, "dnorm": 2.1e-16, "minStep": 2.4e-16, "newStep": 2.2e-16},
}

# ---- the beta of tests/test_gpu_ncg.py::test_each_direction_method_matches_its_restatement: the restatement's spread of every trace row's
# beta when each line search's alpha is moved by +-BRACKET_RTOL relative (ncg_cases.BRACKET_RTOL = 2 tau), largest over five_pose and
# five_pose_huber, the four methods and the four iterations, times 10; see ncg_cases.BETA_RTOL.


# ---------------------------------------------------------------- vector cases
def _plain(n):
    if n == 1:
        return np.array([1.7]), np.array([1.3]), np.array([-0.6])
    rng = np.random.default_rng([7, n])
    gp = rng.normal(size=n)
    g = 0.5 * gp + 0.8 * rng.normal(size=n)
    s = -0.7 * (g - gp) + 0.3 * rng.normal(size=n)
    return g, gp, s


def _scaled(n, where, by=1e3):
    g, gp, s = _plain(n)
    w = np.where(where(np.arange(n)), by, 1.0)
    return g * w, gp * w, s * w


def _int_pairs(n, gd0):
    rng = np.random.default_rng([11, n, int(gd0)])
    m = (n - 1) // 2
    a, b = rng.integers(1, 4, m), rng.integers(-3, 4, m)
    d = np.zeros(n)
    d[0:2 * m:2], d[1:2 * m:2] = a, b
    perp = np.zeros(n)
    perp[0:2 * m:2], perp[1:2 * m:2] = b, -a
    s = perp.copy()
    s[:2 * m] *= np.repeat(rng.integers(1, 3, m), 2)  # pair j of s = k_j (b_j, -a_j): s.d = 0 pair by pair
    if gd0:
        g = perp.copy()
        g[:2 * m] *= np.repeat(rng.integers(1, 4, m), 2)
    else:
        g = d.copy()
        g[0:2 * m:2] += rng.integers(0, 3, m)  # g.d = d.d + (terms >= 0, a_j >= 1) > 0
    g[2 * m:] = 3.0  # beyond the pairs d = 0: g = gp
    return g, g - d, s


def _special(kind, n):
    rng = np.random.default_rng([13, n])
    g = rng.normal(size=n)
    if kind == "negquot_prhs":
        return g, 2.0 * g + 0.1 * rng.normal(size=n), g + 0.1 * rng.normal(size=n)
    if kind == "negquot_dy":
        return g, 2.0 * g + 0.1 * rng.normal(size=n), -g + 0.1 * rng.normal(size=n)
    if kind == "pp0":
        s = rng.normal(size=n)
        s[::3] = 0.0
        return g, np.zeros(n), s
    if kind == "allzero_g":
        return np.zeros(n), np.zeros(n), rng.normal(size=n)
    if kind == "cancel":
        return g, g * (1.0 + 1e-9 * rng.normal(size=n)), rng.normal(size=n)
    if kind == "zero":
        return np.zeros(n), np.zeros(n), np.zeros(n)
    raise KeyError(kind)


def _vector_table():
    T = {}
    for n in SIZES:
        T["plain[%d]" % n] = ("plain", n, lambda n=n: _plain(n))
    for n in (65537, 131073):
        T["tail[%d]" % n] = ("tail", n, lambda n=n: _scaled(n, lambda i: i >= ref.STRIDE, 1e4 if n == 65537 else 1e3))
    for n in (65536, 65537, 131073):
        T["lastpart[%d]" % n] = ("lastpart", n, lambda n=n: _scaled(n, lambda i: (i // 256) % 256 == 255))
    for kind in ("negquot_prhs", "negquot_dy", "pp0", "allzero_g", "zero"):
        T[kind] = (kind, 257, lambda kind=kind: _special(kind, 257))
    T["sd0"] = ("sd0", 257, lambda: _int_pairs(257, False))
    T["sd0_gd0"] = ("sd0_gd0", 257, lambda: _int_pairs(257, True))
    for n in (257, 65537):
        T["cancel[%d]" % n] = ("cancel", n, lambda n=n: _special("cancel", n))
    return T


VECTOR_CASES = _vector_table()
VECTOR_NAMES = list(VECTOR_CASES)


@functools.lru_cache(maxsize=None)
def vector_case(name):
    kind, n, make = VECTOR_CASES[name]
    g, gp, s = (np.ascontiguousarray(a, dtype=np.float64) for a in make())
    assert len(g) == len(gp) == len(s) == n
    for a in (g, gp, s):
        a.setflags(write=False)
    return dict(name=name, kind=kind, n=n, g=g, gp=gp, s=s)


@functools.lru_cache(maxsize=None)
def vector_reference(name, method, alias):
    """(the long-double result, the floor of every quantity) of one vector case and method: computed once per process"""
    c = vector_case(name)
    return ref.floors(method, c["g"], c["gp"], c["s"], alias)


def vector_stats(name):
    c = vector_case(name)
    r = {m: vector_reference(name, m, 0)[0] for m in (0, 1, 2, 3)}
    q = {k: float(r[1][k]) for k in ("gg", "gd", "pp", "sd")}
    w = np.asarray(c["g"], dtype=ref.LD) ** 2
    i = np.arange(c["n"])
    total = float(w.sum())
    return dict(name=name, kind=c["kind"], n=c["n"], npart=ref.npart_of(c["n"]), passes=-(-c["n"] // ref.STRIDE), **q,
                beta={m: float(r[m]["beta"]) for m in r}, dnorm={m: float(r[m]["dnorm"]) for m in r}, dir={m: np.asarray(r[m]["dir"], dtype=np.float64) for m in r},
                tail_share=float(w[i >= ref.STRIDE].sum()) / total if total else 0.0,
                last_share=float(w[(i // 256) % 256 == ref.npart_of(c["n"]) - 1].sum()) / total if total else 0.0)


def _betas_positive(s):
    return all(0 < s["beta"][m] < math.inf for m in s["beta"])


VECTOR_EDGES = {
    **{"plain, n = %d, every beta positive" % n: (lambda s, n=n: s["kind"] == "plain" and s["n"] == n and _betas_positive(s)) for n in SIZES},
    "one block partial, not full": lambda s: s["npart"] == 1 and s["n"] == 255,
    "one full block partial": lambda s: s["npart"] == 1 and s["n"] == 256,
    "two block partials": lambda s: s["npart"] == 2,
    "255 full partials and one short of one": lambda s: s["n"] == 65535 and s["npart"] == 256,
    "256 full partials, one pass": lambda s: s["n"] == 65536 and s["npart"] == 256 and s["passes"] == 1,
    "the first strided element": lambda s: s["n"] == 65537 and s["passes"] == 2,
    "a third pass": lambda s: s["passes"] == 3,
    "the strided elements carry most of every sum (one element)": lambda s: s["n"] == 65537 and s["tail_share"] > 0.9,
    "the strided elements carry most of every sum (two passes)": lambda s: s["n"] == 131073 and s["tail_share"] > 0.9,
    "the last partial carries most of every sum": lambda s: s["npart"] == 256 and s["kind"] == "lastpart" and s["last_share"] > 0.9,
    "Polak-Ribiere and Hestenes-Stiefel clamp a negative quotient": lambda s: s["gd"] < 0 < s["pp"] and s["sd"] < 0 and s["beta"][1] == 0 == s["beta"][2],
    "Dai-Yuan clamps a negative quotient": lambda s: s["sd"] > 0 and s["gg"] > 0 and s["beta"][3] == 0,
    "pp = 0: Fletcher-Reeves is +inf, the direction holds inf and NaN": lambda s: s["pp"] == 0 < s["gg"] and s["beta"][0] == math.inf
        and np.isinf(s["dir"][0]).any() and np.isnan(s["dir"][0]).any(),
    "pp = 0 and gd = 0: Polak-Ribiere's NaN quotient gives 0, Fletcher-Reeves' stays": lambda s: s["pp"] == 0 == s["gd"] and s["beta"][1] == 0
        and math.isnan(s["beta"][0]),
    "sd = 0 exactly, an infinite quotient": lambda s: s["sd"] == 0 and s["gd"] > 0 and s["beta"][2] == 0 == s["beta"][3],
    "sd = 0 = gd exactly: Hestenes-Stiefel's NaN quotient gives 0": lambda s: s["sd"] == 0 == s["gd"] and s["gg"] > 0 and s["beta"][2] == 0,
    "cancellation: g.(g - gp) nine digits below g.g": lambda s: 0 < abs(s["gd"]) < 1e-8 * s["gg"],
    "cancellation at a strided size": lambda s: 0 < abs(s["gd"]) < 1e-8 * s["gg"] and s["passes"] == 2,
    "an all-zero direction into ls_begin": lambda s: s["kind"] == "zero" and s["dnorm"][1] == 0,
    "a clamped beta makes the direction zero": lambda s: s["kind"] == "allzero_g" and s["dnorm"][1] == 0 and math.isnan(s["dnorm"][0]),
}


# ---------------------------------------------------------------- control cases
def _closed_loop(dnorm, f, max_k=140, final_error=0.125):
    """errors[i] = f(record before evaluation i, i) until done (or max_k), EXTRA more past done, and the final advance's error"""
    rec = nr.ls_begin(dnorm)
    errors, flags = [], []
    while not rec["done"] and len(errors) < max_k:
        e = float(f(rec, len(errors)))
        flags.append((rec["first"], rec["flag"], (not rec["first"]) and e >= rec["newError"], (not rec["first"]) and e == rec["newError"]))
        errors.append(e)
        rec = nr.ls_step(rec, e)
    done_at = len(errors) if rec["done"] else None
    errors += [0.0, math.nan, -1.0][:EXTRA] + [final_error]
    return dict(rec0=nr.ls_begin(dnorm), errors=errors, final=1, done_at=done_at, flags=flags, dnorm=dnorm)


def _quad(r):
    return lambda rec, i: (rec["step"] * rec["dnorm"] + r) ** 2


def _tie(want_flag):
    q = _quad(0.3)
    seen = [0]

    def f(rec, i):
        if not rec["first"] and rec["flag"] == want_flag:
            seen[0] += 1
            if seen[0] % 3 == 1:
                return rec["newError"]
        return q(rec, i)
    return f


def _nan_at(k):
    q = _quad(0.5)
    return lambda rec, i: math.nan if i == k else q(rec, i)


CONTROL_CASES = {
    "quad[0.001]": lambda: _closed_loop(1.0, _quad(1e-3)),
    "quad[0.1]": lambda: _closed_loop(3.7, _quad(0.1)),
    "quad[0.5]": lambda: _closed_loop(1.0, _quad(0.5)),
    "quad[1]": lambda: _closed_loop(1.0, _quad(1.0)),
    "quad[2]": lambda: _closed_loop(0.25, _quad(2.0)),
    "tie[flag 0]": lambda: _closed_loop(1.0, _tie(0)),
    "tie[flag 1]": lambda: _closed_loop(1.0, _tie(1)),
    "constant": lambda: _closed_loop(1.0, lambda rec, i: 1.0),
    "nan_first": lambda: _closed_loop(1.0, _nan_at(0)),
    "nan_mid": lambda: _closed_loop(1.0, _nan_at(3)),
    "zero_dir": lambda: _closed_loop(0.0, lambda rec, i: math.nan, max_k=10),
}
CONTROL_NAMES = list(CONTROL_CASES)


@functools.lru_cache(maxsize=None)
def control_case(name):
    c = CONTROL_CASES[name]()
    c["name"] = name
    c["records"] = ref.run_control(c["rec0"], c["errors"], c["final"])
    return c


def _branches(c):
    """(flag, testError >= newError) of every evaluation after the first"""
    return {(int(fl), bool(ge)) for first, fl, ge, _ in c["flags"] if not first}


CONTROL_EDGES = {
    **{"minimiser ratio %s" % r: (lambda c, r=r: c["name"] == "quad[%s]" % r and c["done_at"] is not None) for r in ("0.001", "0.1", "0.5", "1", "2")},
    "the first evaluation": lambda c: c["flags"][0][0] == 1,
    "all four bracket updates in one search": lambda c: _branches(c) == {(0, False), (0, True), (1, False), (1, True)},
    "a tie with flag 0": lambda c: any(tie and not fl for first, fl, _, tie in c["flags"] if not first),
    "a tie with flag 1": lambda c: any(tie and fl for first, fl, _, tie in c["flags"] if not first),
    "a constant error sequence": lambda c: c["name"] == "constant" and c["done_at"] is not None,
    "a NaN as newError": lambda c: c["name"] == "nan_first",
    "a NaN as testError": lambda c: c["name"] == "nan_mid" and c["done_at"] is not None,
    "evaluations past done": lambda c: c["done_at"] is not None and len(c["errors"]) == c["done_at"] + EXTRA + 1,
    "the final error joins a finished record": lambda c: c["done_at"] is not None and c["records"][-1]["error"] == c["errors"][-1],
    "the final kernel in front of done": lambda c: c["done_at"] is None and c["records"][-1]["error"] == 0.0,
    "the record of an all-zero direction": lambda c: c["rec0"]["minStep"] == -math.inf and math.isnan(c["rec0"]["step"]),
    "a bracket that is not [-1, 0]": lambda c: c["dnorm"] not in (0.0, 1.0),
}


# ---------------------------------------------------------------- queueing cases
class PriorPoint3System:
    """NonlinearConjugateGradientOptimizer::System of one PriorFactorPoint3 at the origin with unit sigma: error = |x|^2 / 2, gradient x.
    perturb = (eps, numpy Generator): every error is multiplied by (1 +- eps), the probe of tests/ncg_cases.py"""

    def __init__(self, perturb=None):
        self.perturb = perturb

    def error(self, x):
        e = 0.5 * float(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        if self.perturb is not None:
            eps, rng = self.perturb
            e *= 1.0 + (eps if rng.integers(0, 2) else -eps)
        return e

    def gradient(self, x):
        return np.array(x, dtype=np.float64)

    def advance(self, x, alpha, g):
        return x + alpha * g


def prior_trials(r, perturb=None):
    """(alpha, trials) of the first line search of prior[r]"""
    s = PriorPoint3System(perturb)
    x = np.array([r, 0.0, 0.0])
    st = {}
    alpha = nr.line_search(s, x, s.gradient(x), st)
    return alpha, st["trials"]


def ratio_is_robust(r, trials):
    if prior_trials(r)[1] != trials:
        return False
    return all(prior_trials(r, (eps, np.random.default_rng(seed)))[1] == trials for eps in PERTURB_EPS for seed in PERTURB_SEEDS)


def find_ratio(trials):
    """the first two-digit r, scanning downwards from the value the count formula of csrc/ncg.hpp gives, at which the search takes
    exactly `trials` evaluations with and without the perturbations; None if 400 candidates hold none"""
    golden = 0.5 * (math.sqrt(5.0) - 1.0)
    r0 = golden ** (trials - 1.5) / (2 * nr.TAU)
    exp = math.floor(math.log10(r0))
    cands = sorted({float("%d.%de%d" % (m // 10, m % 10, e)) for e in (exp - 1, exp, exp + 1) for m in range(10, 100)}, reverse=True)
    for r in cands:
        if r < 1.0 and ratio_is_robust(float(r), trials):
            return float(r)
    return None


def prior_problem(trials):
    from gtsam_personal_amd import NonlinearFactorGraph, Values, noiseModel
    g, v = NonlinearFactorGraph(), Values()
    g.add_PriorFactorPoint3(0, [0.0, 0.0, 0.0], noiseModel.Unit.Create(3))
    v.insert_point3(0, np.array([RATIOS[trials], 0.0, 0.0]))
    return g, v


QUEUE_EDGES = {
    "a search that ends on trial 40, the last of the first queue": lambda q: q == 40,
    "a search that ends on trial 41, the first of the second queue": lambda q: q == 41,
    "a search that ends on trial 84, the last of the second queue": lambda q: q == 84,
    "a search that ends on trial 85, the first of the third queue": lambda q: q == 85,
}

EDGES = {"vector": VECTOR_EDGES, "control": CONTROL_EDGES, "queue": QUEUE_EDGES}
