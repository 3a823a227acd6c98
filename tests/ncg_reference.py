"""TEST INFRASTRUCTURE: the reference of the nonlinear conjugate gradient edge tests (CPU only, numpy only).

Vector quantities -- the four dot products ncg_dots_kernel forms, every beta formula, direction = g + beta * direction, its norm and
the record ncg_ls_begin_kernel writes (csrc/kernels_ncg.hpp) -- in np.longdouble: `direction(method, g, gp, s)`.
direction(dtype=np.float64, seed=s) runs the same code in float64 with a seeded permutation of every sum's terms: a sample of the
freedom a correct FP64 implementation has.  `floors` takes the largest distance of such runs (the unpermuted one and three seeds) from
the long-double run as the floor of a comparison, per quantity; the tolerance of a comparison is FLOOR_FACTOR x that floor.

The control rule (one evaluation of lineSearch, record + error -> record) is float64 and lives in tests/ncg_restatement.py (ls_begin,
ls_step): the device is held to it bit for bit.  ls_step_planted is a copy of it that takes a planted defect.

Planted defects (test_ncg_edges_reference.py shows that each is seen):
  vector    "stride_ignored"   the elements at index >= 65 536 (a grid-stride loop without its second trip) enter no sum and keep their direction
            "npart_minus_1"    the last block partial is left out of every sum
            "pr_gg"            Polak-Ribiere with g.g in the numerator
            "sd_sign"          Hestenes-Stiefel / Dai-Yuan divide by +s.d
            "no_max0"          beta without max(0, .)
            "nan_kept"         max(0, x) written so that a NaN quotient stays NaN
            "dir_g_beta_g"     direction = g + beta * g
  control   "gt"               testError > newError for >=
            "flag_swapped"     the two bracket updates of each branch exchanged
            "exit_no_newstep"  the exit test without |newStep|
            "alpha_newstep"    alpha = newStep
            "first_kept"       `first` not cleared"""
from __future__ import annotations

import math

import numpy as np

import ncg_restatement as nr

LD = np.longdouble
FLOOR_FACTOR = 16
CAP = 1e-9                       # what 16 x floor stays below for every case that is not a cancellation case
STRIDE = 65536                   # NCG_MAXPART * 256: scalars one pass of the clamped grid covers
SEEDS = (None, 1, 2, 3)
QUANTITIES = ("gg", "gd", "pp", "sd", "beta", "dir", "dnorm", "minStep", "newStep")
VECTOR_DEFECTS = ("stride_ignored", "npart_minus_1", "pr_gg", "sd_sign", "no_max0", "nan_kept", "dir_g_beta_g")
CONTROL_DEFECTS = ("gt", "flag_swapped", "exit_no_newstep", "alpha_newstep", "first_kept")


def npart_of(n):
    """block partials of n scalars: ncg_grid of csrc/ncg.hpp"""
    return min(256, max(1, (n + 255) // 256))


def _kept(n, defect):
    """the elements a sum takes"""
    i = np.arange(n)
    if defect == "stride_ignored":
        return i < STRIDE
    if defect == "npart_minus_1":
        return (i // 256) % 256 != npart_of(n) - 1
    return np.ones(n, dtype=bool)


def _sum(t, rng):
    if rng is not None:
        t = t[rng.permutation(len(t))]
    return t.sum() if len(t) else t.dtype.type(0)


def _max0(x, defect=None):
    """std::max(0.0, x) as the reference evaluates it: (0.0 < x) ? x : 0.0"""
    if defect == "no_max0":
        return x
    if defect == "nan_kept":
        return type(x)(0) if x < 0 else x
    return x if 0 < x else type(x)(0)


def beta_of(method, gg, gd, pp, sd, defect=None):
    """NonlinearConjugateGradientOptimizer.h:28-70 on the four sums; IEEE division (a zero divisor gives inf or NaN)"""
    with np.errstate(all="ignore"):
        if method == nr.FLETCHER_REEVES:
            return gg / pp
        den = sd if defect == "sd_sign" else -sd
        if method == nr.POLAK_RIBIERE:
            return _max0((gg if defect == "pr_gg" else gd) / pp, defect)
        if method == nr.HESTENES_STIEFEL:
            return _max0(gd / den, defect)
        return _max0(gg / den, defect)


def begin(dd, dtype):
    """head of lineSearch (.h:138-145) in `dtype` from the squared norm of the direction"""
    with np.errstate(all="ignore"):
        g = np.sqrt(dd)
        phi = dtype(0.5) * (dtype(1) + np.sqrt(dtype(5)))
        minStep = dtype(-1) / g
        newStep = minStep + (dtype(0) - minStep) / (phi + dtype(1))
    return dict(dnorm=g, minStep=minStep, newStep=newStep)


def direction(method, g, gp, s, dtype=LD, seed=None, defect=None, alias=0):
    """-> dict of QUANTITIES.  method 0..3: the dots of (g, gp, s), beta, dir = g + beta * s.  method -1: dir = g (alias 0) or dir = s
    (alias 1), beta 0, the dots absent (NaN)."""
    rng = None if seed is None else np.random.default_rng([int(seed), 20261021])
    g, s = np.asarray(g, dtype=np.float64).astype(dtype), np.asarray(s, dtype=np.float64).astype(dtype)
    n = len(g)
    keep = _kept(n, defect)
    out = {}
    with np.errstate(all="ignore"):
        if method < 0:
            new = (s if alias else g).copy()
            beta = dtype(0)
            out.update(gg=dtype(np.nan), gd=dtype(np.nan), pp=dtype(np.nan), sd=dtype(np.nan))
        else:
            gp = np.asarray(gp, dtype=np.float64).astype(dtype)
            d = g - gp
            gg, gd, pp, sd = (_sum(t[keep], rng) for t in (g * g, g * d, gp * gp, s * d))
            out.update(gg=gg, gd=gd, pp=pp, sd=sd)
            beta = beta_of(method, gg, gd, pp, sd, defect)
            new = g + beta * (g if defect == "dir_g_beta_g" else s)
        if defect == "stride_ignored":
            new[STRIDE:] = s[STRIDE:]
        dd = _sum((new * new)[keep], rng)
    out.update(beta=beta, dir=new, **begin(dd, dtype))
    return out


# ---------------------------------------------------------------- distances
def scalar_dist(a, b):
    """relative distance of a from the reference's b; 0 when both are NaN, the same infinity or both zero, inf when only one is"""
    a, b = LD(a), LD(b)
    if np.isnan(a) or np.isnan(b):
        return 0.0 if (np.isnan(a) and np.isnan(b)) else math.inf
    if np.isinf(a) or np.isinf(b) or b == 0:
        return 0.0 if a == b else math.inf
    return float(abs(a - b) / abs(b))


def vec_dist(a, b):
    """norm-wise relative distance over the finite elements; inf unless NaNs sit at the same places and infinities are the same"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not np.array_equal(fa, fb):
        return math.inf
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb) or not np.array_equal(a[~fb & ~nb], b[~fb & ~nb]):
        return math.inf
    a, b = a[fb], b[fb]
    norm = np.sqrt((b * b).sum())
    if norm == 0:
        return 0.0 if not a.any() else math.inf
    return float(np.sqrt(((a - b) ** 2).sum()) / norm)


def distances(got, want):
    return {q: (vec_dist if q == "dir" else scalar_dist)(got[q], want[q]) for q in QUANTITIES}


HALF_ULP = 0.5 * float(np.finfo(np.float64).eps)
NOISE = 64 * float(np.finfo(np.float64).eps)
NOISE_QUANTITIES = ("dir", "dnorm", "minStep", "newStep")


def _norm(a):
    a = np.asarray(a, dtype=LD)
    a = a[np.isfinite(a)]
    return float(np.sqrt((a * a).sum()))


def floors(method, g, gp, s, alias=0, ref=None):
    """(the long-double result, {quantity: largest distance of the float64 runs from it, "noise": bound or None}).
    noise: the new direction's norm lies below NOISE x |g| without being zero -- g + beta * s cancels to rounding errors (with ONE scalar
    Hestenes-Stiefel gives g - g (d s) / (s d) = 0 identically).  Such a direction has no digits to compare: it, and the record that
    follows from it, are bounded by NOISE x |g| instead (misses applies whichever holds)."""
    ref = direction(method, g, gp, s, alias=alias) if ref is None else ref
    out = dict.fromkeys(QUANTITIES, 0.0)
    for seed in SEEDS:
        d = distances(direction(method, g, gp, s, np.float64, seed, alias=alias), ref)
        out = {q: max(out[q], d[q]) for q in QUANTITIES}
    # Four samples can all land next to the long-double value by chance (measured: 1.3e-17 for one sum of plain[256]); the nearest
    # float64 to a real number lies up to half an ulp from it, so no floor that is not exactly 0 is taken below that.  A floor of
    # exactly 0 stays: every float64 operation of that quantity was exact (small integers, a zero vector, a copied direction).
    out = {q: (max(v, HALF_ULP) if v > 0 else 0.0) for q, v in out.items()}
    bound = NOISE * _norm(g)
    out["noise"] = bound if (method >= 0 and 0 < _norm(ref["dir"]) < bound and np.isfinite(np.asarray(ref["dir"], dtype=np.float64)).all()) else None
    return ref, out


def misses(got, want, floor):
    """{quantity: distance / (FLOOR_FACTOR x floor)}: <= 1 passes; a zero floor admits a zero distance only"""
    d = distances(got, want)
    out = {q: (0.0 if d[q] == 0 else (math.inf if floor[q] == 0 else d[q] / (FLOOR_FACTOR * floor[q]))) for q in QUANTITIES}
    if floor.get("noise") is not None:
        if not np.isfinite(np.asarray(got["dir"], dtype=np.float64)).all():
            return dict(out, dir=math.inf)
        out.update(dir=_norm(got["dir"]) / floor["noise"], dnorm=abs(float(got["dnorm"])) / floor["noise"], minStep=0.0, newStep=0.0)
    return out


# ---------------------------------------------------------------- the control rule with a planted defect
def ls_step_planted(rec, e, defect=None):
    """ncg_restatement.ls_step, copied, with the switches of CONTROL_DEFECTS (defect None: the same bits as ls_step)"""
    rec = dict(rec)
    if rec["done"]:
        return rec
    phi = 0.5 * (1.0 + math.sqrt(5.0))
    resphi = 2.0 - phi
    tau = nr.TAU
    minStep, maxStep, newStep, newError = rec["minStep"], rec["maxStep"], rec["newStep"], rec["newError"]
    if rec["first"]:
        newError = e
        if defect != "first_kept":
            rec["first"] = 0
    else:
        testStep, testError, flag = rec["step"], e, rec["flag"]
        if defect == "flag_swapped":
            flag = not flag
        if (testError > newError) if defect == "gt" else (testError >= newError):
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
    rec["trials"] += 1
    flag = (maxStep - newStep > newStep - minStep)
    testStep = newStep + resphi * (maxStep - newStep) if flag else newStep - resphi * (newStep - minStep)
    rec["minStep"], rec["maxStep"], rec["newStep"], rec["newError"] = minStep, maxStep, newStep, newError
    if (maxStep - minStep) < tau * (abs(testStep) + (0.0 if defect == "exit_no_newstep" else abs(newStep))):
        rec["alpha"] = newStep if defect == "alpha_newstep" else 0.5 * (minStep + maxStep)
        rec["done"] = 1
    else:
        rec["flag"] = int(flag)
        rec["step"] = testStep
    return rec


def final_step(rec, e):
    """ncg_final_kernel: the error of the final advance joins a finished record"""
    rec = dict(rec)
    if rec["done"]:
        rec["error"] = e
    return rec


def run_control(rec0, errors, final, step=nr.ls_step):
    """the records after every evaluation of an open-loop error sequence (final: the last error goes to final_step)"""
    out, rec = [], dict(rec0)
    k = len(errors) - (1 if final else 0)
    for i, e in enumerate(errors):
        rec = step(rec, e) if i < k else final_step(rec, e)
        out.append(rec)
    return out


def same_bits(a, b):
    """two records field for field, NaN equal to NaN, -0.0 different from 0.0"""
    for f in nr.RECORD_FIELDS:
        x, y = a[f], b[f]
        if isinstance(x, float) or isinstance(y, float):
            if np.float64(x).tobytes() != np.float64(y).tobytes() and not (math.isnan(x) and math.isnan(y)):
                return False
        elif int(x) != int(y):
            return False
    return True
