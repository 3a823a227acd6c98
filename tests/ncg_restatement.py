"""TEST INFRASTRUCTURE: float64 restatement of the reference's nonlinear conjugate gradient, written from
gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h (lineSearch :135-181, nonlinearConjugateGradient :195-289, the four beta
formulas :28-70) and .cpp (System :51-69, iterate :71-80, optimize :82-90).  It depends on no device.

The templates are restated over a `system` with error(state), gradient(state) -> flat numpy vector and advance(state, alpha, g).
OracleSystem takes graph.error, the whitened Jacobians and retract from the CPU oracle (tests/oracle_harness.py) and forms
gradientAtZero = -sum_f A_f^T b_f (GaussianFactorGraph.cpp:357-367) from the oracle's Jacobians with numpy; its gradients are the
concatenation over the variables in ascending Key order (the order of Values and VectorValues)."""
from __future__ import annotations

import math

import numpy as np

FLETCHER_REEVES, POLAK_RIBIERE, HESTENES_STIEFEL, DAI_YUAN = 0, 1, 2, 3
TAU = 1e-5          # .h:143
MAX_TRIALS = 128    # the bound the device code uses (csrc/ncg.hpp, NCG_MAX_TRIALS)


class Params:
    """NonlinearOptimizerParams defaults (gtsam/nonlinear/NonlinearOptimizerParams.h:41-44)"""

    def __init__(self, maxIterations=100, relativeErrorTol=1e-5, absoluteErrorTol=1e-5, errorTol=0.0):
        self.maxIterations, self.relativeErrorTol, self.absoluteErrorTol, self.errorTol = maxIterations, relativeErrorTol, absoluteErrorTol, errorTol


def check_convergence(relTol, absTol, errTol, currentError, newError):
    """checkConvergence, gtsam/nonlinear/NonlinearOptimizer.cpp:182-231 (verbosity left out)"""
    if newError <= errTol:
        return True
    absoluteDecrease = currentError - newError
    relativeDecrease = absoluteDecrease / currentError
    return bool((relTol and relativeDecrease <= relTol) or absoluteDecrease <= absTol)


def _max0(x):
    """std::max(0.0, x): (0.0 < x) ? x : 0.0 -- a NaN gives 0"""
    return x if 0.0 < x else 0.0


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def fletcher_reeves(g, gp):
    return _div(g @ g, gp @ gp)  # .h:32-35


def polak_ribiere(g, gp):
    return _max0(_div(g @ (g - gp), gp @ gp))  # .h:42-46


def hestenes_stiefel(g, gp, direction):
    d = g - gp
    return _max0(_div(g @ d, -(direction @ d)))  # .h:55-58


def dai_yuan(g, gp, direction):
    return _max0(_div(g @ g, -(direction @ (g - gp))))  # .h:65-69


RECORD_FIELDS = ("minStep", "maxStep", "newStep", "newError", "step", "alpha", "error", "beta", "dnorm", "done", "trials", "flag", "first")


def ls_begin(g, beta=0.0):
    """head of lineSearch (.h:138-145) as a record: g = |direction|, the bracket [-1 / g, 0], the first interior point.  The record has
    the fields of the device's NcgCtl (csrc/kernels_ncg.hpp): `step` is the step whose error the next ls_step takes (newStep first,
    then every testStep), `first` says that newError is still pending, `flag` is the flag of the testStep under evaluation."""
    phi = 0.5 * (1.0 + math.sqrt(5.0))
    minStep = _div(-1.0, g)
    maxStep = 0.0
    newStep = minStep + (maxStep - minStep) / (phi + 1.0)
    return dict(minStep=minStep, maxStep=maxStep, newStep=newStep, newError=0.0, step=newStep, alpha=0.0, error=0.0, beta=beta, dnorm=g,
                done=0, trials=0, flag=0, first=1)


def ls_step(rec, e):
    """one evaluation of lineSearch: e = the error at rec['step'].  The first call takes it as newError (.h:147-148), every later one as
    testError and updates the working range (:163-178); then the next testStep and the exit test (:151-157).  Returns a new record;
    a record that is done comes back unchanged."""
    rec = dict(rec)
    if rec["done"]:
        return rec
    phi = 0.5 * (1.0 + math.sqrt(5.0))
    resphi = 2.0 - phi
    tau = TAU
    minStep, maxStep, newStep, newError = rec["minStep"], rec["maxStep"], rec["newStep"], rec["newError"]
    if rec["first"]:
        newError = e
        rec["first"] = 0
    else:
        testStep, testError, flag = rec["step"], e, rec["flag"]
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
    rec["trials"] += 1
    flag = (maxStep - newStep > newStep - minStep)
    testStep = newStep + resphi * (maxStep - newStep) if flag else newStep - resphi * (newStep - minStep)
    rec["minStep"], rec["maxStep"], rec["newStep"], rec["newError"] = minStep, maxStep, newStep, newError
    if (maxStep - minStep) < tau * (abs(testStep) + abs(newStep)):
        rec["alpha"] = 0.5 * (minStep + maxStep)
        rec["done"] = 1
    else:
        rec["flag"] = int(flag)
        rec["step"] = testStep
    return rec


def line_search(system, currentValues, gradient, stats=None):
    """lineSearch (.h:135-181) as ls_begin and a loop of ls_step.  stats (a dict, optional): 'trials' = error evaluations, 'bracket' =
    (minStep, maxStep) at exit."""
    rec = ls_begin(float(np.linalg.norm(gradient)))
    while True:
        rec = ls_step(rec, system.error(system.advance(currentValues, rec["step"], gradient)))
        if rec["done"]:
            if stats is not None:
                stats["trials"] = rec["trials"]
                stats["bracket"] = (rec["minStep"], rec["maxStep"])
            return rec["alpha"]
        if rec["trials"] >= 100000:
            raise RuntimeError("lineSearch does not terminate (the reference would loop for ever)")


def nonlinear_conjugate_gradient(system, initial, params, singleIteration, directionMethod=POLAK_RIBIERE, gradientDescent=False, trace=None,
                                 moveAlpha=None):
    """nonlinearConjugateGradient (.h:195-289) -> (values, iterations).  trace (a list, optional) receives one
    (alpha, beta, error, trials) per line search, the uncounted gradient-descent step first.  moveAlpha (a function, optional): every
    line search's alpha goes through it before the advance -- the probe of how far the bracket tolerance moves what follows."""
    moveAlpha = moveAlpha or (lambda a: a)
    iteration = 0
    currentError = system.error(initial)
    if currentError <= params.errorTol:
        return initial, iteration
    currentValues = initial
    currentGradient = system.gradient(currentValues)
    prevGradient = None
    direction = currentGradient.copy()
    st = {}
    prevValues = currentValues
    prevError = currentError
    alpha = moveAlpha(line_search(system, currentValues, direction, st))
    currentValues = system.advance(prevValues, alpha, direction)
    currentError = system.error(currentValues)
    if trace is not None:
        trace.append((alpha, 0.0, currentError, st["trials"]))
    while True:
        if gradientDescent:
            direction = system.gradient(currentValues)
            beta = 0.0
        else:
            prevGradient = currentGradient
            currentGradient = system.gradient(currentValues)
            if directionMethod == FLETCHER_REEVES:
                beta = fletcher_reeves(currentGradient, prevGradient)
            elif directionMethod == POLAK_RIBIERE:
                beta = polak_ribiere(currentGradient, prevGradient)
            elif directionMethod == HESTENES_STIEFEL:
                beta = hestenes_stiefel(currentGradient, prevGradient, direction)
            elif directionMethod == DAI_YUAN:
                beta = dai_yuan(currentGradient, prevGradient, direction)
            else:
                raise RuntimeError("NonlinearConjugateGradientOptimizer: Invalid directionMethod")
            direction = currentGradient + (beta * direction)
        alpha = moveAlpha(line_search(system, currentValues, direction, st))
        prevValues = currentValues
        prevError = currentError
        currentValues = system.advance(prevValues, alpha, direction)
        currentError = system.error(currentValues)
        if trace is not None:
            trace.append((alpha, beta, currentError, st["trials"]))
        iteration += 1
        if not (iteration < params.maxIterations and not singleIteration
                and not check_convergence(params.relativeErrorTol, params.absoluteErrorTol, params.errorTol, prevError, currentError)):
            break
    return currentValues, iteration


class Quadratic1D:
    """error(x) = 0.5 a (x - c)^2 on the real line: the line search's minimiser along the gradient is alpha = -1 / a"""

    def __init__(self, a, c):
        self.a, self.c = float(a), float(c)

    def error(self, x):
        return 0.5 * self.a * (x - self.c) ** 2

    def gradient(self, x):
        return np.array([self.a * (x - self.c)])

    def advance(self, x, alpha, g):
        return x + alpha * float(g[0])


class OracleSystem:
    """NonlinearConjugateGradientOptimizer::System (.h:83-98, .cpp:51-69) over the CPU oracle.  A state is a Values.
    perturb (a numpy Generator, optional): every error is multiplied by (1 +- eps), sign drawn from it -- the probe of how far the
    last bits of the error move the bracket sequence (the branch testError >= newError)."""

    def __init__(self, graph, perturb=None, eps=1e-15):
        self.eps = eps
        import oracle_harness as oh
        self._oh = oh
        self.graph = graph
        self.fkeys = graph.factor_keys_in_graph_order()
        self.perturb = perturb
        self._cache = (None, None)

    def _problem(self, values):
        if self._cache[0] is not values:
            self._cache = (values, self._oh.OracleProblem(self.graph, values, values.keys()))
        return self._cache[1]

    def offsets(self, values):
        from gtsam_personal_amd.graph import VAR_DIM
        off, o = {}, 0
        for k in values.keys():
            off[k] = (o, o + VAR_DIM[values.type(k)])
            o += VAR_DIM[values.type(k)]
        return off, o

    def error(self, values):
        e = self._problem(values).error()
        if self.perturb is not None:
            e *= 1.0 + (self.eps if self.perturb.integers(0, 2) else -self.eps)
        return e

    def gradient(self, values):
        p = self._problem(values)
        p.linearize()
        off, n = self.offsets(values)
        g = np.zeros(n)
        for i, keys in enumerate(self.fkeys):
            if keys is None:
                continue
            Ab = p.jacobian(i)
            b = Ab[:, -1]
            c = 0
            for k in keys:
                lo, hi = off[k]
                g[lo:hi] -= Ab[:, c:c + hi - lo].T @ b
                c += hi - lo
        return g

    def by_key(self, values, g):
        off, _ = self.offsets(values)
        return {k: g[lo:hi].copy() for k, (lo, hi) in off.items()}

    def advance(self, values, alpha, g):
        step = g * alpha  # Gradient step = g; step *= alpha (.cpp:66-67)
        p = self._oh.OracleProblem(self.graph, values, values.keys())
        p.retract(self.by_key(values, step))
        out = values.copy()
        for k, v in p.values().items():
            out.update(k, v)
        self._cache = (out, p)  # the oracle problem now sits at the new values
        return out
