"""numpy restatement of the reference's iterative linear solver, line by line (test helper, CPU only).

  GaussianFactorGraphSystem          gtsam/linear/PCGSolver.cpp:69-145   (residual, multiply, getb, left/right precondition)
  preconditionedConjugateGradient    gtsam/linear/ConjugateGradientSolver.h:109-171
  DummyPreconditioner                gtsam/linear/Preconditioner.h (solve / transposeSolve = copy)
  BlockJacobiPreconditioner          gtsam/linear/Preconditioner.cpp:80-177 (L = chol(H_jj) lower; solve L^-1 x, transposeSolve L^-T x)

Input: whitened factors as (keys, [A_1 .. A_k], b) and {key: dim}; LM's damping priors as {key: vector added to the diagonal}.
The vector layout follows `order` (default: keys ascending = KeyInfo(gfg), IterativeSolver.cpp:111-114)."""
from __future__ import annotations

import numpy as np

DUMMY, BLOCK_JACOBI = 0, 1


class PCGParams:
    """ConjugateGradientParameters defaults (ConjugateGradientSolver.h:46-50)"""

    def __init__(self, minIterations=1, maxIterations=500, reset=501, epsilon_rel=1e-3, epsilon_abs=1e-3, preconditioner=BLOCK_JACOBI):
        self.minIterations, self.maxIterations, self.reset = minIterations, maxIterations, reset
        self.epsilon_rel, self.epsilon_abs, self.preconditioner = epsilon_rel, epsilon_abs, preconditioner


class System:
    """GaussianFactorGraphSystem over the factors plus the damping diagonal"""

    def __init__(self, factors, dims, damping=None, order=None):
        self.keys = sorted(dims) if order is None else [int(k) for k in order]
        self.dims = {int(k): int(dims[k]) for k in self.keys}
        self.off, o = {}, 0
        for k in self.keys:
            self.off[k] = o
            o += self.dims[k]
        self.n = o
        rows, cols, vals, bs = [], [], [], []
        self.blocks = {k: np.zeros((self.dims[k], self.dims[k])) for k in self.keys}
        r0 = 0
        for keys, As, b in factors:
            b = np.asarray(b, dtype=float)
            m = len(b)
            for k, A in zip(keys, As):
                A = np.asarray(A, dtype=float).reshape(m, -1)
                d = A.shape[1]
                rows.append(r0 + np.repeat(np.arange(m), d))
                cols.append(self.off[int(k)] + np.tile(np.arange(d), m))
                vals.append(A.reshape(-1))
                self.blocks[int(k)] += A.T @ A  # JacobianFactor::hessianBlockDiagonal
            bs.append(b)
            r0 += m
        self.m = r0
        self.rows = np.concatenate(rows) if rows else np.zeros(0, dtype=int)
        self.cols = np.concatenate(cols) if cols else np.zeros(0, dtype=int)
        self.vals = np.concatenate(vals) if vals else np.zeros(0)
        self.brow = np.concatenate(bs) if bs else np.zeros(0)
        self.damp = np.zeros(self.n)
        for k, v in (damping or {}).items():  # LM's damping priors (LevenbergMarquardtOptimizer.cpp:139-176): lambda * w on the diagonal
            k = int(k)
            self.damp[self.off[k]:self.off[k] + self.dims[k]] = np.asarray(v, dtype=float)
            self.blocks[k] = self.blocks[k] + np.diag(np.asarray(v, dtype=float))

    def _J(self, x):
        return np.bincount(self.rows, self.vals * x[self.cols], minlength=self.m)

    def _Jt(self, y):
        return np.bincount(self.cols, self.vals * y[self.rows], minlength=self.n)

    def multiply(self, x):  # A^T A x (multiplyHessianAdd over every factor, damping priors included)
        return self._Jt(self._J(x)) + self.damp * x

    def getb(self):  # -gradientAtZero
        return self._Jt(self.brow)

    def residual(self, x):  # b - A x
        return self.getb() - self.multiply(x)


class Preconditioner:
    def __init__(self, system: System, kind):
        self.s, self.kind, self.L = system, kind, {}
        if kind == BLOCK_JACOBI:
            for k in system.keys:
                self.L[k] = np.linalg.cholesky(system.blocks[k])  # blocks[i].llt().matrixL()

    def _each(self, x, fn):
        y = np.array(x, dtype=float)
        if self.kind == DUMMY:
            return y
        for k in self.s.keys:
            o, d = self.s.off[k], self.s.dims[k]
            y[o:o + d] = fn(self.L[k], y[o:o + d])
        return y

    def solve(self, x):  # L^-1 x
        return self._each(x, lambda L, v: _forward(L, v))

    def transposeSolve(self, x):  # L^-T x
        return self._each(x, lambda L, v: _backward(L.T, v))


def _forward(L, v):
    y = np.array(v, dtype=float)
    for i in range(len(y)):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def _backward(U, v):
    y = np.array(v, dtype=float)
    for i in range(len(y) - 1, -1, -1):
        y[i] = (y[i] - U[i, i + 1:] @ y[i + 1:]) / U[i, i]
    return y


def pcg(system: System, params: PCGParams):
    """preconditionedConjugateGradient from x = 0.  Returns (x, iterations = loop bodies executed, gammas = [gamma0, gamma_1, ..],
    threshold)."""
    P = Preconditioner(system, params.preconditioner)
    estimate = np.zeros(system.n)
    q1 = system.residual(estimate)
    residual = P.solve(q1)
    direction = P.transposeSolve(residual)
    currentGamma = float(residual @ residual)
    threshold = max(params.epsilon_abs, params.epsilon_rel * params.epsilon_rel * currentGamma)
    gammas = [currentGamma]
    k = 1
    while k <= params.maxIterations and (currentGamma > threshold or k <= params.minIterations):
        if k % params.reset == 0:
            q1 = system.residual(estimate)
            residual = P.solve(q1)
            direction = P.transposeSolve(residual)
            currentGamma = float(residual @ residual)
        q1 = system.multiply(direction)
        alpha = currentGamma / float(direction @ q1)
        estimate = estimate + alpha * direction
        q2 = P.solve(q1)
        residual = residual + (-alpha) * q2
        prevGamma = currentGamma
        currentGamma = float(residual @ residual)
        beta = currentGamma / prevGamma
        q1 = P.transposeSolve(residual)
        direction = beta * direction + q1
        gammas.append(currentGamma)
        k += 1
    return estimate, k - 1, gammas, threshold


def by_key(system: System, x):
    return {k: x[system.off[k]:system.off[k] + system.dims[k]].copy() for k in system.keys}
