"""TEST INFRASTRUCTURE: the reference of the PCG edge tests (CPU only, numpy only).

The algorithm is tests/pcg_restatement.py's (GaussianFactorGraphSystem, preconditionedConjugateGradient, Dummy / BlockJacobi), vectorised
and in np.longdouble so that a chain of 65 537 poses takes seconds:
  * input: the raw arrays of lmgpu_get_jacobians as GaussianFactorGraph._fetch reads them (`Arrays`: graph index, rows, columns with
    the b column, offsets, column-major data), the slots of every factor's keys, the dimension of every slot, and the damping vector
    lambda * w that LM adds to the diagonal;
  * factors are batched by shape (rows, d0, d1, d2), variables by dimension; the batched Cholesky and the two triangular solves are
    written out (numpy's are float64 only); every scatter-add is a stable sort by target and np.add.reduceat (np.bincount rounds its
    weights to float64);
  * output: the whole trajectory, x_k and gamma_k for every k, and the threshold.

System(dtype=np.float64, seed=s) runs the same code in float64 with a seeded permutation of the factor order, of every variable's
incidence order and of the dot products' terms: a sample of the freedom a correct FP64 implementation has.  `tolerances` takes the
largest distance of three such runs from the long-double run as the floor of a comparison.

trajectory(defect=...) plants one defect of the device code (test_pcg_edges_reference.py shows that each is seen):
  ("stride_tail", cap)   the direction step leaves p of the variables >= cap * 256 as it was (a grid-stride loop without its second trip)
  "pq_beyond_256"        p . q without the block partials beyond the first 256 (scalars >= 65 536)
  "last_rr_partial"      gamma_k without the r . r partial of the last 256-variable block
  "key2_at_d0"           the third key's columns read at d0 + c in the transposed product and the diagonal blocks (System(key2_at_d0=True))
  "no_damping"           A p without lambda * w * p (the preconditioner keeps its damped blocks)
  ("stale", other)       H and b of another linearization (`other` is its System)
  "reset_prev_gamma"     a reset iteration divides by gamma_(k-1) instead of the fresh gamma in beta.  In exact arithmetic the two are the
                         same number (b - A x_k IS the residual the recurrence carries), so this one cannot be seen above the floor: the
                         floor is the size of their difference.  It is kept to show exactly that
  "reset_stale_partials" a reset iteration takes the partials of the FIRST residual (gamma_0) for its gamma: what the device would do if
                         the reset's precondition pass did not rewrite the buffer that pcg_start_kernel summed"""
from __future__ import annotations

import functools

import numpy as np

LD = np.longdouble
DUMMY, BLOCK_JACOBI = 0, 1
EPS64 = float(np.finfo(np.float64).eps)
CAP = 1e-9        # the bound tests/test_gpu_pcg.py holds BlockJacobi to
FLOOR_FACTOR = 16  # as the dense-front pin


class Params:
    """ConjugateGradientParameters (ConjugateGradientSolver.h:46-50)"""

    def __init__(self, minIterations=1, maxIterations=500, reset=501, epsilon_rel=1e-3, epsilon_abs=1e-3, preconditioner=BLOCK_JACOBI):
        self.minIterations, self.maxIterations, self.reset = int(minIterations), int(maxIterations), int(reset)
        self.epsilon_rel, self.epsilon_abs, self.preconditioner = epsilon_rel, epsilon_abs, preconditioner


class Arrays:
    """what lmgpu_get_jacobians returns plus the layout: factor i is graph factor gi[i], rows[i] x cols[i] column-major at off[i] (its last
    column is b); slots[g] = the slots of graph factor g's keys (-1 beyond its arity); dims[s] = dimension of slot s"""

    def __init__(self, gi, rows, cols, off, data, slots, dims):
        self.gi, self.rows, self.cols = (np.asarray(a, dtype=np.int64) for a in (gi, rows, cols))
        self.off, self.data = np.asarray(off, dtype=np.int64), np.asarray(data, dtype=np.float64)
        self.slots, self.dims = np.asarray(slots, dtype=np.int64).reshape(-1, 3), np.asarray(dims, dtype=np.int64)

    @staticmethod
    def from_blocks(blocks, slots, dims):
        """blocks: one (rows, cols + 1) [A b] per graph factor, in graph order"""
        rows = np.array([b.shape[0] for b in blocks], dtype=np.int64)
        cols = np.array([b.shape[1] for b in blocks], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(rows * cols)])
        data = np.concatenate([np.asarray(b, dtype=np.float64).T.reshape(-1) for b in blocks]) if len(blocks) else np.zeros(0)
        return Arrays(np.arange(len(blocks)), rows, cols, off, data, slots, dims)


def _scatter_plan(targets, rng):
    """(order, starts, unique targets) of a scatter-add as sort + reduceat; rng permutes the order of the terms of every target"""
    n = len(targets)
    pre = np.arange(n) if rng is None else rng.permutation(n)
    order = pre[np.argsort(targets[pre], kind="stable")]
    t = targets[order]
    starts = np.flatnonzero(np.concatenate([[True], t[1:] != t[:-1]])) if n else np.zeros(0, dtype=np.int64)
    return order, starts, (t[starts] if n else t)


class System:
    """A = sum J^T J + diag(damp), b = sum J^T b_f over the factors of `arr`"""

    def __init__(self, arr: Arrays, damp, dtype=LD, seed=None, key2_at_d0=False):
        self.dtype, self.arr = dtype, arr
        rng = None if seed is None else np.random.default_rng([int(seed), 20261021])
        self.rng = rng
        dims = arr.dims
        self.nvars = len(dims)
        self.xoff = np.concatenate([[0], np.cumsum(dims)])
        self.n = int(self.xoff[-1])
        self.damp = np.asarray(damp, dtype=np.float64).astype(dtype)
        assert self.damp.shape == (self.n,)
        s = arr.slots[arr.gi]
        fd = np.where(s >= 0, dims[np.maximum(s, 0)], 0)
        assert np.array_equal(fd.sum(axis=1) + 1, arr.cols), "columns do not match the keys' dimensions"
        shape = np.concatenate([arr.rows[:, None], fd], axis=1)
        uniq, inv = np.unique(shape, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        self.groups = []
        targets, vtargets = [], {}
        for g, (m, d0, d1, d2) in enumerate(uniq.tolist()):
            F = np.flatnonzero(inv == g)
            if rng is not None:
                F = rng.permutation(F)
            c = d0 + d1 + d2
            Ab = arr.data[arr.off[F][:, None] + np.arange(m * (c + 1))[None, :]].reshape(len(F), c + 1, m).transpose(0, 2, 1).astype(dtype)
            A, b = np.ascontiguousarray(Ab[:, :, :c]), np.ascontiguousarray(Ab[:, :, c])
            At = A
            if key2_at_d0 and d2 > 0:
                At = A.copy()
                At[:, :, d0 + d1:] = A[:, :, d0:d0 + d2]
            idx, o = [], 0
            for p, d in enumerate((d0, d1, d2)):
                if d:
                    idx.append(self.xoff[s[F, p]][:, None] + np.arange(d)[None, :])
                    vtargets.setdefault(d, []).append((g, o, s[F, p]))
                    o += d
            idx = np.concatenate(idx, axis=1)
            self.groups.append(dict(A=A, At=At, b=b, idx=idx))
            targets.append(idx.reshape(-1))
        targets = np.concatenate(targets) if targets else np.zeros(0, dtype=np.int64)
        self._order, self._starts, self._uniq = _scatter_plan(targets, rng)
        # the undamped diagonal blocks, by dimension
        self.vars_of, self.H = {}, {}
        for d in sorted(set(dims.tolist())):
            V = np.flatnonzero(dims == d)
            self.vars_of[d] = V
            local = np.full(self.nvars, -1, dtype=np.int64)
            local[V] = np.arange(len(V))
            H = np.zeros((len(V), d, d), dtype=dtype)
            if d in vtargets:
                blocks, tg = [], []
                for g, o, sl in vtargets[d]:
                    Ap = self.groups[g]["At"][:, :, o:o + d]
                    blocks.append((Ap[:, :, :, None] * Ap[:, :, None, :]).sum(axis=1))
                    tg.append(local[sl])
                blocks, tg = np.concatenate(blocks), np.concatenate(tg)
                order, starts, uq = _scatter_plan(tg, rng)
                H[uq] = np.add.reduceat(blocks[order], starts, axis=0)
            self.H[d] = H
        self.rhs = self._Jt([G["b"] for G in self.groups])

    # -- products
    def _J(self, x):
        return [(G["A"] * x[G["idx"]][:, None, :]).sum(axis=2) for G in self.groups]

    def _Jt(self, ys):
        out = np.zeros(self.n, dtype=self.dtype)
        if not self.groups:
            return out
        vals = np.concatenate([(G["At"] * y[:, :, None]).sum(axis=1).reshape(-1) for G, y in zip(self.groups, ys)])
        out[self._uniq] = np.add.reduceat(vals[self._order], self._starts)
        return out

    def multiply(self, x, damping=True):
        q = self._Jt(self._J(x))
        return q + self.damp * x if damping else q

    def dot(self, a, b, keep=None):
        t = a * b
        if keep is not None:
            t = t[:keep]
        if self.rng is not None:
            t = t[self.rng.permutation(len(t))]
        return t.sum()

    def hessian_diagonal(self):
        out = np.zeros(self.n, dtype=self.dtype)
        for d, V in self.vars_of.items():
            out[self.xoff[V][:, None] + np.arange(d)[None, :]] = self.H[d][:, np.arange(d), np.arange(d)]
        return out

    def residual_norm(self, x):
        """|b - A x| (2-norm)"""
        r = self.rhs - self.multiply(x)
        return np.sqrt((r * r).sum())


def damping_vector(arr: Arrays, lam, diagonal, min_diag=1e-6, max_diag=1e32):
    """lambda * w: w = 1, or the clamped Hessian diagonal (LevenbergMarquardtOptimizer.cpp:291-298) summed in long double"""
    n = int(arr.dims.sum())
    if not diagonal:
        return np.full(n, float(lam))
    h = System(arr, np.zeros(n)).hessian_diagonal().astype(np.float64)
    return float(lam) * np.clip(h, min_diag, max_diag)


# ---------------------------------------------------------------- batched Cholesky and triangular solves
def _chol(H):
    n, d, _ = H.shape
    L = np.zeros_like(H)
    for j in range(d):
        s = H[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(axis=1)
        assert (s > 0).all(), "a diagonal block is not positive definite"
        L[:, j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            L[:, i, j] = (H[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
    return L


def _lsolve(L, y):
    y = y.copy()
    for i in range(L.shape[1]):
        y[:, i] = (y[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
    return y


def _ltsolve(L, y):
    y = y.copy()
    for i in range(L.shape[1] - 1, -1, -1):
        y[:, i] = (y[:, i] - (L[:, i + 1:, i] * y[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return y


class _Precond:
    def __init__(self, S: System, kind, H=None):
        self.S, self.kind, self.L, self.X = S, kind, {}, {}
        if kind == BLOCK_JACOBI:
            for d, V in S.vars_of.items():
                X = S.xoff[V][:, None] + np.arange(d)[None, :]
                Hd = (S.H if H is None else H)[d].copy()
                Hd[:, np.arange(d), np.arange(d)] += S.damp[X]
                self.L[d], self.X[d] = _chol(Hd), X

    def _each(self, x, fn):
        if self.kind == DUMMY:
            return x.copy()
        y = x.copy()
        for d, X in self.X.items():
            y[X] = fn(self.L[d], x[X])
        return y

    def solve(self, x):
        return self._each(x, _lsolve)

    def transposeSolve(self, x):
        return self._each(x, _ltsolve)


class Trajectory:
    def __init__(self, x, gammas, threshold, iterations):
        self.x, self.gammas, self.threshold, self.iterations = x, gammas, threshold, iterations

    def x64(self, k):
        return np.asarray(self.x[k], dtype=np.float64)


def trajectory(S: System, p: Params, defect=None):
    """preconditionedConjugateGradient from x = 0 (ConjugateGradientSolver.h:109-171): x[k], gammas[k] for k = 0 .. iterations"""
    name = defect[0] if isinstance(defect, tuple) else defect
    H, b = (defect[1].H, defect[1].rhs) if name == "stale" else (None, S.rhs)
    P = _Precond(S, p.preconditioner, H)
    damping = name != "no_damping"
    keep_pq = 65536 if name == "pq_beyond_256" else None
    keep_rr = int(S.xoff[256 * ((S.nvars + 255) // 256 - 1)]) if name == "last_rr_partial" else None
    tail = int(S.xoff[min(S.nvars, defect[1] * 256)]) if name == "stride_tail" else None
    estimate = np.zeros(S.n, dtype=S.dtype)
    residual = P.solve(b - S.multiply(estimate, damping))
    direction = P.transposeSolve(residual)
    gamma = S.dot(residual, residual)
    threshold = max(S.dtype(p.epsilon_abs), S.dtype(p.epsilon_rel) * S.dtype(p.epsilon_rel) * gamma)
    xs, gammas = [estimate], [gamma]
    k = 1
    while k <= p.maxIterations and (gamma > threshold or k <= p.minIterations):
        reset = k % p.reset == 0
        if reset:
            residual = P.solve(b - S.multiply(estimate, damping))
            direction = P.transposeSolve(residual)
            gamma = gammas[0] if name == "reset_stale_partials" else S.dot(residual, residual)
        q1 = S.multiply(direction, damping)
        alpha = gamma / S.dot(direction, q1, keep_pq)
        estimate = estimate + alpha * direction
        residual = residual + (-alpha) * P.solve(q1)
        prev = gammas[-1] if (reset and name == "reset_prev_gamma") else gamma
        gamma = S.dot(residual, residual, keep_rr)
        beta = gamma / prev
        new = beta * direction + P.transposeSolve(residual)
        if tail is not None:
            new[tail:] = direction[tail:]
        direction = new
        xs.append(estimate)
        gammas.append(gamma)
        k += 1
    return Trajectory(xs, gammas, threshold, k - 1)


# ---------------------------------------------------------------- distances and tolerances
def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(LD(1e-300), np.sqrt((b * b).sum())))


def relg(a, b):
    return float(abs(LD(a) - LD(b)) / max(LD(1e-300), abs(LD(b))))


NOISE = 1e-24  # gamma_k below NOISE * gamma_0: the solve has ended, gamma_k is the square of rounding errors and has no digits to compare


def tolerances(arr: Arrays, damp, p: Params, ks, seeds=(1, 2, 3), ref=None):
    """(the long-double trajectory, {k: dict(floor_x, floor_g, raw_x, raw_g, tol_x, tol_g, noise)}): floor = the largest distance of the
    permuted float64 runs from the long-double run at iteration k, raw = 16 x floor and never below 64 ulps, tol = raw capped at 1e-9.  A
    test asserts raw <= CAP on its own (check_cap): the cap is a condition on the case, not something the device can be excused by.
    Where the long-double gamma_k and every float64 one lie below NOISE * gamma_0, gamma_k is not compared but bounded (noise = that
    bound, else None; gamma_miss applies whichever holds)."""
    ref = trajectory(System(arr, damp), p) if ref is None else ref
    runs = [trajectory(System(arr, damp, np.float64, s), p) for s in seeds]
    out = {}
    for k in ks:
        assert k <= ref.iterations and all(k <= r.iterations for r in runs), (k, ref.iterations)
        fx = max(rel(r.x[k], ref.x[k]) for r in runs) if k > 0 else 0.0
        bound = NOISE * float(ref.gammas[0])
        noise = bound if all(float(r.gammas[k]) < bound for r in runs + [ref]) else None
        fg = 0.0 if noise is not None else max(relg(r.gammas[k], ref.gammas[k]) for r in runs)
        rx, rg = max(FLOOR_FACTOR * fx, 64 * EPS64), max(FLOOR_FACTOR * fg, 64 * EPS64)
        out[k] = dict(floor_x=fx, floor_g=fg, raw_x=rx, raw_g=rg, tol_x=min(rx, CAP), tol_g=min(rg, CAP), noise=noise)
    return ref, out


def check_cap(tol, ks):
    for k in ks:
        assert tol[k]["raw_x"] <= CAP and tol[k]["raw_g"] <= CAP, (k, tol[k])


def gamma_miss(t, got, want):
    """distance of a gamma_k from the reference's in tolerances (<= 1 passes)"""
    if t["noise"] is not None:
        return float(got) / t["noise"]
    return relg(got, want) / t["tol_g"]


def x_miss(t, got, want):
    return rel(got, want) / t["tol_x"]


def oracle_arrays(case, slots, dims, moved=False):
    """Arrays of a pcg_cases case from the CPU oracle's Jacobians (a device test reads the device's own instead).  moved: linearized
    at values retracted by a seeded step of a few hundredths -- a second linearization of the same graph"""
    import oracle_harness as oh
    keys = case["initial"].keys()
    orc = oh.OracleProblem(case["graph"], case["initial"], keys)
    if moved:
        rng = np.random.default_rng(5)
        orc.retract({k: rng.normal(0.0, 0.02, int(d)) for k, d in zip(keys, dims)})
    orc.linearize()
    return Arrays.from_blocks([orc.jacobian(g) for g in range(case["graph"].size())], slots, dims)


MODES = [(pre, diag) for pre in (BLOCK_JACOBI, DUMMY) for diag in (False, True)]
MODE_IDS = ["%s-%s" % ("bj" if p else "dummy", "diag" if d else "identity") for p, d in MODES]


def mode_id(pre, diag):
    return MODE_IDS[MODES.index((pre, diag))]


def params(pre, **kw):
    """eps 0 unless given: a run of exactly maxIterations iterations"""
    kw.setdefault("epsilon_rel", 0.0)
    kw.setdefault("epsilon_abs", 0.0)
    return Params(preconditioner=pre, **kw)


@functools.lru_cache(maxsize=None)
def cpu_arrays(name, moved=False):
    import pcg_cases as pc
    c = pc.case(name)
    slots, dims = pc.layout(c)
    return oracle_arrays(c, slots, dims, moved)


@functools.lru_cache(maxsize=None)
def cpu_compared(name, pre, diag, kmax, reset=501, lam=1e-3):
    """(arrays, damping vector, long-double trajectory, tolerances of k = 0 .. kmax, seconds of the long-double run) on the CPU oracle's
    Jacobians"""
    import time
    arr = cpu_arrays(name)
    damp = damping_vector(arr, lam, diag)
    t0 = time.time()
    r = trajectory(System(arr, damp), params(pre, maxIterations=kmax, reset=reset))
    t1 = time.time() - t0
    r, tol = tolerances(arr, damp, params(pre, maxIterations=kmax, reset=reset), range(kmax + 1), ref=r)
    return arr, damp, r, tol, t1


def stop_epsilon(ref: Trajectory, kstar):
    """eps_abs that stops the loop after exactly kstar iterations: the geometric mean of gamma_(kstar-1) and gamma_kstar, after asserting on
    the reference alone that both lie a factor 16 from it and that no earlier gamma is below it"""
    g = [float(x) for x in ref.gammas]
    eps = float(np.sqrt(g[kstar - 1] * g[kstar]))
    assert g[kstar] * 16 <= eps and eps * 16 <= g[kstar - 1], (kstar, g[kstar - 1], eps, g[kstar])
    assert all(x > eps for x in g[:kstar]), (kstar, eps, g[:kstar])
    return eps
