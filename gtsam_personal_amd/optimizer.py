"""LevenbergMarquardtOptimizer mirror over the C ABI (include/lmgpu.h).

Same names / argument meaning / error behaviour as the reference interface it stands in for:
  LevenbergMarquardtParams       gtsam/nonlinear/LevenbergMarquardtParams.h:35-157
  LevenbergMarquardtOptimizer    gtsam/nonlinear/LevenbergMarquardtOptimizer.h  (iterate :103, linearize :113, lambda, getInnerIterations)
  NonlinearOptimizer             gtsam/nonlinear/NonlinearOptimizer.h (optimize :98, error, iterations, values, solve :129)
  PCGSolverParameters            gtsam/linear/PCGSolver.h:36-50, ConjugateGradientSolver.h:34-50 (linearSolverType = "ITERATIVE")
All numerics run in liblmgpu.so on the GPU; this file only marshals arrays.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib
from .graph import (CAM_BUNDLER, POINT3, F_PRIOR_CAM, F_SFM, FACTOR_ARITY, N_UNIT, VAR_DIM, VAR_STORE, VAR_STORE_DEV, NonlinearFactorGraph, Ordering,
                    Values)


class DummyPreconditionerParameters:
    """gtsam/linear/Preconditioner.h: the identity preconditioner"""
    kind = _lib.LMGPU_PRECOND_DUMMY


class BlockJacobiPreconditionerParameters:
    """gtsam/linear/Preconditioner.h: L = chol(H_jj) per variable of the damped graph's hessianBlockDiagonal"""
    kind = _lib.LMGPU_PRECOND_BLOCK_JACOBI


class PCGSolverParameters:
    """PCGSolverParameters (gtsam/linear/PCGSolver.h:36-50) = ConjugateGradientParameters (ConjugateGradientSolver.h:34-50, defaults
    minIterations 1, maxIterations 500, reset 501, epsilon_rel 1e-3, epsilon_abs 1e-3) + the preconditioner's parameters (default none:
    the reference's createPreconditioner throws for it, Preconditioner.cpp:189-205, and so does the optimizer here)."""

    def __init__(self, preconditioner=None):
        self.minIterations = 1
        self.maxIterations = 500
        self.reset = 501
        self.epsilon_rel = 1e-3
        self.epsilon_abs = 1e-3
        self.preconditioner = preconditioner

    def _c(self):
        pre = self.preconditioner
        if not isinstance(pre, (DummyPreconditionerParameters, BlockJacobiPreconditionerParameters)):
            raise ValueError("createPreconditioner: unexpected preconditioner parameter type (Dummy or BlockJacobi are bound)")
        if int(self.reset) < 1:
            raise ValueError("PCGSolverParameters.reset must be >= 1")
        return _lib.lmgpu_pcg_params(pre.kind, int(self.minIterations), int(self.maxIterations), int(self.reset), float(self.epsilon_rel),
                                     float(self.epsilon_abs))


LINEAR_SOLVER_TYPES = ("MULTIFRONTAL_CHOLESKY", "ITERATIVE")


def _check_linear_solver(params):
    """NonlinearOptimizer::solve (NonlinearOptimizer.cpp:154-173): ITERATIVE needs iterativeParams of a bound type.  Returns the
    lmgpu_pcg_params to select, or None for the direct solver.  Runs before any device handle exists."""
    t = getattr(params, "linearSolverType", "MULTIFRONTAL_CHOLESKY")
    if t not in LINEAR_SOLVER_TYPES:
        raise ValueError(f"linearSolverType {t!r} is not bound (one of {LINEAR_SOLVER_TYPES})")
    if t != "ITERATIVE":
        return None
    ip = getattr(params, "iterativeParams", None)
    if ip is None:
        raise RuntimeError("NonlinearOptimizer::solve: cg parameter has to be assigned ...")
    if not isinstance(ip, PCGSolverParameters):
        raise RuntimeError("NonlinearOptimizer::solve: special cg parameter type is not handled in LM solver ...")
    return ip._c()


class LevenbergMarquardtParams:
    def __init__(self):
        self.ordering = None
        self.linearSolverType = "MULTIFRONTAL_CHOLESKY"
        self.iterativeParams = None
        LevenbergMarquardtParams.SetLegacyDefaults(self)
        self.errorTol = 0.0
        self.minDiagonal = 1e-6
        self.maxDiagonal = 1e32

    @staticmethod
    def SetLegacyDefaults(p):  # LevenbergMarquardtParams.h:69-82
        p.maxIterations = 100
        p.relativeErrorTol = 1e-5
        p.absoluteErrorTol = 1e-5
        p.lambdaInitial = 1e-5
        p.lambdaFactor = 10.0
        p.lambdaUpperBound = 1e5
        p.lambdaLowerBound = 0.0
        p.minModelFidelity = 1e-3
        p.diagonalDamping = False
        p.useFixedLambdaFactor = True

    @staticmethod
    def SetCeresDefaults(p):  # LevenbergMarquardtParams.h:85-98
        p.maxIterations = 50
        p.absoluteErrorTol = 0.0
        p.relativeErrorTol = 1e-6
        p.lambdaUpperBound = 1e32
        p.lambdaLowerBound = 1e-16
        p.lambdaInitial = 1e-4
        p.lambdaFactor = 2.0
        p.minModelFidelity = 1e-3
        p.diagonalDamping = True
        p.useFixedLambdaFactor = False

    def isIterative(self):
        return self.linearSolverType == "ITERATIVE"

    @staticmethod
    def LegacyDefaults():
        return LevenbergMarquardtParams()

    @staticmethod
    def CeresDefaults():
        p = LevenbergMarquardtParams()
        LevenbergMarquardtParams.SetCeresDefaults(p)
        return p

    def _c(self):
        return _lib.lmgpu_lm_params(int(self.maxIterations), self.relativeErrorTol, self.absoluteErrorTol, self.errorTol, self.lambdaInitial,
                                    self.lambdaFactor, self.lambdaUpperBound, self.lambdaLowerBound, self.minModelFidelity,
                                    int(bool(self.diagonalDamping)), int(bool(self.useFixedLambdaFactor)), self.minDiagonal, self.maxDiagonal)


def _dp(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


def _ip(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_int32))


class LevenbergMarquardtOptimizer:
    """LevenbergMarquardtOptimizer(graph, initialValues, ordering, params).

    `ordering` (an Ordering = list of keys in elimination order) is a boundary input, as it is for the
    reference's hot loop (computed once at construction, LevenbergMarquardtParams.h:112-117).
    `device=-1` builds a structure-only handle (symbolic analysis and launch tables, no compute); `finalize_only=True` stops a device
    handle after lmgpu_finalize_structure as well: no communicator, no values, no LM state."""

    def __init__(self, graph: NonlinearFactorGraph, initialValues: Values, ordering=None, params: LevenbergMarquardtParams | None = None,
                 device: int = 0, rank: int = 0, world_size: int = 1, comm_id: bytes | None = None,
                 local_group=None, split_root: bool = False, finalize_only: bool = False):
        self.params = params or LevenbergMarquardtParams()
        pcg = _check_linear_solver(self.params)
        ordering = ordering if ordering is not None else self.params.ordering
        if ordering is None and pcg is not None:
            ordering = Ordering.Natural(graph)  # PCGSolver's KeyInfo(gfg) orders by key (IterativeSolver.cpp:111-114)
        if ordering is None:
            raise ValueError("an elimination Ordering is required (Ordering.Schur / Ordering.Natural, or COLAMD/METIS from the caller)")
        self.graph, self.ordering = graph, Ordering(ordering)
        self.lib = _lib.load(test_hooks=local_group is not None)  # the in-process communicator lives in liblmgpu_test.so only
        self._h = ct.c_void_p()
        cfg = _lib.lmgpu_config(device, rank, world_size, 1 if split_root else 0)
        self._check(self.lib.lmgpu_create(ct.byref(cfg), ct.byref(self._h)))
        self.device = device
        # variables in elimination order
        self._keys = np.array(self.ordering, dtype=np.uint64)
        if len(set(self.ordering)) != len(self.ordering):
            raise ValueError("ordering has duplicate keys")
        self._slot = {int(k): i for i, k in enumerate(self.ordering)}
        self._types = np.array([initialValues.type(k) for k in self.ordering], dtype=np.int32)
        self._check(self.lib.lmgpu_set_variables(self._h, len(self.ordering), self._keys.ctypes.data_as(ct.POINTER(ct.c_uint64)), _ip(self._types)))
        self._template = initialValues.copy()
        order_sorted = np.argsort(self._keys, kind="stable")
        keys_sorted = self._keys[order_sorted]
        for ftype, kind, gi, keys, meas, noise, models in graph.buckets():
            ar = FACTOR_ARITY[ftype]
            pos = np.searchsorted(keys_sorted, keys.reshape(-1))
            if (pos >= len(keys_sorted)).any() or (keys_sorted[np.minimum(pos, len(keys_sorted) - 1)] != keys.reshape(-1)).any():
                raise KeyError("a factor references a key that is not in the ordering")
            slots = order_sorted[pos].astype(np.int32).reshape(-1, ar)
            meas = meas.copy()
            if ftype == F_SFM:
                # fold Cal3Bundler's constant principal point into z (see include/lmgpu.h, CAM_BUNDLER)
                ucam, inv = np.unique(keys[:, 0], return_inverse=True)
                uv = np.array([initialValues.at(k)[15:17] for k in ucam])[inv]
                meas = meas - uv
            if ftype == F_PRIOR_CAM:
                meas = np.ascontiguousarray(meas[:, :15])
            meas = np.ascontiguousarray(meas, dtype=np.float64)
            gi32 = np.ascontiguousarray(gi, dtype=np.int32)
            slots = np.ascontiguousarray(slots)
            nptr = _dp(np.ascontiguousarray(noise)) if kind != N_UNIT else None
            self._check(self.lib.lmgpu_add_factor_bucket_robust(self._h, ftype, len(gi32), _ip(gi32), _ip(slots), _dp(meas), kind, nptr,
                                                                models[0].robust_kind, models[0].robust_k))
        self._smart = graph.smart_factors() if hasattr(graph, "smart_factors") else []
        self._add_smart_factors()
        if pcg is not None:  # before finalize: no symbolic analysis, no fronts
            self._check(self.lib.lmgpu_set_linear_solver(self._h, _lib.LMGPU_SOLVER_PCG, ct.byref(pcg)))
        self._check(self.lib.lmgpu_finalize_structure(self._h))
        self._ntot = self.lib.lmgpu_total_dim(self._h)
        self._nstore = self.lib.lmgpu_total_store(self._h)
        self._voff = np.concatenate([[0], np.cumsum([VAR_STORE_DEV[t] for t in self._types])]).astype(np.int64)
        self._xoff = np.concatenate([[0], np.cumsum([VAR_DIM[t] for t in self._types])]).astype(np.int64)
        self.state = _lib.lmgpu_lm_state()
        if device >= 0 and not finalize_only:
            if world_size > 1 or split_root:
                if local_group is not None:  # in-process communicator (tests): one thread per rank
                    self._check(self.lib.lmgpu_comm_init_local(self._h, local_group))
                elif comm_id is None:
                    raise ValueError("world_size > 1 needs comm_id (lmgpu_comm_unique_id bytes broadcast from rank 0)")
                else:
                    self.comm_init(comm_id)
            self.set_values(initialValues)
            cp = self.params._c()
            self._check(self.lib.lmgpu_lm_init(self._h, ct.byref(cp), ct.byref(self.state)))

    # ------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc == _lib.LMGPU_OK:
            return
        if rc == _lib.LMGPU_INDETERMINATE:
            raise _lib.IndeterminantLinearSystemException(self.lib.lmgpu_last_failed_slot(self._h))
        msg = self.lib.lmgpu_last_error(self._h)
        raise _lib.LmgpuError(f"lmgpu status {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.lmgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _pack(self, values: Values):
        out = np.empty(self._nstore)
        for i, k in enumerate(self.ordering):
            n = VAR_STORE_DEV[self._types[i]]
            out[self._voff[i]:self._voff[i] + n] = values.at(k)[:n]
        return out

    def set_values(self, values: Values):
        packed = self._pack(values)
        self._check(self.lib.lmgpu_set_values(self._h, _dp(packed)))

    # ------------------------------------------------------------ smart projection factors (smart.py; lmgpu_add_smart_factors ...)
    def _add_smart_factors(self):
        """one lmgpu_add_smart_factors call per SmartProjectionParams object, in graph order"""
        if not self._smart:
            return
        groups = {}
        for g, f in self._smart:
            groups.setdefault(id(f.params), (f.params, []))[1].append((g, f))
        for params, members in groups.values():
            cp = params._c()  # ValueError for a mode that is not bound
            gi = np.array([g for g, _ in members], dtype=np.int32)
            off = np.concatenate([[0], np.cumsum([f.size() for _, f in members])]).astype(np.int32)
            try:
                slots = np.array([self._slot[k] for _, f in members for k in f.keys()], dtype=np.int32)
            except KeyError:
                raise KeyError("a smart factor references a key that is not in the ordering") from None
            z = np.ascontiguousarray(np.array([zz for _, f in members for zz in f.measured()], dtype=np.float64).reshape(-1, 2))
            K5 = np.ascontiguousarray(np.array([f.K for _, f in members], dtype=np.float64))
            isig = np.array([f.inv_sigma for _, f in members], dtype=np.float64)
            self._check(self.lib.lmgpu_add_smart_factors(self._h, len(members), _ip(gi), _ip(off), _ip(slots), _dp(z), _dp(K5), _dp(isig),
                                                         ct.byref(cp)))

    def num_smart_factors(self) -> int:
        return self.lib.lmgpu_num_smart_factors(self._h)

    def smart_points(self):
        """(points (n, 3), NaN unless VALID; status (n,)) of the smart factors in graph order: SmartProjectionFactor::point() of each,
        as the last linearization / error evaluation on the device left it.  Also refreshes the factor objects' point() / isValid() ...
        (optimize() calls it at its end; iterate() does not: per factor object it is host work)"""
        n = max(0, self.num_smart_factors())
        pts, st = np.full((n, 3), np.nan), np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.lib.lmgpu_smart_get_points(self._h, _dp(pts), _ip(st)))
            order = [f for _, f in self._smart_in_add_order()]
            for f, p, s in zip(order, pts, st):
                f._set_result(int(s), p.copy())
            back = np.argsort(np.array([g for g, _ in self._smart_in_add_order()]), kind="stable")
            pts, st = pts[back], st[back]
        return pts, st

    def _smart_in_add_order(self):
        groups = {}
        for g, f in self._smart:
            groups.setdefault(id(f.params), []).append((g, f))
        return [m for members in groups.values() for m in members]

    def smart_hessian(self, graph_index):
        """the augmented information matrix ((6 m + 1) x (6 m + 1)) of the smart factor with this graph index from the device's F, E, b
        of the last linearization (lmgpu_smart_get_hessian)"""
        m = ct.c_int32()
        self._check(self.lib.lmgpu_smart_get_hessian(self._h, int(graph_index), ct.byref(m), None))
        N = 6 * m.value + 1
        out = np.empty(N * N)
        self._check(self.lib.lmgpu_smart_get_hessian(self._h, int(graph_index), ct.byref(m), _dp(out)))
        return out.reshape(N, N).T.copy()

    def smart_reset(self):
        """empty every smart factor's triangulation cache (= newly constructed factors)"""
        self._check(self.lib.lmgpu_smart_reset(self._h))

    def smart_stats(self):
        st = _lib.lmgpu_smart_stats()
        self._check(self.lib.lmgpu_get_smart_stats(self._h, ct.byref(st)))
        return dict(n_factors=st.n_factors, retriangulations=st.retriangulations, n_status=list(st.n_status), triangulate_ms=st.triangulate_ms,
                    linearize_ms=st.linearize_ms)

    # ------------------------------------------------------------ triangulation (lmgpu_triangulate_landmarks)
    def num_points3(self) -> int:
        return self.lib.lmgpu_num_points3(self._h)

    def triangulate_landmarks(self, params=None, write=True):
        """triangulateSafe (gtsam/geometry/triangulation.h:701-758) of every POINT3 variable from its GeneralSFMFactor / GenericProjectionFactor
        observations and the current cameras, on the device.  write=True stores the VALID points into the optimizer's values (the error
        of `state` is not refreshed, as after set_values).  Returns LandmarkTriangulation(keys, points, status, n_valid, stats): the
        POINT3 keys in elimination order, their points (NaN where not VALID) and TriangulationResult statuses."""
        from .triangulation import LandmarkTriangulation, TriangulationParameters, TriangulationStats
        cp = (params or TriangulationParameters())._c()
        n = self.num_points3()
        points, status, n_valid = np.full((n, 3), np.nan), np.zeros(n, dtype=np.int32), ct.c_int32(0)
        self._check(self.lib.lmgpu_triangulate_landmarks(self._h, ct.byref(cp), 1 if write else 0, _dp(points), _ip(status), ct.byref(n_valid)))
        st = _lib.lmgpu_triangulation_stats()
        self._check(self.lib.lmgpu_get_triangulation_stats(self._h, ct.byref(st)))
        keys = [int(k) for k, t in zip(self.ordering, self._types) if t == POINT3]
        return LandmarkTriangulation(keys, points, status, n_valid.value, TriangulationStats(st))

    # ------------------------------------------------------------ NonlinearOptimizer interface
    def values(self) -> Values:
        packed = np.empty(self._nstore)
        self._check(self.lib.lmgpu_get_values(self._h, _dp(packed)))
        out = self._template.copy()
        for i, k in enumerate(self.ordering):
            n = VAR_STORE_DEV[self._types[i]]
            v = out.at(k).copy()
            v[:n] = packed[self._voff[i]:self._voff[i] + n]
            out.update(k, v)
        return out

    def error(self) -> float:
        return self.state.error

    def iterations(self) -> int:
        return self.state.iterations

    def lambda_(self) -> float:
        return self.state.lambda_

    def getInnerIterations(self) -> int:
        return self.state.totalNumberInnerIterations

    def iterate(self):
        """one outer iteration; returns the linearized graph like the reference (NonlinearOptimizer.h:136,
        LevenbergMarquardtOptimizer.cpp:281,307): the whitened Jacobians of the linearization this iteration solved, fetched from
        the device when first read"""
        cp = self.params._c()
        self._check(self.lib.lmgpu_iterate(self._h, ct.byref(cp), ct.byref(self.state)))
        return self._returned_linear_graph()

    def _returned_linear_graph(self):
        self._lin_generation = getattr(self, "_lin_generation", 0) + 1
        return GaussianFactorGraph(self, self._lin_generation)

    def linear_graph(self):
        """the linearization currently on the device as a GaussianFactorGraph (one copy per factor bucket)"""
        return GaussianFactorGraph(self, getattr(self, "_lin_generation", 0))

    def optimize(self) -> Values:
        cp = self.params._c()
        self._check(self.lib.lmgpu_optimize(self._h, ct.byref(cp), ct.byref(self.state)))
        self._lin_generation = getattr(self, "_lin_generation", 0) + 1
        if self._smart:
            self.smart_points()
        return self.values()

    def set_linear_solver(self, params):
        """switch the linear solver of this handle: `params` = a LevenbergMarquardtParams-like object (linearSolverType, iterativeParams)"""
        pcg = _check_linear_solver(params)
        if pcg is None:
            self._check(self.lib.lmgpu_set_linear_solver(self._h, _lib.LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY, None))
        else:
            self._check(self.lib.lmgpu_set_linear_solver(self._h, _lib.LMGPU_SOLVER_PCG, ct.byref(pcg)))

    def pcg_stats(self):
        """statistics of the last PCG solve (lmgpu_get_pcg_stats)"""
        st = _lib.lmgpu_pcg_stats()
        self._check(self.lib.lmgpu_get_pcg_stats(self._h, ct.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def timings(self):
        t = _lib.lmgpu_timings()
        self._check(self.lib.lmgpu_get_timings(self._h, ct.byref(t)))
        return {f: getattr(t, f) for f, _ in t._fields_}

    def save_values(self):
        self._check(self.lib.lmgpu_save_values(self._h))

    def restore_values(self, state=None):
        """restore the device-side snapshot; optionally also the LM state (a copy of a previous `opt.state`)"""
        self._check(self.lib.lmgpu_restore_values(self._h))
        if state is not None:
            ct.memmove(ct.byref(self.state), ct.byref(state), ct.sizeof(_lib.lmgpu_lm_state))

    def copy_state(self):
        s = _lib.lmgpu_lm_state()
        ct.memmove(ct.byref(s), ct.byref(self.state), ct.sizeof(_lib.lmgpu_lm_state))
        return s

    def set_kernel_timing(self, on=True):
        """True / 1: every category; 2: only the two roofline kernels (linearize, chain); False: off"""
        self._check(self.lib.lmgpu_set_kernel_timing(self._h, int(on)))

    def kernel_times(self):
        """{category: dict(ms, work, launches)} accumulated since set_kernel_timing(True)"""
        n = len(_lib.KT_NAMES)
        ms, work, cnt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
        self._check(self.lib.lmgpu_get_kernel_times(self._h, _dp(ms), _dp(work), cnt.ctypes.data_as(ct.POINTER(ct.c_int64))))
        return {name: dict(ms=float(ms[i]), work=float(work[i]), launches=int(cnt[i])) for i, name in enumerate(_lib.KT_NAMES)}

    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclUniqueId bytes (rank 0 creates it; the caller broadcasts it to the other ranks)"""
        buf = ct.create_string_buffer(128)
        rc = _lib.load().lmgpu_comm_unique_id(buf)
        if rc != 0:
            raise _lib.LmgpuError("lmgpu_comm_unique_id failed")
        return buf.raw

    def comm_init(self, id128: bytes):
        self._check(self.lib.lmgpu_comm_init(self._h, id128))

    # ------------------------------------------------------------ piecewise hot path (tryLambda's calls)
    def graph_error(self) -> float:
        e = ct.c_double()
        self._check(self.lib.lmgpu_error(self._h, ct.byref(e)))
        return e.value

    def linearize(self):
        """LevenbergMarquardtOptimizer::linearize() (LevenbergMarquardtOptimizer.h:113): returns the linear graph (fetched on first read)"""
        self._check(self.lib.lmgpu_linearize(self._h))
        return self._returned_linear_graph()

    def solve(self, lam, diagonal_damping=False, min_diag=1e-6, max_diag=1e32):
        """returns (delta by key dict, packed delta in slot order, linear error at 0, linear error at delta)"""
        d = np.empty(self._ntot)
        e0, e1 = ct.c_double(), ct.c_double()
        self._check(self.lib.lmgpu_solve(self._h, lam, int(diagonal_damping), min_diag, max_diag, _dp(d), ct.byref(e0), ct.byref(e1)))
        return self.delta_by_key(d), d, e0.value, e1.value

    def delta_by_key(self, packed):
        return {int(k): packed[self._xoff[i]:self._xoff[i + 1]].copy() for i, k in enumerate(self.ordering)}

    def retract(self, packed_delta=None):
        p = None if packed_delta is None else _dp(np.ascontiguousarray(packed_delta, dtype=np.float64))
        self._check(self.lib.lmgpu_retract(self._h, p))

    def hessian_diagonal(self):
        d = np.empty(self._ntot)
        self._check(self.lib.lmgpu_hessian_diagonal(self._h, _dp(d)))
        return self.delta_by_key(d)

    # ------------------------------------------------------------ parity taps
    def bt_products(self, x=None, alpha=0.0):
        """the Dogleg's two products with the Bayes tree of the last solve (lmgpu_bt_products; nothing on the device changes):
        (sum over the cliques of ||[R S] x - alpha d||^2, or None without x;  the gradient - sum [R S]^T d), both packed by slot"""
        g, sq = np.empty(self._ntot), ct.c_double()
        xp = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        assert xp is None or xp.shape == (self._ntot,)
        self._check(self.lib.lmgpu_bt_products(self._h, None if xp is None else _dp(xp), float(alpha), ct.byref(sq), _dp(g)))
        return (None if xp is None else sq.value), g

    def jacobian(self, graph_index):
        r, c = ct.c_int32(), ct.c_int32()
        self._check(self.lib.lmgpu_get_jacobian(self._h, graph_index, None, ct.byref(r), ct.byref(c)))
        out = np.empty(r.value * c.value)
        self._check(self.lib.lmgpu_get_jacobian(self._h, graph_index, _dp(out), ct.byref(r), ct.byref(c)))
        return out.reshape(c.value, r.value).T.copy()  # column-major -> (rows, cols)

    def num_fronts(self):
        return self.lib.lmgpu_num_fronts(self._h)

    def leaf_group_launches(self):
        """structure only: how many gather-leaf bin launches of the plan take the lane-group kernel (four leaves per wave)"""
        return self.lib.lmgpu_leaf_group_launches(self._h)

    def backsub_group_launches(self):
        """structure only: (levels whose plain back-substitution launch takes the lane-group kernel, how many of them its <4, 9> form)"""
        wide = np.zeros(1, dtype=np.int32)
        return self.lib.lmgpu_backsub_group_launches(self._h, _ip(wide)), int(wide[0])

    def leaf_corner(self, i):
        """after a solve: the (rhs, rhs) corner scalar of gather leaf i (what its parent's Schur gather sums)"""
        out = np.zeros(1)
        self._check(self.lib.lmgpu_get_leaf_corner(self._h, i, _dp(out)))
        return float(out[0])

    def front_info(self, i):
        info = np.zeros(8, dtype=np.int32)
        self._check(self.lib.lmgpu_front_info(self._h, i, _ip(info)))
        return dict(n_keys=int(info[0]), n_frontal_keys=int(info[1]), nf=int(info[2]), n=int(info[3]), parent=int(info[4]), cls=int(info[5]),
                    owner=int(info[6]), level=int(info[7]))

    def front(self, i, numeric=True):
        """(keys in Scatter order, [R S d] as (nf, n) array or None)"""
        fi = self.front_info(i)
        slots = np.zeros(fi["n_keys"], dtype=np.int32)
        rsd = np.empty(fi["nf"] * fi["n"]) if numeric else None
        self._check(self.lib.lmgpu_get_front(self._h, i, _ip(slots), _dp(rsd) if numeric else None))
        keys = [int(self._keys[s]) for s in slots]
        return keys, (rsd.reshape(fi["n"], fi["nf"]).T.copy() if numeric else None)


class JacobianFactor:
    """the part of gtsam/linear/JacobianFactor.h the returned linear graph is read through: keys(), getA(i) / jacobian(), getb(),
    error(x) = 0.5 ||A x - b||^2 (JacobianFactor.cpp:509-514); unit noise model (already whitened)"""

    def __init__(self, keys, dims, Ab):
        self._keys, self._dims, self._Ab = list(keys), list(dims), Ab
        self._off = np.concatenate([[0], np.cumsum(dims)]).astype(int)

    def keys(self):
        return list(self._keys)

    def getA(self, i):
        return self._Ab[:, self._off[i]:self._off[i + 1]].copy()

    def getb(self):
        return self._Ab[:, -1].copy()

    def jacobian(self):
        return self._Ab[:, :-1].copy(), self.getb()

    def augmentedJacobian(self):
        return self._Ab.copy()

    def error(self, x):
        r = -self._Ab[:, -1]
        for i, k in enumerate(self._keys):
            r = r + self._Ab[:, self._off[i]:self._off[i + 1]] @ np.asarray(x[k], dtype=float)
        return 0.5 * float(r @ r)


class GaussianFactorGraph:
    """What iterate() / linearize() return: the linearization on the device as a list of JacobianFactors, index-preserving like
    NonlinearFactorGraph::linearize (NonlinearFactorGraph.cpp:239-278; a slot without a factor is None).  The numbers are fetched at the
    first read (lmgpu_get_jacobians: one copy per factor bucket); a graph that is first read after the optimizer has linearized again
    refuses — its linearization is no longer on the device."""

    def __init__(self, opt, generation):
        self._opt, self._generation, self._factors = opt, generation, None

    def _fetch(self):
        if self._factors is not None:
            return
        o = self._opt
        if getattr(o, "_lin_generation", 0) != self._generation:
            raise _lib.LmgpuError("this linear graph was not read before the optimizer linearized again")
        n = ct.c_int32()
        o._check(o.lib.lmgpu_get_jacobians(o._h, ct.byref(n), None, None, None, None, None))
        gi, rows, cols = (np.zeros(n.value, dtype=np.int32) for _ in range(3))
        off = np.zeros(n.value + 1, dtype=np.int64)
        o._check(o.lib.lmgpu_get_jacobians(o._h, ct.byref(n), _ip(gi), _ip(rows), _ip(cols), off.ctypes.data_as(ct.POINTER(ct.c_int64)), None))
        out = np.empty(int(off[-1]))
        o._check(o.lib.lmgpu_get_jacobians(o._h, ct.byref(n), None, None, None, None, _dp(out)))
        fac = [None] * o.graph.size()
        fkeys = o.graph.factor_keys_in_graph_order()
        for i in range(n.value):
            Ab = out[off[i]:off[i + 1]].reshape(cols[i], rows[i]).T  # column-major -> (rows, cols)
            keys = fkeys[int(gi[i])]
            dims = [VAR_DIM[o._types[o._slot[int(k)]]] for k in keys]
            fac[int(gi[i])] = JacobianFactor(keys, dims, Ab)
        self._factors = fac

    def size(self):
        self._fetch()
        return len(self._factors)

    __len__ = size

    def at(self, i):
        self._fetch()
        return self._factors[i]

    __getitem__ = at

    def error(self, x):
        """GaussianFactorGraph::error (GaussianFactorGraph.cpp:71-78); x: {key: vector}"""
        self._fetch()
        return sum(f.error(x) for f in self._factors if f is not None)

    def gradientAtZero(self):
        """GaussianFactorGraph::gradientAtZero (GaussianFactorGraph.cpp:357-367): {key: -sum A_k^T b}"""
        self._fetch()
        g = {}
        for f in self._factors:
            if f is None:
                continue
            b = f.getb()
            for i, k in enumerate(f.keys()):
                g[k] = g.get(k, 0.0) - f.getA(i).T @ b
        return g


class GaussNewtonParams(LevenbergMarquardtParams):
    """NonlinearOptimizerParams defaults (gtsam/nonlinear/NonlinearOptimizerParams.h: maxIterations 100, relativeErrorTol 1e-5,
    absoluteErrorTol 1e-5, errorTol 0); the LM-only fields of the shared C struct are ignored by the Gauss-Newton entry points."""

    def __init__(self):
        super().__init__()


class GaussNewtonOptimizer(LevenbergMarquardtOptimizer):
    """gtsam/nonlinear/GaussNewtonOptimizer.h:38-91 on the same device-resident graph and kernels: iterate() = linearize,
    solve the undamped system, retract, new error (GaussNewtonOptimizer.cpp:44-66); optimize() = defaultOptimize."""

    def __init__(self, graph, initialValues, ordering=None, params=None, **kw):
        super().__init__(graph, initialValues, ordering, params or GaussNewtonParams(), **kw)

    def iterate(self):
        self._check(self.lib.lmgpu_gn_iterate(self._h, ct.byref(self.state)))
        return self._returned_linear_graph()  # GaussNewtonOptimizer.cpp:49,65

    def optimize(self) -> Values:
        cp = self.params._c()
        self._check(self.lib.lmgpu_gn_optimize(self._h, ct.byref(cp), ct.byref(self.state)))
        self._lin_generation = getattr(self, "_lin_generation", 0) + 1
        if self._smart:
            self.smart_points()
        return self.values()


class DoglegParams(LevenbergMarquardtParams):
    """gtsam/nonlinear/DoglegOptimizer.h:33-63: NonlinearOptimizerParams + deltaInitial (default 1.0)"""

    def __init__(self):
        super().__init__()
        self.deltaInitial = 1.0


class DoglegOptimizer(LevenbergMarquardtOptimizer):
    """gtsam/nonlinear/DoglegOptimizer.h:69-133 (multifrontal elimination) on the device-resident Bayes tree."""

    def __init__(self, graph, initialValues, ordering=None, params=None, **kw):
        params = params or DoglegParams()
        if getattr(params, "linearSolverType", "MULTIFRONTAL_CHOLESKY") == "ITERATIVE":  # DoglegOptimizer.cpp:108-113
            raise RuntimeError("Dogleg is not currently compatible with the linear conjugate gradient solver")
        super().__init__(graph, initialValues, ordering, params, **kw)
        self.state.lambda_ = float(getattr(params, "deltaInitial", 1.0))

    def getDelta(self) -> float:
        return self.state.lambda_

    def iterate(self):
        self._check(self.lib.lmgpu_dl_iterate(self._h, ct.byref(self.state)))
        return self._returned_linear_graph()  # DoglegOptimizer.cpp:87,122

    def optimize(self) -> Values:
        cp = self.params._c()
        self._check(self.lib.lmgpu_dl_optimize(self._h, ct.byref(cp), ct.byref(self.state)))
        self._lin_generation = getattr(self, "_lin_generation", 0) + 1
        return self.values()


class DirectionMethod:
    """gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h:72-77"""
    FletcherReeves = _lib.LMGPU_NCG_FLETCHER_REEVES
    PolakRibiere = _lib.LMGPU_NCG_POLAK_RIBIERE
    HestenesStiefel = _lib.LMGPU_NCG_HESTENES_STIEFEL
    DaiYuan = _lib.LMGPU_NCG_DAI_YUAN


class NonlinearConjugateGradientOptimizer(LevenbergMarquardtOptimizer):
    """NonlinearConjugateGradientOptimizer(graph, initialValues, params, directionMethod)
    (gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h:80-132, .cpp:44-90): gradient, direction update, the golden-section line
    search and the advance all run in liblmgpu.so (lmgpu_ncg_*), one host wait per iteration.  `params`: NonlinearOptimizerParams
    (GaussNewtonParams here; maxIterations, the three tolerances, ordering, linearSolverType).  The optimizer eliminates nothing, so
    the ordering only fixes the slot order (default: by key); with linearSolverType = "ITERATIVE" the handle is built without fronts,
    which is the form for graphs whose fronts do not fit.  gradientDescent: the template's last switch (.h:200), which the reference's
    class leaves at false."""

    def __init__(self, graph, initialValues, params=None, directionMethod=DirectionMethod.PolakRibiere, ordering=None,
                 gradientDescent=False, **kw):
        params = params or GaussNewtonParams()
        if directionMethod not in (DirectionMethod.FletcherReeves, DirectionMethod.PolakRibiere, DirectionMethod.HestenesStiefel,
                                   DirectionMethod.DaiYuan):
            raise RuntimeError("NonlinearConjugateGradientOptimizer: Invalid directionMethod")
        if ordering is None and getattr(params, "ordering", None) is None:
            ordering = Ordering.Natural(graph)
        self.directionMethod, self.gradientDescent = int(directionMethod), bool(gradientDescent)
        super().__init__(graph, initialValues, ordering, params, **kw)

    def _ncg_c(self):
        p = self.params
        return _lib.lmgpu_ncg_params(self.directionMethod, int(self.gradientDescent), int(p.maxIterations), float(p.relativeErrorTol),
                                     float(p.absoluteErrorTol), float(p.errorTol))

    def iterate(self):
        """.cpp:71-80: a gradient-descent step and one conjugate step from the current values; returns None like the reference
        (it returns nullptr: the system is not linearized for the caller)"""
        cp = self._ncg_c()
        self._check(self.lib.lmgpu_ncg_iterate(self._h, ct.byref(cp), ct.byref(self.state)))
        self._lin_generation = getattr(self, "_lin_generation", 0) + 1
        return None

    def optimize(self) -> Values:
        cp = self._ncg_c()
        self._check(self.lib.lmgpu_ncg_optimize(self._h, ct.byref(cp), ct.byref(self.state)))
        self._lin_generation = getattr(self, "_lin_generation", 0) + 1
        return self.values()

    def gradient(self):
        """System::gradient at the current values (.cpp:56-60): packed by slot; delta_by_key() splits it"""
        g = np.empty(self._ntot)
        self._check(self.lib.lmgpu_gradient(self._h, _dp(g)))
        return g

    def line_search(self, direction=None):
        """lineSearch (.h:135-181) from the current values along `direction` (packed by slot; None: the gradient); the values stay.
        Returns (alpha, trials)."""
        a, n = ct.c_double(), ct.c_int32()
        d = None if direction is None else _dp(np.ascontiguousarray(direction, dtype=np.float64))
        self._check(self.lib.lmgpu_ncg_line_search(self._h, d, ct.byref(a), ct.byref(n)))
        return a.value, n.value

    def trace(self):
        """per line search of the last iterate() / optimize() / line_search(): (alpha, beta, error, trials); row 0 of an iterate /
        optimize is the uncounted gradient-descent step"""
        n = self.lib.lmgpu_ncg_get_trace(self._h, 0, None)
        out = np.zeros((max(n, 1), 4))
        self.lib.lmgpu_ncg_get_trace(self._h, n, _dp(out))
        return out[:n]

    def host_waits(self):
        return int(self.lib.lmgpu_ncg_host_waits(self._h))


class Marginals:
    """Marginals(graph, solution, ordering): marginal covariances of single variables at `solution`
    (gtsam/nonlinear/Marginals.h; constructor Marginals.cpp:28-43: linearize the graph at the solution and eliminate it;
    marginalCovariance :124-127, marginalInformation :109-121).  Cholesky factorization only (the reference's default).
    The elimination ordering is a boundary input as for the optimizers (the reference's default here is COLAMD; the result
    does not depend on it).  Raises IndeterminantLinearSystemException-like LmgpuError where the reference throws."""

    def __init__(self, graph: NonlinearFactorGraph, solution: Values, ordering, device: int = 0, path_solves: bool = False):
        """path_solves: marginalCovariance / marginalInformation answer from ONE cached factorization, each variable along its path to the
        root of the Bayes tree (lmgpu_marginal_covariances), instead of one elimination + back-substitution per column, and
        jointMarginalCovariance / jointMarginalInformation from the same factorization (lmgpu_joint_marginal_covariances).
        marginalCovariances / marginalInformations, crossCovariances and jointMarginalCovariances always take that route."""
        self._opt = LevenbergMarquardtOptimizer(graph, solution, ordering, LevenbergMarquardtParams(), device=device)
        self._path_solves = bool(path_solves)

    def marginalCovariance(self, key) -> np.ndarray:
        if self._path_solves:
            return self.marginalCovariances([key])[int(key)]
        o = self._opt
        slot = o._slot[int(key)]
        d = int(o._xoff[slot + 1] - o._xoff[slot])
        out = np.zeros((d, d))
        o._check(o.lib.lmgpu_marginal_covariance(o._h, slot, _dp(out)))
        return out

    def marginalInformation(self, key) -> np.ndarray:
        return np.linalg.inv(self.marginalCovariance(key))

    def marginalCovariances(self, keys=None) -> dict:
        """{key: marginalCovariance(key)} for `keys` (all variables when None): one factorization, kept until the values move, and one
        walk per variable along its path to the root."""
        o = self._opt
        keys = sorted(o._slot) if keys is None else [int(k) for k in keys]
        slots = np.array([o._slot[k] for k in keys], dtype=np.int32)
        dims = [int(o._xoff[s + 1] - o._xoff[s]) for s in slots]
        off = np.concatenate([[0], np.cumsum([d * d for d in dims])]).astype(np.int64)
        out = np.zeros(max(int(off[-1]), 1))
        o._check(o.lib.lmgpu_marginal_covariances(o._h, len(slots), _ip(slots), _dp(out)))
        return {k: out[off[i]:off[i + 1]].reshape(dims[i], dims[i]).copy() for i, k in enumerate(keys)}

    def marginalInformations(self, keys=None) -> dict:
        return {k: np.linalg.inv(c) for k, c in self.marginalCovariances(keys).items()}

    def marginalsStats(self) -> dict:
        st = _lib.lmgpu_marginals_stats()
        self._opt._check(self._opt.lib.lmgpu_get_marginals_stats(self._opt._h, st))
        return {name: int(getattr(st, name)) for name, _ in st._fields_}

    def crossCovariances(self, pairs) -> dict:
        """{(ki, kj): Sigma[ki, kj]} (dim_i x dim_j) for the (ki, kj) of `pairs`: kj is the source whose path is walked, pairs with one
        kj share the walk, each ki costs the descent of its branch below the junction of the two paths."""
        o = self._opt
        pairs = [(int(a), int(b)) for a, b in pairs]
        si = np.array([o._slot[a] for a, _ in pairs], dtype=np.int32)
        sj = np.array([o._slot[b] for _, b in pairs], dtype=np.int32)
        dim = lambda s: int(o._xoff[s + 1] - o._xoff[s])
        shape = [(dim(a), dim(b)) for a, b in zip(si, sj)]
        off = np.concatenate([[0], np.cumsum([r * c for r, c in shape])]).astype(np.int64)
        out = np.zeros(max(int(off[-1]), 1))
        o._check(o.lib.lmgpu_marginal_cross_covariances(o._h, len(pairs), _ip(si), _ip(sj), _dp(out)))
        return {pr: out[off[q]:off[q + 1]].reshape(shape[q]).copy() for q, pr in enumerate(pairs)}

    def jointMarginalCovariances(self, list_of_key_lists) -> list:
        """[jointMarginalCovariance(keys) for keys in list_of_key_lists] in one request: every block from the one factorization, blocks
        ordered by Key like JointMarginal::fullMatrix, each matrix exactly symmetric."""
        o = self._opt
        sets = [sorted(int(k) for k in keys) for keys in list_of_key_lists]
        begin = np.concatenate([[0], np.cumsum([len(ks) for ks in sets])]).astype(np.int32)
        slots = np.array([o._slot[k] for ks in sets for k in ks], dtype=np.int32)
        dims = [[int(o._xoff[o._slot[k] + 1] - o._xoff[o._slot[k]]) for k in ks] for ks in sets]
        off = np.concatenate([[0], np.cumsum([sum(d) ** 2 for d in dims])]).astype(np.int64)
        out = np.zeros(max(int(off[-1]), 1))
        o._check(o.lib.lmgpu_joint_marginal_covariances(o._h, len(sets), _ip(begin), _ip(slots), _dp(out)))
        return [JointMarginal(ks, dims[q], out[off[q]:off[q + 1]].reshape(sum(dims[q]), sum(dims[q])).copy()) for q, ks in enumerate(sets)]

    def jointMarginalCovariance(self, keys) -> "JointMarginal":
        """Marginals::jointMarginalCovariance (Marginals.cpp:130-137): blocks ordered by Key like JointMarginal::fullMatrix"""
        if self._path_solves:
            return self.jointMarginalCovariances([keys])[0]
        o = self._opt
        keys = sorted(int(k) for k in keys)
        slots = np.array([o._slot[k] for k in keys], dtype=np.int32)
        dims = [int(o._xoff[s + 1] - o._xoff[s]) for s in slots]
        out = np.zeros((sum(dims), sum(dims)))
        o._check(o.lib.lmgpu_joint_marginal_covariance(o._h, len(slots), _ip(slots), _dp(out)))
        return JointMarginal(keys, dims, out)

    def jointMarginalInformation(self, keys) -> "JointMarginal":
        j = self.jointMarginalCovariance(keys)
        return JointMarginal(j.keys, j.dims, np.linalg.inv(j.fullMatrix()))

    def close(self):
        self._opt.close()


class JointMarginal:
    """JointMarginal (gtsam/nonlinear/Marginals.h:141-191): at(iVariable, jVariable) = block (i, j); fullMatrix() with the
    blocks ordered by Key"""

    def __init__(self, keys, dims, full):
        self.keys, self.dims, self._full = list(keys), list(dims), full
        off = np.concatenate([[0], np.cumsum(dims)])
        self._range = {k: (int(off[i]), int(off[i + 1])) for i, k in enumerate(keys)}

    def at(self, iVariable, jVariable) -> np.ndarray:
        (a0, a1), (b0, b1) = self._range[int(iVariable)], self._range[int(jVariable)]
        return self._full[a0:a1, b0:b1].copy()

    __call__ = at

    def fullMatrix(self) -> np.ndarray:
        return self._full.copy()


# ---------------------------------------------------------------- GNC (gtsam/nonlinear/GncParams.h, GncOptimizer.h)
class GncLossType:
    """GncParams.h:36-39"""
    GM = _lib.LMGPU_GNC_GM    # Geman McClure
    TLS = _lib.LMGPU_GNC_TLS  # Truncated least squares


class _GncParams:
    """GncParams<BaseOptimizerParameters> (GncParams.h:42-160): defaults lossType TLS, maxIterations 100, muStep 1.4, relativeCostTol 1e-5,
    weightsTol 1e-4 (:69-73), no known inliers / outliers; setters as there (:84-138)."""
    _base_params = LevenbergMarquardtParams
    _base_kind = _lib.LMGPU_GNC_BASE_LM

    def __init__(self, baseOptimizerParams=None):
        self.baseOptimizerParams = baseOptimizerParams if baseOptimizerParams is not None else self._base_params()
        self.lossType = GncLossType.TLS
        self.maxIterations = 100
        self.muStep = 1.4
        self.relativeCostTol = 1e-5
        self.weightsTol = 1e-4
        self.knownInliers = []
        self.knownOutliers = []

    def setLossType(self, type_):
        self.lossType = type_

    def setMaxIterations(self, maxIter):
        self.maxIterations = int(maxIter)

    def setMuStep(self, step):
        self.muStep = float(step)

    def setRelativeCostTol(self, value):
        self.relativeCostTol = float(value)

    def setWeightsTol(self, value):
        self.weightsTol = float(value)

    def setKnownInliers(self, knownIn):
        """GncParams.h:122-127: appended to the list, which is kept sorted"""
        self.knownInliers = sorted(list(self.knownInliers) + [int(i) for i in knownIn])

    def setKnownOutliers(self, knownOut):
        """GncParams.h:133-138: appended to the list, which is kept sorted"""
        self.knownOutliers = sorted(list(self.knownOutliers) + [int(i) for i in knownOut])

    def _c(self):
        return _lib.lmgpu_gnc_params(int(self.lossType), int(self.maxIterations), self._base_kind, float(self.muStep),
                                     float(self.relativeCostTol), float(self.weightsTol))


class GncLMParams(_GncParams):
    """GncParams<LevenbergMarquardtParams>"""


class GncGaussNewtonParams(_GncParams):
    """GncParams<GaussNewtonParams>"""
    _base_params = GaussNewtonParams
    _base_kind = _lib.LMGPU_GNC_BASE_GN


class GncOptimizer:
    """GncOptimizer<GncParams<...>>(graph, initialValues, params) (gtsam/nonlinear/GncOptimizer.h:44-470) on ONE device handle, created
    once: the outer loop runs in liblmgpu.so (lmgpu_gnc_optimize), the weights / thresholds / known mask stay on the device and only
    cross the bus in getWeights / setWeights / getInlierCostThresholds / setInlierCostThresholds.  `ordering` as for the base optimizers
    (default: baseOptimizerParams.ordering).  The constructor's checks (:75-99) raise before any device work.  Single GPU.
    Unlike the reference's, this object works on the handle's state: initializeMu() and calculateWeights(values, mu) set the handle's
    current values (to the initial values / to `values`), so the values of an earlier optimize() are gone from the device afterwards
    (the Values object optimize() returned is the caller's); optimize() uses the handle's one value snapshot (save_values of the base
    optimizer object) for the initial values; every change of the weights invalidates linear graphs handed out before."""

    def __init__(self, graph: NonlinearFactorGraph, initialValues: Values, params=None, ordering=None, device: int = 0):
        self.params = params if params is not None else GncLMParams()
        if not isinstance(self.params, _GncParams):
            raise ValueError("GncOptimizer: params must be GncLMParams or GncGaussNewtonParams")
        if self.params.lossType not in (GncLossType.GM, GncLossType.TLS):
            raise RuntimeError("GncOptimizer: unknown loss type")
        n = graph.size()
        kin, kout = list(self.params.knownInliers), list(self.params.knownOutliers)
        if set(kin) & set(kout):
            raise RuntimeError("GncOptimizer::constructor: the user has selected one or more measurements to be BOTH a known inlier and a "
                               "known outlier.")
        if any(i < 0 or i > n - 1 for i in kin):
            raise RuntimeError("GncOptimizer::constructor: the user has selected one or more measurements that are not in the factor graph "
                               "to be known inliers.")
        if any(i < 0 or i > n - 1 for i in kout):
            raise RuntimeError("GncOptimizer::constructor: the user has selected one or more measurements that are not in the factor graph "
                               "to be known outliers.")
        base_cls = GaussNewtonOptimizer if self.params._base_kind == _lib.LMGPU_GNC_BASE_GN else LevenbergMarquardtOptimizer
        self._n = n
        self._state = initialValues.copy()
        self._opt = base_cls(graph, initialValues, ordering, self.params.baseOptimizerParams, device=device)
        o = self._opt
        o._check(o.lib.lmgpu_gnc_enable(o._h, 1, n))
        self._set_known(kin, kout)
        self.result = _lib.lmgpu_gnc_result()

    # ------------------------------------------------------------ plumbing
    def _set_known(self, kin, kout):
        o = self._opt
        a, b = np.asarray(kin, dtype=np.uint64), np.asarray(kout, dtype=np.uint64)
        up = ct.POINTER(ct.c_uint64)
        o._check(o.lib.lmgpu_gnc_set_known(o._h, len(a), a.ctypes.data_as(up), len(b), b.ctypes.data_as(up)))
        self._weights_changed()

    def _weights_changed(self):
        """the [A b] on the device carry other weights now: linear graphs handed out earlier refuse to be read"""
        o = self._opt
        o._lin_generation = getattr(o, "_lin_generation", 0) + 1

    def close(self):
        self._opt.close()

    def base(self):
        """the base optimizer object whose handle carries the weighted graph (error(), iterate(), solve(), jacobian(), ... act on it)"""
        return self._opt

    # ------------------------------------------------------------ reference interface
    @staticmethod
    def Chi2inv(alpha, dofs):
        """GncOptimizer.h:38-40"""
        return float(_lib.load().lmgpu_chi2inv(float(alpha), int(dofs)))

    def getFactors(self):
        return self._opt.graph

    def getState(self):
        return self._state

    def getParams(self):
        return self.params

    def setInlierCostThresholds(self, inth):
        """:115-125: one threshold for all factors, or one per factor"""
        v = np.full(self._n, float(inth)) if np.isscalar(inth) else np.ascontiguousarray(inth, dtype=np.float64).reshape(-1)
        if v.size != self._n:
            raise RuntimeError("GncOptimizer::setInlierCostThresholds: the number of thresholds does not match the size of the factor graph.")
        o = self._opt
        o._check(o.lib.lmgpu_gnc_set_inlier_cost_thresholds(o._h, self._n, _dp(v), 0.0))

    def setInlierCostThresholdsAtProbability(self, alpha):
        """:130-137"""
        o = self._opt
        o._check(o.lib.lmgpu_gnc_set_inlier_cost_thresholds(o._h, self._n, None, float(alpha)))

    def getInlierCostThresholds(self):
        out = np.empty(max(1, self._n))
        o = self._opt
        o._check(o.lib.lmgpu_gnc_get_inlier_cost_thresholds(o._h, self._n, _dp(out)))
        return out[:self._n]

    def setWeights(self, w):
        """:142-149"""
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if w.size != self._n:
            raise RuntimeError("GncOptimizer::setWeights: the number of specified weights does not match the size of the factor graph.")
        o = self._opt
        o._check(o.lib.lmgpu_gnc_set_weights(o._h, self._n, _dp(w)))
        self._weights_changed()

    def getWeights(self):
        out = np.empty(max(1, self._n))
        o = self._opt
        o._check(o.lib.lmgpu_gnc_get_weights(o._h, self._n, _dp(out)))
        return out[:self._n]

    def initializeMu(self):
        """:272-314, at the initial values (state_), which become the handle's current values"""
        o = self._opt
        o.set_values(self._state)
        mu = ct.c_double()
        o._check(o.lib.lmgpu_gnc_initialize_mu(o._h, int(self.params.lossType), ct.byref(mu)))
        return mu.value

    def updateMu(self, mu):
        """:317-329"""
        if self.params.lossType == GncLossType.GM:
            return max(1.0, mu / self.params.muStep)
        return mu * self.params.muStep

    def checkMuConvergence(self, mu):
        """:332-348"""
        return self.params.lossType == GncLossType.GM and abs(mu - 1.0) < 1e-9

    def checkCostConvergence(self, cost, prev_cost):
        """:351-359"""
        return abs(cost - prev_cost) / max(prev_cost, 1e-7) < self.params.relativeCostTol

    def checkWeightsConvergence(self, weights):
        """:362-386"""
        if self.params.lossType != GncLossType.TLS:
            return False
        w = np.asarray(weights, dtype=np.float64)
        rounded = np.sign(w) * np.floor(np.abs(w) + 0.5)  # std::round: half away from zero
        return not bool((np.abs(w - rounded) > self.params.weightsTol).any())

    def checkConvergence(self, mu, weights, cost, prev_cost):
        """:389-393"""
        return self.checkCostConvergence(cost, prev_cost) or self.checkWeightsConvergence(weights) or self.checkMuConvergence(mu)

    def calculateWeights(self, currentEstimate: Values, mu):
        """:419-469: the weights at `currentEstimate`.  Side effects: they become the handle's current weights (as weights_ does in
        optimize()) and `currentEstimate` the handle's current values"""
        o = self._opt
        o.set_values(currentEstimate)
        o._check(o.lib.lmgpu_gnc_calculate_weights(o._h, int(self.params.lossType), float(mu)))
        self._weights_changed()
        return self.getWeights()

    def optimize(self) -> Values:
        """:183-269; the summary of the run is in .result (iterations, stop, mu, cost, prev_cost, base_iterations_total)"""
        o = self._opt
        o.set_values(self._state)
        gp, bp = self.params._c(), self.params.baseOptimizerParams._c()
        o._check(o.lib.lmgpu_gnc_optimize(o._h, ct.byref(gp), ct.byref(bp), ct.byref(o.state), ct.byref(self.result)))
        o._lin_generation = getattr(o, "_lin_generation", 0) + 1
        return o.values()

    def trace(self):
        """per outer iteration of the last optimize(): (mu, cost, max |w - round(w)|, weight-update device ms, base optimizer host ms,
        base optimizer iterations)"""
        o = self._opt
        n = o.lib.lmgpu_gnc_get_trace(o._h, 0, None)
        out = np.zeros((max(n, 1), 6))
        o.lib.lmgpu_gnc_get_trace(o._h, n, _dp(out))
        return out[:n]
