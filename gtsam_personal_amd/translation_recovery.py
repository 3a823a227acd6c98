"""TranslationRecovery and MFAS mirrors over the C ABI (include/lmgpu.h, the lmgpu_translation_recovery_* group and
lmgpu_mfas_outlier_weights).

  BinaryMeasurement       gtsam/sfm/BinaryMeasurement.h       (key1, key2, measured, noiseModel)
  TranslationRecovery     gtsam/sfm/TranslationRecovery.h     buildGraph, run, SimulateMeasurements
  MFAS                    gtsam/sfm/MFAS.h                    computeOrdering, computeOutlierWeights; plus the batched form over many
                                                              projection directions that 1dSfM sums (MFAS.outlier_weights)
All numerics run in liblmgpu.so on the GPU; this file marshals arrays.  A Unit3 is its 3-vector; translations are Values of POINT3.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib
from .graph import N_DIAG, N_GAUSS, N_ISO, N_UNIT, POINT3, POSE3, NoiseModel, Values, noiseModel
from .optimizer import LevenbergMarquardtParams, _check_linear_solver, _dp, _ip

_U64 = ct.POINTER(ct.c_uint64)
CONSTRAINED_MESSAGE = "constrained noise models take the QR path (out of scope, SURVEY section 2)"


class _Constrained(NoiseModel):
    """noiseModel::Constrained: accepted as a model object so that a caller's code reads like the reference's, refused where it is used"""

    def __init__(self, dim, mu):
        super().__init__(dim, N_DIAG, np.zeros(dim))
        self.constrained, self.mu = True, mu


class Constrained:
    @staticmethod
    def All(dim, mu=1000.0):
        return _Constrained(dim, mu)


def _is_constrained(model):
    if model is None:
        return False
    if getattr(model, "constrained", False):
        return True
    return model.kind in (N_ISO, N_DIAG) and bool((np.atleast_1d(model.data) < 1e-8).any())


class BinaryMeasurement:
    """gtsam/sfm/BinaryMeasurement.h; model None = the reference's null model (unit)"""

    def __init__(self, key1, key2, measured, model=None):
        self._k1, self._k2 = int(key1), int(key2)
        self._z = np.asarray(measured, dtype=np.float64).reshape(3).copy()
        self._model = model

    def key1(self):
        return self._k1

    def key2(self):
        return self._k2

    def measured(self):
        return self._z

    def noiseModel(self):
        return self._model


def _noise_group(model):
    """(device noise kind, 3 or 9 noise doubles | None, robust kind, robust k) of a 3-row model"""
    if model is None:
        return N_UNIT, None, 0, 0.0
    if _is_constrained(model):
        raise NotImplementedError(CONSTRAINED_MESSAGE)
    if model.dim != 3:
        raise ValueError(f"noise model dim {model.dim} != 3")
    if model.kind == N_UNIT:
        kind, data = N_UNIT, None
    elif model.kind in (N_ISO, N_DIAG):
        kind, data = N_DIAG, model.invsigmas()
    else:
        kind, data = N_GAUSS, model.data.reshape(9)
    return kind, data, int(model.robust_kind), float(model.robust_k)


def _grouped(edges):
    """one (indices, keys, meas, kind, noise, robust kind, k) per (noise kind, robust kind, k), list positions kept"""
    groups = {}
    for i, e in enumerate(edges):
        kind, data, rkind, rk = _noise_group(e.noiseModel())
        g = groups.setdefault((kind, rkind, rk), ([], [], [], []))
        g[0].append(i)
        g[1].append((e.key1(), e.key2()))
        g[2].append(e.measured())
        if data is not None:
            g[3].append(data)
    for (kind, rkind, rk), (idx, keys, meas, noise) in groups.items():
        yield (np.array(idx, dtype=np.int32), np.array(keys, dtype=np.uint64).reshape(-1, 2), np.ascontiguousarray(np.array(meas, dtype=np.float64)),
               kind, np.ascontiguousarray(np.array(noise, dtype=np.float64)) if noise else None, rkind, rk)


class TranslationRecoverySession:
    """one lmgpu_translation_recovery object"""

    def __init__(self, device=0, world_size=1):
        if world_size > 1:
            raise NotImplementedError("TranslationRecovery on more than one rank is out of scope (world_size > 1)")
        self.lib = _lib.load()
        self._tr = ct.c_void_p()
        cfg = _lib.lmgpu_config(device, 0, 1, 0)
        if self.lib.lmgpu_translation_recovery_create(ct.byref(cfg), ct.byref(self._tr)) != _lib.LMGPU_OK:
            raise _lib.LmgpuError("lmgpu_translation_recovery_create failed")

    def _check(self, rc):
        if rc == _lib.LMGPU_OK:
            return
        if rc == _lib.LMGPU_INDETERMINATE:
            h = self.handle()
            raise _lib.IndeterminantLinearSystemException(self.lib.lmgpu_last_failed_slot(h) if h is not None else -1)
        msg = self.lib.lmgpu_translation_recovery_last_error(self._tr)
        raise _lib.LmgpuError(f"lmgpu status {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_tr", None):
            self.lib.lmgpu_translation_recovery_destroy(self._tr)
            self._tr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def seed(self, s):
        self._check(self.lib.lmgpu_translation_recovery_seed(self._tr, int(s)))

    def set_prior_sigma(self, sigma):
        self._check(self.lib.lmgpu_translation_recovery_set_prior_sigma(self._tr, float(sigma)))

    def _add(self, fn, edges):
        for idx, keys, meas, kind, noise, rkind, rk in _grouped(edges):
            self._check(fn(self._tr, len(idx), _ip(idx), keys.ctypes.data_as(_U64), _dp(meas), kind, _dp(noise) if noise is not None else None, rkind, rk))

    def add_directions(self, edges):
        self._add(self.lib.lmgpu_translation_recovery_add_directions, edges)

    def add_betweens(self, edges):
        self._add(self.lib.lmgpu_translation_recovery_add_betweens, edges)

    def finalize(self, scale=1.0, initialValues=None, ordering=None):
        ik = np.array(initialValues.keys() if initialValues is not None else [], dtype=np.uint64)
        iv = np.ascontiguousarray(np.array([initialValues.at(k)[:3] for k in ik.tolist()], dtype=np.float64).reshape(-1, 3))
        o = np.array([int(k) for k in ordering] if ordering is not None else [], dtype=np.uint64)
        self._check(self.lib.lmgpu_translation_recovery_finalize(self._tr, float(scale), len(ik), ik.ctypes.data_as(_U64), _dp(iv), len(o),
                                                                 o.ctypes.data_as(_U64)))

    def handle(self):
        h = self.lib.lmgpu_translation_recovery_handle(self._tr)
        return ct.c_void_p(h) if h else None

    def num_factors(self):
        return self.lib.lmgpu_translation_recovery_num_factors(self._tr)

    def keys(self):
        """(every key by first appearance, its representative)"""
        n = self.lib.lmgpu_translation_recovery_num_keys(self._tr)
        k, r = np.zeros(max(n, 0), dtype=np.uint64), np.zeros(max(n, 0), dtype=np.uint64)
        self.lib.lmgpu_translation_recovery_get_keys(self._tr, k.ctypes.data_as(_U64), r.ctypes.data_as(_U64))
        return [int(x) for x in k], [int(x) for x in r]

    def slots(self):
        n = self.lib.lmgpu_translation_recovery_get_slots(self._tr, None)
        k = np.zeros(max(n, 0), dtype=np.uint64)
        self.lib.lmgpu_translation_recovery_get_slots(self._tr, k.ctypes.data_as(_U64))
        return [int(x) for x in k]

    def initial(self):
        """{representative key: initial Point3}"""
        keys = self.slots()
        out = np.zeros((len(keys), 3))
        self._check(self.lib.lmgpu_translation_recovery_get_initial(self._tr, _dp(out)))
        return {k: out[i].copy() for i, k in enumerate(keys)}

    def run(self, lmParams=None):
        cp = (lmParams or LevenbergMarquardtParams())._c()
        st = _lib.lmgpu_lm_state()
        self._check(self.lib.lmgpu_translation_recovery_run(self._tr, ct.byref(cp), ct.byref(st)))
        return st

    def get(self) -> Values:
        keys, _ = self.keys()
        out = np.zeros((len(keys), 3))
        self._check(self.lib.lmgpu_translation_recovery_get(self._tr, _dp(out)))
        v = Values()
        for i, k in enumerate(keys):
            v.insert(k, POINT3, out[i])
        return v


class TranslationRecovery:
    """gtsam/sfm/TranslationRecovery.h.  Every run() builds one session, whose generator starts at this object's seed (42 unless seed(s)
    was called): the reference's generator is process-wide, seeded 42 once, and goes on from run to run."""

    def __init__(self, lmParams=None, use_bilinear_translation_factor=False, device=0, world_size=1):
        if use_bilinear_translation_factor:
            raise NotImplementedError("use_bilinear_translation_factor needs a 1-D variable type (BilinearAngleTranslationFactor is out of scope)")
        if world_size > 1:
            raise NotImplementedError("TranslationRecovery on more than one rank is out of scope (world_size > 1)")
        self.lmParams = lmParams or LevenbergMarquardtParams()
        if self.lmParams.isIterative():
            raise NotImplementedError("TranslationRecovery solves with the direct solver (linearSolverType ITERATIVE / PCG is refused)")
        _check_linear_solver(self.lmParams)
        self.device = device
        self.priorSigma = 0.01
        self._seed = 42
        self.last_state = None

    def seed(self, s):
        self._seed = int(s)

    def buildGraph(self, relativeTranslations) -> int:
        """the number of TranslationFactors of the graph (one per edge, :99-117)"""
        return len(list(relativeTranslations))

    def session(self, relativeTranslations, scale=1.0, betweenTranslations=(), initialValues=None, ordering=None) -> TranslationRecoverySession:
        """the finalized session of run(), for the parity taps"""
        relativeTranslations, betweenTranslations = list(relativeTranslations), list(betweenTranslations)
        for e in relativeTranslations + betweenTranslations:
            if _is_constrained(e.noiseModel()):
                raise NotImplementedError(CONSTRAINED_MESSAGE)
        s = TranslationRecoverySession(self.device)
        try:
            s.set_prior_sigma(self.priorSigma)
            s.add_directions(relativeTranslations)
            s.add_betweens(betweenTranslations)
            s.seed(self._seed)
            s.finalize(scale, initialValues, ordering)
        except Exception:
            s.close()
            raise
        return s

    def run(self, relativeTranslations, scale=1.0, betweenTranslations=(), initialValues=None, ordering=None) -> Values:
        s = self.session(relativeTranslations, scale, betweenTranslations, initialValues, ordering)
        try:
            self.last_state = s.run(self.lmParams)
            return s.get()
        finally:
            s.close()

    @staticmethod
    def SimulateMeasurements(poses: Values, edges):
        """:230-243: Unit3(Tb - Ta) per edge with Isotropic::Sigma(3, 0.01); a zero difference stays the zero vector"""
        model = noiseModel.Isotropic.Sigma(3, 0.01)
        out = []
        for a, b in edges:
            Ta = poses.at(a)[9:12] if poses.type(a) == POSE3 else poses.at(a)[:3]
            Tb = poses.at(b)[9:12] if poses.type(b) == POSE3 else poses.at(b)[:3]
            d = Tb - Ta
            n = np.sqrt(d @ d)
            out.append(BinaryMeasurement(a, b, d / n if n > 0 else d, model))
        return out


class MFAS:
    """gtsam/sfm/MFAS.h: MFAS(relativeTranslations, projectionDirection) or MFAS(edgeWeights) with edgeWeights = {(key1, key2): weight}.
    Ties go to the lowest key (include/lmgpu.h); an unordered pair given twice is refused."""

    def __init__(self, relativeTranslations=None, projectionDirection=None, edgeWeights=None, device=0):
        self.device = device
        if edgeWeights is not None:
            self._keys = np.array([k for k in edgeWeights], dtype=np.uint64).reshape(-1, 2)
            self._w = np.array([[float(edgeWeights[k]) for k in edgeWeights]], dtype=np.float64)
            self._meas = self._dirs = None
        else:
            edges = list(relativeTranslations)
            self._keys = np.array([(e.key1(), e.key2()) for e in edges], dtype=np.uint64).reshape(-1, 2)
            self._meas = np.ascontiguousarray(np.array([e.measured() for e in edges], dtype=np.float64).reshape(-1, 3))
            self._dirs = np.ascontiguousarray(np.asarray(projectionDirection, dtype=np.float64).reshape(1, 3))
            self._w = None
        self._res = None

    @staticmethod
    def outlier_weights(keys, measured=None, directions=None, edgeWeights=None, device=0):
        """the batched form: keys (E, 2); measured (E, 3) with directions (D, 3), or edgeWeights (D, E).
        Returns (orderings (D, V) keys, weights (D, E), per-edge sum (E,), stats dict)."""
        lib = _lib.load()
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1, 2))
        E = keys.shape[0]
        if edgeWeights is not None:
            W = np.ascontiguousarray(np.asarray(edgeWeights, dtype=np.float64).reshape(-1, E))
            D, m, d, w = W.shape[0], None, None, _dp(W)
        else:
            M = np.ascontiguousarray(np.asarray(measured, dtype=np.float64).reshape(E, 3))
            Dm = np.ascontiguousarray(np.asarray(directions, dtype=np.float64).reshape(-1, 3))
            D, m, d, w = Dm.shape[0], _dp(M), _dp(Dm), None
        V = len(np.unique(keys))
        order = np.zeros((D, V), dtype=np.uint64)
        wout, ssum = np.zeros((D, E)), np.zeros(E)
        st = _lib.lmgpu_mfas_stats()
        rc = lib.lmgpu_mfas_outlier_weights(device, E, keys.ctypes.data_as(_U64), m, D, d, w, order.ctypes.data_as(_U64), _dp(wout), _dp(ssum),
                                            ct.byref(st))
        if rc != _lib.LMGPU_OK:
            msg = lib.lmgpu_mfas_last_error()
            err = ValueError if rc == _lib.LMGPU_INVALID else _lib.LmgpuError
            raise err(f"lmgpu status {rc}: {msg.decode() if msg else ''}")
        return order, wout, ssum, {"n_nodes": st.n_nodes, "global_state": st.global_state, "lds_node_capacity": st.lds_node_capacity,
                                   "kernel_ms": st.kernel_ms}

    def _run(self):
        if self._res is None:
            self._res = MFAS.outlier_weights(self._keys, self._meas, self._dirs, self._w, self.device)
        return self._res

    def computeOrdering(self):
        return [int(k) for k in self._run()[0][0]]

    def computeOutlierWeights(self):
        w = self._run()[1][0]
        return {(int(a), int(b)): float(w[i]) for i, (a, b) in enumerate(self._keys.tolist())}
