"""Smart projection factors: SmartProjectionPoseFactor<Cal3_S2> (gtsam/slam/SmartProjectionPoseFactor.h, SmartProjectionFactor.h,
SmartFactorBase.h) and SmartProjectionParams (gtsam/slam/SmartFactorParams.h) over the C ABI (include/lmgpu.h, "smart projection factors").

A factor object only collects its measurements and keys; triangulation, error and linearization run on the device inside the
optimizer that holds the graph, which fills the factor's result (point(), isValid(), ...) from lmgpu_smart_get_points at the end of
optimize() and on smart_points().  Bound: HESSIAN linearization with ZERO_ON_DEGENERACY; every other mode raises
ValueError naming it when the graph reaches an optimizer."""
from __future__ import annotations

import numpy as np

from . import _lib
from .graph import NoiseModel, N_UNIT
from .triangulation import TriangulationParameters, TriangulationResult

HESSIAN, IMPLICIT_SCHUR, JACOBIAN_Q, JACOBIAN_SVD = range(4)  # LinearizationMode, SmartFactorParams.h:30-32
IGNORE_DEGENERACY, ZERO_ON_DEGENERACY, HANDLE_INFINITY = range(3)  # DegeneracyMode, :35-37
_LIN_NAMES = ("HESSIAN", "IMPLICIT_SCHUR", "JACOBIAN_Q", "JACOBIAN_SVD")
_DEG_NAMES = ("IGNORE_DEGENERACY", "ZERO_ON_DEGENERACY", "HANDLE_INFINITY")


class SmartProjectionParams:
    """SmartFactorParams.h:42-118, the reference's defaults (HESSIAN, IGNORE_DEGENERACY, no cheirality throwing, 1e-5) and setters"""

    def __init__(self, linMode=HESSIAN, degMode=IGNORE_DEGENERACY, throwCheirality=False, verboseCheirality=False, retriangulationTh=1e-5):
        self.linearizationMode = linMode
        self.degeneracyMode = degMode
        self.triangulation = TriangulationParameters()
        self.retriangulationThreshold = retriangulationTh
        self.throwCheirality = throwCheirality
        self.verboseCheirality = verboseCheirality

    def getLinearizationMode(self):
        return self.linearizationMode

    def getDegeneracyMode(self):
        return self.degeneracyMode

    def getTriangulationParameters(self):
        return self.triangulation

    def getVerboseCheirality(self):
        return self.verboseCheirality

    def getThrowCheirality(self):
        return self.throwCheirality

    def getRetriangulationThreshold(self):
        return self.retriangulationThreshold

    def setLinearizationMode(self, linMode):
        self.linearizationMode = linMode

    def setDegeneracyMode(self, degMode):
        self.degeneracyMode = degMode

    def setRetriangulationThreshold(self, retriangulationTh):
        self.retriangulationThreshold = retriangulationTh

    def setRankTolerance(self, rankTol):
        self.triangulation.rankTolerance = rankTol

    def setEnableEPI(self, enableEPI):
        self.triangulation.enableEPI = enableEPI

    def setLandmarkDistanceThreshold(self, landmarkDistanceThreshold):
        self.triangulation.landmarkDistanceThreshold = landmarkDistanceThreshold

    def setDynamicOutlierRejectionThreshold(self, dynOutRejectionThreshold):
        self.triangulation.dynamicOutlierRejectionThreshold = dynOutRejectionThreshold

    def _c(self):
        """the lmgpu_smart_params; ValueError for what the device does not implement"""
        if self.linearizationMode != HESSIAN:
            raise ValueError(f"SmartProjectionParams: linearizationMode {_LIN_NAMES[self.linearizationMode]} is not bound (HESSIAN is)")
        if self.degeneracyMode != ZERO_ON_DEGENERACY:
            raise ValueError(f"SmartProjectionParams: degeneracyMode {_DEG_NAMES[self.degeneracyMode]} is not bound "
                             "(setDegeneracyMode(ZERO_ON_DEGENERACY) is)")
        if self.throwCheirality or self.verboseCheirality:
            raise ValueError("SmartProjectionParams: throwCheirality / verboseCheirality are not bound")
        if self.triangulation.useLOST:
            raise ValueError("SmartProjectionParams: useLOST is not bound (LOST is not implemented)")
        return _lib.lmgpu_smart_params(int(self.linearizationMode), int(self.degeneracyMode), float(self.retriangulationThreshold),
                                       self.triangulation._c())


class SmartProjectionPoseFactor:
    """SmartProjectionPoseFactor<Cal3_S2>(sharedNoiseModel, K, params) (SmartProjectionPoseFactor.h:62-80); K = (fx, fy, s, u0, v0);
    the noise model must be Isotropic of dimension 2 (SmartFactorBase.h:109-115); body_P_sensor is not bound"""

    def __init__(self, sharedNoiseModel, K, params=None, body_P_sensor=None):
        if body_P_sensor is not None:
            raise ValueError("SmartProjectionPoseFactor: body_P_sensor is not bound")
        if not isinstance(sharedNoiseModel, NoiseModel) or sharedNoiseModel.dim != 2 or getattr(sharedNoiseModel, "robust_kind", 0):
            raise ValueError("SmartFactorBase: noise model must be isotropic of dimension 2")
        if sharedNoiseModel.kind == N_UNIT:
            self.inv_sigma = 1.0
        else:
            inv = np.asarray(sharedNoiseModel.invsigmas(), dtype=float).reshape(-1)
            if inv.size != 2 or inv[0] != inv[1]:
                raise ValueError("SmartFactorBase: noise model must be isotropic")
            self.inv_sigma = float(inv[0])
        self.K = np.asarray(K, dtype=np.float64).reshape(5).copy()
        self.params = params if params is not None else SmartProjectionParams()
        self._z, self._keys = [], []
        self._result = TriangulationResult(TriangulationResult.DEGENERATE)

    def add(self, measured, key):
        """add(z, key) or add(zs, keys) (SmartFactorBase.h:127-146)"""
        if np.ndim(key) == 0:
            measured, key = [measured], [key]
        for z, k in zip(measured, key):
            k = int(k)
            if k in self._keys:
                raise ValueError("SmartFactorBase::add: adding duplicate measurement for key")
            self._keys.append(k)
            self._z.append(np.asarray(z, dtype=np.float64).reshape(2).copy())

    def keys(self):
        return list(self._keys)

    def measured(self):
        return [z.copy() for z in self._z]

    def size(self):
        return len(self._keys)

    # -- the result of the last triangulation on the device (SmartProjectionFactor.h:442-461)
    def point(self):
        """TriangulationResult: the point where valid"""
        return self._result

    def isValid(self):
        return self._result.status == TriangulationResult.VALID

    def isDegenerate(self):
        return self._result.status == TriangulationResult.DEGENERATE

    def isPointBehindCamera(self):
        return self._result.status == TriangulationResult.BEHIND_CAMERA

    def isOutlier(self):
        return self._result.status == TriangulationResult.OUTLIER

    def isFarPoint(self):
        return self._result.status == TriangulationResult.FAR_POINT

    def _set_result(self, status, point):
        self._result = TriangulationResult(status, point if status == TriangulationResult.VALID else None)
