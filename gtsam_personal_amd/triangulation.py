"""Triangulation (gtsam/geometry/triangulation.h): triangulatePoint3 / triangulateSafe for PinholeCamera<Cal3Bundler> and
PinholeCamera<Cal3_S2> on the device, batched over landmarks (lmgpu_triangulate_batch, include/lmgpu.h).

Cameras are packed arrays of 17 doubles: `camera_pack(R, t, f, k1, k2, u0, v0)` for PinholeCamera<Cal3Bundler> (the packing of Values'
CAM_BUNDLER), `camera_s2_pack(R, t, fx, fy, s, u0, v0)` = pose3_pack + K for PinholeCamera<Cal3_S2>.  There is no CPU fallback."""
from __future__ import annotations

import collections
import ctypes as ct

import numpy as np

from . import _lib
from .graph import NoiseModel, N_UNIT, camera_pack, pose3_pack  # noqa: F401

CAL3_BUNDLER, CAL3_S2 = _lib.LMGPU_TRI_CAM_BUNDLER, _lib.LMGPU_TRI_CAM_S2


def camera_s2_pack(R, t, fx, fy, s, u0, v0):
    return np.concatenate([pose3_pack(R, t), [fx, fy, s, u0, v0]])


class TriangulationUnderconstrainedException(RuntimeError):
    """triangulation.h:36-41"""

    def __init__(self):
        super().__init__("Triangulation Underconstrained Exception.")


class TriangulationCheiralityException(RuntimeError):
    """triangulation.h:44-49"""

    def __init__(self):
        super().__init__("Triangulation Cheirality Exception: The resulting landmark is behind one or more cameras.")


class TriangulationParameters:
    """triangulation.h:562-609; noiseModel: None (Unit) or an isotropic model of dimension 2"""

    def __init__(self, rankTolerance=1.0, enableEPI=False, landmarkDistanceThreshold=-1.0, dynamicOutlierRejectionThreshold=-1.0,
                 useLOST=False, noiseModel=None):
        self.rankTolerance = rankTolerance
        self.enableEPI = enableEPI
        self.landmarkDistanceThreshold = landmarkDistanceThreshold
        self.dynamicOutlierRejectionThreshold = dynamicOutlierRejectionThreshold
        self.useLOST = useLOST
        self.noiseModel = noiseModel

    def _c(self):
        return _lib.lmgpu_triangulation_params(self.rankTolerance, 1 if self.enableEPI else 0, 1 if self.useLOST else 0,
                                               self.landmarkDistanceThreshold, self.dynamicOutlierRejectionThreshold, _inv_sigma(self.noiseModel))


def _inv_sigma(model):
    """one inverse sigma of a shared noise model: None / Unit -> 0 (Unit); an isotropic model -> 1 / sigma"""
    if model is None:
        return 0.0
    if isinstance(model, (int, float)):
        return float(model)
    if not isinstance(model, NoiseModel) or getattr(model, "robust_kind", 0):
        raise ValueError("triangulation takes a Unit or an Isotropic noise model (a robust model is out of scope)")
    if model.kind == N_UNIT:
        return 0.0
    inv = np.asarray(model.invsigmas(), dtype=float).reshape(-1)
    if inv.size != 2 or inv[0] != inv[1]:
        raise ValueError("triangulation takes a Unit or an Isotropic noise model of dimension 2")
    return float(inv[0])


class TriangulationResult:
    """triangulation.h:616-698"""
    VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT, CALIBRATE_FAILED = range(6)

    def __init__(self, status, point=None):
        self.status = int(status)
        self._point = None if point is None else np.asarray(point, dtype=float)

    def valid(self):
        return self.status == self.VALID

    def degenerate(self):
        return self.status == self.DEGENERATE

    def outlier(self):
        return self.status == self.OUTLIER

    def farPoint(self):
        return self.status == self.FAR_POINT

    def behindCamera(self):
        return self.status == self.BEHIND_CAMERA

    def get(self):
        if not self.valid():
            raise RuntimeError("TriangulationResult::get called on an invalid result")
        return self._point

    def __repr__(self):
        names = ("VALID", "DEGENERATE", "BEHIND_CAMERA", "OUTLIER", "FAR_POINT", "CALIBRATE_FAILED")
        return f"TriangulationResult({names[self.status]}, {self._point})"


class TriangulationStats:
    def __init__(self, c):
        self.n_points = c.n_points
        self.n_status = list(c.n_status)
        self.max_iterations, self.sum_iterations, self.device_ms = c.max_iterations, c.sum_iterations, c.device_ms


# what LevenbergMarquardtOptimizer.triangulate_landmarks returns
LandmarkTriangulation = collections.namedtuple("LandmarkTriangulation", "keys points status n_valid stats")


def _dp(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


def _ip(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_int32))


def pack_for_device(cameras, camera_model, obs_cam, obs_z):
    """the arrays lmgpu_triangulate_batch takes: Cal3Bundler cameras lose (u0, v0), which is folded into their measurements"""
    cams = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 17)
    z = np.array(obs_z, dtype=np.float64).reshape(-1, 2)
    oc = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    if camera_model == CAL3_BUNDLER:
        if len(oc) and 0 <= oc.min() and oc.max() < len(cams):
            z = z - cams[oc, 15:17]
        cams = np.ascontiguousarray(cams[:, :15])
    return cams, oc, np.ascontiguousarray(z)


def triangulateSafeBatch(cameras, camera_model, obs_offsets, obs_cam, obs_z, params=None, device=0, return_stats=False):
    """triangulateSafe for every landmark of a CSR batch: landmark i is observed by cameras obs_cam[obs_offsets[i]:obs_offsets[i + 1]] at
    the pixels obs_z[...].  Returns (points (n, 3), NaN where not VALID; status (n,))[, TriangulationStats]."""
    params = params or TriangulationParameters()
    lib = _lib.load()
    off = np.ascontiguousarray(obs_offsets, dtype=np.int32).reshape(-1)
    n = len(off) - 1
    cams, oc, z = pack_for_device(cameras, camera_model, obs_cam, obs_z)
    points, status = np.full((max(n, 0), 3), np.nan), np.zeros(max(n, 0), dtype=np.int32)
    cp = params._c()
    rc = lib.lmgpu_triangulate_batch(device, camera_model, len(cams), _dp(cams), n, _ip(off), _ip(oc), _dp(z), ct.byref(cp), _dp(points), _ip(status))
    if rc != _lib.LMGPU_OK:
        raise _lib.LmgpuError(f"lmgpu_triangulate_batch: status {rc}")
    if not return_stats:
        return points, status
    st = _lib.lmgpu_triangulation_stats()
    lib.lmgpu_get_triangulation_stats(None, ct.byref(st))
    return points, status, TriangulationStats(st)


def triangulateSafe(cameras, measured, params=None, camera_model=CAL3_S2, device=0) -> TriangulationResult:
    """triangulateSafe(cameras, measured, params), triangulation.h:701-758"""
    m = len(measured)
    pts, st = triangulateSafeBatch(cameras, camera_model, [0, m], np.arange(m), measured, params, device)
    return TriangulationResult(st[0], pts[0] if st[0] == 0 else None)


def triangulatePoint3(cameras, measurements, rank_tol=1e-9, optimize=False, model=None, camera_model=CAL3_S2, device=0):
    """triangulatePoint3(cameras, measurements, rank_tol, optimize, model), triangulation.h:491-549"""
    r = triangulateSafe(cameras, measurements, TriangulationParameters(rank_tol, optimize, noiseModel=model), camera_model, device)
    if r.degenerate():
        raise TriangulationUnderconstrainedException()
    if r.behindCamera():
        raise TriangulationCheiralityException()
    if not r.valid():
        raise RuntimeError("Cal3Bundler::calibrate fails to converge. need a better initialization")
    return r.get()
