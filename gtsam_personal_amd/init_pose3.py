"""InitializePose3 mirror over the C ABI (include/lmgpu.h, the lmgpu_init_pose3_* group).

Same static methods as the reference class (gtsam/slam/InitializePose3.h; InitializePose3.cpp, InitializePose.h):
  buildPose3graph, buildLinearOrientationGraph, computeOrientationsChordal, computeOrientationsGradient,
  normalizeRelaxedRotations, initializeOrientations, computePoses, initialize
Rotations are returned as {key: 3x3 array}; poses as Values.  All numerics run in liblmgpu.so on the GPU; this file marshals arrays.
Every method takes an optional `ordering` of the pose keys (a boundary input as for the optimizers; default Ordering.Natural); the
anchor key may be part of it, otherwise it is eliminated last.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib
from .graph import F_BETWEEN_POSE3, F_PRIOR_POSE3, N_UNIT, POSE3, NoiseModel, NonlinearFactorGraph, Ordering, Values
from .optimizer import GaussianFactorGraph, LevenbergMarquardtOptimizer, LevenbergMarquardtParams, _check_linear_solver, _dp, _ip

kAnchorKey = _lib.LMGPU_INIT_POSE3_ANCHOR_KEY  # initialize::kAnchorKey, InitializePose.h:30


def _records(graph: NonlinearFactorGraph):
    """[(graph index, ftype, keys, meas, model)] in graph order"""
    rec = []
    for ftype, _, gi, keys, meas, _, models in graph.buckets():
        for i, g in enumerate(gi.tolist()):
            rec.append((g, ftype, keys[i], meas[i], models[i]))
    rec.sort(key=lambda r: r[0])
    return rec


def rotation_precision(model: NoiseModel) -> float:
    """first entry of noiseModel->whitenInPlace(e1) (InitializePose3.cpp:48-51)"""
    if model.kind == N_UNIT:
        return 1.0
    if model.data.ndim == 2:
        return float(model.data[0, 0])
    return float(model.invsigmas()[0])


class _Session:
    """one lmgpu_init_pose3 object: the extracted pose graph on the device"""

    def __init__(self, pose3Graph: NonlinearFactorGraph, ordering=None, params=None, device=0):
        self.lib = _lib.load()
        self._ip = ct.c_void_p()
        cfg = _lib.lmgpu_config(device, 0, 1, 0)
        if self.lib.lmgpu_init_pose3_create(ct.byref(cfg), ct.byref(self._ip)) != _lib.LMGPU_OK:
            raise _lib.LmgpuError("lmgpu_init_pose3_create failed")
        pcg = _check_linear_solver(params) if params is not None else None
        for ftype, kind, gi, keys, meas, noise, _ in pose3Graph.buckets():
            nptr = _dp(np.ascontiguousarray(noise)) if kind != N_UNIT else None
            self._check(self.lib.lmgpu_init_pose3_add_factors(self._ip, ftype, len(gi), _ip(np.ascontiguousarray(gi, dtype=np.int32)),
                                                              np.ascontiguousarray(keys, dtype=np.uint64).ctypes.data_as(ct.POINTER(ct.c_uint64)),
                                                              _dp(np.ascontiguousarray(meas, dtype=np.float64)), kind, nptr))
        ordering = list(ordering) if ordering is not None else [k for k in Ordering.Natural(pose3Graph)]
        o = np.array(ordering, dtype=np.uint64)
        self._check(self.lib.lmgpu_init_pose3_finalize(self._ip, len(o), o.ctypes.data_as(ct.POINTER(ct.c_uint64))))
        self.keys = [int(k) for k in ordering if int(k) != kAnchorKey]
        if pcg is not None:
            h = self.handle(0)
            if self.lib.lmgpu_set_linear_solver(h, _lib.LMGPU_SOLVER_PCG, ct.byref(pcg)) != _lib.LMGPU_OK:
                raise _lib.LmgpuError("lmgpu_set_linear_solver on the orientation handle failed")

    def _check(self, rc):
        if rc == _lib.LMGPU_OK:
            return
        msg = self.lib.lmgpu_init_pose3_last_error(self._ip)
        if rc == _lib.LMGPU_INDETERMINATE:
            raise _lib.IndeterminantLinearSystemException(self.lib.lmgpu_last_failed_slot(self.handle(0)))
        raise _lib.LmgpuError(f"lmgpu status {rc}: {msg.decode() if msg else ''}")

    def handle(self, which):
        return ct.c_void_p(self.lib.lmgpu_init_pose3_handle(self._ip, which))

    def close(self):
        if getattr(self, "_ip", None):
            self.lib.lmgpu_init_pose3_destroy(self._ip)
            self._ip = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rot_dict(self, R):
        return {k: R[i].reshape(3, 3).copy() for i, k in enumerate(self.keys)}

    def _rot_pack(self, rots):
        return np.ascontiguousarray(np.stack([np.asarray(rots[k], dtype=np.float64).reshape(9) for k in self.keys]))

    def chordal(self):
        R = np.empty((len(self.keys), 9))
        self._check(self.lib.lmgpu_init_pose3_orientations_chordal(self._ip, _dp(R)))
        return self._rot_dict(R)

    def gradient(self, guess_rots, maxIter, setRefFrame):
        R = np.empty((len(self.keys), 9))
        it, mg = ct.c_int32(), ct.c_double()
        g = self._rot_pack(guess_rots)
        self._check(self.lib.lmgpu_init_pose3_orientations_gradient(self._ip, _dp(g), int(maxIter), int(bool(setRefFrame)), _dp(R), ct.byref(it),
                                                                    ct.byref(mg)))
        return self._rot_dict(R), it.value, mg.value

    def poses(self, rots=None, singleIter=True):
        out = np.empty((len(self.keys), 12))
        st = _lib.lmgpu_lm_state()
        r = None if rots is None else _dp(self._rot_pack(rots))
        self._check(self.lib.lmgpu_init_pose3_compute_poses(self._ip, r, int(bool(singleIter)), _dp(out), ct.byref(st)))
        v = Values()
        for i, k in enumerate(self.keys):
            v.insert(k, POSE3, out[i])
        return v, st

    def initialize(self, guess_rots=None, useGradient=False):
        out = np.empty((len(self.keys), 12))
        g = None if guess_rots is None else _dp(self._rot_pack(guess_rots))
        self._check(self.lib.lmgpu_init_pose3_initialize(self._ip, g, int(bool(useGradient)), _dp(out)))
        v = Values()
        for i, k in enumerate(self.keys):
            v.insert(k, POSE3, out[i])
        return v


def _guess_rotations(givenGuess: Values):
    return {k: givenGuess.at(k)[:9].reshape(3, 3) for k in givenGuess.keys() if givenGuess.type(k) == POSE3}


class InitializePose3:
    """gtsam/slam/InitializePose3.h"""

    kAnchorKey = kAnchorKey

    @staticmethod
    def buildPose3graph(graph: NonlinearFactorGraph) -> NonlinearFactorGraph:
        """initialize::buildPoseGraph<Pose3> (InitializePose.h:36-52): BetweenFactor<Pose3> kept, PriorFactor<Pose3> -> BetweenFactor from
        kAnchorKey with the prior's noise model, everything else dropped"""
        out = NonlinearFactorGraph()
        for _, ftype, keys, meas, model in _records(graph):
            if ftype == F_BETWEEN_POSE3:
                out._add(F_BETWEEN_POSE3, [keys], [meas], model)
            elif ftype == F_PRIOR_POSE3:
                out._add(F_BETWEEN_POSE3, [[kAnchorKey, keys[0]]], [meas], model)
        return out

    @staticmethod
    def _orientation_problem(pose3Graph: NonlinearFactorGraph, ordering=None, params=None, device=0):
        lin, zeros = NonlinearFactorGraph(), Values()
        for _, ftype, keys, meas, model in _records(pose3Graph):
            if ftype != F_BETWEEN_POSE3:
                raise ValueError("Error in buildLinearOrientationGraph: not a BetweenFactor<Pose3>")
            lin.add_ChordalBetweenFactor(int(keys[0]), int(keys[1]), meas[:9], rotation_precision(model))
        lin.add_PriorFactorVec9(kAnchorKey, np.eye(3).reshape(9), None)
        for k in lin.keys():
            zeros.insert_vec9(k, np.zeros(9))
        order = list(ordering) if ordering is not None else list(Ordering.Natural(lin))
        if kAnchorKey not in [int(k) for k in order]:
            order = order + [kAnchorKey]
        return LevenbergMarquardtOptimizer(lin, zeros, Ordering(order), params or LevenbergMarquardtParams(), device=device)

    @staticmethod
    def buildLinearOrientationGraph(pose3Graph: NonlinearFactorGraph, ordering=None, device=0) -> GaussianFactorGraph:
        """InitializePose3.cpp:37-71: one [-I9 | M9 | 0] JacobianFactor per between factor and the anchor's prior, as the linearization
        of the CHORDAL_BETWEEN / PRIOR_VEC9 factors at zero (whitened, read back from the device)"""
        return InitializePose3._orientation_problem(pose3Graph, ordering, None, device).linearize()

    @staticmethod
    def normalizeRelaxedRotations(relaxedRot3: dict, device=0) -> dict:
        """InitializePose3.cpp:75-92; relaxedRot3 = {key: 9-vector}; the anchor is left out of the result"""
        keys = [int(k) for k in sorted(relaxedRot3) if int(k) != kAnchorKey]
        if not keys:
            return {}
        M = np.ascontiguousarray(np.stack([np.asarray(relaxedRot3[k], dtype=np.float64).reshape(9) for k in keys]))
        R = np.empty_like(M)
        rc = _lib.load().lmgpu_init_pose3_closest_rotations(device, len(keys), _dp(M), _dp(R))
        if rc != _lib.LMGPU_OK:
            raise _lib.LmgpuError(f"lmgpu_init_pose3_closest_rotations: status {rc}")
        return {k: R[i].reshape(3, 3).copy() for i, k in enumerate(keys)}

    @staticmethod
    def computeOrientationsChordal(pose3Graph: NonlinearFactorGraph, ordering=None, params=None, device=0) -> dict:
        """InitializePose3.cpp:102-114; `params` (optional) selects the linear solver like an optimizer's (linearSolverType,
        iterativeParams)"""
        s = _Session(pose3Graph, ordering, params, device)
        try:
            return s.chordal()
        finally:
            s.close()

    @staticmethod
    def computeOrientationsGradient(pose3Graph: NonlinearFactorGraph, givenGuess: Values, maxIter=10000, setRefFrame=True, ordering=None,
                                    device=0, return_info=False):
        """InitializePose3.cpp:117-218; return_info: also (iterations run, last maxGrad)"""
        s = _Session(pose3Graph, ordering, None, device)
        try:
            R, it, mg = s.gradient(_guess_rotations(givenGuess), maxIter, setRefFrame)
        finally:
            s.close()
        return (R, it, mg) if return_info else R

    @staticmethod
    def initializeOrientations(graph: NonlinearFactorGraph, ordering=None, device=0) -> dict:
        """InitializePose3.cpp:278-285"""
        return InitializePose3.computeOrientationsChordal(InitializePose3.buildPose3graph(graph), ordering, None, device)

    @staticmethod
    def computePoses(initialRot: dict, posegraph: NonlinearFactorGraph, singleIter=True, ordering=None, device=0) -> Values:
        """initialize::computePoses<Pose3> (InitializePose.h:57-97).  Like the reference, the anchor's Unit(6) prior is ADDED to
        `posegraph` (it takes the graph by pointer, :75)."""
        s = _Session(posegraph, ordering, None, device)
        try:
            v, _ = s.poses(initialRot, singleIter)
        finally:
            s.close()
        posegraph.add_PriorFactorPose3(kAnchorKey, np.eye(3), np.zeros(3), NoiseModel(6, N_UNIT))
        return v

    @staticmethod
    def initialize(graph: NonlinearFactorGraph, givenGuess: Values | None = None, useGradient=False, ordering=None, device=0) -> Values:
        """InitializePose3.cpp:296-319"""
        s = _Session(InitializePose3.buildPose3graph(graph), ordering, None, device)
        try:
            guess = _guess_rotations(givenGuess) if (useGradient and givenGuess is not None) else None
            if useGradient and guess is None:
                raise ValueError("initialize(useGradient=True) needs givenGuess")
            return s.initialize(guess, useGradient)
        finally:
            s.close()
