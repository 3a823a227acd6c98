"""The device PCG solver (linearSolverType = ITERATIVE, PCGSolverParameters; kernels_pcg.hpp) against the numpy restatement of the
reference's loop (tests/pcg_restatement.py) run on the device's own Jacobians, against the frozen oracle's direct solves and LM / GN
traces as the converged limit, and on a graph the direct path cannot hold."""
import ctypes as ct
import os

import numpy as np
import pytest

import oracle_harness as oh
import pcg_restatement as pr
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, DoglegOptimizer, DoglegParams, DummyPreconditionerParameters,
                                GaussNewtonOptimizer, GaussNewtonParams, LevenbergMarquardtOptimizer, LevenbergMarquardtParams,
                                NonlinearFactorGraph, Ordering, PCGSolverParameters, Values, _lib, noiseModel)
from gtsam_personal_amd.graph import L, X
from gtsam_personal_amd.datasets import SfmData, bal_graph, load3D
from gtsam_personal_amd.synthetic import make_bal

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.linalg.norm(a - b) / max(1e-300, np.linalg.norm(b)))


def _iterative(params, pre="bj", **kw):
    pcg = PCGSolverParameters(BlockJacobiPreconditionerParameters() if pre == "bj" else DummyPreconditionerParameters())
    for k, v in kw.items():
        setattr(pcg, k, v)
    params.linearSolverType = "ITERATIVE"
    params.iterativeParams = pcg
    return params


def _dubrovnik():
    db = SfmData.FromBalFile(os.path.join(GOLD, "dubrovnik-3-7-pre.txt"))
    return bal_graph(db)


def _bal100():
    graph, initial, _, _ = make_bal(n_cam=100, n_pt=1500, obs_per_point=6, seed=42)
    return graph, initial


def _pose3():
    graph, initial = load3D(os.path.join(GOLD, "pose3example.txt"))
    graph.add_PriorFactorPose3(0, initial.at(0)[:9].reshape(3, 3), initial.at(0)[9:12],
                               noiseModel.Diagonal.Variances([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]))
    return graph, initial


WORKLOADS = {"dubrovnik": _dubrovnik, "bal100": _bal100, "pose3example": _pose3}


def _device_system(opt, lam, diagonal, min_diag=1e-6, max_diag=1e32):
    """the restatement's System on the device's own linearization (lmgpu_get_jacobians) with LM's damping"""
    lg = opt.linear_graph()
    facs, dims = [], {}
    for i in range(lg.size()):
        f = lg.at(i)
        if f is None:
            continue
        As = [f.getA(j) for j in range(len(f.keys()))]
        facs.append((f.keys(), As, f.getb()))
        for k, A in zip(f.keys(), As):
            dims[int(k)] = A.shape[1]
    s0 = pr.System(facs, dims)
    if diagonal:  # clamp(hessianDiagonal) (LevenbergMarquardtOptimizer.cpp:291-298: sqrt, squared again by the prior)
        w = {k: np.sqrt(np.clip(np.diag(s0.blocks[k]), min_diag, max_diag)) ** 2 for k in s0.keys}
    else:
        w = {k: np.ones(dims[k]) for k in s0.keys}
    return pr.System(facs, dims, damping={k: lam * v for k, v in w.items()})


def _restated_params(pcg: PCGSolverParameters):
    kind = pr.BLOCK_JACOBI if isinstance(pcg.preconditioner, BlockJacobiPreconditionerParameters) else pr.DUMMY
    return pr.PCGParams(pcg.minIterations, pcg.maxIterations, pcg.reset, pcg.epsilon_rel, pcg.epsilon_abs, kind)


def _compare(opt, sysr, pcg, lam, diagonal):
    x, iters, gammas, thr = pr.pcg(sysr, _restated_params(pcg))
    # the stop decision of every executed test is clear of the threshold (else a summation-order rounding could flip it)
    for g in gammas[:iters + 1]:
        assert abs(g - thr) > 1e-6 * thr, (g, thr)
    opt.set_linear_solver(opt.params)
    byk, _, _, _ = opt.solve(lam, diagonal_damping=diagonal)
    st = opt.pcg_stats()
    assert st["iterations"] == iters, (st, iters)
    assert abs(st["gamma0"] - gammas[0]) <= 1e-12 * gammas[0] + 1e-300
    assert abs(st["threshold"] - thr) <= 1e-12 * thr
    xr = pr.by_key(sysr, x)
    dev = np.concatenate([byk[k] for k in sysr.keys])
    ref = np.concatenate([xr[k] for k in sysr.keys])
    if iters == 0:
        assert not dev.any()
    else:
        # Dummy: the unpreconditioned systems here have gamma0 ~ 1e11 and amplify summation-order rounding ~100x per few iterations
        tol = 1e-9 if isinstance(pcg.preconditioner, BlockJacobiPreconditionerParameters) else 1e-5
        assert rel(dev, ref) <= tol, rel(dev, ref)
    assert st["host_waits"] <= (iters + 15) // 16 + 2
    return st, iters


CASES = ["defaults", "reset3", "min_above", "max0", "eps_abs_above"]


@pytest.mark.parametrize("work", ["dubrovnik", "bal100", "pose3example"])
@pytest.mark.parametrize("pre", ["bj", "dummy"])
@pytest.mark.parametrize("diagonal", [False, True])
def test_device_matches_restatement(work, pre, diagonal):
    graph, initial = WORKLOADS[work]()
    params = _iterative(LevenbergMarquardtParams(), pre)
    opt = LevenbergMarquardtOptimizer(graph, initial, None, params, device=0)
    assert opt.num_fronts() == 0
    opt.linearize()
    lam = 1e-3
    sysr = _device_system(opt, lam, diagonal)
    pcg = params.iterativeParams
    # Without a preconditioner CG on these systems loses orthogonality within a few dozen iterations, and rounding differences of
    # the summation order grow with it: the Dummy cases compare the first eight iterations (eps 0), where the two agree to 1e-9.
    short = pre == "dummy"
    if short:
        pcg.maxIterations, pcg.epsilon_rel, pcg.epsilon_abs = 8, 0.0, 0.0
    _, natural = _compare(opt, sysr, pcg, lam, diagonal)
    for case in CASES[1:]:
        if case == "min_above" and (work == "bal100" or short or natural + 4 > 500):
            continue
        pcg = PCGSolverParameters(pcg.preconditioner)
        if case == "reset3":
            pcg.reset = 3
            pcg.maxIterations = 8 if short else 60
            if short:
                pcg.epsilon_rel = pcg.epsilon_abs = 0.0
        elif case == "min_above":
            pcg.minIterations = natural + 4
        elif case == "max0":
            pcg.maxIterations = 0
        elif case == "eps_abs_above":
            x, _, gammas, _ = pr.pcg(sysr, pr.PCGParams(maxIterations=0, preconditioner=_restated_params(pcg).preconditioner))
            pcg.epsilon_abs = 10.0 * gammas[0]  # above this preconditioner's own gamma0
        params.iterativeParams = pcg
        st, iters = _compare(opt, sysr, pcg, lam, diagonal)
        if case == "eps_abs_above":
            assert iters == 1  # minIterations = 1: one body always runs
        if case == "max0":
            assert iters == 0
        if case == "min_above":
            assert iters >= natural + 4
    opt.close()


@pytest.mark.parametrize("work", ["dubrovnik", "pose3example"])
def test_converged_limit_equals_direct_solve(work):
    """eps 1e-14 and enough iterations: the PCG step is the direct step of the same handle (Cholesky-finalized, switched over)"""
    graph, initial = WORKLOADS[work]()
    opt = LevenbergMarquardtOptimizer(graph, initial, Ordering.Natural(graph), LevenbergMarquardtParams(), device=0)
    opt.linearize()
    _, d_direct, e0d, e1d = opt.solve(1e-4)
    params = _iterative(LevenbergMarquardtParams(), "bj", epsilon_rel=1e-14, epsilon_abs=1e-28, maxIterations=20000)
    opt.set_linear_solver(params)
    _, d_pcg, e0, e1 = opt.solve(1e-4)
    assert rel(d_pcg, d_direct) <= 1e-7, rel(d_pcg, d_direct)
    assert abs(e0 - e0d) <= 1e-12 * e0d and abs(e1 - e1d) <= 1e-7 * e0d
    opt.set_linear_solver(LevenbergMarquardtParams())  # and back to the direct solver
    _, d_again, _, _ = opt.solve(1e-4)
    assert np.array_equal(d_again, d_direct)


def _lm_trace_case(graph, initial, params, n_iter, gn=False):
    ordering = Ordering.Natural(graph)
    orc = oh.OracleProblem(graph, initial, ordering)
    if gn:
        opt = GaussNewtonOptimizer(graph, initial, None, params, device=0)
    else:
        opt = LevenbergMarquardtOptimizer(graph, initial, None, params, device=0)
    orc.lm_init(params)
    for _ in range(n_iter):
        if gn:
            opt.iterate()
            assert orc.gn_iterate() == 0
        else:
            opt.iterate()
            orc.lm_iterate(params)
        so = orc.lm_state()
        assert opt.iterations() == so["iterations"]
        assert abs(opt.error() - so["error"]) <= 1e-6 * so["error"], (opt.error(), so)
        if not gn:
            assert opt.getInnerIterations() == so["inner"]
            assert abs(opt.lambda_() - so["lambda_"]) <= 1e-6 * so["lambda_"]
    return opt


@pytest.mark.parametrize("work,mode", [("dubrovnik", "legacy"), ("dubrovnik", "ceres"), ("bal100", "legacy"), ("bal100", "ceres"), ("bal100", "gn")])
def test_lm_gn_trajectory_tight_pcg(work, mode):
    """(Gauss-Newton on dubrovnik is left out: its undamped system has the gauge freedom of an unanchored BA, the oracle refuses it too)"""
    graph, initial = WORKLOADS[work]()
    base = {"legacy": LevenbergMarquardtParams(), "ceres": LevenbergMarquardtParams.CeresDefaults(), "gn": GaussNewtonParams()}[mode]
    params = _iterative(base, "bj", epsilon_rel=1e-14, epsilon_abs=1e-26, maxIterations=20000)
    _lm_trace_case(graph, initial, params, 4, gn=(mode == "gn"))


def test_lm_default_pcg_dubrovnik_final_error():
    """LM with default PCG parameters on dubrovnik ends no worse than the direct path's minimum.  One-sided on purpose: the default
    PCG steps are inexact (eps_rel 1e-3), so the trajectory leaves the direct one, and on this graph it reaches a LOWER minimum
    (0.0156 against 0.0200); a two-sided 1e-4 bound would pin which local minimum an inexact step happens to fall into."""
    graph, initial = _dubrovnik()
    params = _iterative(LevenbergMarquardtParams(), "bj")
    opt = LevenbergMarquardtOptimizer(graph, initial, None, params, device=0)
    opt.optimize()
    orc = oh.OracleProblem(graph, initial, Ordering.Natural(graph))
    p0 = LevenbergMarquardtParams()
    orc.lm_init(p0)
    orc.lm_optimize(p0)
    ref = orc.lm_state()["error"]
    # default PCG steps are inexact (eps_rel 1e-3), so the trajectory leaves the direct one; it must end no worse than the direct minimum
    assert opt.error() <= ref * (1 + 1e-4), (opt.error(), ref)


def test_pcg_bitwise_reproducible():
    graph, initial = _bal100()
    params = _iterative(LevenbergMarquardtParams(), "bj")
    opt = LevenbergMarquardtOptimizer(graph, initial, None, params, device=0)
    opt.linearize()
    _, a, ea0, ea1 = opt.solve(1e-3, diagonal_damping=True)
    sa = opt.pcg_stats()
    _, b, eb0, eb1 = opt.solve(1e-3, diagonal_damping=True)
    sb = opt.pcg_stats()
    assert np.array_equal(a, b) and ea0 == eb0 and ea1 == eb1
    assert sa["iterations"] == sb["iterations"] and sa["gamma"] == sb["gamma"]


def test_refusals():
    graph, initial = _dubrovnik()
    # Dogleg: the C ABI refuses PCG, the Python optimizer raises before it builds anything
    params = _iterative(DoglegParams(), "bj")
    with pytest.raises(RuntimeError):
        DoglegOptimizer(graph, initial, None, params, device=0)
    opt = LevenbergMarquardtOptimizer(graph, initial, None, _iterative(LevenbergMarquardtParams(), "bj"), device=0)
    st = _lib.lmgpu_lm_state()
    ct.memmove(ct.byref(st), ct.byref(opt.state), ct.sizeof(st))
    assert opt.lib.lmgpu_dl_iterate(opt._h, ct.byref(st)) == _lib.LMGPU_INVALID
    # no fronts: marginals and the switch back to Cholesky are refused
    out = np.zeros((9, 9))
    assert opt.lib.lmgpu_marginal_covariance(opt._h, 0, out.ctypes.data_as(ct.POINTER(ct.c_double))) == _lib.LMGPU_INVALID
    assert opt.lib.lmgpu_set_linear_solver(opt._h, _lib.LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY, None) == _lib.LMGPU_INVALID
    assert opt.num_fronts() == 0
    assert opt.lib.lmgpu_get_front(opt._h, 0, None, None) == _lib.LMGPU_INVALID
    # no ordering given under ITERATIVE: Ordering.Natural
    assert list(opt.ordering) == list(Ordering.Natural(graph))


def test_gn_single_projection_point_is_indeterminate():
    """Under Gauss-Newton a point seen by ONE projection has a rank-2 3x3 block of J^T J: BlockJacobi's Cholesky fails and the solve
    returns LMGPU_INDETERMINATE with that point's slot (documented deviation: the reference carries Eigen's failed LLT on).  Camera at
    the identity, point on its optical axis: the point's Jacobian has an exactly zero third column, so the block is exactly singular.
    Under LM (lambda > 0) the same system is solved."""
    graph = NonlinearFactorGraph()
    initial = Values()
    K = (500.0, 500.0, 0.0, 320.0, 240.0)
    pose_noise = noiseModel.Diagonal.Sigmas([1e-3] * 6)
    px = noiseModel.Isotropic.Sigma(2, 1.0)
    initial.insert_pose3(X(0), np.eye(3), np.zeros(3))
    initial.insert_pose3(X(1), np.eye(3), np.array([1.0, 0.0, 0.0]))
    graph.add_PriorFactorPose3(X(0), np.eye(3), np.zeros(3), pose_noise)
    graph.add_PriorFactorPose3(X(1), np.eye(3), np.array([1.0, 0.0, 0.0]), pose_noise)
    initial.insert_point3(L(0), np.array([1.0, 0.5, 6.0]))  # seen twice: well determined
    graph.add_GenericProjectionFactor([405.0, 282.0], px, X(0), L(0), K)
    graph.add_GenericProjectionFactor([321.0, 281.0], px, X(1), L(0), K)
    initial.insert_point3(L(1), np.array([0.0, 0.0, 5.0]))  # seen once, on the optical axis of x0
    graph.add_GenericProjectionFactor([322.0, 239.0], px, X(0), L(1), K)
    params = _iterative(GaussNewtonParams(), "bj")
    opt = GaussNewtonOptimizer(graph, initial, None, params, device=0)
    slot = list(opt.ordering).index(L(1))
    assert slot != 0  # the slot reported is the failing variable's, not simply the first
    st = _lib.lmgpu_lm_state()
    ct.memmove(ct.byref(st), ct.byref(opt.state), ct.sizeof(st))
    values0 = opt.values()
    assert opt.lib.lmgpu_gn_iterate(opt._h, ct.byref(st)) == _lib.LMGPU_INDETERMINATE
    assert opt.lib.lmgpu_last_failed_slot(opt._h) == slot
    assert st.iterations == 0  # nothing was retracted
    v1 = opt.values()
    for k in initial.keys():
        assert np.array_equal(v1.at(k), values0.at(k))
    with pytest.raises(_lib.IndeterminantLinearSystemException) as ei:
        opt.iterate()
    assert ei.value.slot == slot
    # LM: lambda * I makes every block positive definite
    lm = LevenbergMarquardtOptimizer(graph, initial, None, _iterative(LevenbergMarquardtParams(), "bj"), device=0)
    lm.linearize()
    _, d, _, _ = lm.solve(1e-3)
    assert np.isfinite(d).all()


def test_beyond_the_direct_path():
    """20 000 cameras, 100 000 points, 1 M projections, random co-visibility: no fronts, < 3 GB of device memory, one LM iteration"""
    graph, initial, _, _ = make_bal(n_cam=20000, n_pt=100000, obs_per_point=10, seed=42)
    hip = ct.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ct.c_size_t(), ct.c_size_t()
        assert hip.hipMemGetInfo(ct.byref(f), ct.byref(t)) == 0
        return f.value

    _lib.load()
    assert hip.hipSetDevice(0) == 0
    free0 = free_bytes()
    params = _iterative(LevenbergMarquardtParams(), "bj")
    opt = LevenbergMarquardtOptimizer(graph, initial, None, params, device=0)
    free1 = free_bytes()
    assert opt.num_fronts() == 0
    assert free0 - free1 < 3 * 2**30, (free0 - free1) / 2**30
    e0 = opt.error()
    opt.iterate()
    st = opt.pcg_stats()
    free2 = free_bytes()  # the PCG working set (blocks, vectors, y, partials) is allocated at the first solve
    assert free0 - free2 < 3 * 2**30, (free0 - free2) / 2**30
    assert opt.error() < e0
    assert st["iterations"] <= 500 and (st["gamma"] <= st["threshold"] or st["iterations"] == 500)
    opt.close()
