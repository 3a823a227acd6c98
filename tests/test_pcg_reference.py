"""CPU checks of the PCG feature: the numpy restatement (tests/pcg_restatement.py) against the reference's own known answers and
against the frozen oracle's direct solve; the exported C ABI; the Python parameter objects (no device needed)."""
import ctypes as ct
import os

import numpy as np
import pytest

import oracle_harness as oh
import pcg_restatement as pr
from gtsam_personal_amd import (BlockJacobiPreconditionerParameters, DoglegOptimizer, DoglegParams, DummyPreconditionerParameters,
                                GaussNewtonParams, LevenbergMarquardtOptimizer, LevenbergMarquardtParams, Ordering, PCGSolverParameters)
from gtsam_personal_amd.datasets import SfmData, bal_graph
from gtsam_personal_amd.graph import VAR_DIM

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gtsam_personal_amd", "liblmgpu.so")


def _simple_gfg():
    """tests/testPCGSolver.cpp:82-95 / testPreconditioner.cpp:92-101: seven factors on keys 0, 1, 2, Diagonal::Sigmas(0.5, 0.3)"""
    w = np.array([1 / 0.5, 1 / 0.3])
    I2 = np.eye(2)
    raw = [([2], [10 * I2], [-1, -1]), ([2, 0], [-10 * I2, 10 * I2], [2, -1]), ([2, 1], [-5 * I2, 5 * I2], [0, 1]),
           ([0, 1], [-5 * I2, 5 * I2], [-1, 1.5]), ([0], [I2], [0, 0]), ([1], [I2], [0, 0]), ([2], [I2], [0, 0])]
    return [(k, [w[:, None] * A for A in As], w * np.array(b, dtype=float)) for k, As, b in raw], {0: 2, 1: 2, 2: 2}


def test_restatement_multiply_getb():
    """testPCGSolver.cpp:82-120: expectedAp and expectedb of the first iteration"""
    facs, dims = _simple_gfg()
    s = pr.System(facs, dims)
    P = pr.Preconditioner(s, pr.DUMMY)
    r = s.residual(np.zeros(6))
    p = P.transposeSolve(P.solve(r))
    Ap = s.multiply(p)
    assert np.allclose(Ap, [100400, -249074.074, -2080, 148148.148, -146480, 37962.963], atol=1e-3)
    assert np.allclose(s.getb(), [100.0, -194.444, -20.0, 138.889, -120.0, -55.556], atol=1e-3)


@pytest.mark.parametrize("kind", [pr.DUMMY, pr.BLOCK_JACOBI])
def test_restatement_very_simple_system(kind):
    """testPreconditioner.cpp:32-79: [4 1; 1 3] x = [1 2], eps 0, x = [1/11, 7/11]"""
    s = pr.System([([0], [np.array([[4.0, 1.0], [1.0, 3.0]])], [1.0, 2.0])], {0: 2})
    x, _, _, _ = pr.pcg(s, pr.PCGParams(maxIterations=500 if kind == pr.DUMMY else 1500, epsilon_rel=0.0, epsilon_abs=0.0, preconditioner=kind))
    assert np.allclose(x, [1 / 11, 7 / 11], atol=1e-7 if kind == pr.DUMMY else 1e-5)


@pytest.mark.parametrize("kind", [pr.DUMMY, pr.BLOCK_JACOBI])
def test_restatement_simple_system(kind):
    """testPreconditioner.cpp:82-126: the seven-factor graph, eps 0, to 1e-5"""
    facs, dims = _simple_gfg()
    s = pr.System(facs, dims)
    x, _, _, _ = pr.pcg(s, pr.PCGParams(maxIterations=500, epsilon_rel=0.0, epsilon_abs=0.0, preconditioner=kind))
    xk = pr.by_key(s, x)
    assert np.allclose(xk[0], [0.100498, -0.196756], atol=1e-5)
    assert np.allclose(xk[1], [-0.0973252, 0.100582], atol=1e-5)
    assert np.allclose(xk[2], [-0.0990413, -0.0980577], atol=1e-5)


@pytest.mark.parametrize("kind", [pr.DUMMY, pr.BLOCK_JACOBI])
def test_restatement_equals_oracle_direct_solve(kind):
    """dubrovnik linearized by the oracle; the restatement with eps 1e-14 is the oracle's damped direct solve to 1e-9"""
    graph, initial = bal_graph(SfmData.FromBalFile(os.path.join(GOLD, "dubrovnik-3-7-pre.txt")))
    orc = oh.OracleProblem(graph, initial, Ordering.Natural(graph))
    orc.linearize()
    fkeys = graph.factor_keys_in_graph_order()
    facs, dims = [], {}
    for g in range(graph.size()):
        J = orc.jacobian(g)
        keys = [int(k) for k in fkeys[g]]
        d = [VAR_DIM[initial.type(k)] for k in keys]
        off = np.concatenate([[0], np.cumsum(d)]).astype(int)
        facs.append((keys, [J[:, off[i]:off[i + 1]] for i in range(len(keys))], J[:, -1]))
        for k, dk in zip(keys, d):
            dims[k] = dk
    lam = 1e-3
    s = pr.System(facs, dims, damping={k: lam * np.ones(dims[k]) for k in dims})
    x, iters, _, _ = pr.pcg(s, pr.PCGParams(maxIterations=20000, epsilon_rel=1e-14, epsilon_abs=1e-28, preconditioner=kind))
    rc, ref, _, _ = orc.solve(lam)
    assert rc == 0
    xk = pr.by_key(s, x)
    a = np.concatenate([xk[k] for k in sorted(ref)])
    b = np.concatenate([ref[k] for k in sorted(ref)])
    assert np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(b), (np.linalg.norm(a - b) / np.linalg.norm(b), iters)


def test_pcg_symbols_exported():
    lib = ct.CDLL(LIB)
    for name in ("lmgpu_set_linear_solver", "lmgpu_get_pcg_stats"):
        assert hasattr(lib, name), name


def test_python_parameter_defaults():
    """ConjugateGradientSolver.h:46-50 and PCGSolver.h:42-46"""
    p = PCGSolverParameters()
    assert (p.minIterations, p.maxIterations, p.reset, p.epsilon_rel, p.epsilon_abs) == (1, 500, 501, 1e-3, 1e-3)
    assert p.preconditioner is None
    assert isinstance(PCGSolverParameters(BlockJacobiPreconditionerParameters()).preconditioner, BlockJacobiPreconditionerParameters)
    lm = LevenbergMarquardtParams()
    assert lm.linearSolverType == "MULTIFRONTAL_CHOLESKY" and lm.iterativeParams is None and not lm.isIterative()
    gn = GaussNewtonParams()
    assert gn.linearSolverType == "MULTIFRONTAL_CHOLESKY" and gn.iterativeParams is None


def test_iterative_without_params_raises_before_any_handle():
    """NonlinearOptimizer.cpp:156-158 / :166-169: raised before the library is asked for a device"""
    graph, initial = bal_graph(SfmData.FromBalFile(os.path.join(GOLD, "dubrovnik-3-7-pre.txt")))
    p = LevenbergMarquardtParams()
    p.linearSolverType = "ITERATIVE"
    with pytest.raises(RuntimeError, match="cg parameter has to be assigned"):
        LevenbergMarquardtOptimizer(graph, initial, None, p, device=0)
    p.iterativeParams = object()
    with pytest.raises(RuntimeError, match="special cg parameter type"):
        LevenbergMarquardtOptimizer(graph, initial, None, p, device=0)
    p.iterativeParams = PCGSolverParameters()  # no preconditioner: createPreconditioner throws
    with pytest.raises(ValueError, match="createPreconditioner"):
        LevenbergMarquardtOptimizer(graph, initial, None, p, device=0)
    d = DoglegParams()
    d.linearSolverType = "ITERATIVE"
    d.iterativeParams = PCGSolverParameters(DummyPreconditionerParameters())
    with pytest.raises(RuntimeError, match="Dogleg"):
        DoglegOptimizer(graph, initial, None, d, device=0)
