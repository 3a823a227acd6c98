"""Type-check of the adapter's iterative-solver mapping (include/lmgpu_gtsam_adapter.h: lmgpu_detail::toPcg, the optimizers'
constructors) against the reference's headers, like tests/test_adapter_header_compiles.py: a translation unit that selects
linearSolverType = Iterative with PCGSolverParameters for LM and Gauss-Newton, and asks Dogleg for it.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
using namespace gtsam;

double usePcg(const NonlinearFactorGraph& graph, const Values& initial) {
  LevenbergMarquardtParams lp;
  lp.linearSolverType = NonlinearOptimizerParams::Iterative;
  lp.iterativeParams = std::make_shared<PCGSolverParameters>(std::make_shared<BlockJacobiPreconditionerParameters>());
  GpuLevenbergMarquardtOptimizer lm(graph, initial, lp);
  double e = lm.optimize().size();
  GaussNewtonParams gp;
  gp.linearSolverType = NonlinearOptimizerParams::Iterative;
  gp.iterativeParams = std::make_shared<PCGSolverParameters>(std::make_shared<DummyPreconditionerParameters>());
  GpuGaussNewtonOptimizer gn(graph, initial, gp);
  e += gn.iterate()->size();
  lmgpu_pcg_params c{};
  e += lmgpu_detail::toPcg(lp, &c) ? c.maxIterations : 0;
  DoglegParams dp;
  dp.linearSolverType = NonlinearOptimizerParams::Iterative;
  try {
    GpuDoglegOptimizer dl(graph, initial, dp);
  } catch (const std::invalid_argument&) {
    e += 1;
  }
  lmgpu_adapter::Problem p(-1);
  p.set_linear_solver(LMGPU_SOLVER_PCG, &c);
  return e;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_pcg_mapping_type_checks(tmp_path):
    (tmp_path / "gtsam").mkdir()
    (tmp_path / "gtsam" / "config.h").write_text(CONFIG_H)
    (tmp_path / "gtsam" / "dllexport.h").write_text(DLLEXPORT_H)
    (tmp_path / "tu.cpp").write_text(TU)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-deprecated-copy",
           f"-I{tmp_path}", f"-I{ROOT}/include", f"-I{REF}", f"-I{REF}/gtsam/3rdparty/Eigen",
           f"-I{REF}/gtsam/3rdparty/CCOLAMD/Include", f"-I{REF}/gtsam/3rdparty/SuiteSparse_config", str(tmp_path / "tu.cpp")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    ours = [ln for ln in r.stdout.splitlines() if "lmgpu_" in ln and ("error" in ln or "warning" in ln)]
    assert r.returncode == 0, r.stdout[-6000:]
    assert not ours, "\n".join(ours)
