"""Type-check of the adapter's nonlinear conjugate gradient binding (include/lmgpu_gtsam_adapter.h:
GpuNonlinearConjugateGradientOptimizer; include/lmgpu_adapter_core.hpp: ncgIterate / ncgOptimize) against the reference's headers,
like tests/test_adapter_pcg_compiles.py.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
using namespace gtsam;

double useNcg(const NonlinearFactorGraph& graph, const Values& initial) {
  NonlinearOptimizerParams param;
  param.maxIterations = 500;
  GpuNonlinearConjugateGradientOptimizer cg(graph, initial, param);
  double e = cg.optimize().size();
  GpuNonlinearConjugateGradientOptimizer dy(graph, initial, param, DirectionMethod::DaiYuan, 0);
  GaussianFactorGraph::shared_ptr none = dy.iterate();
  e += none ? 1 : 0;
  e += dy.error() + dy.iterations();
  NonlinearConjugateGradientOptimizer& base = dy;  // a subclass of the reference's class
  e += base.values().size();
  param.linearSolverType = NonlinearOptimizerParams::Iterative;
  param.iterativeParams = std::make_shared<PCGSolverParameters>(std::make_shared<BlockJacobiPreconditionerParameters>());
  GpuNonlinearConjugateGradientOptimizer nofronts(graph, initial, param, DirectionMethod::FletcherReeves);
  e += nofronts.optimize().size();
  lmgpu_adapter::Problem p(-1);
  lmgpu_ncg_params c{LMGPU_NCG_HESTENES_STIEFEL, 0, 100, 1e-5, 1e-5, 0.0};
  lmgpu_lm_state st{};
  p.ncgIterate(c, &st);
  p.ncgOptimize(c, &st);
  return e;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_ncg_type_checks(tmp_path):
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
