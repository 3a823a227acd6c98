"""Type-check of the adapter's smart projection factor binding (include/lmgpu_gtsam_adapter.h: the graph conversion recognises
SmartProjectionPoseFactor<Cal3_S2>, gpuSmartPoints; include/lmgpu_adapter_core.hpp: Problem::addSmartFactor ...) against the reference's
headers, like tests/test_adapter_triangulation_compiles.py.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
using namespace gtsam;

double useSmart(const Values& initial, const Point2Vector& measured, const KeyVector& views) {
  SmartProjectionParams params(HESSIAN, ZERO_ON_DEGENERACY);
  params.setRankTolerance(1.0);
  params.setEnableEPI(true);
  params.setLandmarkDistanceThreshold(10.0);
  params.setDynamicOutlierRejectionThreshold(3.0);
  params.setRetriangulationThreshold(1e-3);
  std::shared_ptr<Cal3_S2> K(new Cal3_S2(1500, 1200, 0, 640, 480));
  auto factor = std::make_shared<SmartProjectionPoseFactor<Cal3_S2>>(noiseModel::Isotropic::Sigma(2, 0.1), K, params);
  factor->add(measured, views);
  NonlinearFactorGraph graph;
  graph.push_back(factor);
  graph.addPrior(views[0], initial.at<Pose3>(views[0]), noiseModel::Isotropic::Sigma(6, 0.1));
  GpuLevenbergMarquardtOptimizer lm(graph, initial);
  const Values& r = lm.optimize();
  std::vector<TriangulationResult> pts = lm.gpuSmartPoints();
  double e = r.size() + pts.size() + (pts[0].valid() ? pts[0]->x() : 0.0) + factor->point().valid();
  GpuGaussNewtonOptimizer gn(graph, initial);
  gn.iterate();
  e += gn.gpuSmartPoints().size();
  const lmgpu_smart_params c = lmgpu_detail::toC(params);
  e += c.retriangulationThreshold + c.triangulation.enableEPI;
  lmgpu_adapter::Problem p(-1);
  p.setVariables({1, 2}, {LMGPU_POSE3, LMGPU_POSE3});
  const double K5[5] = {1500, 1200, 0, 640, 480};
  p.addSmartFactor(0, {1, 2}, {1.0, 2.0, 3.0, 4.0}, K5, 10.0, c);
  p.finalize();
  int32_t m = 0;
  e += p.numSmartFactors() + p.smartGraphIndices().size() + p.smartHessian(0, &m).size() + p.smartStats().n_factors;
  p.smartReset();
  return e;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_smart_type_checks(tmp_path):
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
