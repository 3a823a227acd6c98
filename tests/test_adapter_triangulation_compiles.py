"""Type-check of the adapter's triangulation binding (include/lmgpu_gtsam_adapter.h: gpuTriangulateSafe and its batched overload;
include/lmgpu_adapter_core.hpp: TriangulationBatch) against the reference's headers, like tests/test_adapter_ncg_compiles.py.  Nothing is
linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
using namespace gtsam;

double useTriangulation(const CameraSet<PinholeCamera<Cal3Bundler>>& bundler, const CameraSet<PinholeCamera<Cal3_S2>>& s2,
                        const Point2Vector& measured) {
  TriangulationParameters params(1.0, true, 10.0, 5.0, false, noiseModel::Isotropic::Sigma(2, 0.5));
  TriangulationResult a = gpuTriangulateSafe(bundler, measured, params);
  TriangulationResult b = gpuTriangulateSafe(s2, measured, TriangulationParameters(), 0);
  double e = a.valid() ? a->x() : 0.0;
  e += b.farPoint() + b.outlier() + b.degenerate() + b.behindCamera() + static_cast<int>(b.status);
  std::vector<CameraSet<PinholeCamera<Cal3_S2>>> sets{s2, s2};
  std::vector<Point2Vector> zs{measured, measured};
  std::vector<TriangulationResult> many = gpuTriangulateSafe(sets, zs, params);
  e += many.size();
  TriangulationResult ref = triangulateSafe(s2, measured, params);  // the reference's own call has the same shape
  e += ref.valid();
  lmgpu_adapter::TriangulationBatch batch(1);
  const double pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  batch.addObservation(batch.addS2Camera(pose, 500, 500, 0, 320, 240), 1.0, 2.0);
  batch.addObservation(batch.addBundlerCamera(pose, 500, 0, 0, 320, 240), 1.0, 2.0);
  batch.endLandmark();
  std::vector<double> points;
  std::vector<int32_t> status;
  batch.run(0, lmgpu_triangulation_params{1.0, 0, 0, -1.0, -1.0, 0.0}, &points, &status);
  lmgpu_triangulation_stats st{};
  e += lmgpu_get_triangulation_stats(nullptr, &st) + lmgpu_num_points3(nullptr);
  return e + points.size() + status.size() + batch.numLandmarks();
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_triangulation_type_checks(tmp_path):
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
