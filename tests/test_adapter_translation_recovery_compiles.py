"""Type-check of the adapter's TranslationRecovery and MFAS replacements (include/lmgpu_gtsam_adapter.h: gtsam::GpuTranslationRecovery,
gtsam::GpuMFAS) against the reference's headers, like tests/test_adapter_init_pose3_compiles.py: a translation unit that calls them the way
tests/testTranslationRecovery.cpp and gtsam/sfm/tests/testMFAS.cpp call the originals.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
using namespace gtsam;

size_t useTranslationRecovery(const Values& initial) {
  std::vector<BinaryMeasurement<Unit3>> rel;
  rel.emplace_back(0, 1, Unit3(1, 0, 0), noiseModel::Isotropic::Sigma(3, 0.01));
  rel.emplace_back(1, 3, Unit3(-1, -1, 0), noiseModel::Robust::Create(noiseModel::mEstimator::Huber::Create(1.345), noiseModel::Isotropic::Sigma(3, 0.01)));
  std::vector<BinaryMeasurement<Point3>> between;
  between.emplace_back(0, 3, Point3(1, -1, 0), noiseModel::Isotropic::Sigma(3, 1e-2));
  GpuTranslationRecovery algorithm;
  const Values a = algorithm.run(rel, /*scale=*/3.0);
  const Values b = algorithm.run(rel, 0.0, between, initial);
  LevenbergMarquardtParams params;
  GpuTranslationRecovery seeded(params, false, 0);
  seeded.seed(7);
  const Ordering order(KeyVector{3, 1, 0});
  const Values c = seeded.run(rel, 3.0, {}, Values(), &order);
  const Point3 p = a.at<Point3>(3);
  return a.size() + b.size() + c.size() + static_cast<size_t>(p.x());
}

double useMFAS(const std::vector<BinaryMeasurement<Unit3>>& rel) {
  GpuMFAS one(rel, Unit3(0, 0, 1));
  const KeyVector ordering = one.computeOrdering();
  const std::map<GpuMFAS::KeyPair, double> w = one.computeOutlierWeights();
  std::map<GpuMFAS::KeyPair, double> edgeWeights;
  edgeWeights[{3, 2}] = 0.5;
  edgeWeights[{0, 1}] = 0.75;
  GpuMFAS given(edgeWeights);
  const std::vector<double> sums = GpuMFAS::outlierWeightSums(rel, {Unit3(1, 0, 0), Unit3(0, 1, 0)});
  return w.begin()->second + sums.front() + static_cast<double>(ordering.size() + given.computeOrdering().size());
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_translation_recovery_type_checks(tmp_path):
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
