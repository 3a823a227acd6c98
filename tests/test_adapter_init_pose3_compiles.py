"""Type-check of the adapter's InitializePose3 replacement (include/lmgpu_gtsam_adapter.h: gtsam::GpuInitializePose3) against the
reference's headers, like tests/test_adapter_header_compiles.py: a translation unit that calls it the way
examples/Pose3SLAMExample_initializePose3Chordal.cpp calls InitializePose3::initialize.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
using namespace gtsam;

size_t useInit(NonlinearFactorGraph& graph, const Values& guess) {
  graph.addPrior(Key(0), Pose3(), noiseModel::Diagonal::Variances((Vector(6) << 1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4).finished()));
  Values a = GpuInitializePose3::initialize(graph);
  Values b = GpuInitializePose3::initialize(graph, guess, true);
  Ordering order = Ordering::Natural(graph);
  Values c = GpuInitializePose3::initialize(graph, guess, false, &order, 0);
  Values r = GpuInitializePose3::initializeOrientations(graph);
  Values g = GpuInitializePose3::computeOrientationsGradient(graph, guess, 10, false);
  const Pose3 p = a.at<Pose3>(0);
  const Rot3 q = r.at<Rot3>(0);
  static_assert(LMGPU_INIT_POSE3_ANCHOR_KEY == 99999999ull, "kAnchorKey");
  return a.size() + b.size() + c.size() + g.size() + static_cast<size_t>(p.x() + q.yaw());
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_init_pose3_type_checks(tmp_path):
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
