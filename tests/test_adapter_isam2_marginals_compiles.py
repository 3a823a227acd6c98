"""Type-check of the adapter's ISAM2 marginals binding (include/lmgpu_gtsam_adapter.h: GpuISAM2::marginalCovariances /
jointMarginalCovariance / crossCovariance, returning the GpuJointMarginal GpuMarginals returns) against the reference's headers, like
tests/test_adapter_joint_marginals_compiles.py.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
#include <gtsam/nonlinear/ISAM2.h>
#include <gtsam/nonlinear/Marginals.h>
using namespace gtsam;

double useIsam2Marginals(const NonlinearFactorGraph& newFactors, const Values& newTheta, Key a, Key b, const KeyVector& many) {
  GpuISAM2 gpu;
  gpu.update(newFactors, newTheta);
  Matrix one = gpu.marginalCovariance(a);  // the single-key entry stays
  std::vector<Matrix> blocks = gpu.marginalCovariances(many);
  GpuJointMarginal joint = gpu.jointMarginalCovariance(many);
  Matrix cross = gpu.crossCovariance(a, b);
  // what a user of the reference writes instead: the graph refactored at the linearization point (tests/testGaussianISAM2.cpp:983)
  ISAM2 ref;
  ref.update(newFactors, newTheta);
  Marginals refactored(ref.getFactorsUnsafe(), ref.getLinearizationPoint());
  JointMarginal want = refactored.jointMarginalCovariance(many);
  Matrix wantOne = ref.marginalCovariance(a);
  Matrix blockAt = joint.at(a, b), blockCall = joint(a, b);
  double e = (blockAt - Matrix(want.at(a, b))).norm() + (blockCall - Matrix(want(a, b))).norm() + (joint.fullMatrix() - want.fullMatrix()).norm();
  e += (one - wantOne).norm() + (blocks.front() - one).norm() + (cross - blockAt).norm() + joint.keys().size();
  const lmgpu_marginals_stats st = gpu.marginalsStats();
  e += st.launches + st.chunks + st.cross_launches + st.cross_chunks + st.cross_walks + st.cross_targets + st.factorizations;
  return e;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_isam2_marginals_type_checks(tmp_path):
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
