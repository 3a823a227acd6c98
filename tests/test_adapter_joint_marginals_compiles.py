"""Type-check of the adapter's joint-marginals binding (include/lmgpu_gtsam_adapter.h: GpuMarginals::jointMarginalCovariance /
jointMarginalInformation / crossCovariance, GpuJointMarginal; include/lmgpu_adapter_core.hpp: Problem::jointMarginalCovariance /
marginalCrossCovariances) against the reference's headers, like tests/test_adapter_marginals_compiles.py.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
#include <gtsam/nonlinear/Marginals.h>
using namespace gtsam;

double useJointMarginals(const NonlinearFactorGraph& graph, const Values& solution, const Ordering& ordering, Key a, Key b, const KeyVector& many) {
  GpuMarginals gpu(graph, solution, ordering);
  GpuJointMarginal joint = gpu.jointMarginalCovariance(many);
  GpuJointMarginal info = gpu.jointMarginalInformation(KeyVector{a, b});
  Matrix cross = gpu.crossCovariance(a, b);
  Marginals ref(graph, solution, ordering);  // the reference's own calls have the same shape
  JointMarginal want = ref.jointMarginalCovariance(many);
  JointMarginal wantInfo = ref.jointMarginalInformation(KeyVector{a, b});
  Matrix blockAt = joint.at(a, b), blockCall = joint(a, b);
  double e = (blockAt - Matrix(want.at(a, b))).norm() + (blockCall - Matrix(want(a, b))).norm() + (joint.fullMatrix() - want.fullMatrix()).norm();
  e += (info.fullMatrix() - wantInfo.fullMatrix()).norm() + (cross - blockAt).norm() + joint.keys().size();
  const lmgpu_marginals_stats st = gpu.stats();
  e += st.cross_launches + st.cross_chunks + st.cross_walks + st.cross_targets + st.cross_lds + st.cross_scratch + st.longest_union + st.cross_cap;
  lmgpu_adapter::Problem p(-1);
  std::vector<double> packed = p.jointMarginalCovariance(std::vector<int32_t>{0, 1});
  std::vector<double> blocks = p.marginalCrossCovariances(std::vector<int32_t>{0, 1}, std::vector<int32_t>{1, 1});
  e += packed.size() + blocks.size();
  e += lmgpu_marginals_junction(p.handle(), 0, 1) + lmgpu_set_marginals_cross_cap(p.handle(), 0);
  return e;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_joint_marginals_type_checks(tmp_path):
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
