"""Type-check of the adapter's marginals binding (include/lmgpu_gtsam_adapter.h: GpuMarginals; include/lmgpu_adapter_core.hpp:
Problem::marginalsFactor / marginalCovariances / marginalsStats) against the reference's headers, like
tests/test_adapter_triangulation_compiles.py.  Nothing is linked or run."""
import os
import shutil
import subprocess

import pytest

from test_adapter_header_compiles import CONFIG_H, DLLEXPORT_H, REF, ROOT

TU = r"""
#include "lmgpu_gtsam_adapter.h"
#include <gtsam/nonlinear/Marginals.h>
using namespace gtsam;

double useMarginals(const NonlinearFactorGraph& graph, const Values& solution, const Ordering& ordering, Key one, const KeyVector& many) {
  GpuMarginals gpu(graph, solution, ordering);
  Matrix cov = gpu.marginalCovariance(one);
  Matrix info = gpu.marginalInformation(one);
  std::vector<Matrix> all = gpu.marginalCovariances(many);
  const lmgpu_marginals_stats st = gpu.stats();
  Marginals ref(graph, solution, ordering);  // the reference's own calls have the same shape
  Matrix want = ref.marginalCovariance(one);
  double e = (cov - want).norm() + (info - ref.marginalInformation(one)).norm() + all.size();
  e += st.launches + st.chunks + st.factorizations + st.vars_lds + st.vars_scratch + st.scratch_bytes + st.longest_path + st.lds_capacity;
  lmgpu_adapter::Problem p(-1);
  p.marginalsFactor();
  std::vector<double> packed = p.marginalCovariances(std::vector<int32_t>{0, 0});
  e += packed.size() + p.marginalsStats().launches;
  int32_t fronts[4], poff = 0, spos[4];
  e += lmgpu_marginals_path(p.handle(), 0, fronts, 4) + lmgpu_marginals_front_offsets(p.handle(), 0, &poff, spos, 4);
  e += lmgpu_set_marginals_params(p.handle(), int64_t(1) << 20, 0);
  return e;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gtsam", "nonlinear")), reason="reference headers not present (GPU box)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_marginals_type_checks(tmp_path):
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
