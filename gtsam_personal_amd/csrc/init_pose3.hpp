// InitializePose3 on the device (gtsam/slam/InitializePose3.cpp, InitializePose.h): host side of the lmgpu_init_pose3_* group.
// Included by lmgpu.hip after the handle's own entry points: the two inner handles are driven through the public C ABI, and the
// kernels of kernels_init_pose3.hpp read / write their device vectors (the solve's step, the pose values) in place.
#pragma once

#include "kernels_init_pose3.hpp"

struct lmgpu_init_pose3 {
  lmgpu_config cfg{};
  std::string err;
  struct Fac {
    int32_t graph_index;
    bool prior;
    uint64_t k0, k1;  // prior: k0 = anchor
    double meas[12];
    int32_t noise_kind;
    double noise[36];
  };
  std::vector<Fac> facs;  // as added
  bool finalized = false;
  // after finalize
  std::vector<uint64_t> slot_keys;  // by slot, anchor included
  std::vector<int32_t> out_slot;    // result position -> slot (ordering without the anchor)
  int anchor = -1, anchor_deg = 0, n_fac = 0;
  lmgpu_handle* hO = nullptr;
  lmgpu_handle* hP = nullptr;
  double* d_R = nullptr;     // [slots][9] rotations of the last orientation call
  double* d_buf[2] = {};     // gradient mode: inverse rotations, two buffers
  double* d_part[2] = {};
  double* d_Rij = nullptr;
  int32_t *d_ptr = nullptr, *d_other = nullptr, *d_edge = nullptr;
  int8_t* d_pos = nullptr;
  GradCtl* d_ctl = nullptr;
  GradCtl* h_ctl = nullptr;  // pinned
  int max_deg = 0;
  bool have_R = false;
};

#define IPCHECK(expr)                                                  \
  do {                                                                 \
    hipError_t _e = (expr);                                            \
    if (_e != hipSuccess) {                                            \
      ip->err = std::string(#expr) + ": " + hipGetErrorString(_e);     \
      return LMGPU_HIP_ERROR;                                          \
    }                                                                  \
  } while (0)

namespace {

void ip_release(lmgpu_init_pose3* ip) {
  if (ip->hO) lmgpu_destroy(ip->hO);
  if (ip->hP) lmgpu_destroy(ip->hP);
  ip->hO = ip->hP = nullptr;
  void* ptrs[] = {ip->d_R, ip->d_buf[0], ip->d_buf[1], ip->d_part[0], ip->d_part[1], ip->d_Rij, ip->d_ptr, ip->d_other, ip->d_edge, ip->d_pos, ip->d_ctl};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (ip->h_ctl) (void)hipHostFree(ip->h_ctl);
  ip->d_R = ip->d_buf[0] = ip->d_buf[1] = ip->d_part[0] = ip->d_part[1] = ip->d_Rij = nullptr;
  ip->d_ptr = ip->d_other = ip->d_edge = nullptr;
  ip->d_pos = nullptr;
  ip->d_ctl = ip->h_ctl = nullptr;
  ip->finalized = false;
  ip->have_R = false;
}

int ip_inner(lmgpu_init_pose3* ip, lmgpu_handle* h, int rc) {
  if (rc != LMGPU_OK) ip->err = std::string("inner handle: ") + lmgpu_last_error(h);
  return rc;
}

template <class T>
int ip_upload(lmgpu_init_pose3* ip, T** dst, const std::vector<T>& src) {
  IPCHECK(hipMalloc((void**)dst, std::max<size_t>(1, src.size()) * sizeof(T)));
  if (!src.empty()) IPCHECK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return LMGPU_OK;
}

int ip_ready(lmgpu_init_pose3* ip, const char* who) {
  if (!ip) return LMGPU_INVALID;
  if (!ip->finalized) {
    ip->err = std::string(who) + ": refused (lmgpu_init_pose3_finalize has not succeeded)";
    return LMGPU_INVALID;
  }
  IPCHECK(hipSetDevice(ip->cfg.device));
  return LMGPU_OK;
}

// results leave in the order of the ordering without the anchor
int ip_download(lmgpu_init_pose3* ip, const double* dev, int per, double* out) {
  const int ns = (int)ip->slot_keys.size();
  std::vector<double> buf((size_t)ns * per);
  IPCHECK(hipMemcpy(buf.data(), dev, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < ip->out_slot.size(); i++) std::memcpy(out + i * per, &buf[(size_t)ip->out_slot[i] * per], per * sizeof(double));
  return LMGPU_OK;
}

}  // namespace

extern "C" {

int lmgpu_init_pose3_create(const lmgpu_config* cfg, lmgpu_init_pose3** out) {
  if (!cfg || !out || cfg->world_size > 1 || cfg->device < 0) return LMGPU_INVALID;
  lmgpu_init_pose3* ip = new lmgpu_init_pose3();
  ip->cfg = *cfg;
  ip->cfg.rank = 0;
  ip->cfg.world_size = 1;
  ip->cfg.flags = 0;
  *out = ip;
  return LMGPU_OK;
}

int lmgpu_init_pose3_destroy(lmgpu_init_pose3* ip) {
  if (!ip) return LMGPU_INVALID;
  ip_release(ip);
  delete ip;
  return LMGPU_OK;
}

const char* lmgpu_init_pose3_last_error(const lmgpu_init_pose3* ip) { return ip ? ip->err.c_str() : "null object"; }

int lmgpu_init_pose3_add_factors(lmgpu_init_pose3* ip, int32_t factor_type, int32_t n, const int32_t* graph_index, const uint64_t* keys,
                                 const double* meas, int32_t noise_kind, const double* noise) {
  if (!ip) return LMGPU_INVALID;
  if (factor_type < 0 || factor_type >= LMGPU_NUM_FACTOR_TYPES || n < 0 ||
      (noise_kind != LMGPU_N_UNIT && noise_kind != LMGPU_N_DIAG && noise_kind != LMGPU_N_GAUSS)) {
    ip->err = "lmgpu_init_pose3_add_factors: bad factor type, count or noise kind";
    return LMGPU_INVALID;
  }
  if (factor_type != LMGPU_F_BETWEEN_POSE3 && factor_type != LMGPU_F_PRIOR_POSE3) return LMGPU_OK;  // buildPoseGraph drops it silently
  if (n == 0) return LMGPU_OK;
  if (!graph_index || !keys || !meas || (noise_kind != LMGPU_N_UNIT && !noise)) {
    ip->err = "lmgpu_init_pose3_add_factors: null array";
    return LMGPU_INVALID;
  }
  const bool prior = factor_type == LMGPU_F_PRIOR_POSE3;
  const int nl = factor_noise_doubles(factor_type, noise_kind);
  for (int i = 0; i < n; i++) {
    lmgpu_init_pose3::Fac f{};
    f.graph_index = graph_index[i];
    f.prior = prior;
    f.k0 = prior ? (uint64_t)LMGPU_INIT_POSE3_ANCHOR_KEY : keys[2 * i];
    f.k1 = prior ? keys[i] : keys[2 * i + 1];
    std::memcpy(f.meas, meas + (size_t)i * 12, 12 * sizeof(double));
    f.noise_kind = noise_kind;
    if (nl) std::memcpy(f.noise, noise + (size_t)i * nl, nl * sizeof(double));
    ip->facs.push_back(f);
  }
  if (ip->finalized) ip_release(ip);  // the graph changed: the handles are rebuilt by the next finalize
  return LMGPU_OK;
}

int lmgpu_init_pose3_finalize(lmgpu_init_pose3* ip, int32_t n_order, const uint64_t* ordering) {
  if (!ip) return LMGPU_INVALID;
  if (n_order <= 0 || !ordering) {
    ip->err = "lmgpu_init_pose3_finalize: empty ordering";
    return LMGPU_INVALID;
  }
  // ---- checks first: nothing changes on a refusal
  const uint64_t AK = LMGPU_INIT_POSE3_ANCHOR_KEY;
  int n_between = 0;
  for (const auto& f : ip->facs) n_between += f.prior ? 0 : 1;
  if (n_between == 0) {
    ip->err = "lmgpu_init_pose3_finalize: the graph has no BetweenFactor<Pose3>";
    return LMGPU_INVALID;
  }
  std::vector<uint64_t> slot_keys(ordering, ordering + n_order);
  if (std::find(slot_keys.begin(), slot_keys.end(), AK) == slot_keys.end()) slot_keys.push_back(AK);
  std::map<uint64_t, int> slot_of;
  for (size_t s = 0; s < slot_keys.size(); s++)
    if (!slot_of.emplace(slot_keys[s], (int)s).second) {
      ip->err = "lmgpu_init_pose3_finalize: duplicate key in the ordering";
      return LMGPU_INVALID;
    }
  std::vector<int> deg(slot_keys.size(), 0);
  std::vector<lmgpu_init_pose3::Fac> facs = ip->facs;
  std::stable_sort(facs.begin(), facs.end(), [](const lmgpu_init_pose3::Fac& a, const lmgpu_init_pose3::Fac& b) { return a.graph_index < b.graph_index; });
  for (size_t i = 0; i < facs.size(); i++) {
    if (i > 0 && facs[i].graph_index == facs[i - 1].graph_index) {
      ip->err = "lmgpu_init_pose3_finalize: duplicate graph_index";
      return LMGPU_INVALID;
    }
    for (uint64_t k : {facs[i].k0, facs[i].k1}) {
      auto it = slot_of.find(k);
      if (it == slot_of.end()) {
        ip->err = "lmgpu_init_pose3_finalize: a factor's key is not in the ordering";
        return LMGPU_INVALID;
      }
      deg[it->second]++;
    }
  }
  const int anchor = slot_of.at(AK);
  for (size_t s = 0; s < slot_keys.size(); s++)
    if ((int)s != anchor && deg[s] == 0) {
      ip->err = "lmgpu_init_pose3_finalize: a variable of the ordering has no factor in the extracted pose graph";
      return LMGPU_INVALID;
    }
  // ---- build
  ip_release(ip);
  IPCHECK(hipSetDevice(ip->cfg.device));
  const int ns = (int)slot_keys.size(), m = (int)facs.size();
  ip->slot_keys = slot_keys;
  ip->anchor = anchor;
  ip->n_fac = m;
  ip->out_slot.clear();
  for (int s = 0; s < ns; s++)
    if (s != anchor) ip->out_slot.push_back(s);
  ip->anchor_deg = deg[anchor];
  int rc;
  auto fail = [&](int code) {
    const std::string keep = ip->err;
    ip_release(ip);
    ip->err = keep;
    return code;
  };
  // orientation handle: buildLinearOrientationGraph (InitializePose3.cpp:37-71)
  {
    if ((rc = lmgpu_create(&ip->cfg, &ip->hO))) return fail(rc);
    std::vector<int32_t> types(ns, LMGPU_VEC9);
    if ((rc = ip_inner(ip, ip->hO, lmgpu_set_variables(ip->hO, ns, slot_keys.data(), types.data())))) return fail(rc);
    std::vector<int32_t> gi(m), slots(2 * (size_t)m);
    std::vector<double> meas(9 * (size_t)m), noise(9 * (size_t)m);
    for (int i = 0; i < m; i++) {
      gi[i] = i;
      slots[2 * i] = slot_of.at(facs[i].k0);
      slots[2 * i + 1] = slot_of.at(facs[i].k1);
      std::memcpy(&meas[9 * (size_t)i], facs[i].meas, 9 * sizeof(double));
      // rotationPrecision = whitenInPlace(e1)[0] (:48-51); Isotropic::Precision(9, p) whitens with sqrt(p)
      const double p = facs[i].noise_kind == LMGPU_N_UNIT ? 1.0 : facs[i].noise[0];
      for (int r = 0; r < 9; r++) noise[9 * (size_t)i + r] = std::sqrt(p);
    }
    if ((rc = ip_inner(ip, ip->hO, lmgpu_add_factor_bucket(ip->hO, LMGPU_F_CHORDAL_BETWEEN, m, gi.data(), slots.data(), meas.data(), LMGPU_N_DIAG, noise.data()))))
      return fail(rc);
    const int32_t pgi = m, pslot = anchor;
    const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if ((rc = ip_inner(ip, ip->hO, lmgpu_add_factor_bucket(ip->hO, LMGPU_F_PRIOR_VEC9, 1, &pgi, &pslot, I9, LMGPU_N_UNIT, nullptr)))) return fail(rc);
    if ((rc = ip_inner(ip, ip->hO, lmgpu_finalize_structure(ip->hO)))) return fail(rc);
    std::vector<double> zeros(9 * (size_t)ns, 0.0);
    if ((rc = ip_inner(ip, ip->hO, lmgpu_set_values(ip->hO, zeros.data())))) return fail(rc);
  }
  // pose handle: the extracted pose graph + PriorFactor<Pose3>(kAnchorKey, Pose3(), Unit(6)) (InitializePose.h:72-75)
  {
    if ((rc = lmgpu_create(&ip->cfg, &ip->hP))) return fail(rc);
    std::vector<int32_t> types(ns, LMGPU_POSE3);
    if ((rc = ip_inner(ip, ip->hP, lmgpu_set_variables(ip->hP, ns, slot_keys.data(), types.data())))) return fail(rc);
    for (int kind : {LMGPU_N_UNIT, LMGPU_N_DIAG, LMGPU_N_GAUSS}) {
      const int nl = factor_noise_doubles(LMGPU_F_BETWEEN_POSE3, kind);
      std::vector<int32_t> gi, slots;
      std::vector<double> meas, noise;
      for (int i = 0; i < m; i++) {
        if (facs[i].noise_kind != kind) continue;
        gi.push_back(i);
        slots.push_back(slot_of.at(facs[i].k0));
        slots.push_back(slot_of.at(facs[i].k1));
        meas.insert(meas.end(), facs[i].meas, facs[i].meas + 12);
        noise.insert(noise.end(), facs[i].noise, facs[i].noise + nl);
      }
      if (gi.empty()) continue;
      if ((rc = ip_inner(ip, ip->hP, lmgpu_add_factor_bucket(ip->hP, LMGPU_F_BETWEEN_POSE3, (int)gi.size(), gi.data(), slots.data(), meas.data(), kind,
                                                             nl ? noise.data() : nullptr))))
        return fail(rc);
    }
    const int32_t pgi = m, pslot = anchor;
    const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    if ((rc = ip_inner(ip, ip->hP, lmgpu_add_factor_bucket(ip->hP, LMGPU_F_PRIOR_POSE3, 1, &pgi, &pslot, I12, LMGPU_N_UNIT, nullptr)))) return fail(rc);
    if ((rc = ip_inner(ip, ip->hP, lmgpu_finalize_structure(ip->hP)))) return fail(rc);
  }
  // gradient mode: createSymbolicGraph (:221-253) as CSR, edges of a node in factor-index order
  {
    std::vector<std::vector<int>> adj(ns);
    for (int i = 0; i < m; i++) {
      adj[slot_of.at(facs[i].k0)].push_back(i);
      if (facs[i].k1 != facs[i].k0) adj[slot_of.at(facs[i].k1)].push_back(i);
    }
    std::vector<int32_t> ptr(ns + 1, 0), other, edge;
    std::vector<int8_t> pos;
    std::vector<double> Rij(9 * (size_t)m);
    for (int i = 0; i < m; i++) std::memcpy(&Rij[9 * (size_t)i], facs[i].meas, 9 * sizeof(double));
    ip->max_deg = 0;
    for (int s = 0; s < ns; s++) {
      ptr[s] = (int32_t)other.size();
      ip->max_deg = std::max(ip->max_deg, (int)adj[s].size());
      for (int i : adj[s]) {
        const bool first = slot_of.at(facs[i].k0) == s;  // `if (key == keys[0])` comes first in the reference (:171)
        other.push_back(first ? slot_of.at(facs[i].k1) : slot_of.at(facs[i].k0));
        edge.push_back(i);
        pos.push_back(first ? 0 : 1);
      }
    }
    ptr[ns] = (int32_t)other.size();
    if ((rc = ip_upload(ip, &ip->d_ptr, ptr)) || (rc = ip_upload(ip, &ip->d_other, other)) || (rc = ip_upload(ip, &ip->d_edge, edge)) ||
        (rc = ip_upload(ip, &ip->d_pos, pos)) || (rc = ip_upload(ip, &ip->d_Rij, Rij)))
      return fail(rc);
    const int nb = (ns + 63) / 64;
    hipError_t e = hipMalloc((void**)&ip->d_R, (size_t)ns * 9 * sizeof(double));
    for (int w = 0; w < 2 && e == hipSuccess; w++) {
      e = hipMalloc((void**)&ip->d_buf[w], (size_t)ns * 9 * sizeof(double));
      if (e == hipSuccess) e = hipMalloc((void**)&ip->d_part[w], (size_t)nb * sizeof(double));
    }
    if (e == hipSuccess) e = hipMalloc((void**)&ip->d_ctl, sizeof(GradCtl));
    if (e == hipSuccess) e = hipHostMalloc((void**)&ip->h_ctl, sizeof(GradCtl));
    if (e != hipSuccess) {
      ip->err = std::string("lmgpu_init_pose3_finalize: ") + hipGetErrorString(e);
      return fail(LMGPU_HIP_ERROR);
    }
  }
  ip->finalized = true;
  return LMGPU_OK;
}

int lmgpu_init_pose3_num_poses(const lmgpu_init_pose3* ip) { return (ip && ip->finalized) ? (int)ip->out_slot.size() : -1; }
int lmgpu_init_pose3_num_factors(const lmgpu_init_pose3* ip) { return (ip && ip->finalized) ? ip->n_fac : -1; }
int lmgpu_init_pose3_get_slots(const lmgpu_init_pose3* ip, uint64_t* keys_out) {
  if (!ip || !ip->finalized) return -1;
  if (keys_out) std::memcpy(keys_out, ip->slot_keys.data(), ip->slot_keys.size() * sizeof(uint64_t));
  return (int)ip->slot_keys.size();
}
lmgpu_handle* lmgpu_init_pose3_handle(lmgpu_init_pose3* ip, int32_t which) {
  if (!ip || !ip->finalized) return nullptr;
  return which == 0 ? ip->hO : (which == 1 ? ip->hP : nullptr);
}

int lmgpu_init_pose3_orientations_chordal(lmgpu_init_pose3* ip, double* R_out) {
  int rc = ip_ready(ip, "lmgpu_init_pose3_orientations_chordal");
  if (rc) return rc;
  lmgpu_handle* h = ip->hO;
  if ((rc = ip_inner(ip, h, lmgpu_linearize(h)))) return rc;
  if ((rc = ip_inner(ip, h, lmgpu_solve(h, 0.0, 0, 0.0, 0.0, nullptr, nullptr, nullptr)))) return rc;  // zero values: the step is the solution
  const int ns = (int)ip->slot_keys.size();
  // single variable type: slot s is row s of the step vector
  hipLaunchKernelGGL(init_pose3_project_kernel, dim3((ns + 63) / 64), dim3(64), 0, h->stream, ns, (const double*)h->delta, ip->d_R);
  IPCHECK(hipGetLastError());
  IPCHECK(hipStreamSynchronize(h->stream));
  ip->have_R = true;
  if (R_out) return ip_download(ip, ip->d_R, 9, R_out);
  return LMGPU_OK;
}

int lmgpu_init_pose3_closest_rotations(int32_t device, int32_t n, const double* relaxed9, double* R_out) {
  if (device < 0 || n < 0 || (n > 0 && (!relaxed9 || !R_out))) return LMGPU_INVALID;
  if (n == 0) return LMGPU_OK;
  if (hipSetDevice(device) != hipSuccess) return LMGPU_HIP_ERROR;
  double *d_in = nullptr, *d_out = nullptr;
  const size_t bytes = (size_t)n * 9 * sizeof(double);
  hipError_t e = hipMalloc((void**)&d_in, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, bytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, relaxed9, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(init_pose3_project_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, (const double*)d_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(R_out, d_out, bytes, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return e == hipSuccess ? LMGPU_OK : LMGPU_HIP_ERROR;
}

int lmgpu_init_pose3_orientations_gradient(lmgpu_init_pose3* ip, const double* guess_R, int32_t max_iter, int32_t set_ref_frame, double* R_out,
                                           int32_t* iterations, double* max_grad) {
  int rc = ip_ready(ip, "lmgpu_init_pose3_orientations_gradient");
  if (rc) return rc;
  if (!guess_R || max_iter < 0) {
    ip->err = "lmgpu_init_pose3_orientations_gradient: refused (!guess_R || max_iter < 0)";
    return LMGPU_INVALID;
  }
  if (ip->anchor_deg == 0) {
    ip->err = "lmgpu_init_pose3_orientations_gradient: the anchor has no edge (the graph has no PriorFactor<Pose3>)";
    return LMGPU_INVALID;
  }
  const int ns = (int)ip->slot_keys.size(), nb = (ns + 63) / 64;
  hipStream_t s = ip->hO->stream;
  {
    std::vector<double> g((size_t)ns * 9, 0.0);
    for (size_t i = 0; i < ip->out_slot.size(); i++) std::memcpy(&g[(size_t)ip->out_slot[i] * 9], guess_R + i * 9, 9 * sizeof(double));
    IPCHECK(hipMemcpy(ip->d_R, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
    ip->have_R = false;
  }
  hipLaunchKernelGGL(init_pose3_gradient_start_kernel, dim3(nb), dim3(64), 0, s, ns, (const double*)ip->d_R, ip->anchor, ip->d_buf[0]);
  IPCHECK(hipMemsetAsync(ip->d_ctl, 0, sizeof(GradCtl), s));
  // the constants of :147-152
  const double b = 1.0, PI = 3.14159265358979323846;
  const double f0 = 1 / b - (1 / b + PI) * std::exp(-b * PI);
  const double a = (PI * PI) / (2 * f0);
  const double rho = 2 * a * b;
  const double mu_max = ip->max_deg * rho;
  const double stepsize = 2 / mu_max;
  // launches k = 0 .. max_iter: launch k closes iteration k - 1 (stop rule, maxIter) and, if the loop goes on, runs iteration k
  const int kChunk = 128;
  int k = 0;
  ip->h_ctl->done = 0;
  while (k <= max_iter) {
    const int end = std::min(max_iter + 1, k + kChunk);
    for (; k < end; k++)
      hipLaunchKernelGGL(init_pose3_gradient_kernel, dim3(nb), dim3(64), 0, s, ns, k, (int)max_iter, (const int32_t*)ip->d_ptr, (const int32_t*)ip->d_other,
                         (const int32_t*)ip->d_edge, (const int8_t*)ip->d_pos, (const double*)ip->d_Rij, ip->d_buf[0], ip->d_buf[1], ip->d_part[0],
                         ip->d_part[1], ip->d_ctl, a, b, stepsize);
    IPCHECK(hipGetLastError());
    IPCHECK(hipMemcpyAsync(ip->h_ctl, ip->d_ctl, sizeof(GradCtl), hipMemcpyDeviceToHost, s));
    IPCHECK(hipStreamSynchronize(s));
    if (ip->h_ctl->done) break;
  }
  const int iters = ip->h_ctl->iters;
  hipLaunchKernelGGL(init_pose3_gradient_result_kernel, dim3(nb), dim3(64), 0, s, ns, (const double*)ip->d_buf[iters & 1], ip->anchor, (int)set_ref_frame,
                     ip->d_R);
  IPCHECK(hipGetLastError());
  IPCHECK(hipStreamSynchronize(s));
  ip->have_R = true;
  if (iterations) *iterations = iters;
  if (max_grad) *max_grad = ip->h_ctl->max_grad;
  if (R_out) return ip_download(ip, ip->d_R, 9, R_out);
  return LMGPU_OK;
}

int lmgpu_init_pose3_compute_poses(lmgpu_init_pose3* ip, const double* R, int32_t single_iter, double* poses_out, lmgpu_lm_state* gn_state_out) {
  int rc = ip_ready(ip, "lmgpu_init_pose3_compute_poses");
  if (rc) return rc;
  const int ns = (int)ip->slot_keys.size();
  if (R) {
    std::vector<double> g((size_t)ns * 9, 0.0);
    for (size_t i = 0; i < ip->out_slot.size(); i++) std::memcpy(&g[(size_t)ip->out_slot[i] * 9], R + i * 9, 9 * sizeof(double));
    IPCHECK(hipMemcpy(ip->d_R, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
    ip->have_R = true;
  } else if (!ip->have_R) {
    ip->err = "lmgpu_init_pose3_compute_poses: no rotations (R == NULL needs an orientation call first)";
    return LMGPU_INVALID;
  }
  lmgpu_handle* h = ip->hP;
  // single variable type: slot s is row s of the POSE3 value array
  hipLaunchKernelGGL(init_pose3_upgrade_kernel, dim3((ns + 63) / 64), dim3(64), 0, h->stream, ns, (const double*)ip->d_R, ip->anchor,
                     h->vals[h->cur][LMGPU_POSE3]);
  IPCHECK(hipGetLastError());
  h->have_values = true;
  h->linearized = false;
  // GaussNewtonParams (NonlinearOptimizerParams' defaults), maxIterations = 1 for singleIter (InitializePose.h:78-85)
  lmgpu_lm_params p{};
  p.maxIterations = single_iter ? 1 : 100;
  p.relativeErrorTol = 1e-5;
  p.absoluteErrorTol = 1e-5;
  p.errorTol = 0.0;
  p.lambdaInitial = 1e-5;
  p.lambdaFactor = 10.0;
  p.lambdaUpperBound = 1e5;
  p.minModelFidelity = 1e-3;
  p.useFixedLambdaFactor = 1;
  p.minDiagonal = 1e-6;
  p.maxDiagonal = 1e32;
  lmgpu_lm_state st{};
  if ((rc = ip_inner(ip, h, lmgpu_lm_init(h, &p, &st)))) return rc;
  rc = ip_inner(ip, h, lmgpu_gn_optimize(h, &p, &st));
  if (gn_state_out) *gn_state_out = st;
  if (rc) return rc;
  IPCHECK(hipStreamSynchronize(h->stream));
  if (poses_out) return ip_download(ip, h->vals[h->cur][LMGPU_POSE3], 12, poses_out);
  return LMGPU_OK;
}

int lmgpu_init_pose3_initialize(lmgpu_init_pose3* ip, const double* guess_R, int32_t use_gradient, double* poses_out) {
  int rc = ip_ready(ip, "lmgpu_init_pose3_initialize");
  if (rc) return rc;
  rc = use_gradient ? lmgpu_init_pose3_orientations_gradient(ip, guess_R, 10000, 1, nullptr, nullptr, nullptr)
                    : lmgpu_init_pose3_orientations_chordal(ip, nullptr);
  if (rc) return rc;
  return lmgpu_init_pose3_compute_poses(ip, nullptr, 1, poses_out, nullptr);
}

}  // extern "C"
