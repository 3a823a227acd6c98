// Host side of the batched triangulation (include/lmgpu.h, "triangulation"): lmgpu_triangulate_batch on caller-supplied cameras and
// measurements, lmgpu_triangulate_landmarks on the POINT3 variables of a handle.  Included from lmgpu.hip.
//
// Degree sort: a wave runs as long as its highest-degree lane, so the host sorts the landmarks by their number of observations once
// (stable: ties keep the landmark order) and launches one grid per degree bin (degree < 2, 2, 3-4, 5-8, 9-16, ...) over that order; the
// kernel stores every result at the landmark's own index.  For the handle form the order is part of the cached point -> factor index.
#pragma once
#include "kernels_triangulation.hpp"

struct TriBin {
  int model, first, count;
};

struct TriState {
  bool built = false;
  std::string refusal;  // the structure cannot be triangulated: the message of every call
  int n_pts = 0;
  std::vector<TriBin> bins;
  int32_t *d_order = nullptr, *d_ptr = nullptr, *d_obs_cam = nullptr, *d_validx = nullptr, *d_status = nullptr, *d_iters = nullptr;
  int2* d_ref = nullptr;
  const double** d_tab = nullptr;
  double* d_points = nullptr;
  bool on_device = false;
  std::vector<int32_t> h_ptr, h_obs_cam, h_order, h_validx;
  std::vector<int2> h_ref;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool have_stats = false;
  lmgpu_triangulation_stats stats{};
};

static void tri_release(lmgpu_handle* h) {
  TriState* s = h->tri;
  if (!s) return;
  void* ptrs[] = {s->d_order, s->d_ptr, s->d_obs_cam, s->d_validx, s->d_status, s->d_iters, s->d_ref, (void*)s->d_tab, s->d_points};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (int i = 0; i < 2; i++)
    if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
  delete s;
  h->tri = nullptr;
}

namespace {

int tri_degree_class(int d) {
  if (d < 2) return 0;
  int c = 1, top = 2;
  while (d > top) {
    top *= 2;
    c++;
  }
  return c;
}

// landmarks [0, n) with a model each (-1: no observation) -> order sorted by (model, degree), one bin per (model, degree class)
void tri_make_order(int n, const std::vector<int32_t>& ptr, const std::vector<int>& model, std::vector<int32_t>& order, std::vector<TriBin>& bins) {
  order.resize(n);
  for (int i = 0; i < n; i++) order[i] = i;
  auto mdl = [&](int i) { return model[i] < 0 ? 0 : model[i]; };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    if (mdl(a) != mdl(b)) return mdl(a) < mdl(b);
    return ptr[a + 1] - ptr[a] < ptr[b + 1] - ptr[b];
  });
  bins.clear();
  for (int i = 0; i < n; i++) {
    const int l = order[i], c = tri_degree_class(ptr[l + 1] - ptr[l]);
    if (bins.empty() || bins.back().model != mdl(l) || tri_degree_class(ptr[order[i - 1] + 1] - ptr[order[i - 1]]) != c)
      bins.push_back(TriBin{mdl(l), i, 0});
    bins.back().count++;
  }
}

struct TriArgs {
  const int32_t *order, *ptr, *obs_cam, *validx;
  const int2* ref;
  const double* const* tab;
  const double* cams[3];  // per model
  double *points, *values;
  int32_t *status, *iters;
};

template <int MODEL>
void tri_launch_model(const TriBin& b, bool epi, const TriArgs& a, const TriParamsDev& prm, hipStream_t s) {
  const dim3 grid((b.count + 63) / 64), block(64);
  if (epi)
    hipLaunchKernelGGL((triangulate_kernel<MODEL, true>), grid, block, 0, s, b.first, b.count, a.order, a.ptr, a.obs_cam, a.ref, a.tab, a.cams[MODEL],
                       prm, a.points, a.status, a.iters, a.values, a.validx);
  else
    hipLaunchKernelGGL((triangulate_kernel<MODEL, false>), grid, block, 0, s, b.first, b.count, a.order, a.ptr, a.obs_cam, a.ref, a.tab, a.cams[MODEL],
                       prm, a.points, a.status, a.iters, a.values, a.validx);
}

void tri_launch(const std::vector<TriBin>& bins, bool epi, const TriArgs& a, const TriParamsDev& prm, hipStream_t s) {
  for (const TriBin& b : bins) {
    if (b.count == 0) continue;
    if (b.model == TRI_BUNDLER)
      tri_launch_model<TRI_BUNDLER>(b, epi, a, prm, s);
    else if (b.model == TRI_S2)
      tri_launch_model<TRI_S2>(b, epi, a, prm, s);
    else
      tri_launch_model<TRI_POSE_K>(b, epi, a, prm, s);
  }
}

TriParamsDev tri_params_dev(const lmgpu_triangulation_params* p) {
  return TriParamsDev{p->rankTolerance, p->landmarkDistanceThreshold, p->dynamicOutlierRejectionThreshold, p->noise_inv_sigma};
}

void tri_fill_stats(lmgpu_triangulation_stats& st, int n, const int32_t* status, const int32_t* iters, double ms) {
  st = lmgpu_triangulation_stats{};
  st.n_points = n;
  for (int i = 0; i < n; i++) {
    if (status[i] >= 0 && status[i] < 6) st.n_status[status[i]]++;
    st.max_iterations = std::max(st.max_iterations, iters[i]);
    st.sum_iterations += iters[i];
  }
  st.device_ms = ms;
}

thread_local lmgpu_triangulation_stats tri_batch_stats{};
thread_local bool tri_batch_have_stats = false;

// the point -> factor CSR of a handle, from the buckets it already holds (host only)
void tri_build_index(lmgpu_handle* h) {
  TriState* s = h->tri;
  const Plan& P = h->plan;
  s->built = true;
  std::vector<int32_t> pt_of_slot(P.n_vars, -1), pt_slot;
  for (int v = 0; v < P.n_vars; v++)
    if (P.types[v] == LMGPU_POINT3) {
      pt_of_slot[v] = (int32_t)pt_slot.size();
      pt_slot.push_back(v);
    }
  const int n = s->n_pts = (int)pt_slot.size();
  std::vector<int> model(n, -1);
  std::vector<int32_t> deg(n, 0);
  char msg[160];
  // P.factors is sorted by graph index
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) {
      s->h_ptr.assign(n + 1, 0);
      for (int i = 0; i < n; i++) s->h_ptr[i + 1] = s->h_ptr[i] + deg[i];
      s->h_obs_cam.resize(s->h_ptr[n]);
      s->h_ref.resize(s->h_ptr[n]);
      std::fill(deg.begin(), deg.end(), 0);
    }
    for (const FactorRef& f : P.factors) {
      const Bucket& b = h->buckets[f.bucket];
      const int t = b.type;
      if (t != LMGPU_F_SFM && t != LMGPU_F_PROJECTION && t != LMGPU_F_PROJECTION_BPS && t != LMGPU_F_SFM2) continue;
      const int p = pt_of_slot[f.slots[1]];  // key order of all four: (camera / pose, point[, calibration])
      if (p < 0) continue;
      if (t == LMGPU_F_PROJECTION_BPS || t == LMGPU_F_SFM2) {
        std::snprintf(msg, sizeof msg, "lmgpu_triangulate_landmarks: refused (point slot %d has a PROJECTION_BPS / SFM2 factor)", (int)f.slots[1]);
        s->refusal = msg;
        return;
      }
      const int m = t == LMGPU_F_SFM ? TRI_BUNDLER : TRI_POSE_K;
      if (model[p] >= 0 && model[p] != m) {
        std::snprintf(msg, sizeof msg, "lmgpu_triangulate_landmarks: refused (point slot %d has both SFM and PROJECTION factors)", (int)f.slots[1]);
        s->refusal = msg;
        return;
      }
      model[p] = m;
      if (pass == 1) {
        const int o = s->h_ptr[p] + deg[p];
        s->h_obs_cam[o] = P.tidx[f.slots[0]];
        s->h_ref[o] = make_int2(f.bucket, b.loc_of.empty() ? f.idx : b.loc_of[f.idx]);
      }
      deg[p]++;
    }
  }
  s->h_validx.resize(n);
  for (int i = 0; i < n; i++) s->h_validx[i] = P.tidx[pt_slot[i]];
  tri_make_order(n, s->h_ptr, model, s->h_order, s->bins);
}

int tri_upload_index(lmgpu_handle* h) {
  TriState* s = h->tri;
  int rc;
  if ((rc = upload(h, &s->d_order, s->h_order))) return rc;
  if ((rc = upload(h, &s->d_ptr, s->h_ptr))) return rc;
  if ((rc = upload(h, &s->d_obs_cam, s->h_obs_cam))) return rc;
  if ((rc = upload(h, &s->d_ref, s->h_ref))) return rc;
  if ((rc = upload(h, &s->d_validx, s->h_validx))) return rc;
  std::vector<const double*> tab(h->buckets.size());
  for (size_t i = 0; i < h->buckets.size(); i++) tab[i] = h->buckets[i].d_meas;
  if ((rc = upload(h, &s->d_tab, tab))) return rc;
  const size_t n = std::max(1, s->n_pts);
  HIPCHECK(hipMalloc((void**)&s->d_points, n * 3 * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&s->d_status, n * sizeof(int32_t)));
  HIPCHECK(hipMalloc((void**)&s->d_iters, n * sizeof(int32_t)));
  HIPCHECK(hipEventCreate(&s->ev[0]));
  HIPCHECK(hipEventCreate(&s->ev[1]));
  s->on_device = true;
  return LMGPU_OK;
}

}  // namespace

extern "C" {

int lmgpu_num_points3(const lmgpu_handle* h) { return (h && h->finalized) ? (int)h->plan.type_count[LMGPU_POINT3] : -1; }

int lmgpu_get_triangulation_stats(const lmgpu_handle* h, lmgpu_triangulation_stats* out) {
  if (!out) return LMGPU_INVALID;
  if (!h) {
    if (!tri_batch_have_stats) return LMGPU_INVALID;
    *out = tri_batch_stats;
    return LMGPU_OK;
  }
  if (!h->tri || !h->tri->have_stats) return LMGPU_INVALID;
  *out = h->tri->stats;
  return LMGPU_OK;
}

int lmgpu_triangulate_batch(int32_t device, int32_t camera_model, int32_t n_cams, const double* cams, int32_t n_points, const int32_t* obs_offsets,
                            const int32_t* obs_cam, const double* obs_z, const lmgpu_triangulation_params* params, double* points_out,
                            int32_t* status_out) {
  if (!params || params->useLOST != 0) return LMGPU_INVALID;
  if (camera_model != TRI_BUNDLER && camera_model != TRI_S2) return LMGPU_INVALID;
  if (n_points < 0 || n_cams < 0) return LMGPU_INVALID;
  if (n_points == 0) {
    tri_batch_stats = lmgpu_triangulation_stats{};
    tri_batch_have_stats = true;
    return LMGPU_OK;
  }
  if (!obs_offsets || !points_out || !status_out || obs_offsets[0] < 0) return LMGPU_INVALID;
  for (int i = 0; i < n_points; i++)
    if (obs_offsets[i + 1] < obs_offsets[i]) return LMGPU_INVALID;
  const int n_obs = obs_offsets[n_points];
  if (n_obs > 0 && (!obs_cam || !obs_z || !cams)) return LMGPU_INVALID;
  for (int o = obs_offsets[0]; o < n_obs; o++)
    if (obs_cam[o] < 0 || obs_cam[o] >= n_cams) return LMGPU_INVALID;
  if (device < 0) return LMGPU_INVALID;
  if (hipSetDevice(device) != hipSuccess) return LMGPU_HIP_ERROR;

  std::vector<int32_t> ptr(obs_offsets, obs_offsets + n_points + 1), order;
  std::vector<int> model(n_points, camera_model);
  std::vector<TriBin> bins;
  tri_make_order(n_points, ptr, model, order, bins);

  const int cs = camera_model == TRI_BUNDLER ? 15 : 17;
  int32_t *d_order = nullptr, *d_ptr = nullptr, *d_cam = nullptr, *d_status = nullptr, *d_iters = nullptr;
  double *d_cams = nullptr, *d_z = nullptr, *d_points = nullptr;
  const double** d_tab = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::vector<int32_t> iters(n_points);
  float ms = 0.f;
  auto up = [](void** dst, const void* src, size_t bytes) {
    hipError_t e = hipMalloc(dst, std::max<size_t>(bytes, 8));
    if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    return e;
  };
  hipError_t e = up((void**)&d_order, order.data(), (size_t)n_points * sizeof(int32_t));
  if (e == hipSuccess) e = up((void**)&d_ptr, ptr.data(), (size_t)(n_points + 1) * sizeof(int32_t));
  if (e == hipSuccess) e = up((void**)&d_cam, obs_cam, (size_t)n_obs * sizeof(int32_t));
  if (e == hipSuccess) e = up((void**)&d_z, obs_z, (size_t)n_obs * 2 * sizeof(double));
  if (e == hipSuccess) e = up((void**)&d_cams, cams, (size_t)n_cams * cs * sizeof(double));
  if (e == hipSuccess) e = up((void**)&d_tab, &d_z, sizeof(double*));
  if (e == hipSuccess) e = hipMalloc((void**)&d_points, (size_t)n_points * 3 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&d_status, (size_t)n_points * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&d_iters, (size_t)n_points * sizeof(int32_t));
  if (e == hipSuccess) e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) {
    TriArgs a{};
    a.order = d_order; a.ptr = d_ptr; a.obs_cam = d_cam; a.validx = nullptr; a.ref = nullptr; a.tab = d_tab;
    a.cams[0] = a.cams[1] = a.cams[2] = d_cams;
    a.points = d_points; a.values = nullptr; a.status = d_status; a.iters = d_iters;
    e = hipEventRecord(ev[0], nullptr);
    tri_launch(bins, params->enableEPI != 0, a, tri_params_dev(params), nullptr);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  }
  if (e == hipSuccess) e = hipMemcpy(points_out, d_points, (size_t)n_points * 3 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(status_out, d_status, (size_t)n_points * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(iters.data(), d_iters, (size_t)n_points * sizeof(int32_t), hipMemcpyDeviceToHost);
  void* ptrs[] = {d_order, d_ptr, d_cam, d_status, d_iters, d_cams, d_z, d_points, (void*)d_tab};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (int i = 0; i < 2; i++)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  if (e != hipSuccess) return LMGPU_HIP_ERROR;
  tri_fill_stats(tri_batch_stats, n_points, status_out, iters.data(), ms);
  tri_batch_have_stats = true;
  return LMGPU_OK;
}

int lmgpu_triangulate_landmarks(lmgpu_handle* h, const lmgpu_triangulation_params* params, int32_t write_values, double* points_out,
                                int32_t* status_out, int32_t* n_valid) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !params) {
    h->err = "lmgpu_triangulate_landmarks: refused (!h->finalized || !params)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "lmgpu_triangulate_landmarks")) return LMGPU_INVALID;
  if (params->useLOST != 0) {
    h->err = "lmgpu_triangulate_landmarks: refused (useLOST: LOST is not implemented)";
    return LMGPU_INVALID;
  }
  if (h->gnc_on) {
    h->err = "lmgpu_triangulate_landmarks: refused (GNC is enabled)";
    return LMGPU_INVALID;
  }
  if (h->cfg.world_size > 1) {
    h->err = "lmgpu_triangulate_landmarks: refused (world_size > 1)";
    return LMGPU_INVALID;
  }
  if (!h->tri) h->tri = new TriState();
  TriState* s = h->tri;
  if (!s->built) tri_build_index(h);
  if (!s->refusal.empty()) {
    h->err = s->refusal;
    return LMGPU_INVALID;
  }
  if (!h->have_values) {
    h->err = "lmgpu_triangulate_landmarks: refused (no values: call lmgpu_set_values first)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  if (!s->on_device && (rc = tri_upload_index(h))) return rc;
  const int n = s->n_pts;
  if (n_valid) *n_valid = 0;
  std::vector<int32_t> status(n), iters(n);
  float ms = 0.f;
  if (n > 0) {
    TriArgs a{};
    a.order = s->d_order; a.ptr = s->d_ptr; a.obs_cam = s->d_obs_cam; a.validx = s->d_validx; a.ref = s->d_ref; a.tab = s->d_tab;
    a.cams[TRI_BUNDLER] = h->vals[h->cur][LMGPU_CAM_BUNDLER];
    a.cams[TRI_S2] = nullptr;
    a.cams[TRI_POSE_K] = h->vals[h->cur][LMGPU_POSE3];
    a.points = s->d_points; a.status = s->d_status; a.iters = s->d_iters;
    a.values = write_values ? h->vals[h->cur][LMGPU_POINT3] : nullptr;
    if (write_values) h->marg_valid = false;
    HIPCHECK(hipEventRecord(s->ev[0], h->stream));
    tri_launch(s->bins, params->enableEPI != 0, a, tri_params_dev(params), h->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(s->ev[1], h->stream));
    HIPCHECK(hipEventSynchronize(s->ev[1]));
    HIPCHECK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    HIPCHECK(hipMemcpy(status.data(), s->d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(iters.data(), s->d_iters, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (points_out) HIPCHECK(hipMemcpy(points_out, s->d_points, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (status_out) std::memcpy(status_out, status.data(), (size_t)n * sizeof(int32_t));
  }
  tri_fill_stats(s->stats, n, status.data(), iters.data(), ms);
  s->have_stats = true;
  if (n_valid) *n_valid = s->stats.n_status[LMGPU_TRI_VALID];
  return LMGPU_OK;
}

}  // extern "C"
