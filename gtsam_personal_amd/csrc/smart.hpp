// Host side of the smart projection factors (include/lmgpu.h, "smart projection factors"; kernels in kernels_smart.hpp).  Included from
// lmgpu.hip.
//
// Integration: lmgpu_finalize_structure turns every smart factor with m >= 2 observations into a hidden POINT3 variable
// in front of the caller's slots (so the caller's packed vectors are a contiguous suffix of the internal ones) and its observations into
// factors of one internal bucket of type kSmartObsType (factor_types.hpp).  Leaf elimination, Schur gather and back-substitution then run unchanged;
// the damping weight of the hidden scalars is 0 (fill_dampw), the retract skips them (do_retract), and their value is never read: the
// point lives in the cache below.  The caller's graph indices are renumbered densely over (graph index, observation) so that every internal
// factor has an index of its own and the error sum keeps the caller's order.
//
// The cache (cameraPosesTriangulation_ and result_ of every factor) exists twice: a triangulate launch reads set `cur` and writes the
// other; every caller but tryLambda's speculative error evaluation commits at once (smart_commit), that one only when the reference
// would have evaluated the error (LevenbergMarquardtOptimizer.cpp:206-216).
#pragma once
#include "kernels_smart.hpp"

struct SmartState {
  // ---- as added (host)
  std::vector<lmgpu_smart_params> groups;  // one per lmgpu_add_smart_factors call
  std::vector<int32_t> f_group, f_gi, f_ptr{0};
  std::vector<double> f_K, f_isig;
  std::vector<int32_t> o_slot;  // the caller's slot of every observation
  std::vector<double> o_z;
  // ---- after smart_prepare
  bool prepared = false;
  int n = 0, nh = 0, n_int = 0, bucket = -1;
  std::vector<int32_t> hid_of;   // smart factor -> hidden point (-1: m < 2)
  std::vector<int32_t> hp_fptr;  // hidden point -> its range of internal factors
  struct Bin {
    int group, first, count;
  };
  std::vector<Bin> bins;
  std::vector<int32_t> order;
  // ---- device
  bool on_device = false;
  int32_t *d_order = nullptr, *d_ptr = nullptr, *d_obs_cam = nullptr, *d_sf_of = nullptr, *d_j_of = nullptr, *d_hp_fptr = nullptr;
  int2* d_ref = nullptr;  // per observation: (0, its factor in the internal bucket), the measurement reference of tri_load
  const double** d_tab = nullptr;
  lmgpu::SmartCacheDev set[2] = {};
  int32_t* d_retri[2] = {nullptr, nullptr};
  double *d_corr = nullptr, *d_corr_sum = nullptr;
  int cur = 0, last = 0;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // triangulate launches that wrote set 0, set 1; linearize
  bool timed_tri[2] = {false, false}, timed_lin = false;
};

static void smart_release(lmgpu_handle* h) {
  SmartState* s = h->smart;
  if (!s) return;
  void* ptrs[] = {s->d_order, s->d_ptr, s->d_obs_cam, s->d_sf_of, s->d_j_of, s->d_hp_fptr, s->d_ref, (void*)s->d_tab, s->d_corr, s->d_corr_sum,
                  s->set[0].poses, s->set[0].points, s->set[0].status, s->set[0].have, s->set[1].poses, s->set[1].points, s->set[1].status,
                  s->set[1].have, s->d_retri[0], s->d_retri[1]};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (int i = 0; i < 6; i++)
    if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
  delete s;
  h->smart = nullptr;
}

// the one message of everything a handle with smart factors refuses (each would need the Schur complement itself, not the Jacobians)
static bool smart_refused(lmgpu_handle* h, const char* who) {
  if (!h->smart || h->smart->f_gi.empty()) return false;
  h->err = std::string(who) + ": refused (the handle has smart projection factors; supported on it: error, linearize, solve / LM without "
                              "diagonal damping, Gauss-Newton, retract, save / restore)";
  return true;
}

static int smart_prepare(lmgpu_handle* h) {
  SmartState* s = h->smart;
  if (s->prepared) return LMGPU_OK;
  if (h->solver == LMGPU_SOLVER_PCG) {
    (void)smart_refused(h, "LMGPU_SOLVER_PCG");
    return LMGPU_INVALID;
  }
  Plan& P = h->plan;
  const int n = (int)s->f_gi.size();
  s->n = n;
  s->hid_of.assign(n, -1);
  int nh = 0, n_int = 0;
  for (int i = 0; i < n; i++) {
    const int m = s->f_ptr[i + 1] - s->f_ptr[i];
    if (m >= 2) {
      s->hid_of[i] = nh++;
      n_int += m;
    }
  }
  // hidden keys: the top of the key range, so that no separator order among the caller's variables changes
  for (uint64_t k : P.keys)
    if (k > UINT64_MAX - (uint64_t)nh - 1) {
      h->err = "lmgpu_finalize_structure: a variable key collides with the keys reserved for the hidden points of smart factors";
      return LMGPU_INVALID;
    }
  // dense renumbering of the graph indices over (caller's graph index, observation)
  struct Ent {
    int32_t gi, sub, src, a;  // src 0: plan factor a; 1: smart factor a, observation sub; 2: a smart factor without internal factors
  };
  std::vector<Ent> ents;
  ents.reserve(P.factors.size() + n_int + n);
  for (size_t k = 0; k < P.factors.size(); k++) ents.push_back({P.factors[k].graph_index, 0, 0, (int32_t)k});
  for (int i = 0; i < n; i++) {
    const int m = s->f_ptr[i + 1] - s->f_ptr[i];
    if (m < 2)
      ents.push_back({s->f_gi[i], 0, 2, i});
    else
      for (int j = 0; j < m; j++) ents.push_back({s->f_gi[i], j, 1, i});
  }
  std::sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) { return x.gi != y.gi ? x.gi < y.gi : x.sub < y.sub; });
  for (size_t k = 1; k < ents.size(); k++)
    if (ents[k].gi == ents[k - 1].gi && !(ents[k].src == 1 && ents[k - 1].src == 1 && ents[k].a == ents[k - 1].a)) {
      h->err = "duplicate graph_index";
      return LMGPU_INVALID;
    }
  // ---- from here on the handle's structure is rewritten
  s->prepared = true;
  s->nh = nh;
  s->n_int = n_int;
  h->n_hidden = nh;
  for (Bucket& b : h->buckets)
    for (int32_t& v : b.slots) v += nh;
  for (FactorRef& f : P.factors)
    for (int k = 0; k < kMaxArity; k++)
      if (f.slots[k] >= 0) f.slots[k] += nh;
  std::vector<uint64_t> keys(nh);
  for (int i = 0; i < nh; i++) keys[i] = UINT64_MAX - (uint64_t)i;
  P.keys.insert(P.keys.begin(), keys.begin(), keys.end());
  P.types.insert(P.types.begin(), (size_t)nh, (int32_t)LMGPU_POINT3);
  P.n_vars += nh;
  Bucket ib;
  ib.type = kSmartObsType;
  ib.n = n_int;
  ib.noise_kind = LMGPU_N_DIAG;
  const BucketShape sh = bucket_shape(kSmartObsType, LMGPU_N_DIAG);  // (pose, point), (z, K), (1 / sigma, 1 / sigma)
  ib.rows = sh.rows;
  ib.cols = sh.cols;
  ib.graph_index.resize(n_int);
  ib.slots.resize((size_t)n_int * sh.ar);
  ib.meas.resize((size_t)n_int * sh.ml);
  ib.noise.resize((size_t)n_int * sh.nl);
  s->hp_fptr.assign(nh + 1, 0);
  std::vector<int32_t> first_of(n, -1);
  {
    int at = 0;
    for (int i = 0; i < n; i++) {
      if (s->hid_of[i] < 0) continue;
      first_of[i] = at;
      s->hp_fptr[s->hid_of[i]] = at;
      for (int o = s->f_ptr[i]; o < s->f_ptr[i + 1]; o++, at++) {
        ib.slots[2 * at] = s->o_slot[o] + nh;
        ib.slots[2 * at + 1] = s->hid_of[i];
        double* m = &ib.meas[(size_t)at * 7];
        m[0] = s->o_z[2 * o];
        m[1] = s->o_z[2 * o + 1];
        for (int k = 0; k < 5; k++) m[2 + k] = s->f_K[(size_t)i * 5 + k];
        ib.noise[2 * at] = ib.noise[2 * at + 1] = s->f_isig[i];
      }
    }
    s->hp_fptr[nh] = at;
  }
  const int bi = (int)h->buckets.size();
  for (size_t r = 0; r < ents.size(); r++) {
    const Ent& e = ents[r];
    if (e.src == 0) {
      FactorRef& f = P.factors[e.a];
      f.graph_index = (int32_t)r;
      h->buckets[f.bucket].graph_index[f.idx] = (int32_t)r;
    } else if (e.src == 1) {
      ib.graph_index[first_of[e.a] + e.sub] = (int32_t)r;
    }
  }
  if (n_int > 0) {
    for (int i = 0; i < n_int; i++) {
      FactorRef f;
      f.bucket = bi;
      f.idx = i;
      f.slots[0] = ib.slots[2 * i];
      f.slots[1] = ib.slots[2 * i + 1];
      f.slots[2] = -1;
      f.graph_index = ib.graph_index[i];
      P.factors.push_back(f);
    }
    s->bucket = bi;
    h->buckets.push_back(std::move(ib));
  }
  // launch order of the triangulation: by (parameter group, degree class), one bin each (triangulation.hpp)
  s->order.resize(n);
  for (int i = 0; i < n; i++) s->order[i] = i;
  auto deg = [&](int i) { return s->f_ptr[i + 1] - s->f_ptr[i]; };
  std::stable_sort(s->order.begin(), s->order.end(), [&](int a, int b) {
    if (s->f_group[a] != s->f_group[b]) return s->f_group[a] < s->f_group[b];
    return deg(a) < deg(b);
  });
  s->bins.clear();
  for (int i = 0; i < n; i++) {
    const int l = s->order[i], c = tri_degree_class(deg(l));
    if (s->bins.empty() || s->bins.back().group != s->f_group[l] || tri_degree_class(deg(s->order[i - 1])) != c)
      s->bins.push_back(SmartState::Bin{s->f_group[l], i, 0});
    s->bins.back().count++;
  }
  return LMGPU_OK;
}

static int smart_upload(lmgpu_handle* h) {
  SmartState* s = h->smart;
  const Plan& P = h->plan;
  const int n = s->n, nh = s->nh, n_obs = s->f_ptr[n];
  int rc;
  HIPCHECK(hipSetDevice(h->device));
  // (the measurements are read where the internal bucket has them; an observation of a factor with m < 2 is never loaded)
  std::vector<int32_t> obs_cam(n_obs);
  std::vector<int2> ref(n_obs, make_int2(0, 0));
  for (int i = 0; i < n; i++)
    for (int o = s->f_ptr[i]; o < s->f_ptr[i + 1]; o++) {
      obs_cam[o] = P.tidx[s->o_slot[o] + nh];
      if (s->hid_of[i] >= 0) ref[o] = make_int2(0, s->hp_fptr[s->hid_of[i]] + (o - s->f_ptr[i]));
    }
  std::vector<int32_t> sf_of(s->n_int), j_of(s->n_int);
  if (s->bucket >= 0) {
    const Bucket& b = h->buckets[s->bucket];
    for (int i = 0; i < n; i++) {
      if (s->hid_of[i] < 0) continue;
      const int f0 = s->hp_fptr[s->hid_of[i]];
      for (int j = 0; j < s->f_ptr[i + 1] - s->f_ptr[i]; j++) {
        if (b.loc_of[f0 + j] != f0 + j) {
          h->err = "smart factors: the internal bucket is not evaluated whole on this rank";
          return LMGPU_INVALID;
        }
        sf_of[f0 + j] = i;
        j_of[f0 + j] = j;
      }
    }
  }
  if ((rc = upload(h, &s->d_order, s->order))) return rc;
  if ((rc = upload(h, &s->d_ptr, s->f_ptr))) return rc;
  if ((rc = upload(h, &s->d_obs_cam, obs_cam))) return rc;
  if ((rc = upload(h, &s->d_ref, ref))) return rc;
  if ((rc = upload(h, &s->d_sf_of, sf_of))) return rc;
  if ((rc = upload(h, &s->d_j_of, j_of))) return rc;
  if ((rc = upload(h, &s->d_hp_fptr, s->hp_fptr))) return rc;
  std::vector<const double*> tab(1, s->bucket >= 0 ? (const double*)h->buckets[s->bucket].d_meas : nullptr);
  if ((rc = upload(h, &s->d_tab, tab))) return rc;
  const size_t n1 = std::max(1, n), o1 = std::max(1, n_obs);
  std::vector<double> nans(n1 * 3, std::numeric_limits<double>::quiet_NaN());
  std::vector<int32_t> deg(n1, LMGPU_TRI_DEGENERATE);
  for (int k = 0; k < 2; k++) {
    HIPCHECK(hipMalloc((void**)&s->set[k].poses, o1 * 12 * sizeof(double)));
    HIPCHECK(hipMemset(s->set[k].poses, 0, o1 * 12 * sizeof(double)));
    HIPCHECK(hipMalloc((void**)&s->set[k].points, n1 * 3 * sizeof(double)));
    HIPCHECK(hipMemcpy(s->set[k].points, nans.data(), n1 * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMalloc((void**)&s->set[k].status, n1 * sizeof(int32_t)));
    HIPCHECK(hipMemcpy(s->set[k].status, deg.data(), n1 * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHECK(hipMalloc((void**)&s->set[k].have, n1 * sizeof(int32_t)));
    HIPCHECK(hipMemset(s->set[k].have, 0, n1 * sizeof(int32_t)));
    HIPCHECK(hipMalloc((void**)&s->d_retri[k], n1 * sizeof(int32_t)));
    HIPCHECK(hipMemset(s->d_retri[k], 0, n1 * sizeof(int32_t)));
  }
  HIPCHECK(hipMalloc((void**)&s->d_corr, std::max(1, nh) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&s->d_corr_sum, sizeof(double)));
  HIPCHECK(hipMemset(s->d_corr_sum, 0, sizeof(double)));
  for (int i = 0; i < 6; i++) HIPCHECK(hipEventCreate(&s->ev[i]));
  s->on_device = true;
  return LMGPU_OK;
}

static void smart_enqueue_triangulate(lmgpu_handle* h, int which) {
  SmartState* s = h->smart;
  if (!s->on_device || s->n == 0) return;
  hipStream_t st = h->stream;
  const int to = s->cur ^ 1;
  (void)hipEventRecord(s->ev[2 * to], st);
  for (const SmartState::Bin& b : s->bins) {
    if (b.count == 0) continue;
    const lmgpu_smart_params& p = s->groups[b.group];
    const lmgpu::SmartParamsDev prm{tri_params_dev(&p.triangulation), p.retriangulationThreshold};
    const dim3 grid((b.count + 63) / 64), block(64);
    if (p.triangulation.enableEPI)
      hipLaunchKernelGGL((lmgpu::smart_triangulate_kernel<true>), grid, block, 0, st, b.first, b.count, (const int32_t*)s->d_order,
                         (const int32_t*)s->d_ptr, (const int32_t*)s->d_obs_cam, (const int2*)s->d_ref, (const double* const*)s->d_tab,
                         (const double*)h->vals[which][LMGPU_POSE3], prm, s->set[s->cur], s->set[to], s->d_retri[to]);
    else
      hipLaunchKernelGGL((lmgpu::smart_triangulate_kernel<false>), grid, block, 0, st, b.first, b.count, (const int32_t*)s->d_order,
                         (const int32_t*)s->d_ptr, (const int32_t*)s->d_obs_cam, (const int2*)s->d_ref, (const double* const*)s->d_tab,
                         (const double*)h->vals[which][LMGPU_POSE3], prm, s->set[s->cur], s->set[to], s->d_retri[to]);
  }
  (void)hipEventRecord(s->ev[2 * to + 1], st);
  s->timed_tri[to] = true;
  s->last = to;
  if (!h->smart_speculative) s->cur = to;
}

static void smart_commit(lmgpu_handle* h) { h->smart->cur = h->smart->last; }

static void smart_launch_factors(lmgpu_handle* h, const lmgpu::BucketDev& d, const lmgpu::ValuesDev& vals, bool jac) {
  SmartState* s = h->smart;
  const dim3 grid((d.n + 127) / 128), block(128);
  const lmgpu::SmartCacheDev& c = s->set[s->last];
  if (jac) {
    (void)hipEventRecord(s->ev[4], h->stream);
    hipLaunchKernelGGL((lmgpu::smart_factor_kernel<true>), grid, block, 0, h->stream, d, vals, h->ebuf0, (const int32_t*)s->d_sf_of,
                       (const int32_t*)s->d_j_of, (const double*)c.points, (const int32_t*)c.status);
  } else {
    hipLaunchKernelGGL((lmgpu::smart_factor_kernel<false>), grid, block, 0, h->stream, d, vals, h->ebuf0, (const int32_t*)s->d_sf_of,
                       (const int32_t*)s->d_j_of, (const double*)c.points, (const int32_t*)c.status);
  }
}

// behind a linearization: the scalar the constant terms of the Hessian factors lack against the observations' b'b (fixed-order sum)
static void smart_enqueue_const(lmgpu_handle* h) {
  SmartState* s = h->smart;
  if (!s->on_device || s->nh == 0) return;
  const Bucket& b = h->buckets[s->bucket];
  hipLaunchKernelGGL(lmgpu::smart_const_kernel, dim3((s->nh + 63) / 64), dim3(64), 0, h->stream, s->nh, (const int32_t*)s->d_hp_fptr,
                     (const double*)(h->pool + b.joff), s->d_corr);
  reduce_to(h, s->d_corr, s->nh, s->d_corr_sum);
  (void)hipEventRecord(s->ev[5], h->stream);
  s->timed_lin = true;
}

// linear.error(0) of the reference's graph: the Hessian factors' constant terms instead of the observations' b'b
static void smart_fix_lin0(lmgpu_handle* h) {
  SmartState* s = h->smart;
  if (!s->on_device || s->nh == 0) return;
  hipLaunchKernelGGL(lmgpu::smart_sub_scalar_kernel, dim3(1), dim3(1), 0, h->stream, h->dscal + 1, (const double*)s->d_corr_sum);
}

namespace {
// inverse of a symmetric 3x3 (row-major 9) by its adjugate
void smart_inv3(const double* A, double* P) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  P[0] = c00 / det;
  P[1] = (A[2] * A[7] - A[1] * A[8]) / det;
  P[2] = (A[1] * A[5] - A[2] * A[4]) / det;
  P[3] = c01 / det;
  P[4] = (A[0] * A[8] - A[2] * A[6]) / det;
  P[5] = (A[2] * A[3] - A[0] * A[5]) / det;
  P[6] = c02 / det;
  P[7] = (A[1] * A[6] - A[0] * A[7]) / det;
  P[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}
}  // namespace

extern "C" {

int lmgpu_add_smart_factors(lmgpu_handle* h, int32_t n, const int32_t* graph_index, const int32_t* obs_offsets, const int32_t* obs_slots,
                            const double* obs_z, const double* K5, const double* inv_sigma, const lmgpu_smart_params* params) {
  if (!h) return LMGPU_INVALID;
  auto refuse = [&](const char* why) {
    h->err = std::string("lmgpu_add_smart_factors: refused (") + why + ")";
    return (int)LMGPU_INVALID;
  };
  if (h->finalized) return refuse("the structure is finalized");
  if (h->plan.n_vars == 0) return refuse("lmgpu_set_variables comes first");
  if (!params) return refuse("!params");
  if (h->cfg.world_size > 1 || (h->cfg.flags & LMGPU_FLAG_SPLIT_ROOT)) return refuse("world_size > 1: smart factors are single-rank");
  if (params->linearizationMode != LMGPU_SMART_HESSIAN)
    return refuse("linearizationMode: only HESSIAN is implemented (IMPLICIT_SCHUR, JACOBIAN_Q, JACOBIAN_SVD are not)");
  if (params->degeneracyMode != LMGPU_SMART_ZERO_ON_DEGENERACY)
    return refuse("degeneracyMode: only ZERO_ON_DEGENERACY is implemented (IGNORE_DEGENERACY, HANDLE_INFINITY are not)");
  if (params->triangulation.useLOST != 0) return refuse("useLOST: LOST is not implemented");
  if (!(params->retriangulationThreshold >= 0.0)) return refuse("retriangulationThreshold < 0");
  if (n < 0) return refuse("n < 0");
  if (n == 0) return LMGPU_OK;
  if (!graph_index || !obs_offsets || !obs_slots || !obs_z || !K5 || !inv_sigma) return refuse("a NULL array");
  if (obs_offsets[0] < 0) return refuse("obs_offsets[0] < 0");
  for (int i = 0; i < n; i++) {
    if (obs_offsets[i + 1] < obs_offsets[i]) return refuse("decreasing obs_offsets");
    if (obs_offsets[i + 1] == obs_offsets[i]) return refuse("a factor without observations");
    if (!(inv_sigma[i] > 0.0)) return refuse("inv_sigma <= 0");
    for (int o = obs_offsets[i]; o < obs_offsets[i + 1]; o++) {
      const int sl = obs_slots[o];
      if (sl < 0 || sl >= h->plan.n_vars) return refuse("an observation references an unknown slot");
      if (h->plan.types[sl] != LMGPU_POSE3) return refuse("an observation's slot is not a POSE3 variable");
      for (int q = obs_offsets[i]; q < o; q++)
        if (obs_slots[q] == sl) return refuse("a pose appears twice in one factor");
    }
  }
  if (!h->smart) h->smart = new SmartState();
  SmartState* s = h->smart;
  const int g = (int)s->groups.size();
  s->groups.push_back(*params);
  for (int i = 0; i < n; i++) {
    s->f_group.push_back(g);
    s->f_gi.push_back(graph_index[i]);
    s->f_isig.push_back(inv_sigma[i]);
    for (int k = 0; k < 5; k++) s->f_K.push_back(K5[(size_t)i * 5 + k]);
    for (int o = obs_offsets[i]; o < obs_offsets[i + 1]; o++) {
      s->o_slot.push_back(obs_slots[o]);
      s->o_z.push_back(obs_z[2 * (size_t)o]);
      s->o_z.push_back(obs_z[2 * (size_t)o + 1]);
    }
    s->f_ptr.push_back((int32_t)s->o_slot.size());
  }
  return LMGPU_OK;
}

int lmgpu_num_smart_factors(const lmgpu_handle* h) {
  if (!h || !h->finalized) return -1;
  return h->smart ? h->smart->n : 0;
}

int lmgpu_smart_get_points(lmgpu_handle* h, double* points3, int32_t* status) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized) {
    h->err = "lmgpu_smart_get_points: refused (!h->finalized)";
    return LMGPU_INVALID;
  }
  SmartState* s = h->smart;
  if (!s || s->n == 0) return LMGPU_OK;
  int rc = need_device(h);
  if (rc) return rc;
  HIPCHECK(hipStreamSynchronize(h->stream));
  if (points3) HIPCHECK(hipMemcpy(points3, s->set[s->cur].points, (size_t)s->n * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (status) HIPCHECK(hipMemcpy(status, s->set[s->cur].status, (size_t)s->n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return LMGPU_OK;
}

int lmgpu_smart_get_hessian(lmgpu_handle* h, int32_t graph_index, int32_t* m_out, double* aug) {
  if (!h) return LMGPU_INVALID;
  SmartState* s = h->smart;
  if (!h->finalized || !s) {
    h->err = "lmgpu_smart_get_hessian: refused (!h->finalized, or no smart factors)";
    return LMGPU_INVALID;
  }
  int i = -1;
  for (int k = 0; k < s->n; k++)
    if (s->f_gi[k] == graph_index) i = k;
  if (i < 0) {
    h->err = "lmgpu_smart_get_hessian: no smart factor with this graph index";
    return LMGPU_INVALID;
  }
  const int m = s->f_ptr[i + 1] - s->f_ptr[i];
  if (m_out) *m_out = m;
  if (!aug) return LMGPU_OK;
  const int N = 6 * m + 1;
  std::fill(aug, aug + (size_t)N * N, 0.0);
  if (s->hid_of[i] < 0) return LMGPU_OK;  // m < 2: the empty Hessian factor
  if (!h->have_jacobians) {
    h->err = "lmgpu_smart_get_hessian: no linearization (call lmgpu_linearize or an optimizer iteration first)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  std::vector<double> J((size_t)m * 20);
  HIPCHECK(hipStreamSynchronize(h->stream));
  HIPCHECK(hipMemcpy(J.data(), h->pool + h->buckets[s->bucket].joff + (size_t)s->hp_fptr[s->hid_of[i]] * 20, J.size() * sizeof(double),
                     hipMemcpyDeviceToHost));
  // SchurComplement(Fs, E, b, lambda = 0) (CameraSet.h:145-216): P = (E'E)^-1, G_jk = F_j'(delta_jk - E_j P E_k') F_k,
  // g_j = F_j'(b_j - E_j P E'b), f = b'b - (E'b)'P(E'b).  Column-major blocks of the device: F = J[0:12], E = J[12:18], b = J[18:20].
  auto F = [&](int j, int r, int c) { return J[(size_t)j * 20 + c * 2 + r]; };
  auto E = [&](int j, int r, int c) { return J[(size_t)j * 20 + 12 + c * 2 + r]; };
  auto B = [&](int j, int r) { return J[(size_t)j * 20 + 18 + r]; };
  double EtE[9] = {0}, Etb[3] = {0}, P[9], bb = 0;
  for (int j = 0; j < m; j++)
    for (int r = 0; r < 2; r++) {
      for (int a = 0; a < 3; a++) {
        for (int c = 0; c < 3; c++) EtE[3 * a + c] += E(j, r, a) * E(j, r, c);
        Etb[a] += E(j, r, a) * B(j, r);
      }
      bb += B(j, r) * B(j, r);
    }
  smart_inv3(EtE, P);
  double PEtb[3];
  for (int a = 0; a < 3; a++) PEtb[a] = P[3 * a] * Etb[0] + P[3 * a + 1] * Etb[1] + P[3 * a + 2] * Etb[2];
  // FtE_j = F_j' E_j (6 x 3)
  std::vector<double> FtE((size_t)m * 18, 0.0);
  for (int j = 0; j < m; j++)
    for (int a = 0; a < 6; a++)
      for (int c = 0; c < 3; c++) FtE[(size_t)j * 18 + a * 3 + c] = F(j, 0, a) * E(j, 0, c) + F(j, 1, a) * E(j, 1, c);
  for (int j = 0; j < m; j++)
    for (int k = 0; k < m; k++)
      for (int a = 0; a < 6; a++)
        for (int c = 0; c < 6; c++) {
          double v = j == k ? F(j, 0, a) * F(j, 0, c) + F(j, 1, a) * F(j, 1, c) : 0.0;
          for (int p = 0; p < 3; p++)
            for (int q = 0; q < 3; q++) v -= FtE[(size_t)j * 18 + a * 3 + p] * P[3 * p + q] * FtE[(size_t)k * 18 + c * 3 + q];
          aug[(size_t)(6 * k + c) * N + (6 * j + a)] = v;
        }
  for (int j = 0; j < m; j++)
    for (int a = 0; a < 6; a++) {
      double v = F(j, 0, a) * B(j, 0) + F(j, 1, a) * B(j, 1);
      for (int p = 0; p < 3; p++) v -= FtE[(size_t)j * 18 + a * 3 + p] * PEtb[p];
      aug[(size_t)(N - 1) * N + (6 * j + a)] = v;
      aug[(size_t)(6 * j + a) * N + (N - 1)] = v;
    }
  aug[(size_t)N * N - 1] = bb - (Etb[0] * PEtb[0] + Etb[1] * PEtb[1] + Etb[2] * PEtb[2]);
  return LMGPU_OK;
}

int lmgpu_smart_reset(lmgpu_handle* h) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized) {
    h->err = "lmgpu_smart_reset: refused (!h->finalized)";
    return LMGPU_INVALID;
  }
  SmartState* s = h->smart;
  if (!s || s->n == 0) return LMGPU_OK;
  int rc = need_device(h);
  if (rc) return rc;
  HIPCHECK(hipMemsetAsync(s->set[s->cur].have, 0, (size_t)s->n * sizeof(int32_t), h->stream));
  return LMGPU_OK;
}

int lmgpu_get_smart_stats(const lmgpu_handle* h, lmgpu_smart_stats* out) {
  if (!h || !out) return LMGPU_INVALID;
  *out = lmgpu_smart_stats{};
  const SmartState* s = h->smart;
  if (!h->finalized) return LMGPU_INVALID;
  if (!s || s->n == 0) return LMGPU_OK;
  out->n_factors = s->n;
  if (!s->on_device) return LMGPU_OK;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return LMGPU_HIP_ERROR;
  std::vector<int32_t> st(s->n), re(s->n);
  if (hipMemcpy(st.data(), s->set[s->cur].status, (size_t)s->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return LMGPU_HIP_ERROR;
  if (hipMemcpy(re.data(), s->d_retri[s->cur], (size_t)s->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return LMGPU_HIP_ERROR;
  for (int i = 0; i < s->n; i++) {
    if (st[i] >= 0 && st[i] < 6) out->n_status[st[i]]++;
    out->retriangulations += re[i] != 0;
  }
  float ms = 0.f;
  // (events per cache set: the time of the launches that wrote the committed set, like the counts)
  if (s->timed_tri[s->cur] && hipEventElapsedTime(&ms, s->ev[2 * s->cur], s->ev[2 * s->cur + 1]) == hipSuccess) out->triangulate_ms = ms;
  if (s->timed_lin && hipEventElapsedTime(&ms, s->ev[4], s->ev[5]) == hipSuccess) out->linearize_ms = ms;
  return LMGPU_OK;
}

}  // extern "C"
