// Marginal covariances of many variables from ONE factorization (C ABI: lmgpu_marginals_*, lmgpu_marginal_covariances).
// Marginals::Marginals (gtsam/nonlinear/Marginals.cpp:28-43) linearizes at the solution and eliminates once; every marginalCovariance
// (:124-127) is answered from the Bayes tree.  Here: lmgpu_marginals_factor = linearize + the undamped elimination of every LM step, whose
// [R S d] stay in the pool; a query walks each variable's path to its root (marginal_path_kernel), one workgroup per variable, one launch
// and one download per chunk of requests.  Cross-covariances and joint marginals (lmgpu_marginal_cross_covariances,
// lmgpu_joint_marginal_covariances) come from the same factorization: marginal_cross_kernel walks a source's path and
// then descends each target's branch below the junction of the two paths.  Everything that overwrites the fronts or moves the values clears marg_valid; a stale
// factorization is rebuilt by the next query.  Included by lmgpu.hip.
#pragma once

struct MargState {
  int64_t scratch_bytes = 64ll << 20;  // byte budget of the scratch buffer (lmgpu_set_marginals_params); DESIGN section 17
  int32_t lds_doubles = 6144;          // LDS window of a work vector: 48 KiB, three workgroups per CU at the widest
  lmgpu_marginals_stats stats{};
  MargReq* d_reqs = nullptr;
  double *d_out = nullptr, *d_scratch = nullptr;
  int32_t* d_status = nullptr;
  size_t reqs_cap = 0, status_cap = 0, out_cap = 0, scratch_cap = 0;
  bool attr_set = false;
  // cross-covariances
  int32_t cross_cap = 0;  // targets per workgroup, forced; 0: the built-in rule (lmgpu_set_marginals_cross_cap)
  CrossReq* d_creqs = nullptr;
  CrossTgt* d_ctgts = nullptr;
  size_t creqs_cap = 0, ctgts_cap = 0;
  bool cross_attr_set = false;
};

static void marg_release(lmgpu_handle* h) {
  MargState* s = h->marg;
  if (!s) return;
  void* ptrs[] = {s->d_reqs, s->d_out, s->d_scratch, s->d_status, s->d_creqs, s->d_ctgts};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete s;
  h->marg = nullptr;
}

namespace {

const int kMargChunkMax = 16384;                 // requests per launch at most
const int kMargLdsMax = 18432 - MP_BS * MP_MAXD;  // doubles: 144 KiB of LDS per workgroup less the block staging
// targets of one source that one workgroup of marginal_cross_kernel serves after its walk of the source's path: a source with more is
// split over several workgroups, each repeating the source walk.  A branch descent is serial inside its workgroup, a repeated source walk
// runs beside the others, so a request is first spread over kMargCrossFill workgroups (one target each) and only a larger one gives a
// workgroup more targets, kMargCrossTargets at most (measured: DESIGN section 18).  lmgpu_set_marginals_cross_cap forces a run length.
const int kMargCrossTargets = 16;
const int kMargCrossFill = 1024;

MargState* marg_state(lmgpu_handle* h) {
  if (!h->marg) h->marg = new MargState();
  return h->marg;
}

// columns the kernel carries for a variable of dimension d (marginal_path_kernel's three instantiations)
int marg_dp(int d) { return d <= 3 ? 3 : (d <= 6 ? 6 : 9); }

// the refusals every marginal path call shares (lmgpu_joint_marginal_covariance's, word for word where they coincide)
int marg_refused(lmgpu_handle* h, const char* who) {
  if (!h->finalized) {
    h->err = std::string(who) + ": refused (!h->finalized)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "the marginal covariances")) return LMGPU_INVALID;
  if (h->cfg.world_size > 1) {
    h->err = "marginal covariances are computed on one GPU";
    return LMGPU_INVALID;
  }
  if (h->pcg_structure) {
    h->err = "marginal covariances need the fronts of the direct solver; this handle was finalized under PCG";
    return LMGPU_INVALID;
  }
  if (h->device >= 0 && !h->have_values) {  // (a structure-only handle: need_device has the message)
    h->err = std::string(who) + ": refused (!h->have_values)";
    return LMGPU_INVALID;
  }
  return LMGPU_OK;
}

int marg_factor(lmgpu_handle* h) {
  int rc = do_linearize(h);
  if (rc) return rc;
  if ((rc = fill_dampw(h, 0, 0.0, 0.0))) return rc;
  h->marg_factoring = true;  // (a handle whose solver was switched to PCG after finalize still eliminates here)
  rc = do_solve(h, 0.0);
  h->marg_factoring = false;
  if (rc) return rc;  // LMGPU_INDETERMINATE like Marginals' IndeterminantLinearSystemException
  h->marg_valid = true;
  marg_state(h)->stats.factorizations++;
  return LMGPU_OK;
}

template <typename X>
int marg_reserve(lmgpu_handle* h, X** p, size_t* cap, size_t want) {
  if (want <= *cap) return LMGPU_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  HIPCHECK(hipMalloc((void**)p, want * sizeof(X)));
  *cap = want;
  return LMGPU_OK;
}

}  // namespace

extern "C" {

int lmgpu_set_marginals_params(lmgpu_handle* h, int64_t scratch_bytes, int32_t lds_doubles) {
  if (!h) return LMGPU_INVALID;
  if (scratch_bytes < 0 || lds_doubles < 0 || lds_doubles > kMargLdsMax) {
    h->err = "lmgpu_set_marginals_params: refused (scratch_bytes < 0 || lds_doubles < 0 || lds_doubles > " + std::to_string(kMargLdsMax) + ")";
    return LMGPU_INVALID;
  }
  MargState* s = marg_state(h);
  if (scratch_bytes > 0) s->scratch_bytes = scratch_bytes;
  if (lds_doubles > 0) s->lds_doubles = lds_doubles;
  return LMGPU_OK;
}

int lmgpu_get_marginals_stats(lmgpu_handle* h, lmgpu_marginals_stats* out) {
  if (!h || !out) return LMGPU_INVALID;
  MargState* s = marg_state(h);
  *out = s->stats;
  out->lds_capacity = s->lds_doubles;
  out->scratch_bytes = s->scratch_bytes;
  out->cross_cap = s->cross_cap > 0 ? s->cross_cap : kMargCrossTargets;
  return LMGPU_OK;
}

int lmgpu_marginals_path(const lmgpu_handle* h, int32_t slot, int32_t* fronts_out, int32_t cap) {
  if (!h || !h->finalized || h->pcg_structure || slot < 0 || slot >= h->plan.n_vars - h->n_hidden) return -1;
  const Plan& P = h->plan;
  int n = 0;
  for (int f = P.front_of_var[slot + h->n_hidden]; f >= 0; f = P.fronts[f].parent, n++)
    if (fronts_out && n < cap) fronts_out[n] = f;
  return n;
}

int lmgpu_marginals_front_offsets(const lmgpu_handle* h, int32_t front, int32_t* poff, int32_t* spos, int32_t cap) {
  if (!h || !h->finalized || h->pcg_structure || front < 0 || front >= (int)h->plan.fronts.size() || !h->front_active[front]) return -1;
  const FrontDesc& F = h->h_fronts[front];
  const int ns = F.n - F.nf - 1;
  if (poff) *poff = h->marg_poff[front];
  if (spos)
    for (int j = 0; j < ns && j < cap; j++) spos[j] = h->marg_spos[F.sx_begin + j];
  return ns;
}

int lmgpu_marginals_factor(lmgpu_handle* h) {
  if (!h) return LMGPU_INVALID;
  int rc = marg_refused(h, "lmgpu_marginals_factor");
  if (rc) return rc;
  if ((rc = need_device(h))) return rc;
  return marg_factor(h);
}

int lmgpu_marginal_covariances(lmgpu_handle* h, int32_t n, const int32_t* slots, double* cov_packed) {
  if (!h) return LMGPU_INVALID;
  int rc = marg_refused(h, "lmgpu_marginal_covariances");
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!slots || !cov_packed))) {
    h->err = "lmgpu_marginal_covariances: refused (n < 0 || !slots || !cov_packed)";
    return LMGPU_INVALID;
  }
  const Plan& P = h->plan;
  for (int a = 0; a < n; a++)
    if (slots[a] < 0 || slots[a] >= P.n_vars) {  // before anything is written
      h->err = "lmgpu_marginal_covariances: slot " + std::to_string(slots[a]) + " (request " + std::to_string(a) + ") is out of range";
      return LMGPU_INVALID;
    }
  if (n == 0) return LMGPU_OK;
  if ((rc = need_device(h))) return rc;
  if (!h->marg_valid && (rc = marg_factor(h))) return rc;
  MargState* s = marg_state(h);
  hipStream_t st = h->stream;
  if (!s->attr_set) {
    HIPCHECK(hipFuncSetAttribute((const void*)marginal_path_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (kMargLdsMax + MP_BS * MP_MAXD) * 8));
    s->attr_set = true;
  }
  const int64_t budget = s->scratch_bytes / 8;  // doubles
  std::vector<MargReq> reqs;
  std::vector<int32_t> status;
  std::vector<double> blocks;
  size_t done_out = 0;  // doubles of cov_packed already written
  bool indeterminate = false;
  for (int a0 = 0; a0 < n;) {
    // one chunk: requests in order until the scratch slices would pass the budget or the launch is full
    reqs.clear();
    int64_t used = 0, out_off = 0;
    int lds_need = 0;
    int a = a0;
    for (; a < n && (int)reqs.size() < kMargChunkMax; a++) {
      const int v = slots[a], f = P.front_of_var[v], d = P.dims[v];
      const int L = h->marg_poff[f] + P.fronts[f].nf, need = L * marg_dp(d) + (h->marg_depth[f] + 2) / 2;
      MargReq r{f, h->marg_vcol[v], d, need, -1, out_off};
      if (need > s->lds_doubles) {
        if (need > budget) {
          h->err = "lmgpu_marginal_covariances: the path of slot " + std::to_string(v) + " needs " + std::to_string((int64_t)need * 8) +
                   " bytes of scratch, the budget is " + std::to_string(s->scratch_bytes) + " (lmgpu_set_marginals_params)";
          return LMGPU_INVALID;
        }
        if (used + need > budget) break;  // the next chunk
        r.scratch = used;
        used += need;
      } else {
        lds_need = std::max(lds_need, need);
      }
      reqs.push_back(r);
      out_off += (int64_t)d * d;
      s->stats.longest_path = std::max(s->stats.longest_path, h->marg_depth[f] + 1);
    }
    const int m = (int)reqs.size();
    if ((rc = marg_reserve(h, &s->d_reqs, &s->reqs_cap, (size_t)m))) return rc;
    if ((rc = marg_reserve(h, &s->d_status, &s->status_cap, (size_t)m))) return rc;
    if ((rc = marg_reserve(h, &s->d_out, &s->out_cap, (size_t)out_off))) return rc;
    if ((rc = marg_reserve(h, &s->d_scratch, &s->scratch_cap, (size_t)std::max<int64_t>(used, 1)))) return rc;
    HIPCHECK(hipMemcpyAsync(s->d_reqs, reqs.data(), (size_t)m * sizeof(MargReq), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(s->d_status, 0, (size_t)m * sizeof(int32_t), st));
    const size_t lds = (size_t)(MP_BS * MP_MAXD + lds_need) * sizeof(double);
    hipLaunchKernelGGL(marginal_path_kernel, dim3(m), dim3(MP_THREADS), lds, st, (const MargReq*)s->d_reqs, (const FrontDesc*)h->d_fronts,
                       (const int32_t*)h->d_marg_parent, (const int32_t*)h->d_marg_poff, (const int32_t*)h->d_marg_spos, (const double*)h->pool,
                       s->d_scratch, lds_need, s->d_out, s->d_status);
    HIPCHECK(hipGetLastError());
    // one download per chunk: the blocks lie back to back in the order of the requests, as the caller wants them
    status.resize(m);
    blocks.resize((size_t)out_off);
    HIPCHECK(hipMemcpyAsync(blocks.data(), s->d_out, (size_t)out_off * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(status.data(), s->d_status, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    std::memcpy(cov_packed + done_out, blocks.data(), (size_t)out_off * sizeof(double));
    done_out += (size_t)out_off;
    s->stats.launches++;
    s->stats.chunks++;
    for (int q = 0; q < m; q++) {
      if (reqs[q].scratch >= 0) s->stats.vars_scratch++;
      else s->stats.vars_lds++;
      if (status[q] == 2) {
        h->err = "lmgpu_marginal_covariances: a work vector passed its LDS window (request " + std::to_string(a0 + q) + ")";
        return LMGPU_HIP_ERROR;
      }
      if (status[q] != 0 && !indeterminate) {
        indeterminate = true;
        h->failed_slot = slots[a0 + q];
      }
    }
    a0 = a;
  }
  return indeterminate ? LMGPU_INDETERMINATE : LMGPU_OK;
}

}  // extern "C"

namespace {

// the deepest front on the paths of both fronts; -1: different trees
int marg_junction(const lmgpu_handle* h, int fa, int fb) {
  const Plan& P = h->plan;
  while (h->marg_depth[fa] > h->marg_depth[fb]) fa = P.fronts[fa].parent;
  while (h->marg_depth[fb] > h->marg_depth[fa]) fb = P.fronts[fb].parent;
  while (fa != fb && fa >= 0 && fb >= 0) fa = P.fronts[fa].parent, fb = P.fronts[fb].parent;
  return (fa == fb) ? fa : -1;
}

int marg_path_scalars(const lmgpu_handle* h, int slot) {
  const int f = h->plan.front_of_var[slot];
  return h->marg_poff[f] + h->plan.fronts[f].nf;
}

// the source of an unordered pair, a rule of the pair alone: the variable with the shorter path (scalars), ties to the smaller slot
bool marg_source_is_first(const lmgpu_handle* h, int a, int b) {
  const int la = marg_path_scalars(h, a), lb = marg_path_scalars(h, b);
  return la != lb ? la < lb : a < b;
}

struct CrossPair {
  int32_t i, j;  // Sigma[i, j]: the target and the source
  int64_t out;   // where its dim_i x dim_j block goes in the caller's buffer (doubles)
};

// Sigma[i, j] for every pair, each written at its own offset of `out`.  Pairs are grouped by source, a source's targets ordered deepest
// junction first and cut into runs of at most the cap; one workgroup per run, one launch and one download per chunk of workgroups.
int marg_cross_run(lmgpu_handle* h, const char* who, const std::vector<CrossPair>& pairs, double* out) {
  if (pairs.empty()) return LMGPU_OK;
  int rc = need_device(h);
  if (rc) return rc;
  if (!h->marg_valid && (rc = marg_factor(h))) return rc;
  const Plan& P = h->plan;
  MargState* s = marg_state(h);
  hipStream_t st = h->stream;
  if (!s->cross_attr_set) {
    HIPCHECK(hipFuncSetAttribute((const void*)marginal_cross_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (kMargLdsMax + MP_BS * MP_MAXD) * 8));
    s->cross_attr_set = true;
  }
  const int cap = s->cross_cap > 0 ? s->cross_cap : std::min(kMargCrossTargets, std::max(1, ((int)pairs.size() + kMargCrossFill - 1) / kMargCrossFill));
  const int64_t budget = s->scratch_bytes / 8;  // doubles
  const int np = (int)pairs.size();
  std::vector<int32_t> junc(np), jdepth(np), order(np);
  for (int q = 0; q < np; q++) {
    junc[q] = marg_junction(h, P.front_of_var[pairs[q].i], P.front_of_var[pairs[q].j]);
    jdepth[q] = junc[q] < 0 ? -1 : h->marg_depth[junc[q]];
    order[q] = q;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    if (pairs[a].j != pairs[b].j) return pairs[a].j < pairs[b].j;
    return jdepth[a] > jdepth[b];
  });
  // the workgroups: runs of one source's targets
  struct Run { int begin, count, lw, need; };
  std::vector<Run> runs;
  for (int a = 0; a < np;) {
    const int vj = pairs[order[a]].j, fj = P.front_of_var[vj], dp = marg_dp(P.dims[vj]);
    int b = a, lw = h->marg_poff[fj] + P.fronts[fj].nf, branch = 0;
    for (; b < np && b - a < cap && pairs[order[b]].j == vj; b++) {
      const int q = order[b], fi = P.front_of_var[pairs[q].i];
      if (junc[q] < 0 || junc[q] == fi) continue;
      lw = std::max(lw, h->marg_poff[fi] + P.fronts[fi].nf);
      branch = std::max(branch, h->marg_depth[fi] - jdepth[q]);
    }
    const int need = lw * dp + (h->marg_depth[fj] + 1 + branch + 1) / 2;
    if (need > s->lds_doubles && need > budget) {
      h->err = std::string(who) + ": the paths of slot " + std::to_string(vj) + " and its targets need " + std::to_string((int64_t)need * 8) +
               " bytes of scratch, the budget is " + std::to_string(s->scratch_bytes) + " (lmgpu_set_marginals_params)";
      return LMGPU_INVALID;
    }
    runs.push_back(Run{a, b - a, lw, need});
    s->stats.longest_union = std::max(s->stats.longest_union, h->marg_depth[fj] + 1 + branch);
    a = b;
  }
  std::vector<CrossReq> reqs;
  std::vector<CrossTgt> tgts;
  std::vector<int32_t> status;
  std::vector<double> blocks;
  bool indeterminate = false;
  for (size_t r0 = 0; r0 < runs.size();) {
    reqs.clear();
    tgts.clear();
    int64_t used = 0, out_off = 0;
    int lds_need = 0;
    size_t r = r0;
    for (; r < runs.size() && (int)reqs.size() < kMargChunkMax; r++) {
      const Run& R = runs[r];
      const int vj = pairs[order[R.begin]].j, fj = P.front_of_var[vj], dj = P.dims[vj];
      CrossReq c{fj, h->marg_vcol[vj], dj, R.lw, R.need, (int32_t)tgts.size(), R.count, 0, -1};
      if (R.need > s->lds_doubles) {
        if (used + R.need > budget) break;  // the next chunk
        c.scratch = used;
        used += R.need;
      } else {
        lds_need = std::max(lds_need, R.need);
      }
      reqs.push_back(c);
      for (int k = 0; k < R.count; k++) {
        const int q = order[R.begin + k], vi = pairs[q].i;
        tgts.push_back(CrossTgt{P.front_of_var[vi], h->marg_vcol[vi], P.dims[vi], junc[q], vi == vj ? 1 : 0, 0, out_off});
        out_off += (int64_t)P.dims[vi] * dj;
      }
    }
    const int m = (int)reqs.size();
    if ((rc = marg_reserve(h, &s->d_creqs, &s->creqs_cap, (size_t)m))) return rc;
    if ((rc = marg_reserve(h, &s->d_ctgts, &s->ctgts_cap, tgts.size()))) return rc;
    if ((rc = marg_reserve(h, &s->d_status, &s->status_cap, (size_t)m))) return rc;
    if ((rc = marg_reserve(h, &s->d_out, &s->out_cap, (size_t)out_off))) return rc;
    if ((rc = marg_reserve(h, &s->d_scratch, &s->scratch_cap, (size_t)std::max<int64_t>(used, 1)))) return rc;
    HIPCHECK(hipMemcpyAsync(s->d_creqs, reqs.data(), (size_t)m * sizeof(CrossReq), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(s->d_ctgts, tgts.data(), tgts.size() * sizeof(CrossTgt), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(s->d_status, 0, (size_t)m * sizeof(int32_t), st));
    const size_t lds = (size_t)(MP_BS * MP_MAXD + lds_need) * sizeof(double);
    hipLaunchKernelGGL(marginal_cross_kernel, dim3(m), dim3(MP_THREADS), lds, st, (const CrossReq*)s->d_creqs, (const CrossTgt*)s->d_ctgts,
                       (const FrontDesc*)h->d_fronts, (const int32_t*)h->d_marg_parent, (const int32_t*)h->d_marg_poff,
                       (const int32_t*)h->d_marg_spos, (const double*)h->pool, s->d_scratch, lds_need, s->d_out, s->d_status);
    HIPCHECK(hipGetLastError());
    status.resize(m);
    blocks.resize((size_t)out_off);
    HIPCHECK(hipMemcpyAsync(blocks.data(), s->d_out, (size_t)out_off * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(status.data(), s->d_status, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    s->stats.cross_launches++;
    s->stats.cross_chunks++;
    for (int w = 0; w < m; w++) {
      const Run& R = runs[r0 + w];
      const int vj = pairs[order[R.begin]].j;
      s->stats.cross_walks++;
      s->stats.cross_targets += R.count;
      if (reqs[w].scratch >= 0) s->stats.cross_scratch++;
      else s->stats.cross_lds++;
      if (status[w] == 2) {
        h->err = std::string(who) + ": a work vector passed its LDS window (source slot " + std::to_string(vj) + ")";
        return LMGPU_HIP_ERROR;
      }
      if (status[w] != 0 && !indeterminate) {
        indeterminate = true;
        h->failed_slot = vj;
      }
      for (int k = 0; k < R.count; k++) {
        const int q = order[R.begin + k];
        const CrossTgt& T = tgts[reqs[w].t_begin + k];
        std::memcpy(out + pairs[q].out, blocks.data() + T.out, (size_t)T.dim * P.dims[vj] * sizeof(double));
      }
    }
    r0 = r;
  }
  return indeterminate ? LMGPU_INDETERMINATE : LMGPU_OK;
}

}  // namespace

extern "C" {

int lmgpu_set_marginals_cross_cap(lmgpu_handle* h, int32_t targets_per_workgroup) {
  if (!h) return LMGPU_INVALID;
  if (targets_per_workgroup < 0) {
    h->err = "lmgpu_set_marginals_cross_cap: refused (targets_per_workgroup < 0)";
    return LMGPU_INVALID;
  }
  marg_state(h)->cross_cap = targets_per_workgroup;
  return LMGPU_OK;
}

int lmgpu_marginals_junction(const lmgpu_handle* h, int32_t slot_i, int32_t slot_j) {
  if (!h || !h->finalized || h->pcg_structure) return -1;
  const int nv = h->plan.n_vars - h->n_hidden;
  if (slot_i < 0 || slot_i >= nv || slot_j < 0 || slot_j >= nv) return -1;
  return marg_junction(h, h->plan.front_of_var[slot_i + h->n_hidden], h->plan.front_of_var[slot_j + h->n_hidden]);
}

int lmgpu_marginal_cross_covariances(lmgpu_handle* h, int32_t n, const int32_t* slots_i, const int32_t* slots_j, double* out_packed) {
  if (!h) return LMGPU_INVALID;
  int rc = marg_refused(h, "lmgpu_marginal_cross_covariances");
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!slots_i || !slots_j || !out_packed))) {
    h->err = "lmgpu_marginal_cross_covariances: refused (n < 0 || !slots_i || !slots_j || !out_packed)";
    return LMGPU_INVALID;
  }
  const Plan& P = h->plan;
  for (int a = 0; a < n; a++)
    for (int v : {slots_i[a], slots_j[a]})
      if (v < 0 || v >= P.n_vars) {  // before anything is written
        h->err = "lmgpu_marginal_cross_covariances: slot " + std::to_string(v) + " (pair " + std::to_string(a) + ") is out of range";
        return LMGPU_INVALID;
      }
  std::vector<CrossPair> pairs((size_t)std::max(n, 0));
  int64_t off = 0;
  for (int a = 0; a < n; a++) {
    pairs[a] = CrossPair{slots_i[a], slots_j[a], off};
    off += (int64_t)P.dims[slots_i[a]] * P.dims[slots_j[a]];
  }
  return marg_cross_run(h, "lmgpu_marginal_cross_covariances", pairs, out_packed);
}

int lmgpu_joint_marginal_covariances(lmgpu_handle* h, int32_t n_sets, const int32_t* set_begin, const int32_t* slots, double* cov_packed) {
  if (!h) return LMGPU_INVALID;
  int rc = marg_refused(h, "lmgpu_joint_marginal_covariances");
  if (rc) return rc;
  if (n_sets < 0 || (n_sets > 0 && (!set_begin || !slots || !cov_packed))) {
    h->err = "lmgpu_joint_marginal_covariances: refused (n_sets < 0 || !set_begin || !slots || !cov_packed)";
    return LMGPU_INVALID;
  }
  const Plan& P = h->plan;
  for (int q = 0; q < n_sets; q++) {  // before anything is written
    if (set_begin[q + 1] < set_begin[q] || set_begin[0] != 0) {
      h->err = "lmgpu_joint_marginal_covariances: set_begin does not ascend from 0 (set " + std::to_string(q) + ")";
      return LMGPU_INVALID;
    }
    for (int a = set_begin[q]; a < set_begin[q + 1]; a++) {
      if (slots[a] < 0 || slots[a] >= P.n_vars) {
        h->err = "lmgpu_joint_marginal_covariances: slot " + std::to_string(slots[a]) + " (set " + std::to_string(q) + ") is out of range";
        return LMGPU_INVALID;
      }
      for (int b = set_begin[q]; b < a; b++)
        if (slots[b] == slots[a]) {
          h->err = "lmgpu_joint_marginal_covariances: slot " + std::to_string(slots[a]) + " is listed twice in set " + std::to_string(q);
          return LMGPU_INVALID;
        }
    }
  }
  // every block once: the diagonal ones from their own variable, an off-diagonal one from the pair's source, mirrored below
  std::vector<CrossPair> pairs;
  int64_t off = 0;
  for (int q = 0; q < n_sets; q++)
    for (int a = set_begin[q]; a < set_begin[q + 1]; a++)
      for (int b = a; b < set_begin[q + 1]; b++) {
        const bool first = a == b || marg_source_is_first(h, slots[a], slots[b]);
        const int vj = first ? slots[a] : slots[b], vi = first ? slots[b] : slots[a];
        pairs.push_back(CrossPair{vi, vj, off});
        off += (int64_t)P.dims[vi] * P.dims[vj];
      }
  std::vector<double> blocks((size_t)off);
  rc = marg_cross_run(h, "lmgpu_joint_marginal_covariances", pairs, blocks.data());
  if (rc != LMGPU_OK && rc != LMGPU_INDETERMINATE) return rc;
  size_t p = 0;
  int64_t base = 0;
  std::vector<int> boff;
  for (int q = 0; q < n_sets; q++) {
    const int b0 = set_begin[q], ns = set_begin[q + 1] - b0;
    boff.assign(ns + 1, 0);
    for (int a = 0; a < ns; a++) boff[a + 1] = boff[a] + P.dims[slots[b0 + a]];
    const int D = boff[ns];
    double* M = cov_packed + base;
    for (int a = 0; a < ns; a++)
      for (int b = a; b < ns; b++, p++) {
        const CrossPair& pr = pairs[p];
        const int ti = pr.i == slots[b0 + a] ? a : b, tj = ti == a ? b : a;  // positions of the target and of the source in the set
        const int di = P.dims[pr.i], dj = P.dims[pr.j];
        const double* B = blocks.data() + pr.out;
        for (int r = 0; r < di; r++)
          for (int c = 0; c < dj; c++) {
            M[(size_t)(boff[ti] + r) * D + boff[tj] + c] = B[r * dj + c];
            if (a != b) M[(size_t)(boff[tj] + c) * D + boff[ti] + r] = B[r * dj + c];
          }
      }
    base += (int64_t)D * D;
  }
  return rc;
}

}  // extern "C"
