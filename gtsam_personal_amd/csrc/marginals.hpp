// Marginal covariances of many variables from ONE factorization (C ABI: lmgpu_marginals_*, lmgpu_marginal_covariances).
// Marginals::Marginals (gtsam/nonlinear/Marginals.cpp:28-43) linearizes at the solution and eliminates once; every marginalCovariance
// (:124-127) is answered from the Bayes tree.  Here: lmgpu_marginals_factor = linearize + the undamped elimination of every LM step, whose
// [R S d] stay in the pool; a query walks each variable's path to its root (marginal_path_kernel), one workgroup per variable, one launch
// and one download per chunk of requests.  Everything that overwrites the fronts or moves the values clears marg_valid; a stale
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
};

static void marg_release(lmgpu_handle* h) {
  MargState* s = h->marg;
  if (!s) return;
  void* ptrs[] = {s->d_reqs, s->d_out, s->d_scratch, s->d_status};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete s;
  h->marg = nullptr;
}

namespace {

const int kMargChunkMax = 16384;                 // requests per launch at most
const int kMargLdsMax = 18432 - MP_BS * MP_MAXD;  // doubles: 144 KiB of LDS per workgroup less the block staging

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
