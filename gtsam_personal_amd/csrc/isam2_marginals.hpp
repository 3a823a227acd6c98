// ISAM2: marginal covariances of many variables, cross-covariances of pairs and joint marginals of key sets, answered from the Bayes
// tree the last update left on the device (C ABI: lmgpu_isam2_marginal_covariances, lmgpu_isam2_cross_covariances,
// lmgpu_isam2_joint_marginal_covariances).  Nothing is re-linearized or re-eliminated: the blocks are blocks of
// (R^T R)^-1 of the present tree, the covariance at the linearization point, as ISAM2::marginalCovariance gives it
// (gtsam/nonlinear/ISAM2.h:253-257).  The route is the batch handle's (marginals.hpp: grouping by source, targets deepest junction first,
// chunks by the scratch budget, the source rule of a joint's off-diagonal blocks); the kernel is isam2_marginal_cross_kernel, which finds
// the cliques in ISAM2's device tree.  The tree is rebuilt at its top by every update, so the position tables (IsmClq, spos) are built
// here per call, from the host mirror clq[] and for the cliques on the requested paths only: there is nothing cached that could be stale.
// They travel like an update's lists (is_stage / is_flush) behind the tree patch.  lmgpu_isam2_marginal_covariance(key) keeps its own
// route.  Included by lmgpu.hip after isam2.hpp and marginals.hpp.
#pragma once

#include <unordered_map>

namespace {

struct IsmTables {
  std::vector<IsmClq> cl;                          // parents before children
  std::vector<int32_t> spos, depth, nf;            // depth, nf: parallel to cl
  std::unordered_map<int32_t, int32_t> local_of;   // clique slot -> index in cl
  std::unordered_map<int32_t, int32_t> vpos;       // variable -> path position of its first scalar (frontal variables of cl)
};

struct IsmVar {  // a variable of the request
  uint64_t key;
  int32_t q, col, dim;  // the clique (index in cl) it is frontal in, its first scalar there, its dimension
};

struct IsmPair {
  int32_t i, j;  // Sigma[i, j]: the target and the source, indices into the request's variables
  int64_t out;   // where the dim_i x dim_j block goes in the caller's buffer (doubles)
};

// the clique in `slot` and every ancestor it still lacks enter the tables; *q_out = its index
int ism_add_clique(lmgpu_isam2* S, IsmTables& T, int slot, int* q_out) {
  std::vector<int32_t> chain;
  int id = slot;
  for (; id >= 0 && !T.local_of.count(id); id = S->clq[id].parent) chain.push_back(id);
  int lp = id >= 0 ? T.local_of[id] : -1;
  for (auto it = chain.rbegin(); it != chain.rend(); ++it) {
    const lmgpu_isam2::Clq& c = S->clq[*it];
    IsmClq e{*it, lp, lp < 0 ? 0 : T.cl[lp].poff + T.nf[lp], (int32_t)T.spos.size()};
    bool ok = c.alive;
    int col = 0;
    for (int k = 0; k < c.nfv; k++) {
      T.vpos[c.vars[k]] = e.poff + col;
      col += kVarDim[S->vars[c.vars[k]].type];
    }
    ok = ok && col == c.nf;
    for (size_t k = c.nfv; k < c.vars.size() && ok; k++) {  // a separator variable is frontal in an ancestor: already in the tables
      auto p = T.vpos.find(c.vars[k]);
      ok = p != T.vpos.end() && p->second < e.poff;
      for (int d = 0; ok && d < kVarDim[S->vars[c.vars[k]].type]; d++) T.spos.push_back(p->second + d);
    }
    if (!ok || (int)T.spos.size() - e.sx_begin != c.n - c.nf - 1) {  // (never walk a table that does not describe the tree)
      S->err = "ISAM2 marginals: the host mirror of the Bayes tree is inconsistent at clique " + std::to_string(*it);
      return LMGPU_INVALID;
    }
    lp = (int)T.cl.size();
    T.local_of[*it] = lp;
    T.cl.push_back(e);
    T.nf.push_back(c.nf);
    T.depth.push_back(e.parent < 0 ? 0 : T.depth[e.parent] + 1);
  }
  *q_out = T.local_of[slot];
  return LMGPU_OK;
}

// the clique a key is frontal in; -1: the key is not in the Bayes tree (never added, gone with its last factor, marginalized)
int ism_clique_of_key(const lmgpu_isam2* S, uint64_t key) {
  auto it = S->vid_of.find(key);
  return (it == S->vid_of.end() || S->node_of[it->second] < 0) ? -1 : S->node_of[it->second];
}

int ism_refuse_key(lmgpu_isam2* S, const char* who, uint64_t key) {
  S->err = std::string(who) + ": key " + std::to_string(key) + " is not a variable of the Bayes tree";
  return LMGPU_INVALID;
}

// the request's distinct variables: V[index_of[vid]]
int ism_add_var(lmgpu_isam2* S, IsmTables& T, std::vector<IsmVar>& V, std::unordered_map<int32_t, int32_t>& index_of, uint64_t key, int32_t* at) {
  const int32_t vid = S->vid_of.find(key)->second;  // (the caller has checked the key)
  auto it = index_of.find(vid);
  if (it != index_of.end()) {
    *at = it->second;
    return LMGPU_OK;
  }
  int q;
  const int rc = ism_add_clique(S, T, S->node_of[vid], &q);
  if (rc) return rc;
  *at = (int32_t)V.size();
  index_of[vid] = *at;
  V.push_back(IsmVar{key, q, T.vpos[vid] - T.cl[q].poff, kVarDim[S->vars[vid].type]});
  return LMGPU_OK;
}

int ism_junction(const IsmTables& T, int a, int b) {
  while (T.depth[a] > T.depth[b]) a = T.cl[a].parent;
  while (T.depth[b] > T.depth[a]) b = T.cl[b].parent;
  while (a != b && a >= 0 && b >= 0) a = T.cl[a].parent, b = T.cl[b].parent;
  return a == b ? a : -1;
}

int ism_path_scalars(const IsmTables& T, const IsmVar& v) { return T.cl[v.q].poff + T.nf[v.q]; }

// the source of an unordered pair, a rule of the pair and the tree alone: the variable with the shorter path (scalars), ties to the smaller key
bool ism_source_is_first(const IsmTables& T, const IsmVar& a, const IsmVar& b) {
  const int la = ism_path_scalars(T, a), lb = ism_path_scalars(T, b);
  return la != lb ? la < lb : a.key < b.key;
}

template <typename X>
int ism_reserve(lmgpu_isam2* S, X** p, size_t* cap, size_t want) {
  if (want <= *cap) return LMGPU_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  ISCHECK(hipMalloc((void**)p, want * sizeof(X)));
  *cap = want;
  return LMGPU_OK;
}

// Sigma[i, j] for every pair, each written at its own offset of `out`.  Pairs are grouped by source, a source's targets ordered deepest
// junction first and cut into runs of at most the cap; one workgroup per run, one launch and one download per chunk of workgroups.
// as_marginals: every pair is (i, i) -- counted as launches / chunks / vars_* instead of cross_*.  Nothing is written when it refuses.
int ism_run(lmgpu_isam2* S, const char* who, IsmTables& T, const std::vector<IsmVar>& V, const std::vector<IsmPair>& pairs, double* out,
            bool as_marginals) {
  if (pairs.empty()) return LMGPU_OK;
  lmgpu_isam2::MargQ& M = S->mq;
  const int cap = M.cross_cap > 0 ? M.cross_cap : std::min(kMargCrossTargets, std::max(1, ((int)pairs.size() + kMargCrossFill - 1) / kMargCrossFill));
  const int64_t budget = M.scratch_bytes / 8;  // doubles
  const int np = (int)pairs.size();
  std::vector<int32_t> junc(np), jdepth(np), order(np);
  for (int q = 0; q < np; q++) {
    junc[q] = ism_junction(T, V[pairs[q].i].q, V[pairs[q].j].q);
    jdepth[q] = junc[q] < 0 ? -1 : T.depth[junc[q]];
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
    const int j = pairs[order[a]].j;
    const IsmVar& vj = V[j];
    const int dp = marg_dp(vj.dim);
    int b = a, lw = ism_path_scalars(T, vj), branch = 0;
    for (; b < np && b - a < cap && pairs[order[b]].j == j; b++) {
      const int q = order[b];
      const IsmVar& vi = V[pairs[q].i];
      if (junc[q] < 0 || junc[q] == vi.q) continue;
      lw = std::max(lw, ism_path_scalars(T, vi));
      branch = std::max(branch, T.depth[vi.q] - jdepth[q]);
    }
    const int64_t need = (int64_t)lw * dp + (T.depth[vj.q] + 1 + branch + 1) / 2;
    if (need > M.lds_doubles && (need > budget || need > (int64_t)INT32_MAX)) {
      S->err = std::string(who) + ": the paths of key " + std::to_string(vj.key) + " and its targets need " + std::to_string(need * 8) +
               " bytes of scratch, the budget is " + std::to_string(M.scratch_bytes) + " (lmgpu_isam2_set_marginals_params)";
      return LMGPU_INVALID;
    }
    runs.push_back(Run{a, b - a, lw, (int)need});
    if (as_marginals) M.stats.longest_path = std::max(M.stats.longest_path, T.depth[vj.q] + 1);
    else M.stats.longest_union = std::max(M.stats.longest_union, T.depth[vj.q] + 1 + branch);
    a = b;
  }

  // ---- the device: the tree patch, the call's tables (read by every workgroup, front by front: into the device arena), then the chunks
  ISCHECK(hipSetDevice(S->device));
  int rc;
  if ((rc = is_stage_recycle(S))) return rc;
  if ((rc = is_patch_tree(S))) return rc;
  if (!M.attr_set) {
    ISCHECK(hipFuncSetAttribute((const void*)isam2_marginal_cross_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (kMargLdsMax + MP_BS * MP_MAXD) * 8));
    M.attr_set = true;
  }
  IsmClq* d_cl;
  int32_t* d_spos;
  if ((rc = is_stage(S, T.cl, &d_cl, true))) return rc;
  if ((rc = is_stage(S, T.spos, &d_spos, true))) return rc;
  std::vector<CrossReq> reqs;
  std::vector<CrossTgt> tgts;
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
      const IsmVar& vj = V[pairs[order[R.begin]].j];
      CrossReq c{vj.q, vj.col, vj.dim, R.lw, R.need, (int32_t)tgts.size(), R.count, 0, -1};
      if (R.need > M.lds_doubles) {
        if (used + R.need > budget) break;  // the next chunk
        c.scratch = used;
        used += R.need;
      } else {
        lds_need = std::max(lds_need, R.need);
      }
      reqs.push_back(c);
      for (int k = 0; k < R.count; k++) {
        const int q = order[R.begin + k];
        const IsmVar& vi = V[pairs[q].i];
        tgts.push_back(CrossTgt{vi.q, vi.col, vi.dim, junc[q], pairs[q].i == pairs[q].j ? 1 : 0, 0, out_off});
        out_off += (int64_t)vi.dim * vj.dim;
      }
    }
    const int m = (int)reqs.size();
    const size_t out_doubles = (size_t)out_off + ((size_t)m + 1) / 2;  // the blocks, then one status word per workgroup
    if ((rc = ism_reserve(S, &M.d_out, &M.out_cap, out_doubles))) return rc;
    if ((rc = ism_reserve(S, &M.d_scratch, &M.scratch_cap, (size_t)std::max<int64_t>(used, 1)))) return rc;
    CrossReq* d_reqs;
    CrossTgt* d_tgts;
    if ((rc = is_stage(S, reqs, &d_reqs))) return rc;  // (read once each: in place from the pinned arena)
    if ((rc = is_stage(S, tgts, &d_tgts))) return rc;
    if ((rc = is_flush(S))) return rc;
    int32_t* d_status = (int32_t*)(M.d_out + out_off);
    const size_t lds = (size_t)(MP_BS * MP_MAXD + lds_need) * sizeof(double);
    hipLaunchKernelGGL(isam2_marginal_cross_kernel, dim3(m), dim3(MP_THREADS), lds, S->stream, (const CrossReq*)d_reqs, (const CrossTgt*)d_tgts,
                       (const IsmClq*)d_cl, (const FrontDesc*)S->d_tree, (const int32_t*)d_spos, (const double*)S->pool, M.d_scratch, lds_need,
                       M.d_out, d_status);
    ISCHECK(hipGetLastError());
    blocks.resize(out_doubles);
    ISCHECK(hipMemcpyAsync(blocks.data(), M.d_out, out_doubles * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    ISCHECK(hipStreamSynchronize(S->stream));
    const int32_t* status = (const int32_t*)(blocks.data() + out_off);
    (as_marginals ? M.stats.launches : M.stats.cross_launches)++;
    (as_marginals ? M.stats.chunks : M.stats.cross_chunks)++;
    for (int w = 0; w < m; w++) {
      const Run& R = runs[r0 + w];
      const IsmVar& vj = V[pairs[order[R.begin]].j];
      const bool in_scratch = reqs[w].scratch >= 0;
      if (as_marginals) {
        (in_scratch ? M.stats.vars_scratch : M.stats.vars_lds) += R.count;
      } else {
        M.stats.cross_walks++;
        M.stats.cross_targets += R.count;
        (in_scratch ? M.stats.cross_scratch : M.stats.cross_lds)++;
      }
      if (status[w] == 2) {
        S->err = std::string(who) + ": a work vector passed its LDS window (source key " + std::to_string(vj.key) + ")";
        return LMGPU_HIP_ERROR;
      }
      if (status[w] != 0 && !indeterminate) {
        indeterminate = true;
        S->failed_key = vj.key;
        S->err = std::string("indeterminate linear system in ") + who;
      }
      for (int k = 0; k < R.count; k++) {
        const int q = order[R.begin + k];
        const CrossTgt& G = tgts[reqs[w].t_begin + k];
        std::memcpy(out + pairs[q].out, blocks.data() + G.out, (size_t)G.dim * vj.dim * sizeof(double));
      }
    }
    r0 = r;
  }
  return indeterminate ? LMGPU_INDETERMINATE : LMGPU_OK;
}

// the keys of a request, checked before anything else happens
int ism_check_keys(lmgpu_isam2* S, const char* who, int64_t n, const uint64_t* keys) {
  for (int64_t a = 0; a < n; a++)
    if (ism_clique_of_key(S, keys[a]) < 0) return ism_refuse_key(S, who, keys[a]);
  return LMGPU_OK;
}

}  // namespace

extern "C" {

int lmgpu_isam2_set_marginals_params(lmgpu_isam2* S, int64_t scratch_bytes, int32_t lds_doubles, int32_t targets_per_workgroup) {
  if (!S) return LMGPU_INVALID;
  if (scratch_bytes < 0 || lds_doubles < 0 || lds_doubles > kMargLdsMax || targets_per_workgroup < 0) {
    S->err = "lmgpu_isam2_set_marginals_params: refused (scratch_bytes < 0 || lds_doubles < 0 || lds_doubles > " + std::to_string(kMargLdsMax) +
             " || targets_per_workgroup < 0)";
    return LMGPU_INVALID;
  }
  if (scratch_bytes > 0) S->mq.scratch_bytes = scratch_bytes;
  if (lds_doubles > 0) S->mq.lds_doubles = lds_doubles;
  if (targets_per_workgroup > 0) S->mq.cross_cap = targets_per_workgroup;
  return LMGPU_OK;
}

int lmgpu_isam2_get_marginals_stats(lmgpu_isam2* S, lmgpu_marginals_stats* out) {
  if (!S || !out) return LMGPU_INVALID;
  *out = S->mq.stats;  // (factorizations stays 0: the tree is the update's)
  out->lds_capacity = S->mq.lds_doubles;
  out->scratch_bytes = S->mq.scratch_bytes;
  out->cross_cap = S->mq.cross_cap > 0 ? S->mq.cross_cap : kMargCrossTargets;
  return LMGPU_OK;
}

int lmgpu_isam2_marginals_path(lmgpu_isam2* S, uint64_t key, uint64_t* first_frontal_keys_out, int32_t cap) {
  if (!S) return -1;
  int n = 0;
  int id = ism_clique_of_key(S, key);
  if (id < 0) return -1;
  for (; id >= 0; id = S->clq[id].parent, n++)
    if (first_frontal_keys_out && n < cap) first_frontal_keys_out[n] = S->vars[S->clq[id].vars[0]].key;
  return n;
}

int lmgpu_isam2_marginals_junction(lmgpu_isam2* S, uint64_t key_i, uint64_t key_j, uint64_t* first_frontal_key_out) {
  if (!S) return -1;
  int a = ism_clique_of_key(S, key_i), b = ism_clique_of_key(S, key_j);
  if (a < 0 || b < 0) return -1;
  auto depth = [&](int id) {
    int d = 0;
    for (; S->clq[id].parent >= 0; id = S->clq[id].parent) d++;
    return d;
  };
  int da = depth(a), db = depth(b);
  for (; da > db; da--) a = S->clq[a].parent;
  for (; db > da; db--) b = S->clq[b].parent;
  while (a != b && a >= 0 && b >= 0) a = S->clq[a].parent, b = S->clq[b].parent;
  if (a != b || a < 0) return 0;
  if (first_frontal_key_out) *first_frontal_key_out = S->vars[S->clq[a].vars[0]].key;
  return 1;
}

int lmgpu_isam2_marginal_covariances(lmgpu_isam2* S, int32_t n, const uint64_t* keys, double* cov_packed) {
  if (!S) return LMGPU_INVALID;
  const char* who = "lmgpu_isam2_marginal_covariances";
  if (n < 0 || (n > 0 && (!keys || !cov_packed))) {
    S->err = std::string(who) + ": refused (n < 0 || !keys || !cov_packed)";
    return LMGPU_INVALID;
  }
  if (n == 0) return LMGPU_OK;
  if (S->device < 0) {
    S->err = "no HIP device bound to this handle; the incremental path has no CPU fallback";
    return LMGPU_HIP_ERROR;
  }
  int rc = ism_check_keys(S, who, n, keys);
  if (rc) return rc;
  IsmTables T;
  std::vector<IsmVar> V;
  std::unordered_map<int32_t, int32_t> index_of;
  std::vector<IsmPair> pairs((size_t)n);
  int64_t off = 0;
  for (int a = 0; a < n; a++) {
    int32_t at;
    if ((rc = ism_add_var(S, T, V, index_of, keys[a], &at))) return rc;
    pairs[a] = IsmPair{at, at, off};
    off += (int64_t)V[at].dim * V[at].dim;
  }
  return ism_run(S, who, T, V, pairs, cov_packed, true);
}

int lmgpu_isam2_cross_covariances(lmgpu_isam2* S, int32_t n, const uint64_t* keys_i, const uint64_t* keys_j, double* out_packed) {
  if (!S) return LMGPU_INVALID;
  const char* who = "lmgpu_isam2_cross_covariances";
  if (n < 0 || (n > 0 && (!keys_i || !keys_j || !out_packed))) {
    S->err = std::string(who) + ": refused (n < 0 || !keys_i || !keys_j || !out_packed)";
    return LMGPU_INVALID;
  }
  if (n == 0) return LMGPU_OK;
  if (S->device < 0) {
    S->err = "no HIP device bound to this handle; the incremental path has no CPU fallback";
    return LMGPU_HIP_ERROR;
  }
  int rc;
  if ((rc = ism_check_keys(S, who, n, keys_i)) || (rc = ism_check_keys(S, who, n, keys_j))) return rc;
  IsmTables T;
  std::vector<IsmVar> V;
  std::unordered_map<int32_t, int32_t> index_of;
  std::vector<IsmPair> pairs((size_t)n);
  int64_t off = 0;
  for (int a = 0; a < n; a++) {
    int32_t ai, aj;
    if ((rc = ism_add_var(S, T, V, index_of, keys_i[a], &ai)) || (rc = ism_add_var(S, T, V, index_of, keys_j[a], &aj))) return rc;
    pairs[a] = IsmPair{ai, aj, off};
    off += (int64_t)V[ai].dim * V[aj].dim;
  }
  return ism_run(S, who, T, V, pairs, out_packed, false);
}

int lmgpu_isam2_joint_marginal_covariances(lmgpu_isam2* S, int32_t n_sets, const int32_t* set_begin, const uint64_t* keys, double* cov_packed) {
  if (!S) return LMGPU_INVALID;
  const char* who = "lmgpu_isam2_joint_marginal_covariances";
  if (n_sets < 0 || (n_sets > 0 && (!set_begin || !keys || !cov_packed))) {
    S->err = std::string(who) + ": refused (n_sets < 0 || !set_begin || !keys || !cov_packed)";
    return LMGPU_INVALID;
  }
  if (n_sets == 0) return LMGPU_OK;
  for (int q = 0; q < n_sets; q++) {  // before anything is written
    if (set_begin[0] < 0 || set_begin[q + 1] < set_begin[q]) {
      S->err = std::string(who) + ": set_begin starts below 0 or decreases (set " + std::to_string(q) + ")";
      return LMGPU_INVALID;
    }
    for (int a = set_begin[q]; a < set_begin[q + 1]; a++)
      for (int b = set_begin[q]; b < a; b++)
        if (keys[b] == keys[a]) {
          S->err = std::string(who) + ": key " + std::to_string(keys[a]) + " is listed twice in set " + std::to_string(q);
          return LMGPU_INVALID;
        }
  }
  if (set_begin[n_sets] == set_begin[0]) return LMGPU_OK;  // (empty sets only: 0 x 0 matrices)
  if (S->device < 0) {
    S->err = "no HIP device bound to this handle; the incremental path has no CPU fallback";
    return LMGPU_HIP_ERROR;
  }
  int rc = ism_check_keys(S, who, set_begin[n_sets] - set_begin[0], keys + set_begin[0]);
  if (rc) return rc;
  IsmTables T;
  std::vector<IsmVar> V;
  std::unordered_map<int32_t, int32_t> index_of;
  std::vector<int32_t> at((size_t)set_begin[n_sets], -1);
  for (int a = set_begin[0]; a < set_begin[n_sets]; a++)
    if ((rc = ism_add_var(S, T, V, index_of, keys[a], &at[a]))) return rc;
  // every block once: the diagonal ones from their own variable, an off-diagonal one from the pair's source, mirrored below
  std::vector<IsmPair> pairs;
  int64_t off = 0;
  for (int q = 0; q < n_sets; q++)
    for (int a = set_begin[q]; a < set_begin[q + 1]; a++)
      for (int b = a; b < set_begin[q + 1]; b++) {
        const bool first = a == b || ism_source_is_first(T, V[at[a]], V[at[b]]);
        const int32_t vj = first ? at[a] : at[b], vi = first ? at[b] : at[a];
        pairs.push_back(IsmPair{vi, vj, off});
        off += (int64_t)V[vi].dim * V[vj].dim;
      }
  std::vector<double> blocks((size_t)off);
  rc = ism_run(S, who, T, V, pairs, blocks.data(), false);
  if (rc != LMGPU_OK && rc != LMGPU_INDETERMINATE) return rc;
  size_t p = 0;
  int64_t base = 0;
  std::vector<int> boff;
  for (int q = 0; q < n_sets; q++) {
    const int b0 = set_begin[q], ns = set_begin[q + 1] - b0;
    boff.assign(ns + 1, 0);
    for (int a = 0; a < ns; a++) boff[a + 1] = boff[a] + V[at[b0 + a]].dim;
    const int D = boff[ns];
    double* Mx = cov_packed + base;
    for (int a = 0; a < ns; a++)
      for (int b = a; b < ns; b++, p++) {
        const IsmPair& pr = pairs[p];
        const int ti = pr.i == at[b0 + a] ? a : b, tj = ti == a ? b : a;  // positions of the target and of the source in the set
        const int di = V[pr.i].dim, dj = V[pr.j].dim;
        const double* B = blocks.data() + pr.out;
        for (int r = 0; r < di; r++)
          for (int c = 0; c < dj; c++) {
            Mx[(size_t)(boff[ti] + r) * D + boff[tj] + c] = B[r * dj + c];
            if (a != b) Mx[(size_t)(boff[tj] + c) * D + boff[ti] + r] = B[r * dj + c];
          }
      }
    base += (int64_t)D * D;
  }
  return rc;
}

}  // extern "C"
