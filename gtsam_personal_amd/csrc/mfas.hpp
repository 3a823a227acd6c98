// MFAS on the device: host side of lmgpu_mfas_outlier_weights (kernels_mfas.hpp).  Included by lmgpu.hip.  Stateless: one call checks the
// edge list, builds the node index and the CSR of incident edges, runs one launch over all directions and one for the per-edge sum.
#pragma once

#include "kernels_mfas.hpp"

namespace {

thread_local std::string mfas_err;

int mfas_fail(const char* msg, int code = LMGPU_INVALID) {
  mfas_err = msg;
  return code;
}

struct MfasBuffers {
  std::vector<void*> ptrs;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~MfasBuffers() {
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  template <class T>
  hipError_t alloc(T** dst, size_t n) {
    hipError_t e = hipMalloc((void**)dst, std::max<size_t>(1, n) * sizeof(T));
    if (e == hipSuccess) ptrs.push_back(*dst);
    return e;
  }
  template <class T>
  hipError_t upload(T** dst, const T* src, size_t n) {
    hipError_t e = alloc(dst, n);
    if (e == hipSuccess && n) e = hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};

}  // namespace

extern "C" {

const char* lmgpu_mfas_last_error(void) { return mfas_err.c_str(); }

int lmgpu_mfas_lds_node_capacity(void) { return kMfasLdsNodes; }

int lmgpu_mfas_outlier_weights(int32_t device, int32_t n_edges, const uint64_t* keys, const double* measured, int32_t n_dirs, const double* dirs,
                               const double* edge_weights, uint64_t* ordering_out, double* weights_out, double* sum_out, lmgpu_mfas_stats* stats) {
  if (n_edges <= 0 || n_dirs <= 0 || !keys) return mfas_fail("lmgpu_mfas_outlier_weights: refused (n_edges <= 0 || n_dirs <= 0 || !keys)");
  if ((edge_weights != nullptr) == (measured != nullptr || dirs != nullptr) || (!edge_weights && (!measured || !dirs)))
    return mfas_fail("lmgpu_mfas_outlier_weights: give either measured directions with projection directions, or edge weights");
  const int E = n_edges, D = n_dirs;
  if ((size_t)D * (size_t)E > (size_t)1 << 30) return mfas_fail("lmgpu_mfas_outlier_weights: refused (n_dirs * n_edges > 2^30)");
  const double* fin[3] = {measured, dirs, edge_weights};
  const size_t nfin[3] = {measured ? 3 * (size_t)E : 0, dirs ? 3 * (size_t)D : 0, edge_weights ? (size_t)D * E : 0};
  for (int a = 0; a < 3; a++)
    for (size_t i = 0; i < nfin[a]; i++)
      if (!std::isfinite(fin[a][i])) return mfas_fail("lmgpu_mfas_outlier_weights: refused (a non-finite input)");
  // nodes in ascending key order; an unordered pair at most once, no self edge
  std::vector<uint64_t> nodes(keys, keys + 2 * (size_t)E);
  std::sort(nodes.begin(), nodes.end());
  nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
  const int V = (int)nodes.size();
  std::vector<int32_t> ea(E), eb(E);
  {
    std::vector<std::pair<int32_t, int32_t>> pairs(E);
    for (int e = 0; e < E; e++) {
      ea[e] = (int32_t)(std::lower_bound(nodes.begin(), nodes.end(), keys[2 * e]) - nodes.begin());
      eb[e] = (int32_t)(std::lower_bound(nodes.begin(), nodes.end(), keys[2 * e + 1]) - nodes.begin());
      if (ea[e] == eb[e]) return mfas_fail("lmgpu_mfas_outlier_weights: refused (an edge from a node to itself)");
      pairs[e] = {std::min(ea[e], eb[e]), std::max(ea[e], eb[e])};
    }
    std::sort(pairs.begin(), pairs.end());
    if (std::adjacent_find(pairs.begin(), pairs.end()) != pairs.end())
      return mfas_fail("lmgpu_mfas_outlier_weights: refused (an unordered pair of nodes is given twice)");
  }
  if (stats) {
    stats->n_nodes = V;
    stats->lds_node_capacity = kMfasLdsNodes;
    stats->global_state = 0;
    stats->kernel_ms = 0.0;
  }
  if (device < 0) return mfas_fail("lmgpu_mfas_outlier_weights: no device", LMGPU_HIP_ERROR);
  if (!weights_out && !sum_out && !ordering_out) return LMGPU_OK;
  std::vector<int32_t> ptr(V + 1, 0), inc(2 * (size_t)E);
  for (int e = 0; e < E; e++) {
    ptr[ea[e] + 1]++;
    ptr[eb[e] + 1]++;
  }
  for (int i = 0; i < V; i++) ptr[i + 1] += ptr[i];
  {
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int e = 0; e < E; e++) {  // ascending e: each node's list is in edge order
      inc[fill[ea[e]]++] = e;
      inc[fill[eb[e]]++] = e;
    }
  }
  const bool global = V > kMfasLdsNodes || dev_switch("LMGPU_MFAS_GLOBAL") != nullptr;
  if (stats) stats->global_state = global ? 1 : 0;
#define MFCHECK(expr)                                                        \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      mfas_err = std::string(#expr) + ": " + hipGetErrorString(_e);          \
      return LMGPU_HIP_ERROR;                                                \
    }                                                                        \
  } while (0)
  MFCHECK(hipSetDevice(device));
  MfasBuffers B;
  MfasArgs A{};
  A.V = V;
  A.E = E;
  A.D = D;
  int32_t *d_ea, *d_eb, *d_ptr, *d_inc, *d_order, *d_gpos = nullptr;
  double *d_meas = nullptr, *d_dirs = nullptr, *d_w, *d_wout, *d_sum, *d_gstate = nullptr;
  MFCHECK(B.upload(&d_ea, ea.data(), ea.size()));
  MFCHECK(B.upload(&d_eb, eb.data(), eb.size()));
  MFCHECK(B.upload(&d_ptr, ptr.data(), ptr.size()));
  MFCHECK(B.upload(&d_inc, inc.data(), inc.size()));
  if (edge_weights) {
    MFCHECK(B.upload(&d_w, (double*)edge_weights, (size_t)D * E));
  } else {
    MFCHECK(B.upload(&d_meas, (double*)measured, 3 * (size_t)E));
    MFCHECK(B.upload(&d_dirs, (double*)dirs, 3 * (size_t)D));
    MFCHECK(B.alloc(&d_w, (size_t)D * E));
  }
  MFCHECK(B.alloc(&d_wout, (size_t)D * E));
  MFCHECK(B.alloc(&d_sum, (size_t)E));
  MFCHECK(B.alloc(&d_order, (size_t)D * V));
  if (global) {
    MFCHECK(B.alloc(&d_gstate, (size_t)D * 2 * V));
    MFCHECK(B.alloc(&d_gpos, (size_t)D * V));
  }
  A.ea = d_ea;
  A.eb = d_eb;
  A.meas = d_meas;
  A.dirs = d_dirs;
  A.w = d_w;
  A.ptr = d_ptr;
  A.inc = d_inc;
  A.gstate = d_gstate;
  A.gpos = d_gpos;
  A.order = d_order;
  A.wout = d_wout;
  MFCHECK(hipEventCreate(&B.ev[0]));
  MFCHECK(hipEventCreate(&B.ev[1]));
  MFCHECK(hipEventRecord(B.ev[0], nullptr));
  if (global) {
    hipLaunchKernelGGL(mfas_kernel<true>, dim3(D), dim3(MFAS_THREADS), 0, nullptr, A);
  } else {
    const size_t lds = (size_t)V * 20 + 16;
    if (lds > 64 * 1024)  // above the default limit of a launch only: small calls skip the attribute call
      MFCHECK(hipFuncSetAttribute((const void*)mfas_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kMfasLdsBytes + 16));
    hipLaunchKernelGGL(mfas_kernel<false>, dim3(D), dim3(MFAS_THREADS), lds, nullptr, A);
  }
  MFCHECK(hipGetLastError());
  hipLaunchKernelGGL(mfas_sum_kernel, dim3((E + 255) / 256), dim3(256), 0, nullptr, E, D, (const double*)d_wout, d_sum);
  MFCHECK(hipGetLastError());
  MFCHECK(hipEventRecord(B.ev[1], nullptr));
  MFCHECK(hipEventSynchronize(B.ev[1]));
  float ms = 0;
  MFCHECK(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
  if (stats) stats->kernel_ms = ms;
  if (weights_out) MFCHECK(hipMemcpy(weights_out, d_wout, (size_t)D * E * sizeof(double), hipMemcpyDeviceToHost));
  if (sum_out) MFCHECK(hipMemcpy(sum_out, d_sum, (size_t)E * sizeof(double), hipMemcpyDeviceToHost));
  if (ordering_out) {
    std::vector<int32_t> ord((size_t)D * V);
    MFCHECK(hipMemcpy(ord.data(), d_order, ord.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ord.size(); i++) {
      if (ord[i] < 0 || ord[i] >= V) return mfas_fail("lmgpu_mfas_outlier_weights: the ordering is incomplete", LMGPU_HIP_ERROR);
      ordering_out[i] = nodes[ord[i]];
    }
  }
#undef MFCHECK
  return LMGPU_OK;
}

}  // extern "C"
