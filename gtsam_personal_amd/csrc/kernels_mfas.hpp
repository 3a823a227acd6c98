// MFAS (minimum feedback arc set heuristic of 1dSfM; gtsam/sfm/MFAS.cpp:36-171) for D projection directions at once: one workgroup per
// direction.  Nodes are indices 0 .. V-1 in ascending key order, so "the lowest key" is the lowest index.
//   graphFromEdges       :36-60    weights, then each node's inWeightSum / outWeightSum accumulated in edge order (one lane per node walks its
//                                  incident edges, which the host lists in edge order)
//   selectNextNode...    :63-82    the lowest alive node with inWeightSum < 1e-8, else the alive node of the largest (out + 1) / (in + 1),
//                                  lowest index on ties: a wave reduction, then one over the waves' partials in LDS
//   removeNodeFromGraph  :94-112   one lane per incident edge of the selected node, one subtraction at the alive neighbour (a pair of nodes
//                                  has at most one edge, so no two lanes meet at a neighbour: no atomics)
//   computeOutlierWeights :141-171 |w| where the edge's destination precedes its source in the ordering
// The node state (in, out: double; pos: int, -1 = alive) lives in LDS, or (GLOBAL) in the direction's slice of a scratch buffer.
// Every sum is taken in the sequential algorithm's order, so the results carry its bits.
#pragma once
#include <hip/hip_runtime.h>

namespace lmgpu {

#define MFAS_THREADS 256
// LDS form: 20 B of state per node.  Of the CU's 160 KiB one workgroup asks 120 KiB of dynamic LDS for it (D is 48 in 1dSfM and the device
// has 256 CUs: one workgroup per CU is the case to size for), which leaves room for the reduction's partials and a second small kernel.
static const int kMfasLdsBytes = 120 * 1024;
static const int kMfasLdsNodes = kMfasLdsBytes / 20;  // 6144

struct MfasCand {
  int root;  // lowest alive node with inWeightSum < 1e-8, INT_MAX: none
  int hi;    // alive node of the largest heuristic, INT_MAX: none
  double h;
};
__device__ __forceinline__ MfasCand mfas_better(const MfasCand& a, const MfasCand& b) {
  MfasCand r;
  r.root = min(a.root, b.root);
  const bool takeb = b.hi != INT_MAX && (a.hi == INT_MAX || b.h > a.h || (b.h == a.h && b.hi < a.hi));
  r.hi = takeb ? b.hi : a.hi;
  r.h = takeb ? b.h : a.h;
  return r;
}

// measured.dot(projectionDirection) (:118-121) with every product and every sum rounded once, so that a numpy restatement has the same bits.
// (The HIP headers define __dmul_rn / __dadd_rn as plain * and +, which the compiler's default contraction fuses into FMAs once they are
// inlined; the pragma is what keeps the three products and two sums apart.)
__device__ __forceinline__ double mfas_dot_rn(const double* m, double dx, double dy, double dz) {
#pragma clang fp contract(off)
  const double px = m[0] * dx, py = m[1] * dy, pz = m[2] * dz;
  return (px + py) + pz;
}

struct MfasArgs {
  int V, E, D;
  const int32_t* ea;      // [E] first node of the edge's key pair
  const int32_t* eb;      // [E] second
  const double* meas;     // [E][3] measured directions, or null when the weights are given
  const double* dirs;     // [D][3] projection directions
  double* w;              // [D][E] signed weights: computed here from meas and dirs, or the caller's
  const int32_t* ptr;     // [V + 1] CSR: the incident edges of a node, in edge order
  const int32_t* inc;     // [nnz] edge index
  double* gstate;         // GLOBAL: [D][V] in, [D][V] out
  int32_t* gpos;          // GLOBAL: [D][V]
  int32_t* order;         // [D][V] node selected at each step
  double* wout;           // [D][E] outlier weights
};

template <bool GLOBAL>
__global__ __launch_bounds__(MFAS_THREADS) void mfas_kernel(MfasArgs A) {
  extern __shared__ __attribute__((aligned(16))) double mfas_lds[];
  __shared__ MfasCand part[MFAS_THREADS / 64];
  const int d = blockIdx.x, tid = threadIdx.x, V = A.V, E = A.E;
  double* in = GLOBAL ? A.gstate + (size_t)d * 2 * V : mfas_lds;
  double* out = in + V;
  int* pos = GLOBAL ? A.gpos + (size_t)d * V : (int*)(mfas_lds + 2 * (size_t)V);
  double* w = A.w + (size_t)d * E;
  if (A.meas) {
    const double dx = A.dirs[3 * d], dy = A.dirs[3 * d + 1], dz = A.dirs[3 * d + 2];
    for (int e = tid; e < E; e += MFAS_THREADS) w[e] = mfas_dot_rn(A.meas + 3 * (size_t)e, dx, dy, dz);
  }
  __syncthreads();
  for (int i = tid; i < V; i += MFAS_THREADS) {
    double si = 0.0, so = 0.0;
    for (int k = A.ptr[i]; k < A.ptr[i + 1]; k++) {
      const int e = A.inc[k];
      const double we = w[e];
      const int dest = we >= 0 ? A.eb[e] : A.ea[e];
      if (dest == i) si += fabs(we);
      else so += fabs(we);
    }
    in[i] = si;
    out[i] = so;
    pos[i] = -1;
  }
  __syncthreads();
  int32_t* order = A.order + (size_t)d * V;
  for (int step = 0; step < V; step++) {
    MfasCand c{INT_MAX, INT_MAX, 0.0};
    for (int i = tid; i < V; i += MFAS_THREADS) {
      if (pos[i] >= 0) continue;
      const double a = in[i];
      if (a < 1e-8 && c.root == INT_MAX) c.root = i;  // i ascends within a lane
      const double h = (out[i] + 1) / (a + 1);
      if (c.hi == INT_MAX || h > c.h) {
        c.hi = i;
        c.h = h;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      MfasCand o;
      o.root = __shfl_xor(c.root, off, 64);
      o.hi = __shfl_xor(c.hi, off, 64);
      o.h = __shfl_xor(c.h, off, 64);
      c = mfas_better(c, o);
    }
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    c = part[0];
#pragma unroll
    for (int k = 1; k < MFAS_THREADS / 64; k++) c = mfas_better(c, part[k]);
    const int s = c.root != INT_MAX ? c.root : c.hi;  // the same in every lane
    if (s < 0 || s >= V) {  // no candidate: only with non-finite sums, which the host refuses; leave the rest unordered
      for (int i = step + tid; i < V; i += MFAS_THREADS) order[i] = -1;
      break;
    }
    for (int k = A.ptr[s] + tid; k < A.ptr[s + 1]; k += MFAS_THREADS) {
      const int e = A.inc[k];
      const double we = w[e];
      const int a = A.ea[e], b = A.eb[e];
      const int nb = a == s ? b : a;
      if (pos[nb] >= 0) continue;
      const int dest = we >= 0 ? b : a;
      if (dest == s) out[nb] -= fabs(we);  // nb was an inNeighbor of s (:98-104)
      else in[nb] -= fabs(we);             // an outNeighbor (:106-109)
    }
    if (tid == 0) {
      pos[s] = step;
      order[step] = s;
    }
    __syncthreads();  // the state and part[] before the next selection
  }
  __syncthreads();
  double* wo = A.wout + (size_t)d * E;
  for (int e = tid; e < E; e += MFAS_THREADS) {
    const double we = w[e];
    const int src = we < 0 ? A.eb[e] : A.ea[e], dst = we < 0 ? A.ea[e] : A.eb[e];
    const int ps = pos[src], pd = pos[dst];
    wo[e] = (ps >= 0 && pd >= 0 && pd < ps) ? fabs(we) : 0.0;
  }
}

// the per-edge sum over the directions, added in direction order by one thread per edge: bitwise reproducible
__global__ __launch_bounds__(256) void mfas_sum_kernel(int E, int D, const double* __restrict__ wout, double* __restrict__ sum) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double s = 0.0;
  for (int d = 0; d < D; d++) s += wout[(size_t)d * E + e];
  sum[e] = s;
}

}  // namespace lmgpu
