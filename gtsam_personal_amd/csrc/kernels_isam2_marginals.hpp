// Marginal covariances of many variables, cross-covariances and joint marginals from ISAM2's device tree (isam2_marginals.hpp; DESIGN
// section 19).  The arithmetic is the batch route's (kernels_marginals.hpp: mp_front_up / mp_front_down, the same bodies through an
// MpFront view): one workgroup per SOURCE variable j walks j's path up with R^T y = e and down again with R x = y, all of j's columns
// together, then descends, per TARGET i, the branch of i's path below the junction of the two paths and writes Sigma[i, j].  A marginal
// covariance is the pair (i, i).
//
// What differs is where a clique is found.  ISAM2's tree changes shape with every update, so there are no static position tables: the
// host builds them per call from its mirror of the tree, for the cliques on the requested paths only (IsmClq: the clique's slot in
// d_tree, its parent, the position of its first frontal scalar in a path's work vector, where its separator positions start in spos[]),
// and the kernel reads [R S] where the update left it: d_tree[slot].rsd_off / ld_rsd / nf / n (an LDS clique's dense nf x n rows, a wide
// clique's rows of its n x ld block -- only columns j >= i of a row belong to R, and only those are read).  The delta offsets of the
// tree rows are not needed: the work vector is compact, the frontal scalars of the walked path only, in LDS when it fits the launch's
// window and in the workgroup's slice of a scratch buffer otherwise.  No atomics, one writer per entry and step, fixed summation order.
#pragma once
#include "kernels_marginals.hpp"

namespace lmgpu {

struct IsmClq {  // a clique of the request's tables, parents before children
  int32_t slot;      // its slot in the device tree
  int32_t parent;    // index of its parent in these tables, -1: a root
  int32_t poff;      // path position of its first frontal scalar (0 for a root, the parent's poff + the parent's nf otherwise)
  int32_t sx_begin;  // into spos[]: the path positions of its separator scalars
};

__device__ __forceinline__ MpFront ism_front_of(const int q, const IsmClq* __restrict__ cl, const FrontDesc* __restrict__ tree,
                                                const int32_t* __restrict__ spos, const double* __restrict__ pool) {
  const IsmClq c = cl[q];
  const FrontDesc F = tree[c.slot];
  return MpFront{F.n - 1, F.nf, F.ld_rsd, c.poff, pool + F.rsd_off, spos + c.sx_begin};
}

// CrossReq / CrossTgt as the batch route fills them, with front and junction being indices into cl[]
template <int DP>
__device__ __forceinline__ void isam2_cross_walk(const CrossReq rq, const CrossTgt* __restrict__ tgts, const IsmClq* __restrict__ cl,
                                                 const FrontDesc* __restrict__ tree, const int32_t* __restrict__ spos,
                                                 const double* __restrict__ pool, double* __restrict__ W, double* __restrict__ yb,
                                                 double* __restrict__ out, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  const int p_src = cl[rq.front].poff;
  const int L = p_src + tree[cl[rq.front].slot].nf;  // scalars of the source's path
  int32_t* pathv = (int32_t*)(W + (size_t)rq.lw * DP);
  for (int i = tid; i < L * DP; i += MP_THREADS) W[i] = 0.0;
  if (tid == 0) *status = 0;  // (no memset of the status words: each workgroup clears its own before anything can set it)
  __syncthreads();
  if (tid < rq.dim) W[(size_t)(p_src + rq.col + tid) * DP + tid] = 1.0;
  __syncthreads();
  int npath = 0;
  for (int q = rq.front; q >= 0; q = cl[q].parent, npath++) {
    if (tid == 0) pathv[npath] = q;
    mp_front_up<DP>(ism_front_of(q, cl, tree, spos, pool), W, yb);
  }
  for (int p = npath - 1; p >= 0; p--) mp_front_down<DP>(ism_front_of(pathv[p], cl, tree, spos, pool), W, yb);

  // ---- the targets, deepest junction first (the host's order: a branch descent destroys x of the source's path below its junction only)
  int32_t* branchv = pathv + npath;
  const int dj = rq.dim;
  for (int t = 0; t < rq.t_count; t++) {
    const CrossTgt T = tgts[rq.t_begin + t];
    const int cells = T.dim * dj;
    if (T.junction < 0) {  // another tree of the forest: exact zeros
      if (tid < cells) out[T.out + tid] = 0.0;
      continue;
    }
    const int p_tgt = cl[T.front].poff;
    if (T.front != T.junction) {
      const int z0 = (cl[T.junction].poff + tree[cl[T.junction].slot].nf) * DP, z1 = (p_tgt + tree[cl[T.front].slot].nf) * DP;
      for (int i = z0 + tid; i < z1; i += MP_THREADS) W[i] = 0.0;
      int nb = 0;
      for (int q = T.front; q >= 0 && q != T.junction; q = cl[q].parent, nb++)
        if (tid == 0) branchv[nb] = q;
      __syncthreads();
      for (int p = nb - 1; p >= 0; p--) mp_front_down<DP>(ism_front_of(branchv[p], cl, tree, spos, pool), W, yb);
    }
    const int pv = p_tgt + T.col;
    if (tid < cells) {
      const int r = tid / dj, c = tid % dj;
      double s = W[(size_t)(pv + r) * DP + c];
      if (T.sym) s = 0.5 * (s + W[(size_t)(pv + c) * DP + r]);  // the variable's own block: the two triangles differ by rounding only
      out[T.out + tid] = s;
      if (!(fabs(s) < 1.7e308)) *status = 1;  // (every writer stores the same word)
    }
    __syncthreads();  // the next target zeroes what this one read
  }
}

// grid: one workgroup per CrossReq of the chunk; dynamic LDS: lds_doubles of work-vector window + MP_BS * MP_MAXD of block staging.
// status: one word per workgroup behind the chunk's blocks (0 fine, 1 a non-finite block, 2 a vector beyond its window: a host bug)
__global__ __launch_bounds__(MP_THREADS) void isam2_marginal_cross_kernel(const CrossReq* __restrict__ reqs, const CrossTgt* __restrict__ tgts,
                                                                           const IsmClq* __restrict__ cl, const FrontDesc* __restrict__ tree,
                                                                           const int32_t* __restrict__ spos, const double* __restrict__ pool,
                                                                           double* __restrict__ scratch, int lds_doubles, double* __restrict__ out,
                                                                           int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double ism_lds[];
  const CrossReq rq = reqs[blockIdx.x];
  double* yb = ism_lds;
  double* W = rq.scratch >= 0 ? scratch + rq.scratch : ism_lds + MP_BS * MP_MAXD;
  if (rq.scratch < 0 && rq.need > lds_doubles) {  // never walk past the window
    if (threadIdx.x == 0) status[blockIdx.x] = 2;
    return;
  }
  if (rq.dim <= 3) isam2_cross_walk<3>(rq, tgts, cl, tree, spos, pool, W, yb, out, status + blockIdx.x);
  else if (rq.dim <= 6) isam2_cross_walk<6>(rq, tgts, cl, tree, spos, pool, W, yb, out, status + blockIdx.x);
  else isam2_cross_walk<9>(rq, tgts, cl, tree, spos, pool, W, yb, out, status + blockIdx.x);
}

}  // namespace lmgpu
