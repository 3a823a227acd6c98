// Marginal covariances of single variables from the [R S d] a batch solve left in the pool (marginals.hpp).
//
// Column c of Sigma = (R^T R)^-1 restricted to a variable v is x with R^T y = e_c, R x = y.  In the Bayes tree both solves touch only the
// PATH from the front v is frontal in to its root: y is zero below that front, x is only wanted at v, and every separator variable on the
// way is frontal in an ancestor (isam2_marginal_kernel, isam2.hpp, rests on the same fact for ISAM2's device tree).  Here: one workgroup
// per requested variable, all of its columns through the walk together, so a path front's R and S are read once per variable.
//
// Work vector: compact.  Front f owns the path positions [poff[f], poff[f] + nf) (poff[root] = 0, poff[child] = poff[parent] + nf[parent]),
// spos[] (parallel to sxoff[]) is the path position of each separator scalar: a variable's vector holds the frontal scalars of its front
// and of its ancestors only, MP_DP columns per position, followed by the front ids of the path (stored on the way up, read on the way
// down).  It lives in LDS when it fits the launch's LDS window and in the workgroup's slice of a scratch buffer when it does not.
//
// A front is taken in blocks of MP_BS rows.  Wave 0 solves the diagonal block out of registers (lane k holds column k of the block on the
// way up, row k on the way down; the 32 steps are unrolled and the solved scalar goes round by a lane broadcast); everything right of the
// block is a product over whole rows that all waves share: on the way up each thread owns columns (coalesced along the rows), on the way
// down each wave owns rows and reduces over its lanes in a fixed butterfly.  Every vector entry has one writer per step and no sum
// depends on which other variables share the launch: a variable's block is bitwise the same in every request.  No atomics.
#pragma once
#include "kernels_front.hpp"

namespace lmgpu {

#define MP_BS 32        // rows of a diagonal block
#define MP_THREADS 256  // four waves
#define MP_MAXD 9       // widest variable

struct MargReq {
  int32_t front;    // the front the variable is frontal in
  int32_t col;      // its first scalar inside that front
  int32_t dim;      // 1 .. MP_MAXD
  int32_t need;     // doubles of work vector: (poff + nf) * DP + room for the path's front ids
  int64_t scratch;  // offset (doubles) of its slice of the scratch buffer; -1: the vector fits the LDS window
  int64_t out;      // offset (doubles) of its dim x dim block in the chunk's output
};

// one front of a walk as the two bodies below see it: [R S] (upper; n1 = scalar columns without the right-hand side, nf of them frontal,
// row stride ld), p0 = the path position of its first frontal scalar, sp[] = the path positions of its separator scalars.  The batch route
// reads it from its static tables (mp_front_of), ISAM2 from its device tree and the tables of the request (kernels_isam2_marginals.hpp).
struct MpFront {
  int n1, nf, ld, p0;
  const double* A;
  const int32_t* sp;
};
__device__ __forceinline__ MpFront mp_front_of(const int f, const FrontDesc* __restrict__ fronts, const int32_t* __restrict__ poff,
                                               const int32_t* __restrict__ spos, const double* __restrict__ pool) {
  const FrontDesc F = fronts[f];
  return MpFront{F.n - 1, F.nf, F.ld_rsd, poff[f], pool + F.rsd_off, spos + F.sx_begin};
}

// one front of the way up: R^T y_F = b_F, b_S -= S^T y_F (shared by the path walk and the cross walk: the same operations in the same
// order, so a variable's block has the same bits from both)
template <int DP>
__device__ __forceinline__ void mp_front_up(const MpFront V, double* __restrict__ W, double* __restrict__ yb) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = V.n1, nf = V.nf, ld = V.ld, p0 = V.p0;
  const double* __restrict__ A = V.A;
  const int32_t* __restrict__ sp = V.sp;
  for (int r0 = 0; r0 < nf; r0 += MP_BS) {
    const int bs = min(MP_BS, nf - r0);
    if (wave == 0) {
      // lane k: column k of the block, rows i <= k
      double col[MP_BS], b[DP];
#pragma unroll
      for (int i = 0; i < MP_BS; i++) col[i] = (lane < bs && i <= lane) ? A[(size_t)(r0 + i) * ld + r0 + lane] : 0.0;
#pragma unroll
      for (int c = 0; c < DP; c++) b[c] = lane < bs ? W[(size_t)(p0 + r0 + lane) * DP + c] : 0.0;
      double dg = 1.0;
#pragma unroll
      for (int i = 0; i < MP_BS; i++)
        if (lane == i) dg = col[i];
      const double inv = lane < bs ? 1.0 / dg : 0.0;
#pragma unroll
      for (int i = 0; i < MP_BS; i++) {
        if (i < bs) {  // (wave-uniform)
#pragma unroll
          for (int c = 0; c < DP; c++) {
            if (lane == i) b[c] *= inv;
            const double y = __shfl(b[c], i);
            if (lane > i) b[c] = fma(-col[i], y, b[c]);
          }
        }
      }
      if (lane < bs) {
#pragma unroll
        for (int c = 0; c < DP; c++) {
          W[(size_t)(p0 + r0 + lane) * DP + c] = b[c];
          yb[lane * DP + c] = b[c];
        }
      }
    }
    __syncthreads();
    // everything right of the block: b_k -= sum_i A[r0 + i][k] y_i, a thread per column k
    for (int k = r0 + bs + tid; k < n1; k += MP_THREADS) {
      double acc[DP];
#pragma unroll
      for (int c = 0; c < DP; c++) acc[c] = 0.0;
      const double* Ak = A + (size_t)r0 * ld + k;
#pragma unroll 4
      for (int i = 0; i < bs; i++) {
        const double a = Ak[(size_t)i * ld];
#pragma unroll
        for (int c = 0; c < DP; c++) acc[c] = fma(a, yb[i * DP + c], acc[c]);
      }
      const int pk = k < nf ? p0 + k : sp[k - nf];
#pragma unroll
      for (int c = 0; c < DP; c++) W[(size_t)pk * DP + c] -= acc[c];
    }
    __syncthreads();
  }
}

// one front of the way down: x_F = R^-1 (y_F - S x_S)
template <int DP>
__device__ __forceinline__ void mp_front_down(const MpFront V, double* __restrict__ W, double* __restrict__ yb) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = V.n1, nf = V.nf, ld = V.ld, p0 = V.p0;
  const double* __restrict__ A = V.A;
  const int32_t* __restrict__ sp = V.sp;
  for (int r0 = ((nf - 1) / MP_BS) * MP_BS; r0 >= 0; r0 -= MP_BS) {
    const int bs = min(MP_BS, nf - r0);
    // t_i = y_i - sum_{k right of the block} A[r0 + i][k] x_k: a wave per row, lanes along the row
    for (int i = wave; i < bs; i += MP_THREADS / 64) {
      double acc[DP];
#pragma unroll
      for (int c = 0; c < DP; c++) acc[c] = 0.0;
      const double* Ai = A + (size_t)(r0 + i) * ld;
      for (int k = r0 + bs + lane; k < n1; k += 64) {
        const double a = Ai[k];
        const int pk = k < nf ? p0 + k : sp[k - nf];
#pragma unroll
        for (int c = 0; c < DP; c++) acc[c] = fma(a, W[(size_t)pk * DP + c], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < DP; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
      }
      if (lane < DP) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < DP; c++)
          if (lane == c) s = acc[c];
        yb[i * DP + lane] = W[(size_t)(p0 + r0 + i) * DP + lane] - s;
      }
    }
    __syncthreads();
    if (wave == 0) {
      // lane k: row k of the block, columns i >= k
      double row[MP_BS], t[DP];
#pragma unroll
      for (int i = 0; i < MP_BS; i++) row[i] = (lane < bs && i >= lane && i < bs) ? A[(size_t)(r0 + lane) * ld + r0 + i] : 0.0;
#pragma unroll
      for (int c = 0; c < DP; c++) t[c] = lane < bs ? yb[lane * DP + c] : 0.0;
      double dg = 1.0;
#pragma unroll
      for (int i = 0; i < MP_BS; i++)
        if (lane == i) dg = row[i];
      const double inv = lane < bs ? 1.0 / dg : 0.0;
#pragma unroll
      for (int i = MP_BS - 1; i >= 0; i--) {
        if (i < bs) {  // (wave-uniform)
#pragma unroll
          for (int c = 0; c < DP; c++) {
            if (lane == i) t[c] *= inv;
            const double x = __shfl(t[c], i);
            if (lane < i) t[c] = fma(-row[i], x, t[c]);
          }
        }
      }
      if (lane < bs) {
#pragma unroll
        for (int c = 0; c < DP; c++) W[(size_t)(p0 + r0 + lane) * DP + c] = t[c];
      }
    }
    __syncthreads();
  }
}

template <int DP>
__device__ __forceinline__ void marginal_path_walk(const MargReq rq, const FrontDesc* __restrict__ fronts, const int32_t* __restrict__ parent,
                                                   const int32_t* __restrict__ poff, const int32_t* __restrict__ spos,
                                                   const double* __restrict__ pool, double* __restrict__ W, double* __restrict__ yb,
                                                   double* __restrict__ out, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  const int L = poff[rq.front] + fronts[rq.front].nf;  // path scalars
  int32_t* pathv = (int32_t*)(W + (size_t)L * DP);
  for (int i = tid; i < L * DP; i += MP_THREADS) W[i] = 0.0;
  __syncthreads();
  if (tid < rq.dim) W[(size_t)(poff[rq.front] + rq.col + tid) * DP + tid] = 1.0;
  __syncthreads();

  // ---- up: R^T y_F = b_F, b_S -= S^T y_F, front by front
  int npath = 0;
  for (int f = rq.front; f >= 0; f = parent[f], npath++) {
    if (tid == 0) pathv[npath] = f;
    mp_front_up<DP>(mp_front_of(f, fronts, poff, spos, pool), W, yb);
  }

  // ---- down: x_F = R^-1 (y_F - S x_S), from the root back to the variable's front
  for (int q = npath - 1; q >= 0; q--) mp_front_down<DP>(mp_front_of(pathv[q], fronts, poff, spos, pool), W, yb);

  // ---- the variable's block, symmetrised (the two triangles differ by rounding only); a non-finite entry: a singular front on the path
  const int d = rq.dim, pv = poff[rq.front] + rq.col;
  if (tid < d * d) {
    const int i = tid / d, j = tid % d;
    const double s = 0.5 * (W[(size_t)(pv + i) * DP + j] + W[(size_t)(pv + j) * DP + i]);
    out[rq.out + tid] = s;
    if (!(fabs(s) < 1.7e308)) *status = 1;  // (every writer stores the same word)
  }
}

// grid: one workgroup per request of the chunk; dynamic LDS: lds_doubles of work-vector window + MP_BS * MP_MAXD of block staging
__global__ __launch_bounds__(MP_THREADS) void marginal_path_kernel(const MargReq* __restrict__ reqs, const FrontDesc* __restrict__ fronts,
                                                                    const int32_t* __restrict__ parent, const int32_t* __restrict__ poff,
                                                                    const int32_t* __restrict__ spos, const double* __restrict__ pool,
                                                                    double* __restrict__ scratch, int lds_doubles, double* __restrict__ out,
                                                                    int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double mp_lds[];
  const MargReq rq = reqs[blockIdx.x];
  double* yb = mp_lds;
  double* W = rq.scratch >= 0 ? scratch + rq.scratch : mp_lds + MP_BS * MP_MAXD;
  if (rq.scratch < 0 && rq.need > lds_doubles) {  // (a host bug: never walk past the window)
    if (threadIdx.x == 0) status[blockIdx.x] = 2;
    return;
  }
  if (rq.dim <= 3) marginal_path_walk<3>(rq, fronts, parent, poff, spos, pool, W, yb, out, status + blockIdx.x);
  else if (rq.dim <= 6) marginal_path_walk<6>(rq, fronts, parent, poff, spos, pool, W, yb, out, status + blockIdx.x);
  else marginal_path_walk<9>(rq, fronts, parent, poff, spos, pool, W, yb, out, status + blockIdx.x);
}

// ---- cross-covariances: Sigma[i, j] for a SOURCE variable j and a list of TARGET variables i.  The source's columns go
// up and down its path exactly as above; that leaves x on every position of the path.  A target's path shares everything from the junction
// J (the deepest front on both paths) to the root with the source's, at the same positions (poff[] depends on a front's ancestors only), so
// x at the target needs only the descent of the target's BRANCH, the fronts of its path strictly below J, with y = 0 there.  The branch's
// positions [poff[J] + nf[J], L_i) overlap those of the source's own branch: they are zeroed first, which destroys x of the source's path
// below J -- the host lists a workgroup's targets deepest junction first, and a later target (junction no deeper) reads none of it.
struct CrossReq {  // one workgroup: a source and a run of its targets
  int32_t front, col, dim;   // the source: its front, first scalar there, dimension
  int32_t lw;                // positions of the work vector: the longest of the source's path and of the run's target paths
  int32_t need;              // doubles: lw * DP + room for the front ids of the path and of the longest branch
  int32_t t_begin, t_count;  // its targets in the chunk's target table
  int32_t pad;
  int64_t scratch;           // offset (doubles) of its slice of the scratch buffer; -1: the vector fits the LDS window
};

struct CrossTgt {
  int32_t front, col, dim;  // the target variable
  int32_t junction;         // deepest front on both paths (== front: the target's front is on the source's path); -1: another tree
  int32_t sym;              // the target is the source: its block is symmetrised as marginal_path_walk does
  int32_t pad;
  int64_t out;              // offset (doubles) of the dim x source-dim block in the chunk's output
};

template <int DP>
__device__ __forceinline__ void marginal_cross_walk(const CrossReq rq, const CrossTgt* __restrict__ tgts, const FrontDesc* __restrict__ fronts,
                                                    const int32_t* __restrict__ parent, const int32_t* __restrict__ poff,
                                                    const int32_t* __restrict__ spos, const double* __restrict__ pool, double* __restrict__ W,
                                                    double* __restrict__ yb, double* __restrict__ out, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  const int L = poff[rq.front] + fronts[rq.front].nf;  // scalars of the source's path
  int32_t* pathv = (int32_t*)(W + (size_t)rq.lw * DP);
  for (int i = tid; i < L * DP; i += MP_THREADS) W[i] = 0.0;
  __syncthreads();
  if (tid < rq.dim) W[(size_t)(poff[rq.front] + rq.col + tid) * DP + tid] = 1.0;
  __syncthreads();
  int npath = 0;
  for (int f = rq.front; f >= 0; f = parent[f], npath++) {
    if (tid == 0) pathv[npath] = f;
    mp_front_up<DP>(mp_front_of(f, fronts, poff, spos, pool), W, yb);
  }
  for (int q = npath - 1; q >= 0; q--) mp_front_down<DP>(mp_front_of(pathv[q], fronts, poff, spos, pool), W, yb);

  // ---- the targets, deepest junction first
  int32_t* branchv = pathv + npath;
  const int dj = rq.dim;
  for (int t = 0; t < rq.t_count; t++) {
    const CrossTgt T = tgts[rq.t_begin + t];
    const int cells = T.dim * dj;
    if (T.junction < 0) {  // no path from one tree of a forest into another: exact zeros
      if (tid < cells) out[T.out + tid] = 0.0;
      continue;
    }
    if (T.front != T.junction) {
      const int z0 = (poff[T.junction] + fronts[T.junction].nf) * DP, z1 = (poff[T.front] + fronts[T.front].nf) * DP;
      for (int i = z0 + tid; i < z1; i += MP_THREADS) W[i] = 0.0;
      int nb = 0;
      for (int f = T.front; f >= 0 && f != T.junction; f = parent[f], nb++)
        if (tid == 0) branchv[nb] = f;
      __syncthreads();
      for (int q = nb - 1; q >= 0; q--) mp_front_down<DP>(mp_front_of(branchv[q], fronts, poff, spos, pool), W, yb);
    }
    const int pv = poff[T.front] + T.col;
    if (tid < cells) {
      const int r = tid / dj, c = tid % dj;
      double s = W[(size_t)(pv + r) * DP + c];
      if (T.sym) s = 0.5 * (s + W[(size_t)(pv + c) * DP + r]);
      out[T.out + tid] = s;
      if (!(fabs(s) < 1.7e308)) *status = 1;  // (every writer stores the same word)
    }
    __syncthreads();  // the next target zeroes what this one read
  }
}

// grid: one workgroup per CrossReq of the chunk; dynamic LDS as marginal_path_kernel
__global__ __launch_bounds__(MP_THREADS) void marginal_cross_kernel(const CrossReq* __restrict__ reqs, const CrossTgt* __restrict__ tgts,
                                                                     const FrontDesc* __restrict__ fronts, const int32_t* __restrict__ parent,
                                                                     const int32_t* __restrict__ poff, const int32_t* __restrict__ spos,
                                                                     const double* __restrict__ pool, double* __restrict__ scratch,
                                                                     int lds_doubles, double* __restrict__ out, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double mp_lds[];
  const CrossReq rq = reqs[blockIdx.x];
  double* yb = mp_lds;
  double* W = rq.scratch >= 0 ? scratch + rq.scratch : mp_lds + MP_BS * MP_MAXD;
  if (rq.scratch < 0 && rq.need > lds_doubles) {  // (a host bug: never walk past the window)
    if (threadIdx.x == 0) status[blockIdx.x] = 2;
    return;
  }
  if (rq.dim <= 3) marginal_cross_walk<3>(rq, tgts, fronts, parent, poff, spos, pool, W, yb, out, status + blockIdx.x);
  else if (rq.dim <= 6) marginal_cross_walk<6>(rq, tgts, fronts, parent, poff, spos, pool, W, yb, out, status + blockIdx.x);
  else marginal_cross_walk<9>(rq, tgts, fronts, parent, poff, spos, pool, W, yb, out, status + blockIdx.x);
}

}  // namespace lmgpu
