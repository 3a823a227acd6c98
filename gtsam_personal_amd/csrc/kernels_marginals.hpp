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

template <int DP>
__device__ __forceinline__ void marginal_path_walk(const MargReq rq, const FrontDesc* __restrict__ fronts, const int32_t* __restrict__ parent,
                                                   const int32_t* __restrict__ poff, const int32_t* __restrict__ spos,
                                                   const double* __restrict__ pool, double* __restrict__ W, double* __restrict__ yb,
                                                   double* __restrict__ out, int32_t* __restrict__ status) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    const FrontDesc F = fronts[f];
    const int n1 = F.n - 1, nf = F.nf, ld = F.ld_rsd, p0 = poff[f];
    const double* A = pool + F.rsd_off;
    const int32_t* sp = spos + F.sx_begin;
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

  // ---- down: x_F = R^-1 (y_F - S x_S), from the root back to the variable's front
  for (int q = npath - 1; q >= 0; q--) {
    const int f = pathv[q];
    const FrontDesc F = fronts[f];
    const int n1 = F.n - 1, nf = F.nf, ld = F.ld_rsd, p0 = poff[f];
    const double* A = pool + F.rsd_off;
    const int32_t* sp = spos + F.sx_begin;
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

}  // namespace lmgpu
