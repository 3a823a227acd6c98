// Preconditioned conjugate gradient on the device-resident linearization (linearSolverType = Iterative, PCGSolverParameters).
//   system      GaussianFactorGraphSystem          gtsam/linear/PCGSolver.cpp:69-145  (A = sum J^T J + lambda D, b = -gradientAtZero)
//   CG loop     preconditionedConjugateGradient    gtsam/linear/ConjugateGradientSolver.h:109-171
//   Dummy / BlockJacobi preconditioner              gtsam/linear/Preconditioner.cpp:80-177
// Everything is gathered per variable scalar over the CSR incidence list var -> (factor, key position) that hessianDiagonal
// uses (no atomics: every sum has one writer and a fixed order).  Loop control lives in device memory: iteration k of the loop
// reads done[k - 1] and gamma[k - 1] and is a no-op once the loop has stopped, so the host can queue 16 iterations at a time.
// Dot products: each block writes its partial sum; a consumer kernel lets EVERY block re-reduce all partials in the same fixed
// order (bitwise the same total in every block, no extra launch, no last-block ticket).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_factors.hpp"

namespace lmgpu {

#define PCG_MAXPART 2048  // partial sums per dot product (grids are clamped to this many blocks and stride beyond)
#define PCG_MAXD 9        // largest variable dimension (CAM_BUNDLER)

struct PcgVars {  // per-variable layout
  int nvars;
  const int32_t* xoff;  // nvars + 1 scalar offsets
  const int64_t* loff;  // nvars: offset of the variable's d x d block (column-major) in the block buffers
};

// loop control of one solve (device memory)
struct PcgCtl {
  double gamma0, threshold, gamma;  // gamma: |r|^2 after the last executed iteration
  int32_t iters, status;            // status: smallest slot whose diagonal block is not positive definite (INT_MAX: none)
};

__device__ __forceinline__ int pcg_var_dim(const PcgVars& V, int v) { return V.xoff[v + 1] - V.xoff[v]; }

// block-wide sum (256 threads), result in every thread
__device__ __forceinline__ double pcg_block_sum(double s, double* sh) {
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  const double t = sh[0];
  __syncthreads();
  return t;
}
// the sum of n block partials, in a fixed order (the same bits in every block)
__device__ __forceinline__ double pcg_sum_partials(const double* __restrict__ part, int n, double* sh) {
  double s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  return pcg_block_sum(s, sh);
}

// column of the factor's [A1 A2 A3 b] that holds scalar c of the variable at key position pos
__device__ __forceinline__ int pcg_col(const FacDesc& d, int pos, int c) { return pos == 0 ? c : (pos == 1 ? d.d0 + c : d.d0 + d.d1 + c); }

// ---- once per linearization: undamped diagonal blocks H_vv = sum_f J_fv^T J_fv (hessianBlockDiagonal, GaussianFactorGraph.cpp
//      :290-305 over JacobianFactor::hessianBlockDiagonal) and b = sum_f J_f^T b_f (= -gradientAtZero, PCGSolver.cpp:120-128).
//      One thread per variable scalar (v, c): column c of H_vv and b[i].
__global__ __launch_bounds__(256) void pcg_gram_kernel(int ntot, const int32_t* __restrict__ scalar_var, const int32_t* __restrict__ scalar_col,
                                                        const int32_t* __restrict__ vi_ptr, const int32_t* __restrict__ vi_fac,
                                                        const int8_t* __restrict__ vi_pos, const FacDesc* __restrict__ fd,
                                                        const double* __restrict__ pool, PcgVars V, double* __restrict__ H,
                                                        double* __restrict__ rhs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ntot) return;
  const int v = scalar_var[i], c = scalar_col[i], dv = pcg_var_dim(V, v);
  double h[PCG_MAXD];
#pragma unroll
  for (int j = 0; j < PCG_MAXD; j++) h[j] = 0;
  double g = 0;
  for (int k = vi_ptr[v]; k < vi_ptr[v + 1]; k++) {
    const FacDesc d = fd[vi_fac[k]];
    const int m = d.rows, base = pcg_col(d, vi_pos[k], 0);
    const double* J = pool + d.joff;
    const double* Jc = J + (size_t)(base + c) * m;
    const double* b = J + (size_t)(d.d0 + d.d1 + d.d2) * m;
    for (int r = 0; r < m; r++) {
      const double a = Jc[r];
      g += a * b[r];
#pragma unroll
      for (int j = 0; j < PCG_MAXD; j++)
        if (j < dv) h[j] += J[(size_t)(base + j) * m + r] * a;
    }
  }
  double* Hc = H + V.loff[v] + (size_t)c * dv;
#pragma unroll
  for (int j = 0; j < PCG_MAXD; j++)
    if (j < dv) Hc[j] = h[j];
  rhs[i] = g;
}

// ---- per solve: L = chol(H_vv + lambda diag(dampw_v)), lower (Eigen LLT as in BlockJacobiPreconditioner::build, Preconditioner.cpp
//      :163-171).  One thread per variable, the block in registers.  A non-positive pivot records the slot (smallest wins).
__global__ __launch_bounds__(256) void pcg_chol_kernel(PcgVars V, const double* __restrict__ H, double lambda, const double* __restrict__ dampw,
                                                        double* __restrict__ L, PcgCtl* __restrict__ ctl) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V.nvars) return;
  const int d = pcg_var_dim(V, v), xo = V.xoff[v];
  const double* Hv = H + V.loff[v];
  double A[PCG_MAXD][PCG_MAXD];
#pragma unroll
  for (int i = 0; i < PCG_MAXD; i++)
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++) A[i][j] = (i < d && j < d && j <= i) ? Hv[j * d + i] : 0.0;
#pragma unroll
  for (int i = 0; i < PCG_MAXD; i++)
    if (i < d) A[i][i] += lambda * dampw[xo + i];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < PCG_MAXD; j++) {
    if (j < d) {
      double s = A[j][j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= A[j][k] * A[j][k];
      ok = ok && (s > 0.0);
      const double ljj = sqrt(s > 0.0 ? s : 1.0);
      A[j][j] = ljj;
#pragma unroll
      for (int i = j + 1; i < PCG_MAXD; i++) {
        if (i < d) {
          double t = A[i][j];
#pragma unroll
          for (int k = 0; k < j; k++) t -= A[i][k] * A[j][k];
          A[i][j] = t / ljj;
        }
      }
    }
  }
  if (!ok) atomicMin(&ctl->status, v);
  double* Lv = L + V.loff[v];
#pragma unroll
  for (int j = 0; j < PCG_MAXD; j++)
#pragma unroll
    for (int i = 0; i < PCG_MAXD; i++)
      if (i < d && j < d) Lv[j * d + i] = (i >= j) ? A[i][j] : 0.0;
}

// y = L^-1 y (leftPrecondition) and y = L^-T y (rightPrecondition) on one variable's block
__device__ __forceinline__ void pcg_lsolve(const double* __restrict__ L, int d, double* y) {
#pragma unroll
  for (int i = 0; i < PCG_MAXD; i++) {
    if (i < d) {
      double s = y[i];
#pragma unroll
      for (int j = 0; j < i; j++) s -= L[j * d + i] * y[j];
      y[i] = s / L[i * d + i];
    }
  }
}
__device__ __forceinline__ void pcg_ltsolve(const double* __restrict__ L, int d, double* y) {
#pragma unroll
  for (int i = PCG_MAXD - 1; i >= 0; i--) {
    if (i < d) {
      double s = y[i];
#pragma unroll
      for (int j = i + 1; j < PCG_MAXD; j++)
        if (j < d) s -= L[i * d + j] * y[j];
      y[i] = s / L[i * d + i];
    }
  }
}

// ---- forward half of A p: y_f = J_f p, one thread per factor (its rows back to back in y at yoff[f])
__global__ __launch_bounds__(256) void pcg_forward_kernel(const FacDesc* __restrict__ fd, int nfac, const int64_t* __restrict__ yoff,
                                                           const double* __restrict__ pool, const double* __restrict__ p, double* __restrict__ y,
                                                           const int32_t* __restrict__ done, int k) {
  if (k > 0 && done[k - 1]) return;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nfac) return;
  const FacDesc d = fd[f];
  const int m = d.rows, cols = d.d0 + d.d1 + d.d2;
  const double* J = pool + d.joff;
  double acc[PCG_MAXD];
#pragma unroll
  for (int r = 0; r < PCG_MAXD; r++) acc[r] = 0;
  for (int c = 0; c < cols; c++) {
    const double pc = p[fac_xoff(d, c)];
    const double* Jc = J + (size_t)c * m;
#pragma unroll
    for (int r = 0; r < PCG_MAXD; r++)
      if (r < m) acc[r] += Jc[r] * pc;
  }
  double* yf = y + yoff[f];
#pragma unroll
  for (int r = 0; r < PCG_MAXD; r++)
    if (r < m) yf[r] = acc[r];
}

// ---- transpose half: q_i = sum_f J_f(:, i)^T y_f + lambda dampw_i p_i, one thread per scalar (grid-stride over at most PCG_MAXPART
//      blocks).  RESET: q := b - A p (p = the estimate, ConjugateGradientSolver.h:150-151); else the block partials of p . q -> part.
//      FUSED (development A/B form, LMGPU_PCG_FUSED in the test library): no forward pass, y_f = J_f p recomputed for every incident
//      scalar (d_f times per factor) -- DESIGN section 11 measures both.
template <bool RESET, bool FUSED = false>
__global__ __launch_bounds__(256) void pcg_transpose_kernel(int ntot, const int32_t* __restrict__ scalar_var, const int32_t* __restrict__ scalar_col,
                                                             const int32_t* __restrict__ vi_ptr, const int32_t* __restrict__ vi_fac,
                                                             const int8_t* __restrict__ vi_pos, const FacDesc* __restrict__ fd,
                                                             const double* __restrict__ pool, const int64_t* __restrict__ yoff,
                                                             const double* __restrict__ y, const double* __restrict__ p, double lambda,
                                                             const double* __restrict__ dampw, const double* __restrict__ rhs,
                                                             double* __restrict__ q, double* __restrict__ part, const int32_t* __restrict__ done,
                                                             int k) {
  __shared__ double sh[256];
  if (k > 0 && done[k - 1]) return;
  double pq = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ntot; i += gridDim.x * 256) {
    const int v = scalar_var[i], c = scalar_col[i];
    double s = 0;
    for (int e = vi_ptr[v]; e < vi_ptr[v + 1]; e++) {
      const int f = vi_fac[e];
      const FacDesc d = fd[f];
      const int m = d.rows;
      const double* Jc = pool + d.joff + (size_t)pcg_col(d, vi_pos[e], c) * m;
      if (FUSED) {
        const double* J = pool + d.joff;
        const int cols = d.d0 + d.d1 + d.d2;
        for (int r = 0; r < m; r++) {
          double yr = 0;
          for (int cc = 0; cc < cols; cc++) yr += J[(size_t)cc * m + r] * p[fac_xoff(d, cc)];
          s += Jc[r] * yr;
        }
      } else {
        const double* yf = y + yoff[f];
        for (int r = 0; r < m; r++) s += Jc[r] * yf[r];
      }
    }
    const double qi = s + lambda * dampw[i] * p[i];
    if (RESET) {
      q[i] = rhs[i] - qi;
    } else {
      q[i] = qi;
      pq += p[i] * qi;
    }
  }
  if (!RESET) {
    const double t = pcg_block_sum(pq, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
  }
}

// ---- r = L^-1 src, p = L^-T r, the block partials of r . r -> part (INIT: src = b, x = 0; else src = b - A x of a reset)
template <bool INIT, bool BJ>
__global__ __launch_bounds__(256) void pcg_precond_kernel(PcgVars V, const double* __restrict__ L, const double* __restrict__ src,
                                                           double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                           double* __restrict__ part, const int32_t* __restrict__ done, int k) {
  __shared__ double sh[256];
  if (k > 0 && done[k - 1]) return;
  double rr = 0;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < V.nvars; v += gridDim.x * 256) {
    const int d = pcg_var_dim(V, v), xo = V.xoff[v];
    double t[PCG_MAXD];
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++) t[j] = j < d ? src[xo + j] : 0.0;
    if (BJ) pcg_lsolve(L + V.loff[v], d, t);
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++)
      if (j < d) {
        r[xo + j] = t[j];
        rr += t[j] * t[j];
        if (INIT) x[xo + j] = 0.0;
      }
    if (BJ) pcg_ltsolve(L + V.loff[v], d, t);
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++)
      if (j < d) p[xo + j] = t[j];
  }
  const double s = pcg_block_sum(rr, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- gamma0 = |r0|^2, threshold = max(eps_abs, eps_rel^2 gamma0) (ConjugateGradientSolver.h:120-127), and whether the loop runs at all
__global__ __launch_bounds__(256) void pcg_start_kernel(const double* __restrict__ part, int npart, double eps_rel, double eps_abs, int min_it,
                                                         int max_it, double* __restrict__ gam, int32_t* __restrict__ done, PcgCtl* __restrict__ ctl) {
  __shared__ double sh[256];
  const double g0 = pcg_sum_partials(part, npart, sh);
  if (threadIdx.x == 0) {
    const double thr = fmax(eps_abs, eps_rel * eps_rel * g0);
    gam[0] = g0;
    ctl->gamma0 = g0;
    ctl->threshold = thr;
    ctl->gamma = g0;
    const bool run = 1 <= max_it && (g0 > thr || 1 <= min_it);
    done[0] = run ? 0 : 1;
    ctl->iters = 0;
  }
}

// ---- iteration k, after q = A p: alpha = gamma / (p . q), x += alpha p, r -= alpha L^-1 q; the block partials of r . r -> part_rr.
//      gamma = gamma[k - 1], or (reset iteration) the sum of part_reset.
template <bool BJ>
__global__ __launch_bounds__(256) void pcg_update_kernel(PcgVars V, const double* __restrict__ L, const double* __restrict__ part_pq, int npq,
                                                          const double* __restrict__ part_reset, int nreset, const double* __restrict__ gam,
                                                          const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ x,
                                                          double* __restrict__ r, double* __restrict__ part_rr, const int32_t* __restrict__ done,
                                                          int k, int reset) {
  __shared__ double sh[256];
  if (done[k - 1]) return;
  const double pq = pcg_sum_partials(part_pq, npq, sh);
  const double g = reset ? pcg_sum_partials(part_reset, nreset, sh) : gam[k - 1];
  const double alpha = g / pq;
  double rr = 0;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < V.nvars; v += gridDim.x * 256) {
    const int d = pcg_var_dim(V, v), xo = V.xoff[v];
    double t[PCG_MAXD];
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++)
      if (j < d) {
        x[xo + j] += alpha * p[xo + j];
        t[j] = q[xo + j];
      } else {
        t[j] = 0.0;
      }
    if (BJ) pcg_lsolve(L + V.loff[v], d, t);
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++)
      if (j < d) {
        const double rn = r[xo + j] + (-alpha) * t[j];
        r[xo + j] = rn;
        rr += rn * rn;
      }
  }
  const double s = pcg_block_sum(rr, sh);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = s;
}

// ---- iteration k, end: gamma_k = r . r, beta = gamma_k / gamma, p = L^-T r + beta p; block 0 records gamma_k and whether iteration
//      k + 1 runs (k + 1 <= max && (gamma_k > threshold || k + 1 <= min), ConjugateGradientSolver.h:136)
template <bool BJ>
__global__ __launch_bounds__(256) void pcg_direction_kernel(PcgVars V, const double* __restrict__ L, const double* __restrict__ part_rr, int nrr,
                                                             const double* __restrict__ part_reset, int nreset, double* __restrict__ gam,
                                                             const double* __restrict__ r, double* __restrict__ p, int32_t* __restrict__ done,
                                                             PcgCtl* __restrict__ ctl, int k, int reset, int min_it, int max_it) {
  __shared__ double sh[256];
  if (done[k - 1]) {  // carry the stop forward: iteration k + 1 reads done[k]
    if (blockIdx.x == 0 && threadIdx.x == 0) done[k] = 1;
    return;
  }
  const double gk = pcg_sum_partials(part_rr, nrr, sh);
  const double g = reset ? pcg_sum_partials(part_reset, nreset, sh) : gam[k - 1];
  const double beta = gk / g;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < V.nvars; v += gridDim.x * 256) {
    const int d = pcg_var_dim(V, v), xo = V.xoff[v];
    double t[PCG_MAXD];
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++) t[j] = j < d ? r[xo + j] : 0.0;
    if (BJ) pcg_ltsolve(L + V.loff[v], d, t);
#pragma unroll
    for (int j = 0; j < PCG_MAXD; j++)
      if (j < d) p[xo + j] = beta * p[xo + j] + t[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gam[k] = gk;
    ctl->gamma = gk;
    ctl->iters = k;
    const bool run = k + 1 <= max_it && (gk > ctl->threshold || k + 1 <= min_it);
    done[k] = run ? 0 : 1;
  }
}

}  // namespace lmgpu
