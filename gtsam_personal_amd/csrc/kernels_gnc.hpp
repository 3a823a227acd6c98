// Graduated non-convexity (gtsam/nonlinear/GncOptimizer.h): the two passes over the factor list that the reference runs on the host,
// one factor->error() at a time.  Here the unweighted per-factor errors r_k already sit in device memory (the error kernels with
// BucketDev::gw == nullptr), so the weights, the thresholds and the known-inlier / known-outlier mask never leave the device; each pass
// is three 8-byte streams + one byte stream, one lane per factor in graph order, and ends in a fixed-order reduction (no atomics).
//   g1  calculateWeights          GncOptimizer.h:419-469   (+ the maximum of checkWeightsConvergence :362-386 in the same pass)
//   g2  initializeMu              GncOptimizer.h:272-314
#pragma once
#include <hip/hip_runtime.h>

namespace lmgpu {

#define GNC_MAX_BLOCKS 256

// max (IS_MAX) or min of a workgroup's 256 values, result in sh[0]
template <bool IS_MAX>
__device__ __forceinline__ void gnc_block_reduce(double* sh, double v) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      const double a = sh[threadIdx.x], b = sh[threadIdx.x + k];
      sh[threadIdx.x] = IS_MAX ? fmax(a, b) : fmin(a, b);
    }
    __syncthreads();
  }
}

// w_k from r_k.  fixed_k: 0 free, 1 known inlier (weight 1), 2 known outlier (weight 0).  loss: 0 GM (eq. 12 of the GNC paper), 1 TLS (eq. 14).
// partial[blockIdx.x] = max over the block's factors of |w - round(w)|.  Grid: at most GNC_MAX_BLOCKS workgroups, grid-stride.
__global__ __launch_bounds__(256) void gnc_weights_kernel(int n, const double* __restrict__ r, const double* __restrict__ barc,
                                                           const unsigned char* __restrict__ fixed, double mu, int loss,
                                                           double* __restrict__ w, double* __restrict__ partial) {
  __shared__ double sh[256];
  double dev = 0.0;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
    const int fx = fixed[k];
    double wk;
    if (fx == 1) {
      wk = 1.0;
    } else if (fx == 2) {
      wk = 0.0;
    } else {
      const double u2 = r[k], b = barc[k];
      if (loss == 0) {
        const double q = (mu * b) / (u2 + mu * b);
        wk = q * q;
      } else {
        const double upper = (mu + 1.0) / mu * b, lower = mu / (mu + 1.0) * b;
        wk = sqrt(b * mu * (mu + 1.0) / u2) - mu;  // u2 = 0: inf, which the second test below turns into 1
        if (u2 >= upper || wk < 0.0) {
          wk = 0.0;
        } else if (u2 <= lower || wk > 1.0) {
          wk = 1.0;
        }
      }
    }
    w[k] = wk;
    dev = fmax(dev, fabs(wk - round(wk)));
  }
  gnc_block_reduce<true>(sh, dev);
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// GM: block maxima of 2 r_k / b_k (from 0).  TLS: block minima of b_k / (2 r_k - b_k) over the factors with 2 r_k - b_k > 0 (from +inf).
__global__ __launch_bounds__(256) void gnc_mu_init_kernel(int n, const double* __restrict__ r, const double* __restrict__ barc, int loss,
                                                           double* __restrict__ partial) {
  __shared__ double sh[256];
  double acc = loss == 0 ? 0.0 : INFINITY;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
    const double rk = r[k], b = barc[k];
    if (loss == 0) {
      acc = fmax(acc, 2.0 * rk / b);
    } else {
      const double ex = 2.0 * rk - b;
      if (ex > 0.0) acc = fmin(acc, b / ex);
    }
  }
  if (loss == 0)
    gnc_block_reduce<true>(sh, acc);
  else
    gnc_block_reduce<false>(sh, acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// the block partials -> one scalar.  mode 0: max.  mode 1: min, then initializeMu's TLS tail (:302-307): [0, 1e-6) -> 1e-6, and -1 when
// nothing qualified (inf) or the result is not positive.
__global__ __launch_bounds__(256) void gnc_finish_kernel(const double* __restrict__ partial, int nb, int mode, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = mode == 0 ? 0.0 : INFINITY;
  for (int i = threadIdx.x; i < nb; i += 256) acc = mode == 0 ? fmax(acc, partial[i]) : fmin(acc, partial[i]);
  if (mode == 0)
    gnc_block_reduce<true>(sh, acc);
  else
    gnc_block_reduce<false>(sh, acc);
  if (threadIdx.x == 0) {
    double v = sh[0];
    if (mode == 1) {
      if (v >= 0.0 && v < 1e-6) v = 1e-6;
      v = (v > 0.0 && !isinf(v)) ? v : -1.0;
    }
    *out = v;
  }
}

}  // namespace lmgpu
