// NonlinearConjugateGradientOptimizer on the device-resident graph (gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h, .cpp).
//   gradient       System::gradient = graph.linearize(values)->gradientAtZero()      .cpp:37-42, 56-60
//   beta           FletcherReeves / PolakRibiere / HestenesStiefel / DaiYuan          .h:28-70
//   direction      direction = currentGradient + beta * direction                    .h:257
//   line search    lineSearch (golden section on [-1 / |direction|, 0])              .h:135-181
//   advance        values.retract(alpha * direction)                                 .cpp:62-69
// Every sum has one writer and a fixed order (no floating-point atomics): the gradient is gathered per variable scalar over the CSR
// incidence list var -> (factor, key position) that hessianDiagonal and the PCG kernels walk; the dot products are block partials that
// every block of the consumer kernel re-reduces in the same order (pcg_sum_partials).  The bracket of the line search lives in device
// memory (NcgCtl): a trial = scaled retract (step read from NcgCtl) + the error launches + a one-thread control kernel that applies
// the reference's update rule and writes the next step or sets `done`; every kernel of a trial queued behind `done` -- the retract,
// the error launches (BucketDev::skip), the reduction and the control kernel -- returns at its first instructions.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_factors.hpp"
#include "kernels_pcg.hpp"

namespace lmgpu {

#define NCG_MAXPART 256  // block partials per dot product (grids are clamped to this many blocks and stride beyond)

// state of one line search + the scalars of the direction update (device memory; copied to the host once per NCG iteration)
struct NcgCtl {
  double minStep, maxStep, newStep, newError;  // the bracket of lineSearch (.h:144-148)
  double step;                                 // the step the next trial's retract uses (newStep first, then every testStep)
  double alpha;                                // 0.5 * (minStep + maxStep) once done (.h:156)
  double error;                                // graph.error at advance(values, alpha, direction) (final advance only)
  double beta, dnorm;                          // of the direction the search ran along
  int32_t done, trials, flag, first;           // flag: the `flag` of the testStep under evaluation (.h:151); first: newError is pending
};

// ---- gradientAtZero (GaussianFactorGraph.cpp:357-367: g_j -= A_j^T b per factor, JacobianFactor::gradientAtZero): one thread per
//      variable scalar, factors in VariableIndex order, rows in order
__global__ __launch_bounds__(256) void ncg_gradient_kernel(int ntot, const int32_t* __restrict__ scalar_var, const int32_t* __restrict__ scalar_col,
                                                            const int32_t* __restrict__ vi_ptr, const int32_t* __restrict__ vi_fac,
                                                            const int8_t* __restrict__ vi_pos, const FacDesc* __restrict__ fd,
                                                            const double* __restrict__ pool, double* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ntot) return;
  const int v = scalar_var[i], c = scalar_col[i];
  double g = 0;
  for (int k = vi_ptr[v]; k < vi_ptr[v + 1]; k++) {
    const FacDesc d = fd[vi_fac[k]];
    const int m = d.rows;
    const double* J = pool + d.joff;
    const double* Jc = J + (size_t)pcg_col(d, vi_pos[k], c) * m;
    const double* b = J + (size_t)(d.d0 + d.d1 + d.d2) * m;
    for (int r = 0; r < m; r++) g += Jc[r] * b[r];
  }
  grad[i] = -g;
}

// ---- direction = gradient (the gradient-descent step before the loop, .h:216-217, and the gradientDescent switch, :232-233);
//      block partials of direction . direction -> part_dd.  src == dir is allowed (a caller-supplied direction: only its norm is needed)
__global__ __launch_bounds__(256) void ncg_set_direction_kernel(int ntot, const double* src, double* dir, double* __restrict__ part_dd,
                                                                 NcgCtl* __restrict__ ctl) {
  __shared__ double sh[256];
  double dd = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ntot; i += gridDim.x * 256) {
    const double x = src[i];
    dir[i] = x;
    dd += x * x;
  }
  const double t = pcg_block_sum(dd, sh);
  if (threadIdx.x == 0) part_dd[blockIdx.x] = t;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->beta = 0.0;
}

// ---- the dot products beta needs, as block partials: part[0] g.g, part[1] g.(g - gp), part[2] gp.gp, part[3] s.(g - gp)
//      (g = currentGradient, gp = prevGradient, s = direction; the differences are formed per element like the reference's
//      `currentGradient - prevGradient`, .h:44, 56, 68)
__global__ __launch_bounds__(256) void ncg_dots_kernel(int ntot, const double* __restrict__ g, const double* __restrict__ gp,
                                                        const double* __restrict__ s, double* __restrict__ part) {
  __shared__ double sh[256];
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ntot; i += gridDim.x * 256) {
    const double gi = g[i], pi = gp[i], di = gi - pi;
    a0 += gi * gi;
    a1 += gi * di;
    a2 += pi * pi;
    a3 += s[i] * di;
  }
  const double t0 = pcg_block_sum(a0, sh), t1 = pcg_block_sum(a1, sh), t2 = pcg_block_sum(a2, sh), t3 = pcg_block_sum(a3, sh);
  if (threadIdx.x == 0) {
    part[0 * NCG_MAXPART + blockIdx.x] = t0;
    part[1 * NCG_MAXPART + blockIdx.x] = t1;
    part[2 * NCG_MAXPART + blockIdx.x] = t2;
    part[3 * NCG_MAXPART + blockIdx.x] = t3;
  }
}

// std::max(0.0, x) as the reference evaluates it (a NaN quotient gives 0)
__device__ __forceinline__ double ncg_max0(double x) { return (0.0 < x) ? x : 0.0; }

// ---- beta (.h:28-70, the switch :239-255) and direction = currentGradient + beta * direction (:257); block partials of the new
//      direction . direction -> part_dd.  Every block reduces the npart partials of ncg_dots_kernel in the same order.
__global__ __launch_bounds__(256) void ncg_direction_kernel(int ntot, int method, const double* __restrict__ part, int npart,
                                                             const double* __restrict__ g, double* __restrict__ dir,
                                                             double* __restrict__ part_dd, NcgCtl* __restrict__ ctl) {
  __shared__ double sh[256];
  const double gg = pcg_sum_partials(part + 0 * NCG_MAXPART, npart, sh);
  const double gd = pcg_sum_partials(part + 1 * NCG_MAXPART, npart, sh);
  const double pp = pcg_sum_partials(part + 2 * NCG_MAXPART, npart, sh);
  const double sd = pcg_sum_partials(part + 3 * NCG_MAXPART, npart, sh);
  double beta;
  if (method == 0) beta = gg / pp;                      // Fletcher-Reeves :32-35
  else if (method == 1) beta = ncg_max0(gd / pp);       // Polak-Ribiere :42-46
  else if (method == 2) beta = ncg_max0(gd / -sd);      // Hestenes-Stiefel :55-58
  else beta = ncg_max0(gg / -sd);                       // Dai-Yuan :65-69
  double dd = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ntot; i += gridDim.x * 256) {
    const double x = g[i] + __dmul_rn(beta, dir[i]);
    dir[i] = x;
    dd += x * x;
  }
  const double t = pcg_block_sum(dd, sh);
  if (threadIdx.x == 0) part_dd[blockIdx.x] = t;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->beta = beta;
}

// ---- head of lineSearch (.h:138-145): g = |direction|, the bracket [-1 / g, 0] and the first interior point
__global__ __launch_bounds__(256) void ncg_ls_begin_kernel(const double* __restrict__ part_dd, int npart, NcgCtl* __restrict__ ctl) {
  __shared__ double sh[256];
  const double dd = pcg_sum_partials(part_dd, npart, sh);
  if (threadIdx.x == 0) {
    const double g = sqrt(dd);
    const double phi = 0.5 * (1.0 + sqrt(5.0));
    const double minStep = -1.0 / g, maxStep = 0;
    const double newStep = minStep + (maxStep - minStep) / (phi + 1.0);
    ctl->dnorm = g;
    ctl->minStep = minStep;
    ctl->maxStep = maxStep;
    ctl->newStep = newStep;
    ctl->newError = 0.0;
    ctl->step = newStep;
    ctl->alpha = 0.0;
    ctl->error = 0.0;
    ctl->done = 0;
    ctl->trials = 0;
    ctl->flag = 0;
    ctl->first = 1;
  }
}

// ---- values = retract(base, s * direction) for one variable type: s = the trial's step, or (final) the accepted alpha.  A trial
//      behind `done` and a final advance in front of it do nothing.
__global__ __launch_bounds__(256) void ncg_retract_kernel(int type, int n, const double* base, double* out, const int32_t* __restrict__ xoff,
                                                           const double* __restrict__ dir, const NcgCtl* __restrict__ ctl, int final) {
  const int done = ctl->done;
  if (final ? !done : done) return;
  const double s = final ? ctl->alpha : ctl->step;
  retract_body(type, n, base, out, xoff, dir, nullptr, (int)(blockIdx.x * 256 + threadIdx.x), s, true);
}

// ---- the error sum of a trial: reduce_stage1 / reduce_stage2 (kernels_factors.hpp) operation for operation, so that a trial's error
//      has the bits lmgpu_error gives at the same values, with the early return of a trial queued behind `done`
__global__ __launch_bounds__(256) void ncg_reduce_stage1(const double* __restrict__ buf, int n, double* __restrict__ partial,
                                                          const int32_t* __restrict__ skip) {
  __shared__ double sh[256];
  if (skip && *skip) return;
  double s = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s += buf[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(256) void ncg_reduce_stage2(const double* __restrict__ partial, int n, double* __restrict__ out,
                                                          const int32_t* __restrict__ skip) {
  __shared__ double sh[256];
  if (skip && *skip) return;
  double s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sh[0];
}

// ---- after the error of a trial has been reduced into *err: the body of lineSearch's loop (.h:150-178), one thread
__global__ void ncg_ls_control_kernel(const double* __restrict__ err, NcgCtl* __restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (ctl->done) return;
  const double phi = 0.5 * (1.0 + sqrt(5.0)), resphi = 2.0 - phi, tau = 1e-5;
  double minStep = ctl->minStep, maxStep = ctl->maxStep, newStep = ctl->newStep, newError = ctl->newError;
  const double e = *err;
  if (ctl->first) {  // newError = system.error(advance(currentValues, newStep, gradient)) :147-148
    newError = e;
    ctl->first = 0;
  } else {  // update the working range :163-178
    const double testStep = ctl->step, testError = e;
    const int flag = ctl->flag;
    if (testError >= newError) {
      if (flag) maxStep = testStep;
      else minStep = testStep;
    } else {
      if (flag) minStep = newStep;
      else maxStep = newStep;
      newStep = testStep;
      newError = testError;
    }
  }
  ctl->trials += 1;
  const int flag = (maxStep - newStep > newStep - minStep);
  const double testStep = flag ? newStep + __dmul_rn(resphi, maxStep - newStep) : newStep - __dmul_rn(resphi, newStep - minStep);
  ctl->minStep = minStep;
  ctl->maxStep = maxStep;
  ctl->newStep = newStep;
  ctl->newError = newError;
  if ((maxStep - minStep) < tau * (fabs(testStep) + fabs(newStep))) {
    ctl->alpha = 0.5 * (minStep + maxStep);
    ctl->done = 1;
  } else {
    ctl->flag = flag;
    ctl->step = testStep;
  }
}

// ---- the error of the final advance joins the record the host reads
__global__ void ncg_final_kernel(const double* __restrict__ err, NcgCtl* __restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (ctl->done) ctl->error = *err;
}

}  // namespace lmgpu
