// SmartProjectionPoseFactor<Cal3_S2> on the device (gtsam/slam/SmartProjectionFactor.h, SmartProjectionPoseFactor.h, SmartFactorBase.h,
// SmartFactorParams.h; HESSIAN linearization, ZERO_ON_DEGENERACY).  A smart factor of m >= 2 observations is carried as a HIDDEN POINT3
// variable with m internal binary factors (pose, hidden point): eliminating that point in its leaf front gives exactly the factor's
// Hessian F'(I - E (E'E)^-1 E') F (CameraSet::SchurComplement, gtsam/geometry/CameraSet.h:145-216 with lambda = 0).  Three kernels:
//   smart_triangulate_kernel  the member triangulateSafe (SmartProjectionFactor.h:127-184): one lane per smart factor; the cache test
//                             (decideIfTriangulate :127-165: Pose3::equals -> fpEqual, gtsam/base/Vector.cpp:42-77, without the relative
//                             test as equal_with_abs_tol calls it, gtsam/base/Matrix.h:80-96) against the m x 12 cached doubles, then
//                             gtsam::triangulateSafe (triangulation.h:701-758) = tri_safe_point of kernels_triangulation.hpp.  It reads
//                             one cache set and writes the other, so that the speculative error evaluation of tryLambda can be dropped.
//   smart_factor_kernel       per observation: the whitened [F E b] at the cached point (PinholePose<Cal3_S2> projection Jacobians =
//                             those of GenericProjectionFactor, eval_projection) or the squared error (SmartProjectionFactor.h:411-439);
//                             a factor whose result is not valid gives zero error and F = 0, b = 0, E = two unit rows, which makes the
//                             Schur complement exactly zero (the reference's empty Hessian factor, :214-220) while E'E stays factorable.
//   smart_const_kernel        per smart factor 0.5 b'E (E'E)^-1 E'b: what the constant term of the Hessian factor, b'b - b'E (E'E)^-1 E'b
//                             (CameraSet.h:190-199), lacks against the sum of the observations' b'b.
// Plain FP64, vector stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_factors.hpp"
#include "kernels_triangulation.hpp"

namespace lmgpu {

struct SmartParamsDev {
  TriParamsDev tri;
  double retri_thr;  // SmartProjectionParams::retriangulationThreshold
};

// one set of the cache: cameraPosesTriangulation_ (12 doubles per observation), result_ (point, status) and "the cache is not empty"
struct SmartCacheDev {
  double* poses;
  double* points;
  int32_t* status;
  int32_t* have;
};

// fpEqual(a, b, tol, check_relative_also = false) (gtsam/base/Vector.cpp:42-77; DOUBLE_MIN_NORMAL = min() + 1.0 rounds to 1.0, so the
// branch for small values is the same test |a - b| <= tol)
__device__ __forceinline__ bool smart_fp_equal(double a, double b, double tol) {
  if (isnan(a) || isnan(b)) return isnan(a) && isnan(b);
  if (isinf(a) || isinf(b)) return isinf(a) && isinf(b);
  return fabs(a - b) <= tol;
}

// Smart factor order[first + i], i < count: SmartProjectionFactor::triangulateSafe(cameras) at the poses `poses` (the handle's POSE3 values).
// ptr / obs_cam: CSR of the observations (index of the pose in the POSE3 array); ref[o] = (0, the observation's factor in the internal
// bucket) and meas_tab[0] = that bucket's measurements, 7 doubles each (z, fx, fy, s, u0, v0): no second copy of them.  src -> dst: the cache
// before and after the call; retri[factor] = 1 where gtsam::triangulateSafe ran.
template <bool EPI>
__global__ __launch_bounds__(64) void smart_triangulate_kernel(int first, int count, const int32_t* __restrict__ order, const int32_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ obs_cam, const int2* __restrict__ ref,
                                                               const double* const* __restrict__ meas_tab,
                                                               const double* __restrict__ poses, SmartParamsDev prm, SmartCacheDev src,
                                                               SmartCacheDev dst, int32_t* __restrict__ retri) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const int sf = order[first + i];
  const int beg = ptr[sf], end = ptr[sf + 1];
  const double nan = __builtin_nan("");
  if (end - beg < 2) {  // :176-177: Degenerate(), the cache is not touched
    dst.status[sf] = 1;
    dst.have[sf] = src.have[sf];
    dst.points[(size_t)sf * 3 + 0] = dst.points[(size_t)sf * 3 + 1] = dst.points[(size_t)sf * 3 + 2] = nan;
    retri[sf] = 0;
    return;
  }
  bool re = src.have[sf] == 0;
  if (!re) {
    for (int o = beg; o < end && !re; o++) {
      const double* c = poses + (size_t)obs_cam[o] * 12;
      const double* q = src.poses + (size_t)o * 12;
#pragma unroll
      for (int k = 0; k < 12; k++) re = re || !smart_fp_equal(c[k], q[k], prm.retri_thr);
    }
  }
  if (!re) {
    for (int o = beg; o < end; o++)
#pragma unroll
      for (int k = 0; k < 12; k++) dst.poses[(size_t)o * 12 + k] = src.poses[(size_t)o * 12 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) dst.points[(size_t)sf * 3 + k] = src.points[(size_t)sf * 3 + k];
    dst.status[sf] = src.status[sf];
    dst.have[sf] = 1;
    retri[sf] = 0;
    return;
  }
  for (int o = beg; o < end; o++) {
    const double* c = poses + (size_t)obs_cam[o] * 12;
#pragma unroll
    for (int k = 0; k < 12; k++) dst.poses[(size_t)o * 12 + k] = c[k];
  }
  D3 x{0, 0, 0};
  int iters = 0;
  const int status = tri_safe_point<TRI_POSE_K, EPI>(beg, end, obs_cam, ref, meas_tab, poses, prm.tri, x, iters);
  dst.points[(size_t)sf * 3 + 0] = status == 0 ? x.x : nan;
  dst.points[(size_t)sf * 3 + 1] = status == 0 ? x.y : nan;
  dst.points[(size_t)sf * 3 + 2] = status == 0 ? x.z : nan;
  dst.status[sf] = status;
  dst.have[sf] = 1;
  retri[sf] = 1;
}

// The internal factor bucket (one factor per observation of a smart factor with m >= 2; shape of LMGPU_F_PROJECTION: 2 rows, pose 6 +
// point 3 + 1 columns, 7 measurement doubles, DIAG noise = the Isotropic inverse sigma twice).  sf_of[f] / j_of[f]: the smart factor of
// local factor f and the observation's position in it; points / status: the cache set the preceding smart_triangulate_kernel wrote.
template <bool JAC>
__global__ __launch_bounds__(128) void smart_factor_kernel(BucketDev b, ValuesDev vals, double* __restrict__ ebuf, const int32_t* __restrict__ sf_of,
                                                           const int32_t* __restrict__ j_of, const double* __restrict__ points,
                                                           const int32_t* __restrict__ status) {
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= b.n) return;
  constexpr int M = 2, COLS = 10;
  const int sf = sf_of[f];
  const bool valid = status[sf] == 0;
  double m[7], v0[12], v1[3];
  const double* mp = b.meas + (size_t)f * 7;
#pragma unroll
  for (int i = 0; i < 7; i++) m[i] = mp[i];
  const double* p0 = vals.v[1] + (size_t)b.vidx[2 * f] * 12;
#pragma unroll
  for (int i = 0; i < 12; i++) v0[i] = p0[i];
#pragma unroll
  for (int i = 0; i < 3; i++) v1[i] = valid ? points[(size_t)sf * 3 + i] : 0.0;
  const double* nz = b.noise + (size_t)f * 2;
  if (JAC) {
    double Jl[M * COLS];
    if (valid) {
      double e[2], H1[12], H2[6];
      eval_projection<true>(m, v0, v1, e, H1, H2);
#pragma unroll
      for (int r = 0; r < M; r++) {
#pragma unroll
        for (int c = 0; c < 6; c++) Jl[c * M + r] = H1[r * 6 + c];
#pragma unroll
        for (int c = 0; c < 3; c++) Jl[(6 + c) * M + r] = H2[r * 3 + c];
        Jl[9 * M + r] = -e[r];
      }
      whiten_block<M, COLS>(Jl, 2, nz);
    } else {
#pragma unroll
      for (int i = 0; i < M * COLS; i++) Jl[i] = 0.0;
      const int a0 = (2 * j_of[f]) % 3, a1 = (2 * j_of[f] + 1) % 3;  // observations 0 and 1 together cover the three axes
#pragma unroll
      for (int c = 0; c < 3; c++) {
        Jl[(6 + c) * M + 0] = c == a0 ? 1.0 : 0.0;
        Jl[(6 + c) * M + 1] = c == a1 ? 1.0 : 0.0;
      }
    }
    double* out = b.J + (size_t)f * (M * COLS);
#pragma unroll
    for (int i = 0; i < M * COLS; i++) out[i] = Jl[i];
  } else {
    double err = 0.0;
    if (valid) {
      double e[2], H1[1], H2[1];
      eval_projection<false>(m, v0, v1, e, H1, H2);
      err = whitened_half_sq<M>(e, 2, nz);
    }
    ebuf[b.epos[f]] = err;
  }
}

// Per smart factor with a hidden point (index hp, its internal factors [fptr[hp], fptr[hp + 1]) back to back in the bucket's Jacobians J):
// corr[hp] = 0.5 g'(E'E)^-1 g with g = E'b, by a 3x3 Cholesky.  0 for a factor that is not valid (b = 0).
__global__ __launch_bounds__(64) void smart_const_kernel(int n, const int32_t* __restrict__ fptr, const double* __restrict__ J,
                                                         double* __restrict__ corr) {
  const int hp = blockIdx.x * 64 + threadIdx.x;
  if (hp >= n) return;
  double H00 = 0, H01 = 0, H02 = 0, H11 = 0, H12 = 0, H22 = 0, g0 = 0, g1 = 0, g2 = 0;
  for (int f = fptr[hp]; f < fptr[hp + 1]; f++) {
    const double* A = J + (size_t)f * 20;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const double e0 = A[12 + r], e1 = A[14 + r], e2 = A[16 + r], bb = A[18 + r];
      H00 += e0 * e0; H01 += e0 * e1; H02 += e0 * e2; H11 += e1 * e1; H12 += e1 * e2; H22 += e2 * e2;
      g0 += e0 * bb; g1 += e1 * bb; g2 += e2 * bb;
    }
  }
  const double l00 = sqrt(H00), l10 = H01 / l00, l20 = H02 / l00;
  const double l11 = sqrt(H11 - l10 * l10), l21 = (H12 - l20 * l10) / l11;
  const double l22 = sqrt(H22 - l20 * l20 - l21 * l21);
  const double y0 = g0 / l00, y1 = (g1 - l10 * y0) / l11, y2 = (g2 - l20 * y0 - l21 * y1) / l22;
  corr[hp] = 0.5 * (y0 * y0 + y1 * y1 + y2 * y2);
}

__global__ void smart_sub_scalar_kernel(double* dst, const double* src) { *dst -= *src; }

}  // namespace lmgpu
