// Batched landmark triangulation (gtsam/geometry/triangulation.h, triangulation.cpp): triangulatePoint3 + triangulateSafe for
// PinholeCamera<Cal3Bundler> and PinholeCamera<Cal3_S2>, one lane per landmark, everything in registers, FP64 VALU.
//   DLT         the 2m rows x P.row(2) - P.row(0), y P.row(2) - P.row(1) (triangulation.cpp:27-56) are streamed through Givens rotations
//               into a 4x4 upper-triangular R (A = Q R: the singular values and right singular vectors of R are those of A; A^T A is never
//               formed, squaring would lose the small singular value the rank test and the null vector rest on), then a one-sided Jacobi
//               SVD of R as in kernels_init_pose3.hpp.  rank = singular values > rank_tol (gtsam/base/Matrix.cpp:556-574).
//   refinement  triangulateNonlinear (triangulation.h:153-221, triangulation.cpp:177-195) as a per-lane Levenberg-Marquardt on the 3-vector:
//               3x3 normal equations accumulated over the observations, 3x3 Cholesky, the lambda policy and the stop rules of
//               LevenbergMarquardtOptimizer::tryLambda / iterate and NonlinearOptimizer::defaultOptimize as lmgpu_iterate restates them.
//               Compiled out by the template parameter EPI.
//   checks      cheirality, landmarkDistanceThreshold, dynamicOutlierRejectionThreshold in triangulateSafe's precedence (triangulation.h:701-758).
// Cameras are gathered by index once per observation and pass (1000 cameras are 120 KB: L2-resident); no per-lane array is indexed by a
// runtime value.  Status, iteration count and point are plain vector stores; no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "geometry_dev.hpp"

namespace lmgpu {

// camera / measurement layouts
//   TRI_BUNDLER  camera 15 doubles (R 9, t 3, f, k1, k2), measurement 2 doubles relative to the principal point
//   TRI_S2       camera 17 doubles (R 9, t 3, fx, fy, s, u0, v0), measurement 2 doubles
//   TRI_POSE_K   camera 12 doubles (a POSE3 value), measurement 7 doubles (z, fx, fy, s, u0, v0): LMGPU_F_PROJECTION as it lies in a handle
enum { TRI_BUNDLER = 0, TRI_S2 = 1, TRI_POSE_K = 2 };

struct TriParamsDev {
  double rank_tol, dist_thr, outlier_thr, inv_sigma;  // inv_sigma 0: Unit
};

struct TriCam {
  R3 R;
  D3 t;
  double fx, fy, s, u0, v0, k1, k2;
  double zx, zy;
};

template <int MODEL>
__device__ __forceinline__ constexpr int tri_cam_stride() {
  return MODEL == TRI_BUNDLER ? 15 : (MODEL == TRI_S2 ? 17 : 12);
}

// observation o of the CSR: its camera and its measurement.  ref == nullptr: measurement o of table 0 (the stand-alone form).
template <int MODEL>
__device__ __forceinline__ TriCam tri_load(int o, const int32_t* __restrict__ obs_cam, const int2* __restrict__ ref,
                                           const double* const* __restrict__ meas_tab, const double* __restrict__ cams) {
  constexpr int MS = MODEL == TRI_POSE_K ? 7 : 2;
  const double* c = cams + (size_t)obs_cam[o] * tri_cam_stride<MODEL>();
  const double* m;
  if (ref) {
    const int2 r = ref[o];
    m = meas_tab[r.x] + (size_t)r.y * MS;
  } else {
    m = meas_tab[0] + (size_t)o * MS;
  }
  TriCam k;
#pragma unroll
  for (int i = 0; i < 9; i++) k.R.m[i] = c[i];
  k.t = {c[9], c[10], c[11]};
  k.zx = m[0];
  k.zy = m[1];
  if constexpr (MODEL == TRI_BUNDLER) {
    k.fx = k.fy = c[12];
    k.s = k.u0 = k.v0 = 0.0;
    k.k1 = c[13];
    k.k2 = c[14];
  } else if constexpr (MODEL == TRI_S2) {
    k.fx = c[12]; k.fy = c[13]; k.s = c[14]; k.u0 = c[15]; k.v0 = c[16];
    k.k1 = k.k2 = 0.0;
  } else {
    k.fx = m[2]; k.fy = m[3]; k.s = m[4]; k.u0 = m[5]; k.v0 = m[6];
    k.k1 = k.k2 = 0.0;
  }
  return k;
}

// PinholeCamera<CAL>::project2(point, {}, Dpoint) (PinholeCamera.h:283-300; PinholeBase::project2 CalibratedCamera.cpp:116-136, Dpoint :37-46;
// Cal3Bundler::uncalibrate Cal3Bundler.cpp:64-90, Cal3_S2::uncalibrate).  Returns false where the reference throws CheiralityException.
template <int MODEL, bool JAC>
__device__ __forceinline__ bool tri_project(const TriCam& k, D3 p, double& u, double& v, double* J /* 2x3 row-major */) {
  const D3 q = unrot(k.R, p - k.t);
  if (q.z <= 0.0) return false;
  const double d = 1.0 / q.z;
  const double x = q.x * d, y = q.y * d;
  double D00, D01, D10, D11;  // Dpi_pn
  if constexpr (MODEL == TRI_BUNDLER) {
    const double r = x * x + y * y;
    const double g = 1.0 + (k.k1 + k.k2 * r) * r;
    u = k.u0 + k.fx * (g * x);
    v = k.v0 + k.fx * (g * y);
    if constexpr (JAC) {
      const double a = 2.0 * (k.k1 + 2.0 * k.k2 * r);
      D00 = k.fx * (g + a * x * x);
      D01 = D10 = k.fx * (a * x * y);
      D11 = k.fx * (g + a * y * y);
    }
  } else {
    u = k.fx * x + k.s * y + k.u0;
    v = k.fy * y + k.v0;
    if constexpr (JAC) {
      D00 = k.fx; D01 = k.s; D10 = 0.0; D11 = k.fy;
    }
  }
  if constexpr (JAC) {
#pragma unroll
    for (int j = 0; j < 3; j++) {  // Rt(i, j) = R(j, i)
      const double n0 = d * (k.R.m[3 * j + 0] - x * k.R.m[3 * j + 2]);
      const double n1 = d * (k.R.m[3 * j + 1] - y * k.R.m[3 * j + 2]);
      J[j] = D00 * n0 + D01 * n1;
      J[3 + j] = D10 * n0 + D11 * n1;
    }
  }
  return true;
}

// Cal3Bundler::calibrate (Cal3Bundler.cpp:93-128) of a measurement relative to the principal point, then the pinhole part's uncalibrate
// (undistortMeasurementInternal, triangulation.h:252-268).  false: not converged after 10 passes (the reference throws std::runtime_error).
__device__ __forceinline__ bool tri_undistort_bundler(const TriCam& k, double& zx, double& zy) {
  const double ix = k.zx / k.fx, iy = k.zy / k.fx;
  double px = ix, py = iy, nx = 0.0, ny = 0.0;
  int it = 0;
  do {
    const double rr = px * px + py * py;
    const double g = 1.0 + k.k1 * rr + k.k2 * rr * rr;
    nx = ix / g;
    ny = iy / g;
    const double r = nx * nx + ny * ny;
    const double gu = 1.0 + (k.k1 + k.k2 * r) * r;
    const double du = k.fx * (gu * nx) - k.zx, dv = k.fx * (gu * ny) - k.zy;
    if (sqrt(du * du + dv * dv) <= 1e-5) break;
    px = nx;
    py = ny;
    it++;
  } while (it < 10);
  zx = k.fx * nx;
  zy = k.fx * ny;
  return it < 10;
}

// one row of the DLT matrix into the 4x4 upper-triangular R by Givens rotations
__device__ __forceinline__ void tri_givens_row(double (&R)[4][4], double v0, double v1, double v2, double v3) {
  double v[4] = {v0, v1, v2, v3};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (v[k] != 0.0) {
      const double a = R[k][k], b = v[k];
      const double r = sqrt(a * a + b * b);
      const double c = a / r, s = b / r;
#pragma unroll
      for (int j = k; j < 4; j++) {
        const double rj = R[k][j], vj = v[j];
        R[k][j] = c * rj + s * vj;
        v[j] = c * vj - s * rj;
      }
    }
  }
}

// one-sided Jacobi SVD of the 4x4 R: plane rotations from the right make the columns of B = R V orthogonal; their norms are the singular
// values.  rank = those > rank_tol; vout = the column of V of the smallest one (selected with compares, no runtime index).
__device__ inline int tri_svd4(const double (&R)[4][4], double rank_tol, double (&vout)[4]) {
  double B[4][4], V[4][4];  // [column][row]
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      B[c][r] = r <= c ? R[r][c] : 0.0;
      V[c][r] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          alpha += B[p][r] * B[p][r];
          beta += B[q][r] * B[q][r];
          gamma += B[p][r] * B[q][r];
        }
        if (fabs(gamma) > 1e-16 * sqrt(alpha * beta) && gamma != 0.0) {
          rotated = true;
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const double bp = B[p][r], bq = B[q][r], vp = V[p][r], vq = V[q][r];
            B[p][r] = c * bp - s * bq;
            B[q][r] = s * bp + c * bq;
            V[p][r] = c * vp - s * vq;
            V[q][r] = s * vp + c * vq;
          }
        }
      }
    if (!rotated) break;
  }
  int rank = 0;
  double best = 0.0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double n = sqrt(B[c][0] * B[c][0] + B[c][1] * B[c][1] + B[c][2] * B[c][2] + B[c][3] * B[c][3]);
    if (n > rank_tol) rank++;
    if (c == 0 || n < best) {
      best = n;
#pragma unroll
      for (int r = 0; r < 4; r++) vout[r] = V[c][r];
    }
  }
  return rank;
}

// NonlinearFactorGraph::error of the triangulation graph at p: 0.5 sum |w (project(p) - z)|^2; a point behind a camera contributes the
// error (2 fx, 2 fx) (TriangulationFactor.h:122-136, PinholeCamera.h:321-323)
template <int MODEL>
__device__ inline double tri_graph_error(int beg, int end, const int32_t* __restrict__ obs_cam, const int2* __restrict__ ref,
                                         const double* const* __restrict__ meas_tab, const double* __restrict__ cams, D3 p, double w) {
  double e = 0.0;
  for (int o = beg; o < end; o++) {
    const TriCam k = tri_load<MODEL>(o, obs_cam, ref, meas_tab, cams);
    double u, v, ex, ey;
    if (tri_project<MODEL, false>(k, p, u, v, nullptr)) {
      ex = w * (u - k.zx);
      ey = w * (v - k.zy);
    } else {
      ex = ey = w * (2.0 * k.fx);
    }
    e += ex * ex + ey * ey;
  }
  return 0.5 * e;
}

// The refinement: NonlinearOptimizer::defaultOptimize (NonlinearOptimizer.cpp:62-117) around LevenbergMarquardtOptimizer::iterate / tryLambda
// (LevenbergMarquardtOptimizer.cpp:121-308) with the parameters of triangulation.cpp:177-195: lambdaInitial 1, lambdaFactor 10 (fixed),
// lambdaUpperBound 1e5, lambdaLowerBound 0, minModelFidelity 1e-3, maxIterations 100, relativeErrorTol 1e-5, absoluteErrorTol 1, errorTol 0,
// no diagonal damping.  The damped system of one 3-vector is (H + lambda I) delta = g with H = sum J^T J, g = -sum J^T e; its linear
// error is M(delta) = M(0) - g.delta + 0.5 delta.H.delta, so linearizedCostChange = g.delta - 0.5 delta.H.delta needs no second pass.
// Returns the number of tryLambda calls.
template <int MODEL>
__device__ inline int tri_refine(int beg, int end, const int32_t* __restrict__ obs_cam, const int2* __restrict__ ref,
                                 const double* const* __restrict__ meas_tab, const double* __restrict__ cams, double w, D3& x) {
  double err = tri_graph_error<MODEL>(beg, end, obs_cam, ref, meas_tab, cams, x, w);
  double lambda = 1.0;
  int iterations = 0, inner = 0;
  if (err <= 0.0) return 0;
  double newError = err, currentError;
  bool go_on;
  do {
    currentError = newError;
    // linearize
    double H00 = 0, H01 = 0, H02 = 0, H11 = 0, H12 = 0, H22 = 0, g0 = 0, g1 = 0, g2 = 0, oldLin = 0;
    for (int o = beg; o < end; o++) {
      const TriCam k = tri_load<MODEL>(o, obs_cam, ref, meas_tab, cams);
      double u, v, J[6], b0, b1;
      if (tri_project<MODEL, true>(k, x, u, v, J)) {
        b0 = -w * (u - k.zx);
        b1 = -w * (v - k.zy);
#pragma unroll
        for (int j = 0; j < 6; j++) J[j] *= w;
      } else {
        b0 = b1 = -w * (2.0 * k.fx);
#pragma unroll
        for (int j = 0; j < 6; j++) J[j] = 0.0;
      }
      H00 += J[0] * J[0] + J[3] * J[3];
      H01 += J[0] * J[1] + J[3] * J[4];
      H02 += J[0] * J[2] + J[3] * J[5];
      H11 += J[1] * J[1] + J[4] * J[4];
      H12 += J[1] * J[2] + J[4] * J[5];
      H22 += J[2] * J[2] + J[5] * J[5];
      g0 += J[0] * b0 + J[3] * b1;
      g1 += J[1] * b0 + J[4] * b1;
      g2 += J[2] * b0 + J[5] * b1;
      oldLin += b0 * b0 + b1 * b1;
    }
    oldLin *= 0.5;
    // while (!tryLambda())
    for (;;) {
      inner++;
      bool step_ok = false, stop = false;
      double nerr = INFINITY;
      D3 xn = x;
      // Cholesky of H + lambda I
      const double a00 = H00 + lambda, a11 = H11 + lambda, a22 = H22 + lambda;
      bool solved = a00 > 0.0;
      const double l00 = sqrt(a00);
      const double l10 = H01 / l00, l20 = H02 / l00;
      const double d11 = a11 - l10 * l10;
      solved = solved && d11 > 0.0;
      const double l11 = sqrt(d11);
      const double l21 = (H12 - l20 * l10) / l11;
      const double d22 = a22 - l20 * l20 - l21 * l21;
      solved = solved && d22 > 0.0;
      if (solved) {
        const double l22 = sqrt(d22);
        const double y0 = g0 / l00;
        const double y1 = (g1 - l10 * y0) / l11;
        const double y2 = (g2 - l20 * y0 - l21 * y1) / l22;
        const double dz = y2 / l22;
        const double dy = (y1 - l21 * dz) / l11;
        const double dx = (y0 - l10 * dy - l20 * dz) / l00;
        const double dHd = dx * (H00 * dx + H01 * dy + H02 * dz) + dy * (H01 * dx + H11 * dy + H12 * dz) + dz * (H02 * dx + H12 * dy + H22 * dz);
        const double lcc = (g0 * dx + g1 * dy + g2 * dz) - 0.5 * dHd;
        if (lcc >= 0.0) {
          xn = {x.x + dx, x.y + dy, x.z + dz};
          nerr = tri_graph_error<MODEL>(beg, end, obs_cam, ref, meas_tab, cams, xn, w);
          const double costChange = err - nerr;
          if (lcc > 2.220446049250313e-16 * oldLin) step_ok = (costChange / lcc) > 1e-3;
          if (fabs(costChange) < 1e-5 * err) stop = true;
        }
      }
      if (step_ok) {
        x = xn;
        err = nerr;
        lambda = fmax(0.0, lambda / 10.0);
        iterations++;
        break;
      } else if (!stop) {
        lambda *= 10.0;
        if (lambda >= 1e5) break;
      } else {
        break;
      }
    }
    newError = err;
    // checkConvergence (NonlinearOptimizer.cpp:182-231)
    bool conv = newError <= 0.0;
    if (!conv) {
      const double dec = currentError - newError;
      conv = (dec / currentError <= 1e-5) || (dec <= 1.0);
    }
    go_on = iterations < 100 && !conv && isfinite(currentError);
  } while (go_on);
  return inner;
}

// triangulateSafe of one landmark (triangulation.h:701-758 over triangulatePoint3 :491-549), the observations [beg, end) of the CSR with
// end - beg >= 2: DLT, rank test, optional refinement, then the cheirality / distance / outlier checks in the reference's precedence.
// Returns the status (enum lmgpu_triangulation_status); x = the point, iters = tryLambda calls of the refinement.  The one definition
// behind triangulate_kernel and the smart factors' smart_triangulate_kernel (kernels_smart.hpp).
template <int MODEL, bool EPI>
__device__ inline int tri_safe_point(int beg, int end, const int32_t* __restrict__ obs_cam, const int2* __restrict__ ref,
                                     const double* const* __restrict__ meas_tab, const double* __restrict__ cams, const TriParamsDev& prm, D3& x,
                                     int& iters) {
  int status = 0;
  double R[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) R[r][c] = 0.0;
  bool calib_ok = true;
  for (int o = beg; o < end; o++) {
    const TriCam k = tri_load<MODEL>(o, obs_cam, ref, meas_tab, cams);
    double zx = k.zx, zy = k.zy;
    if constexpr (MODEL == TRI_BUNDLER) calib_ok = tri_undistort_bundler(k, zx, zy) && calib_ok;
    // P = K [R^T | -R^T t] (PinholeCamera.h:316-318): c_i = row i of the calibrated projection matrix
    const D3 tc = unrot(k.R, D3{-k.t.x, -k.t.y, -k.t.z});
    double P0[4], P1[4], P2[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double c0 = j < 3 ? k.R.m[3 * j + 0] : tc.x;
      const double c1 = j < 3 ? k.R.m[3 * j + 1] : tc.y;
      const double c2 = j < 3 ? k.R.m[3 * j + 2] : tc.z;
      P0[j] = k.fx * c0 + k.s * c1 + k.u0 * c2;
      P1[j] = k.fy * c1 + k.v0 * c2;
      P2[j] = c2;
    }
    tri_givens_row(R, zx * P2[0] - P0[0], zx * P2[1] - P0[1], zx * P2[2] - P0[2], zx * P2[3] - P0[3]);
    tri_givens_row(R, zy * P2[0] - P1[0], zy * P2[1] - P1[1], zy * P2[2] - P1[2], zy * P2[3] - P1[3]);
  }
  double v[4];
  const int rank = tri_svd4(R, prm.rank_tol, v);
  if (!calib_ok) {
    status = 5;
  } else if (rank < 3) {
    status = 1;
  } else {
    x = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
    if constexpr (EPI) iters = tri_refine<MODEL>(beg, end, obs_cam, ref, meas_tab, cams, prm.inv_sigma > 0.0 ? prm.inv_sigma : 1.0, x);
    // triangulatePoint3's cheirality check, then triangulateSafe's loop (triangulation.h:540-546, 718-745)
    bool behind = false, far = false;
    double max_rep = 0.0;
    for (int o = beg; o < end; o++) {
      const TriCam k = tri_load<MODEL>(o, obs_cam, ref, meas_tab, cams);
      const D3 dvec = x - k.t;
      double u, w;
      if (!tri_project<MODEL, false>(k, x, u, w, nullptr)) {
        behind = true;
      } else {
        const double eu = u - k.zx, ev = w - k.zy;
        max_rep = fmax(max_rep, sqrt(eu * eu + ev * ev));
      }
      if (prm.dist_thr > 0.0 && sqrt(dot3(dvec, dvec)) > prm.dist_thr) far = true;
    }
    if (behind)
      status = 2;
    else if (far)
      status = 4;
    else if (prm.outlier_thr > 0.0 && max_rep > prm.outlier_thr)
      status = 3;
  }
  return status;
}

// Landmark order[first + i], i < count: status (enum lmgpu_triangulation_status), point (NaN unless VALID) and tryLambda calls, stored at
// the landmark's own index.  values (may be null): the handle's POINT3 values, VALID points are stored at 3 * val_idx[landmark].
template <int MODEL, bool EPI>
__global__ __launch_bounds__(64) void triangulate_kernel(int first, int count, const int32_t* __restrict__ order, const int32_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ obs_cam, const int2* __restrict__ ref,
                                                         const double* const* __restrict__ meas_tab, const double* __restrict__ cams,
                                                         TriParamsDev prm, double* __restrict__ points_out, int32_t* __restrict__ status_out,
                                                         int32_t* __restrict__ iters_out, double* values, const int32_t* __restrict__ val_idx) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const int lm = order[first + i];
  const int beg = ptr[lm], end = ptr[lm + 1];
  int status = 0, iters = 0;
  D3 x{0, 0, 0};
  if (end - beg < 2) {
    status = 1;
  } else {
    status = tri_safe_point<MODEL, EPI>(beg, end, obs_cam, ref, meas_tab, cams, prm, x, iters);
  }
  const double nan = __builtin_nan("");
  points_out[(size_t)lm * 3 + 0] = status == 0 ? x.x : nan;
  points_out[(size_t)lm * 3 + 1] = status == 0 ? x.y : nan;
  points_out[(size_t)lm * 3 + 2] = status == 0 ? x.z : nan;
  status_out[lm] = status;
  iters_out[lm] = iters;
  if (values && status == 0) {
    double* dst = values + (size_t)val_idx[lm] * 3;
    dst[0] = x.x;
    dst[1] = x.y;
    dst[2] = x.z;
  }
}

}  // namespace lmgpu
