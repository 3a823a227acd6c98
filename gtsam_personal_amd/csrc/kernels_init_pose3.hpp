// InitializePose3 kernels (gtsam/slam/InitializePose3.cpp): projection of the relaxed rotations onto SO(3) and the Tron-Vidal
// gradient iteration.  One thread per pose / node, FP64 VALU, rotations as 9 doubles row-major; divergent only in the Logmap branches
// and the degree of a node.  No floating-point atomics: the max-norm goes through block partials read back by every block of the
// next launch.
#pragma once
#include <hip/hip_runtime.h>

#include "geometry_dev.hpp"

namespace lmgpu {

// SO3::Expmap (so3::ExpmapFunctor, gtsam/geometry/SO3.cpp:61-95; nearZero only at theta^2 <= epsilon)
__device__ inline R3 so3_expmap(D3 w) {
  const double theta2 = dot3(w, w);
  double A, B;
  if (theta2 <= 2.220446049250313e-16) {
    A = 1.0 - theta2 * (1.0 / 6.0);
    B = 0.5 - theta2 * (1.0 / 24.0);
  } else {
    const double theta = sqrt(theta2);
    A = sin(theta) / theta;
    const double s2 = sin(theta / 2.0);
    B = 2.0 * s2 * s2 / theta2;
  }
  const double W[9] = {0, -w.z, w.y, w.z, 0, -w.x, -w.y, w.x, 0};
  R3 R;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double ww = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
      R.m[3 * i + j] = (i == j ? 1.0 : 0.0) + A * W[3 * i + j] + B * ww;
    }
  return R;
}

// SO3::ClosestTo(A) = U diag(1, 1, det(U V^T)) V^T of A = U S V^T (gtsam/geometry/SO3.cpp:202-208), A row-major.
// One-sided Jacobi: plane rotations from the right make the columns of B = A V orthogonal (det V = +1); their norms are the singular
// values, B's normalised columns are U.  The column of the SMALLEST singular value is replaced by the cross product of the other
// two, which is that column times det(U) = det(U V^T): exactly the factor diag(1, 1, det) puts on the smallest singular value.
__device__ inline R3 so3_closest_to(const R3& A) {
  double B[3][3], V[3][3];  // [column][row]
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      B[c][r] = A.m[3 * r + c];
      V[c][r] = (r == c) ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double alpha = B[p][0] * B[p][0] + B[p][1] * B[p][1] + B[p][2] * B[p][2];
      const double beta = B[q][0] * B[q][0] + B[q][1] * B[q][1] + B[q][2] * B[q][2];
      const double gamma = B[p][0] * B[q][0] + B[p][1] * B[q][1] + B[p][2] * B[q][2];
      if (fabs(gamma) > 1e-16 * sqrt(alpha * beta) && gamma != 0.0) {
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int r = 0; r < 3; r++) {
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
  double n[3];
#pragma unroll
  for (int c = 0; c < 3; c++) n[c] = sqrt(B[c][0] * B[c][0] + B[c][1] * B[c][1] + B[c][2] * B[c][2]);
  const int k = (n[2] <= n[0] && n[2] <= n[1]) ? 2 : (n[1] <= n[0] ? 1 : 0);
  const int a = (k + 1) % 3, b = (k + 2) % 3;  // (a, b, k) is a cyclic permutation: u_k = u_a x u_b keeps det(U) = +1
  double U[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    U[a][r] = B[a][r] / n[a];
    U[b][r] = B[b][r] / n[b];
  }
  U[k][0] = U[a][1] * U[b][2] - U[a][2] * U[b][1];
  U[k][1] = U[a][2] * U[b][0] - U[a][0] * U[b][2];
  U[k][2] = U[a][0] * U[b][1] - U[a][1] * U[b][0];
  R3 R;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R.m[3 * i + j] = U[0][i] * V[0][j] + U[1][i] * V[1][j] + U[2][i] * V[2][j];
  return R;
}

// normalizeRelaxedRotations (InitializePose3.cpp:75-92): x = the relaxed 9-vector of pose i = M column-major; Rot3::ClosestTo(M^T).
// M^T row-major is x as it stands.
__global__ __launch_bounds__(64) void init_pose3_project_kernel(int n, const double* __restrict__ relaxed, double* __restrict__ R_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  R3 A;
#pragma unroll
  for (int k = 0; k < 9; k++) A.m[k] = relaxed[(size_t)i * 9 + k];
  const R3 R = so3_closest_to(A);
#pragma unroll
  for (int k = 0; k < 9; k++) R_out[(size_t)i * 9 + k] = R.m[k];
}

// gradientTron (InitializePose3.cpp:256-275)
__device__ inline D3 gradient_tron(const R3& R1, const R3& R2, double a, double b) {
  D3 l = so3_logmap(mul3_tn(R1, R2));
  double th = sqrt(dot3(l, l));
  if (th != th) {  // NaN: Logmap near +/- pi; the reference perturbs R1 and tries again
    const R3 R1pert = mul3(R1, so3_expmap(D3{0.01, 0.01, 0.01}));
    l = so3_logmap(mul3_tn(R1pert, R2));
    th = sqrt(dot3(l, l));
  }
  if (th > 1e-5 && th == th) {
    l = (1.0 / th) * l;
  } else {
    l = D3{0, 0, 0};
    th = 0.0;
  }
  const double fdot = a * b * th * exp(-b * th);
  return fdot * l;
}

struct GradCtl {
  double max_grad;  // maxGrad of the last executed iteration
  int32_t iters;    // loop bodies executed
  int32_t done;     // the loop has ended (stop rule or maxIter)
};

// Iteration k of computeOrientationsGradient (InitializePose3.cpp:157-202) on the inverse rotations: reads buf[k & 1], writes buf[(k + 1) & 1].
// Its head finishes iteration k - 1: every block takes the maximum of that iteration's block partials (part[(k - 1) & 1]) and applies
// the stop rule `it > 20 && maxGrad < 5e-3` (and it == maxIter) -- the same decision in every block, no grid-wide barrier.  A block
// that stops marks its partial slot of this iteration with -1, which stops every later launch at once; block 0 records the state.
// CSR per node in factor-index order: other = the node at the far end, edge = index of Rij, pos = this node's key position in the factor.
__global__ __launch_bounds__(64) void init_pose3_gradient_kernel(int n, int k, int max_iter, const int32_t* __restrict__ ptr,
                                                                  const int32_t* __restrict__ other, const int32_t* __restrict__ edge,
                                                                  const int8_t* __restrict__ pos, const double* __restrict__ Rij, double* buf0,
                                                                  double* buf1, double* part0, double* part1, GradCtl* ctl, double a, double b,
                                                                  double stepsize) {
  __shared__ double sh[64];
  __shared__ int stop_sh;
  const int tid = threadIdx.x, nb = gridDim.x;
  double* part_prev = (k & 1) ? part0 : part1;
  double* part_cur = (k & 1) ? part1 : part0;
  {
    double m = 0.0;
    bool stopped = false;
    if (k > 0) {
      for (int i = tid; i < nb; i += 64) {
        const double g = part_prev[i];
        stopped = stopped || (g < 0.0);
        if (g > m) m = g;
      }
    }
    sh[tid] = stopped ? -1.0 : m;
    __syncthreads();
    if (tid == 0) {
      double mm = 0.0;
      bool st = false;
      for (int i = 0; i < 64; i++) {
        st = st || (sh[i] < 0.0);
        if (sh[i] > mm) mm = sh[i];
      }
      int stop = st ? 2 : 0;
      if (!st && ((k - 1 > 20 && mm < 5e-3) || k >= max_iter)) stop = 1;
      if (blockIdx.x == 0 && !st) {
        ctl->iters = k;
        ctl->max_grad = mm;
        if (stop) ctl->done = 1;
      }
      if (stop) part_cur[blockIdx.x] = -1.0;
      stop_sh = stop;
    }
    __syncthreads();
    if (stop_sh) return;
  }
  const double* in = (k & 1) ? buf1 : buf0;
  double* out = (k & 1) ? buf0 : buf1;
  const int i = blockIdx.x * 64 + tid;
  double gn = 0.0;
  if (i < n) {
    R3 Ri;
#pragma unroll
    for (int q = 0; q < 9; q++) Ri.m[q] = in[(size_t)i * 9 + q];
    D3 grad{0, 0, 0};
    for (int e = ptr[i]; e < ptr[i + 1]; e++) {
      R3 Rj, Rm;
      const double* rj = in + (size_t)other[e] * 9;
      const double* rm = Rij + (size_t)edge[e] * 9;
#pragma unroll
      for (int q = 0; q < 9; q++) {
        Rj.m[q] = rj[q];
        Rm.m[q] = rm[q];
      }
      // key == keys[0]: Rij * Rj; key == keys[1]: Rij.between(Rj) = Rij^T Rj   (:171-179)
      const R3 R2 = pos[e] == 0 ? mul3(Rm, Rj) : mul3_tn(Rm, Rj);
      grad = grad + gradient_tron(Ri, R2, a, b);
    }
    gn = sqrt(dot3(grad, grad));
    const R3 Rn = mul3(Ri, so3_expmap(stepsize * grad));  // Ri.retract(stepsize * grad), Rot3 retract = Expmap
#pragma unroll
    for (int q = 0; q < 9; q++) out[(size_t)i * 9 + q] = Rn.m[q];
  }
  // block maximum as the reference takes it (`if (norm > maxGrad)`: a NaN norm is skipped)
  sh[tid] = gn;
  __syncthreads();
  if (tid == 0) {
    double m = 0.0;
    for (int q = 0; q < 64; q++)
      if (sh[q] > m) m = sh[q];
    part_cur[blockIdx.x] = m;
  }
}

// the estimate from the inverse rotations (InitializePose3.cpp:204-217): R^-1, or Rref * R^-1 with Rref = the anchor's entry
__global__ __launch_bounds__(64) void init_pose3_gradient_result_kernel(int n, const double* __restrict__ inv, int anchor, int set_ref_frame,
                                                                         double* __restrict__ R_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  R3 R, Rt, ref;
#pragma unroll
  for (int q = 0; q < 9; q++) {
    R.m[q] = inv[(size_t)i * 9 + q];
    ref.m[q] = inv[(size_t)anchor * 9 + q];
  }
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Rt.m[3 * r + c] = R.m[3 * c + r];
  const R3 o = set_ref_frame ? mul3(ref, Rt) : Rt;
#pragma unroll
  for (int q = 0; q < 9; q++) R_out[(size_t)i * 9 + q] = o.m[q];
}

// inverse rotations of the given guess (:123-129); the anchor starts at the identity
__global__ __launch_bounds__(64) void init_pose3_gradient_start_kernel(int n, const double* __restrict__ guess, int anchor, double* __restrict__ inv) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) inv[(size_t)i * 9 + 3 * r + c] = (i == anchor) ? (r == c ? 1.0 : 0.0) : guess[(size_t)i * 9 + 3 * c + r];
}

// computePoses' start (InitializePose.h:63-74): Pose3(rot, origin) per pose, the anchor at the identity
__global__ __launch_bounds__(64) void init_pose3_upgrade_kernel(int n, const double* __restrict__ R, int anchor, double* __restrict__ poses) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int q = 0; q < 9; q++) poses[(size_t)i * 12 + q] = (i == anchor) ? ((q % 4 == 0) ? 1.0 : 0.0) : R[(size_t)i * 9 + q];
  poses[(size_t)i * 12 + 9] = 0.0;
  poses[(size_t)i * 12 + 10] = 0.0;
  poses[(size_t)i * 12 + 11] = 0.0;
}

}  // namespace lmgpu
