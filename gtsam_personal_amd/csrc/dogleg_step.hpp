// The host arithmetic of one Dogleg trial (dl_iterate in lmgpu.hip calls both; host only, no HIP call): where on the dogleg path the
// trial point lies, and what the gain ratio does to the trust radius.  Pinned without a device by tests/test_bt_products_reference.py
// through lmgpu_selftest_dogleg_step.
//
// DoglegOptimizerImpl::ComputeDoglegPoint / ComputeBlend (gtsam/nonlinear/DoglegOptimizerImpl.cpp:26-91) and the radius update of
// DoglegOptimizerImpl::Iterate (DoglegOptimizerImpl.h:139-254) under ONE_STEP_PER_ITERATION.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

namespace lmgpu {

enum DoglegBranch : int { DOGLEG_STEEPEST = 0, DOGLEG_BLEND = 1, DOGLEG_NEWTON = 2 };

// dx_d = scalar * dx_u (DOGLEG_STEEPEST), (1 - scalar) * dx_u + scalar * dx_n (DOGLEG_BLEND), dx_n (DOGLEG_NEWTON; scalar = 1)
struct DoglegTrial {
  int branch;
  double scalar;
};

// uu = dx_u . dx_u, nn = dx_n . dx_n, un = dx_u . dx_n.  The blend solves |dx_u + tau (dx_n - dx_u)|^2 = delta^2 and takes the root
// inside [-eps, 1 + eps], tau1 first.
inline DoglegTrial dogleg_trial_point(double delta, double uu, double nn, double un) {
  const double deltaSq = delta * delta;
  if (deltaSq < uu) return {DOGLEG_STEEPEST, std::sqrt(deltaSq / uu)};
  if (deltaSq < nn) {
    const double a = uu - 2. * un + nn, b = 2. * (un - uu), c = uu - delta * delta;
    const double sq = std::sqrt(b * b - 4 * a * c);
    const double tau1 = (-b + sq) / (2. * a), tau2 = (-b - sq) / (2. * a);
    const double eps = std::numeric_limits<double>::epsilon();
    return {DOGLEG_BLEND, (-eps <= tau1 && tau1 <= 1.0 + eps) ? tau1 : tau2};
  }
  return {DOGLEG_NEWTON, 1.0};
}

// stay: try again from the same linearization with the new radius; moved = false: the radius is at its floor and f still rises, so
// the step is dropped (dx_d = 0, values and error kept)
struct DoglegRadius {
  double delta;
  bool stay, moved;
};

// norm_dx_d = |dx_d| is only read when rho >= 0.75.  A NaN rho fails every comparison and lands in the last branch.
inline DoglegRadius dogleg_radius_update(double rho, double delta, double norm_dx_d) {
  if (rho >= 0.75) return {std::max(delta, 3.0 * norm_dx_d), false, true};
  if (rho >= 0.25) return {delta, false, true};
  if (rho >= 0.0) return {delta > 1e-5 ? delta * 0.5 : delta, false, true};  // ONE_STEP_PER_ITERATION
  if (delta > 1e-5) return {delta * 0.5, true, true};  // f increased: halve the radius until it does not
  return {delta, false, false};
}

}  // namespace lmgpu
