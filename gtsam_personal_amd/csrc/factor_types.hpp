// What a factor type IS, in one table: rows of its error, doubles of its measurement, the variable types it connects.  Everything else
// the host and the kernels need to know about a type's shape (arity, Jacobian columns, noise doubles, the template constants of
// generic_factor_kernel: FactorDims in kernels_factors.hpp) is derived from a row of it.  Plain C++: plan.cpp reads it through plan.hpp.
#pragma once
#include "../../include/lmgpu.h"

namespace lmgpu {

static const int kNumVarTypes = LMGPU_NUM_VAR_TYPES;
// per lmgpu_var_type: tangent dimension, doubles of a stored value (a POSE3 is R row-major + t, a camera POSE3 + f, k1, k2)
static constexpr int kVarDim[kNumVarTypes] = {3, 6, 3, 9, 2, 5, 9};
static constexpr int kVarStore[kNumVarTypes] = {3, 12, 3, 15, 2, 5, 9};
static const int kMaxArity = 3;

struct FactorType {
  int rows;            // of the error vector = of the Jacobian
  int meas;            // doubles of one measurement on the device
  int var[kMaxArity];  // lmgpu_var_type of each variable, -1 beyond the arity
};
// entries 0 .. 13: the public lmgpu_factor_type; entry 14 (kSmartObsType): one observation of a smart projection factor, (POSE3, hidden
// POINT3) in the shape of LMGPU_F_PROJECTION -- internal to the batch handle (smart.hpp), never accepted at the boundary
// entries 15, 16: the two factor kinds of TranslationRecovery (translation_recovery.hpp), both (POINT3, POINT3) with a 3-vector measurement:
// TranslationFactor (gtsam/sfm/TranslationFactor.h) and BetweenFactor<Point3> -- internal to that session's inner handle in the same way
static const int kSmartObsType = 14;
static const int kTranslationType = 15;
static const int kBetweenPoint3Type = 16;
static const int kNumFactorRows = 17;
static constexpr FactorType kFactorTypes[kNumFactorRows] = {
    {2, 2, {LMGPU_CAM_BUNDLER, LMGPU_POINT3, -1}},        // LMGPU_F_SFM
    {3, 3, {LMGPU_POSE2, LMGPU_POSE2, -1}},               // LMGPU_F_BETWEEN_POSE2
    {6, 12, {LMGPU_POSE3, LMGPU_POSE3, -1}},              // LMGPU_F_BETWEEN_POSE3
    {3, 3, {LMGPU_POSE2, -1, -1}},                        // LMGPU_F_PRIOR_POSE2
    {6, 12, {LMGPU_POSE3, -1, -1}},                       // LMGPU_F_PRIOR_POSE3
    {3, 3, {LMGPU_POINT3, -1, -1}},                       // LMGPU_F_PRIOR_POINT3
    {9, 15, {LMGPU_CAM_BUNDLER, -1, -1}},                 // LMGPU_F_PRIOR_CAM
    {2, 7, {LMGPU_POSE3, LMGPU_POINT3, -1}},              // LMGPU_F_PROJECTION
    {2, 19, {LMGPU_POSE3, LMGPU_POINT3, -1}},             // LMGPU_F_PROJECTION_BPS
    {2, 2, {LMGPU_POSE2, LMGPU_POINT2, -1}},              // LMGPU_F_BEARING_RANGE_2D
    {2, 2, {LMGPU_POSE3, LMGPU_POINT3, LMGPU_CAL3_S2}},   // LMGPU_F_SFM2
    {5, 5, {LMGPU_CAL3_S2, -1, -1}},                      // LMGPU_F_PRIOR_CAL3_S2
    {9, 9, {LMGPU_VEC9, LMGPU_VEC9, -1}},                 // LMGPU_F_CHORDAL_BETWEEN
    {9, 9, {LMGPU_VEC9, -1, -1}},                         // LMGPU_F_PRIOR_VEC9
    {2, 7, {LMGPU_POSE3, LMGPU_POINT3, -1}},              // kSmartObsType
    {3, 3, {LMGPU_POINT3, LMGPU_POINT3, -1}},             // kTranslationType
    {3, 3, {LMGPU_POINT3, LMGPU_POINT3, -1}},             // kBetweenPoint3Type
};
static_assert(LMGPU_NUM_FACTOR_TYPES == kSmartObsType, "one row per public factor type, then the internal ones");

constexpr int var_type(int type, int k) { return kFactorTypes[type].var[k]; }
constexpr int factor_arity(int type) {
  int ar = 0;
  while (ar < kMaxArity && var_type(type, ar) >= 0) ar++;
  return ar;
}
// columns of the whitened [A1 A2 A3 b] of one factor
constexpr int factor_cols(int type) {
  int cols = 1;
  for (int k = 0; k < factor_arity(type); k++) cols += kVarDim[var_type(type, k)];
  return cols;
}
// noise doubles per factor: none (unit), inverse sigmas (diagonal), R row-major (Gaussian)
constexpr int factor_noise_doubles(int type, int noise_kind) {
  const int rows = kFactorTypes[type].rows;
  return noise_kind == LMGPU_N_DIAG ? rows : (noise_kind == LMGPU_N_GAUSS ? rows * rows : 0);
}

// the per-factor sizes of a bucket's arrays: ar variable indices, ml measurement doubles, nl noise doubles, rows x cols Jacobian
struct BucketShape {
  int ar, rows, cols, ml, nl;
};
constexpr BucketShape bucket_shape(int type, int noise_kind) {
  return {factor_arity(type), kFactorTypes[type].rows, factor_cols(type), kFactorTypes[type].meas, factor_noise_doubles(type, noise_kind)};
}

}  // namespace lmgpu
