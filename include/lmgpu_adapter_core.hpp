// lmgpu_adapter_core.hpp — the GTSAM-independent half of the reference-side binding of lmgpu.h.
//
// include/lmgpu_gtsam_adapter.h (the header a GTSAM maintainer adds) only EXTRACTS numbers from GTSAM objects (dynamic casts,
// accessors) and hands them to the classes below; everything that touches the C ABI — slot assignment in elimination order,
// bucketing by (factor type, noise kind, m-estimator), packing, call order, status -> exception mapping — lives here, has no
// GTSAM include and is therefore compiled and tested in this repository (tests/cpp/adapter_harness.cpp drives SFMExample_bal's
// graph through it; GTSAM itself cannot be built here).
//
// Call order (= what GpuLevenbergMarquardtOptimizer's constructor does, gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:40-62):
//   Problem p(device);
//   p.setVariables(keys in elimination order, types);        // after EnsureHasOrdering, LevenbergMarquardtParams.h:112-117
//   p.addFactor(...) for every factor of the NonlinearFactorGraph, in graph order;
//   p.finalize();                                             // buckets -> lmgpu_add_factor_bucket_robust, lmgpu_finalize_structure
//   p.setValues(packed);  p.lmInit(params);                   // State(initialValues, graph.error(initialValues), lambdaInitial, ...)
//   p.iterate(params) ...                                     // LevenbergMarquardtOptimizer::iterate
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "lmgpu.h"

namespace lmgpu_adapter {

// ---- shape tables of include/lmgpu.h (variable / factor / noise enums)
inline int varDim(int32_t t) { static const int d[LMGPU_NUM_VAR_TYPES] = {3, 6, 3, 9, 2, 5}; return d[t]; }
inline int varStore(int32_t t) { static const int s[LMGPU_NUM_VAR_TYPES] = {3, 12, 3, 15, 2, 5}; return s[t]; }
inline int factorArity(int32_t f) { static const int a[LMGPU_NUM_FACTOR_TYPES] = {2, 2, 2, 1, 1, 1, 1, 2, 2, 2, 3, 1}; return a[f]; }
inline int factorRows(int32_t f) { static const int r[LMGPU_NUM_FACTOR_TYPES] = {2, 3, 6, 3, 6, 3, 9, 2, 2, 2, 2, 5}; return r[f]; }
inline int factorMeas(int32_t f) { static const int m[LMGPU_NUM_FACTOR_TYPES] = {2, 3, 12, 3, 12, 3, 15, 7, 19, 2, 2, 5}; return m[f]; }
inline int32_t factorVarType(int32_t f, int i) {
  static const int32_t v[LMGPU_NUM_FACTOR_TYPES][3] = {{LMGPU_CAM_BUNDLER, LMGPU_POINT3, -1}, {LMGPU_POSE2, LMGPU_POSE2, -1}, {LMGPU_POSE3, LMGPU_POSE3, -1},
                                                       {LMGPU_POSE2, -1, -1}, {LMGPU_POSE3, -1, -1}, {LMGPU_POINT3, -1, -1}, {LMGPU_CAM_BUNDLER, -1, -1},
                                                       {LMGPU_POSE3, LMGPU_POINT3, -1}, {LMGPU_POSE3, LMGPU_POINT3, -1}, {LMGPU_POSE2, LMGPU_POINT2, -1},
                                                       {LMGPU_POSE3, LMGPU_POINT3, LMGPU_CAL3_S2}, {LMGPU_CAL3_S2, -1, -1}};
  return v[f][i];
}
inline int noiseDoubles(int32_t kind, int rows) { return kind == LMGPU_N_UNIT ? 0 : (kind == LMGPU_N_DIAG ? rows : rows * rows); }

/// status 1: what the reference throws as IndeterminantLinearSystemException(key) (gtsam/linear/linearExceptions.h;
/// raised at HessianFactor.cpp:475-482 with keys.front() of the failing clique)
struct Indeterminate : std::runtime_error {
  int slot;
  uint64_t key;
  Indeterminate(int s, uint64_t k) : std::runtime_error("lmgpu: indeterminate linear system"), slot(s), key(k) {}
};
struct Error : std::runtime_error {
  int status;
  Error(int st, const std::string& what) : std::runtime_error("lmgpu: " + what), status(st) {}
};

struct SolveResult {
  std::vector<double> delta;  // packed by slot (elimination order), lmgpu_total_dim() doubles
  double linearError0 = 0, linearError = 0;
};

class Problem {
 public:
  /// device < 0: structure-only handle (symbolic analysis; every compute call throws Error(LMGPU_HIP_ERROR))
  explicit Problem(int device = 0, int rank = 0, int worldSize = 1) {
    lmgpu_config cfg{device, rank, worldSize, 0};
    if (lmgpu_create(&cfg, &h_) != LMGPU_OK) {
      const std::string why = h_ ? lmgpu_last_error(h_) : "lmgpu_create failed";
      if (h_) lmgpu_destroy(h_);
      h_ = nullptr;
      throw Error(LMGPU_HIP_ERROR, why);
    }
  }
  ~Problem() { if (h_) lmgpu_destroy(h_); }
  Problem(const Problem&) = delete;
  Problem& operator=(const Problem&) = delete;

  lmgpu_handle* handle() const { return h_; }

  /// variables in ELIMINATION order (the Ordering of NonlinearOptimizerParams::ordering); position = slot
  void setVariables(const std::vector<uint64_t>& keys, const std::vector<int32_t>& types) {
    if (keys.size() != types.size()) throw Error(LMGPU_INVALID, "keys / types size mismatch");
    keys_ = keys;
    types_ = types;
    slot_.clear();
    slot_.reserve(keys.size() * 2);
    xoff_.assign(1, 0);
    voff_.assign(1, 0);
    for (size_t i = 0; i < keys.size(); i++) {
      if (types[i] < 0 || types[i] >= LMGPU_NUM_VAR_TYPES) throw Error(LMGPU_INVALID, "unknown variable type");
      if (!slot_.emplace(keys[i], (int32_t)i).second) throw Error(LMGPU_INVALID, "duplicate key in the ordering");
      xoff_.push_back(xoff_.back() + varDim(types[i]));
      voff_.push_back(voff_.back() + varStore(types[i]));
    }
    check(lmgpu_set_variables(h_, (int32_t)keys.size(), keys_.data(), types_.data()));
  }
  size_t numVariables() const { return keys_.size(); }
  uint64_t keyOfSlot(int s) const { return keys_.at((size_t)s); }
  int32_t typeOfSlot(int s) const { return types_.at((size_t)s); }
  int32_t slotOf(uint64_t key) const {
    auto it = slot_.find(key);
    if (it == slot_.end()) throw Error(LMGPU_INVALID, "a factor references a key that is not in the ordering");
    return it->second;
  }
  /// offsets of slot s in a packed tangent vector (delta, hessian diagonal) / in the packed values
  size_t deltaOffset(int s) const { return xoff_.at((size_t)s); }
  size_t valueOffset(int s) const { return voff_.at((size_t)s); }

  /// one factor of the NonlinearFactorGraph; graphIndex = its position there (VariableIndex order and error-sum order).
  /// meas: factorMeas(type) doubles as documented in lmgpu.h; noise: noiseDoubles(kind, rows) doubles (nullptr for UNIT).
  void addFactor(int32_t type, int32_t graphIndex, const uint64_t* keys, const double* meas, int32_t noiseKind, const double* noise,
                 int32_t robustKind = LMGPU_ROBUST_NONE, double robustK = 0.0) {
    if (type < 0 || type >= LMGPU_NUM_FACTOR_TYPES) throw Error(LMGPU_INVALID, "unknown factor type");
    Bucket& b = buckets_[std::make_tuple(type, noiseKind, robustKind, robustK)];
    b.gi.push_back(graphIndex);
    for (int i = 0; i < factorArity(type); i++) {
      const int32_t s = slotOf(keys[i]);
      if (types_[(size_t)s] != factorVarType(type, i)) throw Error(LMGPU_INVALID, "variable type does not fit the factor");
      b.slots.push_back(s);
    }
    b.meas.insert(b.meas.end(), meas, meas + factorMeas(type));
    const int nn = noiseDoubles(noiseKind, factorRows(type));
    if (nn) b.noise.insert(b.noise.end(), noise, noise + nn);
  }

  /// one SmartProjectionPoseFactor<Cal3_S2> (include/lmgpu.h, "smart projection factors"): its pose keys and measurements (2 doubles
  /// each), K5 = (fx, fy, s, u0, v0), 1 / sigma of its isotropic noise model.  Factors that share `params` travel in one call.
  void addSmartFactor(int32_t graphIndex, const std::vector<uint64_t>& keys, const std::vector<double>& z, const double* K5, double invSigma,
                      const lmgpu_smart_params& params) {
    if (z.size() != 2 * keys.size()) throw Error(LMGPU_INVALID, "smart factor: one measurement per key");
    SmartGroup* g = nullptr;
    for (SmartGroup& c : smart_)
      if (std::memcmp(&c.params, &params, sizeof params) == 0) g = &c;
    if (!g) {
      smart_.emplace_back();
      g = &smart_.back();
      std::memset(&g->params, 0, sizeof params);  // (padding bytes take part in the comparison above)
      g->params.linearizationMode = params.linearizationMode;
      g->params.degeneracyMode = params.degeneracyMode;
      g->params.retriangulationThreshold = params.retriangulationThreshold;
      g->params.triangulation.rankTolerance = params.triangulation.rankTolerance;
      g->params.triangulation.enableEPI = params.triangulation.enableEPI;
      g->params.triangulation.useLOST = params.triangulation.useLOST;
      g->params.triangulation.landmarkDistanceThreshold = params.triangulation.landmarkDistanceThreshold;
      g->params.triangulation.dynamicOutlierRejectionThreshold = params.triangulation.dynamicOutlierRejectionThreshold;
      g->params.triangulation.noise_inv_sigma = params.triangulation.noise_inv_sigma;
      g->offsets.push_back(0);
    }
    g->gi.push_back(graphIndex);
    for (uint64_t k : keys) {
      const int32_t s = slotOf(k);
      if (types_[(size_t)s] != LMGPU_POSE3) throw Error(LMGPU_INVALID, "smart factor: its variables must be Pose3");
      g->slots.push_back(s);
    }
    g->z.insert(g->z.end(), z.begin(), z.end());
    g->K5.insert(g->K5.end(), K5, K5 + 5);
    g->invSigma.push_back(invSigma);
    g->offsets.push_back((int32_t)g->slots.size());
  }
  /// graph indices of the smart factors in the order lmgpu_smart_get_points reports them (valid after finalize())
  const std::vector<int32_t>& smartGraphIndices() const { return smartOrder_; }
  int numSmartFactors() const { return lmgpu_num_smart_factors(h_); }
  /// SmartProjectionFactor::point() of every smart factor: 3 doubles each (NaN unless VALID) and the TriangulationResult status
  void smartPoints(std::vector<double>* points3, std::vector<int32_t>* status) const {
    const size_t n = (size_t)std::max(0, numSmartFactors());
    points3->assign(3 * n, 0.0);
    status->assign(n, 0);
    check(lmgpu_smart_get_points(h_, points3->data(), status->data()));
  }
  /// the augmented information matrix of one smart factor ((6 m + 1)^2, column-major) from the last linearization
  std::vector<double> smartHessian(int32_t graphIndex, int32_t* m) const {
    check(lmgpu_smart_get_hessian(h_, graphIndex, m, nullptr));
    std::vector<double> out((size_t)(6 * *m + 1) * (size_t)(6 * *m + 1));
    check(lmgpu_smart_get_hessian(h_, graphIndex, m, out.data()));
    return out;
  }
  void smartReset() { check(lmgpu_smart_reset(h_)); }
  lmgpu_smart_stats smartStats() const {
    lmgpu_smart_stats st{};
    check(lmgpu_get_smart_stats(h_, &st));
    return st;
  }

  void finalize() {
    smartOrder_.clear();
    for (const SmartGroup& g : smart_) {
      check(lmgpu_add_smart_factors(h_, (int32_t)g.gi.size(), g.gi.data(), g.offsets.data(), g.slots.data(), g.z.data(), g.K5.data(),
                                    g.invSigma.data(), &g.params));
      smartOrder_.insert(smartOrder_.end(), g.gi.begin(), g.gi.end());
    }
    smart_.clear();
    for (auto& kv : buckets_) {
      const Bucket& b = kv.second;
      check(lmgpu_add_factor_bucket_robust(h_, std::get<0>(kv.first), (int32_t)b.gi.size(), b.gi.data(), b.slots.data(), b.meas.data(),
                                           std::get<1>(kv.first), b.noise.empty() ? nullptr : b.noise.data(), std::get<2>(kv.first),
                                           std::get<3>(kv.first)));
    }
    buckets_.clear();
    check(lmgpu_finalize_structure(h_));
  }

  /// NonlinearOptimizerParams::linearSolverType (gtsam/nonlinear/NonlinearOptimizer.cpp:154-173): LMGPU_SOLVER_PCG with its
  /// PCGSolverParameters (before finalize(): the handle is built without fronts), or LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY (pcg unused)
  void set_linear_solver(int32_t solver, const lmgpu_pcg_params* pcg = nullptr) { check(lmgpu_set_linear_solver(h_, solver, pcg)); }

  int totalDim() const { return lmgpu_total_dim(h_); }
  int totalStore() const { return lmgpu_total_store(h_); }
  int numFronts() const { return lmgpu_num_fronts(h_); }

  // ---- values
  void setValues(const std::vector<double>& packed) {
    if ((int)packed.size() != totalStore()) throw Error(LMGPU_INVALID, "packed values have the wrong length");
    check(lmgpu_set_values(h_, packed.data()));
  }
  std::vector<double> getValues() const {
    std::vector<double> v((size_t)totalStore());
    check(lmgpu_get_values(h_, v.data()));
    return v;
  }

  // ---- the hot path, piecewise (LevenbergMarquardtOptimizer::linearize :113, NonlinearOptimizer::solve :129)
  double error() const {
    double e = 0;
    check(lmgpu_error(h_, &e));
    return e;
  }
  void linearize() const { check(lmgpu_linearize(h_)); }
  SolveResult solve(double lambda, bool diagonalDamping, double minDiagonal, double maxDiagonal) const {
    SolveResult r;
    r.delta.resize((size_t)totalDim());
    check(lmgpu_solve(h_, lambda, diagonalDamping ? 1 : 0, minDiagonal, maxDiagonal, r.delta.data(), &r.linearError0, &r.linearError));
    return r;
  }
  void retract(const std::vector<double>* delta = nullptr) const { check(lmgpu_retract(h_, delta ? delta->data() : nullptr)); }
  std::vector<double> hessianDiagonal() const {
    std::vector<double> d((size_t)totalDim());
    check(lmgpu_hessian_diagonal(h_, d.data()));
    return d;
  }
  /// whitened [A1 .. Ak b] of one factor, column-major rows x cols (JacobianFactor's VerticalBlockMatrix)
  std::vector<double> jacobian(int32_t graphIndex, int32_t* rows, int32_t* cols) const {
    check(lmgpu_get_jacobian(h_, graphIndex, nullptr, rows, cols));
    std::vector<double> out((size_t)*rows * (size_t)*cols);
    check(lmgpu_get_jacobian(h_, graphIndex, out.data(), rows, cols));
    return out;
  }

  /// the whole linearization (what iterate() returns in the reference): one copy per factor bucket instead of one per factor
  struct LinearGraph {
    std::vector<int32_t> graphIndex, rows, cols;  // ascending graph index
    std::vector<int64_t> offsets;                 // n + 1
    std::vector<double> data;                     // [A1 .. Ak b] column-major, back to back
  };
  LinearGraph jacobians() const {
    LinearGraph g;
    int32_t n = 0;
    check(lmgpu_get_jacobians(h_, &n, nullptr, nullptr, nullptr, nullptr, nullptr));
    g.graphIndex.resize((size_t)n);
    g.rows.resize((size_t)n);
    g.cols.resize((size_t)n);
    g.offsets.resize((size_t)n + 1);
    check(lmgpu_get_jacobians(h_, &n, g.graphIndex.data(), g.rows.data(), g.cols.data(), g.offsets.data(), nullptr));
    g.data.resize((size_t)g.offsets.back());
    check(lmgpu_get_jacobians(h_, &n, nullptr, nullptr, nullptr, nullptr, g.data.data()));
    return g;
  }

  // ---- the hot path, whole
  lmgpu_lm_state lmInit(const lmgpu_lm_params& p) {
    lmgpu_lm_state st{};
    check(lmgpu_lm_init(h_, &p, &st));
    return st;
  }
  void iterate(const lmgpu_lm_params& p, lmgpu_lm_state* inout) { check(lmgpu_iterate(h_, &p, inout)); }
  void optimize(const lmgpu_lm_params& p, lmgpu_lm_state* inout) { check(lmgpu_optimize(h_, &p, inout)); }
  void gnIterate(lmgpu_lm_state* inout) { check(lmgpu_gn_iterate(h_, inout)); }
  void dlIterate(lmgpu_lm_state* inout) { check(lmgpu_dl_iterate(h_, inout)); }
  /// NonlinearConjugateGradientOptimizer::iterate / optimize (gtsam/nonlinear/NonlinearConjugateGradientOptimizer.cpp:71-90)
  void ncgIterate(const lmgpu_ncg_params& p, lmgpu_lm_state* inout) { check(lmgpu_ncg_iterate(h_, &p, inout)); }
  void ncgOptimize(const lmgpu_ncg_params& p, lmgpu_lm_state* inout) { check(lmgpu_ncg_optimize(h_, &p, inout)); }

  /// Marginals for many variables from ONE factorization (lmgpu.h, "marginal covariances of MANY variables"): factor at the current
  /// values; the dim x dim row-major blocks of `slots`, back to back in their order (a stale factorization is rebuilt first)
  void marginalsFactor() { check(lmgpu_marginals_factor(h_)); }
  std::vector<double> marginalCovariances(const std::vector<int32_t>& slots) {
    size_t total = 0;
    for (int32_t s : slots) {
      const size_t d = (size_t)varDim(typeOfSlot(s));
      total += d * d;
    }
    std::vector<double> out(total);
    check(lmgpu_marginal_covariances(h_, (int32_t)slots.size(), slots.data(), out.data()));
    return out;
  }
  /// the same factorization, off-diagonal blocks too (lmgpu.h, "cross-covariances and joint marginals"): block q = Sigma[slots_i[q],
  /// slots_j[q]], dim_i x dim_j row-major, back to back; slots_j[q] is the source whose path is walked
  std::vector<double> marginalCrossCovariances(const std::vector<int32_t>& slots_i, const std::vector<int32_t>& slots_j) {
    if (slots_i.size() != slots_j.size()) throw Error(LMGPU_INVALID, "marginalCrossCovariances: slots_i and slots_j differ in length");
    size_t total = 0;
    for (size_t q = 0; q < slots_i.size(); q++) total += (size_t)varDim(typeOfSlot(slots_i[q])) * (size_t)varDim(typeOfSlot(slots_j[q]));
    std::vector<double> out(total);
    check(lmgpu_marginal_cross_covariances(h_, (int32_t)slots_i.size(), slots_i.data(), slots_j.data(), out.data()));
    return out;
  }
  /// the joint marginal covariance of `slots` (distinct): D x D row-major, blocks in their order, exactly symmetric
  std::vector<double> jointMarginalCovariance(const std::vector<int32_t>& slots) {
    size_t D = 0;
    for (int32_t s : slots) D += (size_t)varDim(typeOfSlot(s));
    std::vector<double> out(D * D);
    const int32_t begin[2] = {0, (int32_t)slots.size()};
    check(lmgpu_joint_marginal_covariances(h_, 1, begin, slots.data(), out.data()));
    return out;
  }
  lmgpu_marginals_stats marginalsStats() {
    lmgpu_marginals_stats st{};
    check(lmgpu_get_marginals_stats(h_, &st));
    return st;
  }

  /// status -> exception, the mapping the reference-side adapter relies on
  void check(int rc) const {
    if (rc == LMGPU_OK) return;
    if (rc == LMGPU_INDETERMINATE) {
      const int s = lmgpu_last_failed_slot(h_);
      throw Indeterminate(s, (s >= 0 && (size_t)s < keys_.size()) ? keys_[(size_t)s] : 0);
    }
    const char* m = lmgpu_last_error(h_);
    throw Error(rc, m ? m : "");
  }

 private:
  struct Bucket {
    std::vector<int32_t> gi, slots;
    std::vector<double> meas, noise;
  };
  lmgpu_handle* h_ = nullptr;
  std::vector<uint64_t> keys_;
  std::vector<int32_t> types_;
  std::unordered_map<uint64_t, int32_t> slot_;
  std::vector<size_t> xoff_, voff_;
  std::map<std::tuple<int32_t, int32_t, int32_t, double>, Bucket> buckets_;
  struct SmartGroup {
    lmgpu_smart_params params;
    std::vector<int32_t> gi, offsets, slots;
    std::vector<double> z, K5, invSigma;
  };
  std::vector<SmartGroup> smart_;
  std::vector<int32_t> smartOrder_;
};

/// NonlinearOptimizer::defaultOptimize (gtsam/nonlinear/NonlinearOptimizer.cpp:62-117) around an iterate() callable: what the
/// reference's optimize() does with the adapter's iterate() override.  iterate(state) advances state by one outer iteration.
template <class Iterate>
inline void defaultOptimize(const lmgpu_lm_params& p, lmgpu_lm_state* st, Iterate iterate) {
  double currentError = st->error;
  if (st->iterations >= p.maxIterations) return;
  if (currentError <= p.errorTol) return;
  double newError = currentError;
  do {
    currentError = newError;
    iterate(st);
    newError = st->error;
    if (newError <= p.errorTol) break;
    const double absoluteDecrease = currentError - newError, relativeDecrease = absoluteDecrease / currentError;
    if ((p.relativeErrorTol && relativeDecrease <= p.relativeErrorTol) || absoluteDecrease <= p.absoluteErrorTol) break;
  } while (st->iterations < p.maxIterations && std::isfinite(currentError));
}

/// The arrays of lmgpu_triangulate_batch (include/lmgpu.h, "triangulation"), GTSAM-free: cameras once, then per landmark its observations
/// as (camera index, pixel).  A Cal3Bundler camera is packed without its principal point, which is subtracted from every pixel measured
/// in it (the CAM_BUNDLER convention of lmgpu.h).
struct TriangulationBatch {
  int32_t camera_model;  // 0 PinholeCamera<Cal3Bundler>, 1 PinholeCamera<Cal3_S2>
  std::vector<double> cams, obs_z, principal;
  std::vector<int32_t> offsets{0}, obs_cam;
  explicit TriangulationBatch(int32_t model) : camera_model(model) {}
  int32_t numCameras() const { return static_cast<int32_t>(principal.size() / 2); }
  int32_t numLandmarks() const { return static_cast<int32_t>(offsets.size()) - 1; }
  /// pose12: R row-major 9, t 3.  Returns the camera's index.
  int32_t addBundlerCamera(const double* pose12, double f, double k1, double k2, double u0, double v0) {
    cams.insert(cams.end(), pose12, pose12 + 12);
    cams.insert(cams.end(), {f, k1, k2});
    principal.insert(principal.end(), {u0, v0});
    return numCameras() - 1;
  }
  int32_t addS2Camera(const double* pose12, double fx, double fy, double s, double u0, double v0) {
    cams.insert(cams.end(), pose12, pose12 + 12);
    cams.insert(cams.end(), {fx, fy, s, u0, v0});
    principal.insert(principal.end(), {0.0, 0.0});
    return numCameras() - 1;
  }
  void addObservation(int32_t cam, double u, double v) {
    obs_cam.push_back(cam);
    obs_z.push_back(u - principal.at(2 * static_cast<size_t>(cam)));
    obs_z.push_back(v - principal.at(2 * static_cast<size_t>(cam) + 1));
  }
  void endLandmark() { offsets.push_back(static_cast<int32_t>(obs_cam.size())); }
  /// points: 3 per landmark (NaN unless VALID); status: lmgpu_triangulation_status per landmark
  void run(int device, const lmgpu_triangulation_params& params, std::vector<double>* points, std::vector<int32_t>* status) const {
    points->assign(3 * static_cast<size_t>(numLandmarks()), 0.0);
    status->assign(static_cast<size_t>(numLandmarks()), 0);
    const int rc = lmgpu_triangulate_batch(device, camera_model, numCameras(), cams.data(), numLandmarks(), offsets.data(), obs_cam.data(),
                                           obs_z.data(), &params, points->data(), status->data());
    if (rc != LMGPU_OK) throw Error(rc, "lmgpu_triangulate_batch: status " + std::to_string(rc));
  }
};

}  // namespace lmgpu_adapter
