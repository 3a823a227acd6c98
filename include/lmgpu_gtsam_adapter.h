// lmgpu_gtsam_adapter.h — reference-side binding of the C ABI in lmgpu.h.
//
// Header-only adapter a GTSAM maintainer adds next to gtsam/nonlinear/LevenbergMarquardtOptimizer.h: subclasses that override
// the reference's own extension points and forward the hot path to liblmgpu.so:
//   iterate()    virtual, gtsam/nonlinear/NonlinearOptimizer.h:136, LM override LevenbergMarquardtOptimizer.h:103
//   linearize()  virtual, gtsam/nonlinear/LevenbergMarquardtOptimizer.h:113 ("can be overwritten")
//   solve()      virtual, gtsam/nonlinear/NonlinearOptimizer.h:129-130 (precedent: IterativeLM, tests/testNonlinearOptimizer.cpp:507-528)
//
// This file only EXTRACTS numbers from GTSAM objects; slot assignment, bucketing, packing, the call order of the C ABI and
// the status -> exception mapping are in lmgpu_adapter_core.hpp, which has no GTSAM include and is compiled and tested in the
// repository (tests/cpp/adapter_harness.cpp).  This file is type-checked against the reference's headers by
// tests/test_adapter_header_compiles.py (g++ -fsyntax-only; the two CMake-generated headers GTSAM's sources include are written into
// the test's temporary directory); it cannot be LINKED there (libgtsam is not buildable in the repository's container).
//
// Two modes (constructor argument):
//   WholeIterate (default)  iterate() = lmgpu_iterate: the whole tryLambda loop on device-resident data; values come back
//                           to the host once per outer iteration.
//   Piecewise               iterate() is the reference's own (LevenbergMarquardtOptimizer.cpp:273-308); only its two virtual
//                           calls are replaced: linearize() -> lmgpu_linearize (+ download of the whitened Jacobians as
//                           JacobianFactors, which tryLambda needs for linear.error), solve() -> lmgpu_solve at state lambda.
#pragma once

#include <gtsam/base/GenericValue.h>
#include <gtsam/geometry/BearingRange.h>
#include <gtsam/geometry/Cal3Bundler.h>
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/CameraSet.h>
#include <gtsam/geometry/PinholeCamera.h>
#include <gtsam/geometry/Point2.h>
#include <gtsam/geometry/Point3.h>
#include <gtsam/geometry/Pose2.h>
#include <gtsam/geometry/Pose3.h>
#include <gtsam/geometry/Rot2.h>
#include <gtsam/geometry/Rot3.h>
#include <gtsam/geometry/triangulation.h>
#include <gtsam/inference/Ordering.h>
#include <gtsam/linear/GaussianFactorGraph.h>
#include <gtsam/linear/JacobianFactor.h>
#include <gtsam/linear/NoiseModel.h>
#include <gtsam/linear/PCGSolver.h>
#include <gtsam/linear/Preconditioner.h>
#include <gtsam/linear/VectorValues.h>
#include <gtsam/linear/linearExceptions.h>
#include <gtsam/nonlinear/DoglegOptimizer.h>
#include <gtsam/nonlinear/GaussNewtonOptimizer.h>
#include <gtsam/nonlinear/ISAM2.h>
#include <gtsam/3rdparty/CCOLAMD/Include/ccolamd.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/Values.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>
#include <gtsam/nonlinear/internal/NonlinearOptimizerState.h>
#include <gtsam/sam/BearingRangeFactor.h>
#include <gtsam/sfm/BinaryMeasurement.h>
#include <gtsam/geometry/Unit3.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/GeneralSFMFactor.h>
#include <gtsam/slam/ProjectionFactor.h>
#include <gtsam/slam/SmartProjectionPoseFactor.h>

#include <algorithm>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "lmgpu_adapter_core.hpp"

namespace gtsam {

namespace lmgpu_detail {

typedef PinholeCamera<Cal3Bundler> Camera;
typedef GeneralSFMFactor<Camera, Point3> SfmFactor;
typedef GenericProjectionFactor<Pose3, Point3, Cal3_S2> ProjFactor;

inline void packPose3(const Pose3& p, double* v) {  // R row-major 9, t 3 (lmgpu.h, POSE3)
  const Matrix3 R = p.rotation().matrix();
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) v[3 * i + j] = R(i, j);
  v[9] = p.x();
  v[10] = p.y();
  v[11] = p.z();
}
inline Pose3 unpackPose3(const double* q) {
  Matrix3 R;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R(i, j) = q[3 * i + j];
  return Pose3(Rot3(R), Point3(q[9], q[10], q[11]));
}

inline int32_t variableType(const Value& v) {  // gtsam/base/GenericValue.h
  if (dynamic_cast<const GenericValue<Pose2>*>(&v)) return LMGPU_POSE2;
  if (dynamic_cast<const GenericValue<Pose3>*>(&v)) return LMGPU_POSE3;
  if (dynamic_cast<const GenericValue<Point3>*>(&v)) return LMGPU_POINT3;
  if (dynamic_cast<const GenericValue<Camera>*>(&v)) return LMGPU_CAM_BUNDLER;
  if (dynamic_cast<const GenericValue<Point2>*>(&v)) return LMGPU_POINT2;
  if (dynamic_cast<const GenericValue<Cal3_S2>*>(&v)) return LMGPU_CAL3_S2;  // self-calibration: the calibration is a variable
  throw std::invalid_argument("lmgpu adapter: unsupported variable type");
}

/// noise model -> (kind, data, m-estimator, constant); gtsam/linear/NoiseModel.h (Unit :617-660, Diagonal::invsigmas :361,
/// Gaussian::R :263, Robust::robust / noise :705-708), gtsam/linear/LossFunctions.h (modelParameter, reweightScheme :82)
struct Noise {
  int32_t kind = LMGPU_N_UNIT, robust = LMGPU_ROBUST_NONE;
  double robustK = 0.0;
  std::vector<double> data;
};
inline Noise extractNoise(SharedNoiseModel model) {
  Noise out;
  if (auto rob = std::dynamic_pointer_cast<noiseModel::Robust>(model)) {
    const auto est = rob->robust();
    if (est->reweightScheme() != noiseModel::mEstimator::Base::Block)
      throw std::invalid_argument("lmgpu adapter: only the Block reweighting scheme is bound");
    using namespace noiseModel::mEstimator;
    if (auto e1 = std::dynamic_pointer_cast<Huber>(est)) { out.robust = LMGPU_ROBUST_HUBER; out.robustK = e1->modelParameter(); }
    else if (auto e2 = std::dynamic_pointer_cast<Cauchy>(est)) { out.robust = LMGPU_ROBUST_CAUCHY; out.robustK = e2->modelParameter(); }
    else if (auto e3 = std::dynamic_pointer_cast<Tukey>(est)) { out.robust = LMGPU_ROBUST_TUKEY; out.robustK = e3->modelParameter(); }
    else if (auto e4 = std::dynamic_pointer_cast<GemanMcClure>(est)) { out.robust = LMGPU_ROBUST_GEMAN_MCCLURE; out.robustK = e4->modelParameter(); }
    else if (auto e5 = std::dynamic_pointer_cast<Welsch>(est)) { out.robust = LMGPU_ROBUST_WELSCH; out.robustK = e5->modelParameter(); }
    else if (auto e6 = std::dynamic_pointer_cast<Fair>(est)) { out.robust = LMGPU_ROBUST_FAIR; out.robustK = e6->modelParameter(); }
    else if (auto e7 = std::dynamic_pointer_cast<DCS>(est)) { out.robust = LMGPU_ROBUST_DCS; out.robustK = e7->modelParameter(); }
    else if (auto e8 = std::dynamic_pointer_cast<L2WithDeadZone>(est)) { out.robust = LMGPU_ROBUST_L2_WITH_DEAD_ZONE; out.robustK = e8->modelParameter(); }
    else throw std::invalid_argument("lmgpu adapter: m-estimator not bound");
    model = rob->noise();
  }
  if (!model || model->isUnit()) return out;
  if (model->isConstrained()) throw std::invalid_argument("lmgpu adapter: constrained noise models take the QR path (not bound)");
  if (auto d = std::dynamic_pointer_cast<noiseModel::Diagonal>(model)) {  // Isotropic is a Diagonal
    out.kind = LMGPU_N_DIAG;
    const Vector& s = d->invsigmas();
    out.data.assign(s.data(), s.data() + s.size());
  } else if (auto g = std::dynamic_pointer_cast<noiseModel::Gaussian>(model)) {
    out.kind = LMGPU_N_GAUSS;
    const Matrix R = g->R();
    for (int r = 0; r < R.rows(); r++)
      for (int c = 0; c < R.cols(); c++) out.data.push_back(R(r, c));
  } else {
    throw std::invalid_argument("lmgpu adapter: unsupported noise model");
  }
  return out;
}

/// one nonlinear factor -> (factor type, measurement doubles) in the packing lmgpu.h documents; false if the type is not bound
inline bool extractFactor(const NonlinearFactor::shared_ptr& f, const Values& initial, int32_t* type, std::vector<double>* m) {
  if (auto s = std::dynamic_pointer_cast<SfmFactor>(f)) {  // gtsam/slam/GeneralSFMFactor.h:70-206
    *type = LMGPU_F_SFM;
    const Cal3Bundler& K = initial.at<Camera>(s->key1()).calibration();
    *m = {s->measured().x() - K.px(), s->measured().y() - K.py()};  // fold the constant principal point (lmgpu.h, CAM_BUNDLER)
  } else if (auto b3 = std::dynamic_pointer_cast<BetweenFactor<Pose3>>(f)) {  // gtsam/slam/BetweenFactor.h
    *type = LMGPU_F_BETWEEN_POSE3;
    m->resize(12);
    packPose3(b3->measured(), m->data());
  } else if (auto b2 = std::dynamic_pointer_cast<BetweenFactor<Pose2>>(f)) {
    *type = LMGPU_F_BETWEEN_POSE2;
    *m = {b2->measured().x(), b2->measured().y(), b2->measured().theta()};
  } else if (auto p2 = std::dynamic_pointer_cast<PriorFactor<Pose2>>(f)) {  // gtsam/nonlinear/PriorFactor.h:104 prior()
    *type = LMGPU_F_PRIOR_POSE2;
    *m = {p2->prior().x(), p2->prior().y(), p2->prior().theta()};
  } else if (auto p3 = std::dynamic_pointer_cast<PriorFactor<Pose3>>(f)) {
    *type = LMGPU_F_PRIOR_POSE3;
    m->resize(12);
    packPose3(p3->prior(), m->data());
  } else if (auto pp = std::dynamic_pointer_cast<PriorFactor<Point3>>(f)) {
    *type = LMGPU_F_PRIOR_POINT3;
    *m = {pp->prior().x(), pp->prior().y(), pp->prior().z()};
  } else if (auto pc = std::dynamic_pointer_cast<PriorFactor<Camera>>(f)) {  // graph.addPrior(C(0), camera, ...) SFMExample_bal.cpp:67
    *type = LMGPU_F_PRIOR_CAM;
    m->resize(15);
    packPose3(pc->prior().pose(), m->data());
    (*m)[12] = pc->prior().calibration().fx();
    (*m)[13] = pc->prior().calibration().k1();
    (*m)[14] = pc->prior().calibration().k2();
  } else if (auto pr = std::dynamic_pointer_cast<ProjFactor>(f)) {  // gtsam/slam/ProjectionFactor.h:169-187
    if (pr->throwCheirality()) {
      // the reference lets CheiralityException escape from linearize in this configuration; the device path zeroes the factor
      // like the default build of GeneralSFMFactor does.  Bind only the non-throwing form.
      throw std::invalid_argument("lmgpu adapter: GenericProjectionFactor with throwCheirality is not bound");
    }
    const Cal3_S2& K = *pr->calibration();
    *m = {pr->measured().x(), pr->measured().y(), K.fx(), K.fy(), K.skew(), K.px(), K.py()};
    if (pr->body_P_sensor()) {
      *type = LMGPU_F_PROJECTION_BPS;
      m->resize(19);
      packPose3(*pr->body_P_sensor(), m->data() + 7);
    } else {
      *type = LMGPU_F_PROJECTION;
    }
  } else if (auto s2 = std::dynamic_pointer_cast<GeneralSFMFactor2<Cal3_S2>>(f)) {  // gtsam/slam/GeneralSFMFactor.h:208-262 (keys: pose, point, K)
    *type = LMGPU_F_SFM2;
    *m = {s2->measured().x(), s2->measured().y()};
  } else if (auto pk = std::dynamic_pointer_cast<PriorFactor<Cal3_S2>>(f)) {  // graph.addPrior(Symbol('K', 0), K, calNoise) SelfCalibrationExample.cpp:83
    *type = LMGPU_F_PRIOR_CAL3_S2;
    const Cal3_S2& K = pk->prior();
    *m = {K.fx(), K.fy(), K.skew(), K.px(), K.py()};
  } else if (auto br = std::dynamic_pointer_cast<BearingRangeFactor<Pose2, Point2>>(f)) {  // gtsam/sam/BearingRangeFactor.h:33-77
    *type = LMGPU_F_BEARING_RANGE_2D;
    *m = {br->measured().bearing().theta(), br->measured().range()};  // ExpressionFactor::measured :82, BearingRange.h:73-76
  } else {
    return false;
  }
  return true;
}

typedef SmartProjectionPoseFactor<Cal3_S2> SmartPoseFactor;

/// The parameters, noise model, sensor pose and cached result of a smart factor are protected members without accessors
/// (gtsam/slam/SmartProjectionFactor.h:57-66, SmartFactorBase.h:73-83): read through pointers to members formed in a derived class.
struct SmartAccess : SmartPoseFactor {
  static const SmartProjectionParams& params(const SmartPoseFactor& f) { return f.*(&SmartAccess::params_); }
  static double sigma(const SmartPoseFactor& f) { return (f.*(&SmartAccess::noiseModel_))->sigma(); }
  static bool hasSensorPose(const SmartPoseFactor& f) {
    const auto& b = f.*(&SmartAccess::body_P_sensor_);
    return b && !b->equals(Pose3(), 0.0);
  }
  /// result_ is mutable (SmartProjectionFactor.h:62): point() / isValid() ... of the caller's factor answer with the device's result
  static void setResult(const SmartPoseFactor& f, const TriangulationResult& r) {
    const_cast<TriangulationResult&>(f.*(&SmartAccess::result_)) = r;  // (a pointer to member does not carry `mutable`)
  }
};

inline lmgpu_triangulation_params smartTriangulationToC(const TriangulationParameters& p) {  // triangulation.h:562-609
  if (p.useLOST) throw lmgpu_adapter::Error(LMGPU_INVALID, "smart factor: useLOST is not bound");
  double inv = 0.0;
  if (p.noiseModel && !std::dynamic_pointer_cast<noiseModel::Unit>(p.noiseModel)) {
    const auto iso = std::dynamic_pointer_cast<noiseModel::Isotropic>(p.noiseModel);
    if (!iso || iso->dim() != 2) throw lmgpu_adapter::Error(LMGPU_INVALID, "smart factor: the triangulation noise model must be Unit or Isotropic(2)");
    inv = 1.0 / iso->sigma();
  }
  return lmgpu_triangulation_params{p.rankTolerance, p.enableEPI ? 1 : 0, 0, p.landmarkDistanceThreshold, p.dynamicOutlierRejectionThreshold, inv};
}

/// SmartProjectionParams (gtsam/slam/SmartFactorParams.h:42-133) -> lmgpu_smart_params; what the device does not implement throws
inline lmgpu_smart_params toC(const SmartProjectionParams& p) {
  if (p.linearizationMode != HESSIAN) throw lmgpu_adapter::Error(LMGPU_INVALID, "smart factor: only linearizationMode HESSIAN is bound");
  if (p.degeneracyMode != ZERO_ON_DEGENERACY) throw lmgpu_adapter::Error(LMGPU_INVALID, "smart factor: only degeneracyMode ZERO_ON_DEGENERACY is bound");
  if (p.throwCheirality || p.verboseCheirality) throw lmgpu_adapter::Error(LMGPU_INVALID, "smart factor: throwCheirality / verboseCheirality are not bound");
  return lmgpu_smart_params{LMGPU_SMART_HESSIAN, LMGPU_SMART_ZERO_ON_DEGENERACY, p.retriangulationThreshold, smartTriangulationToC(p.triangulation)};
}

inline TriangulationResult smartResult(int32_t status, const double* p) {  // triangulation.h:631-660
  switch (status) {
    case LMGPU_TRI_VALID: return TriangulationResult(Point3(p[0], p[1], p[2]));
    case LMGPU_TRI_BEHIND_CAMERA: return TriangulationResult::BehindCamera();
    case LMGPU_TRI_OUTLIER: return TriangulationResult::Outlier();
    case LMGPU_TRI_FAR_POINT: return TriangulationResult::FarPoint();
    default: return TriangulationResult::Degenerate();
  }
}

/// shared by the three optimizers: the device-resident problem + Values / VectorValues marshalling
class Device {
 public:
  /// pcg != nullptr: the linear solver is PCG, selected before finalize (no fronts are built)
  Device(const NonlinearFactorGraph& graph, const Values& initial, const Ordering& ordering, int device,
         const lmgpu_pcg_params* pcg = nullptr)
      : p_(device) {
    std::vector<uint64_t> keys(ordering.begin(), ordering.end());
    std::vector<int32_t> types;
    types.reserve(keys.size());
    for (Key k : ordering) types.push_back(variableType(initial.at(k)));
    p_.setVariables(keys, types);
    for (size_t i = 0; i < graph.size(); i++) {
      if (!graph[i]) continue;  // NonlinearFactorGraph::linearize keeps null factors null (NonlinearFactorGraph.cpp:214-233)
      if (auto sp = std::dynamic_pointer_cast<SmartPoseFactor>(graph[i])) {  // gtsam/slam/SmartProjectionPoseFactor.h:43-152
        if (SmartAccess::hasSensorPose(*sp)) throw lmgpu_adapter::Error(LMGPU_INVALID, "smart factor: body_P_sensor is not bound");
        const Cal3_S2& K = *sp->calibration();
        const double K5[5] = {K.fx(), K.fy(), K.skew(), K.px(), K.py()};
        std::vector<uint64_t> fk(sp->keys().begin(), sp->keys().end());
        std::vector<double> z;
        for (const Point2& m : sp->measured()) { z.push_back(m.x()); z.push_back(m.y()); }
        p_.addSmartFactor((int32_t)i, fk, z, K5, 1.0 / SmartAccess::sigma(*sp), toC(SmartAccess::params(*sp)));
        continue;
      }
      auto nm = std::dynamic_pointer_cast<NoiseModelFactor>(graph[i]);
      if (!nm) throw std::invalid_argument("lmgpu adapter: only NoiseModelFactors are bound");
      int32_t type;
      std::vector<double> meas;
      if (!extractFactor(graph[i], initial, &type, &meas)) throw std::invalid_argument("lmgpu adapter: factor type not bound");
      const Noise nz = extractNoise(nm->noiseModel());
      std::vector<uint64_t> fk(nm->keys().begin(), nm->keys().end());
      p_.addFactor(type, (int32_t)i, fk.data(), meas.data(), nz.kind, nz.data.empty() ? nullptr : nz.data.data(), nz.robust, nz.robustK);
    }
    if (pcg) p_.set_linear_solver(LMGPU_SOLVER_PCG, pcg);
    p_.finalize();
    upload(initial);
  }

  lmgpu_adapter::Problem& problem() { return p_; }
  const lmgpu_adapter::Problem& problem() const { return p_; }

  void upload(const Values& v) const {
    std::vector<double> packed((size_t)p_.totalStore());
    for (size_t s = 0; s < p_.numVariables(); s++) {
      const Key k = p_.keyOfSlot((int)s);
      double* o = &packed[p_.valueOffset((int)s)];
      switch (p_.typeOfSlot((int)s)) {
        case LMGPU_POSE2: { const Pose2& q = v.at<Pose2>(k); o[0] = q.x(); o[1] = q.y(); o[2] = q.theta(); break; }
        case LMGPU_POSE3: packPose3(v.at<Pose3>(k), o); break;
        case LMGPU_POINT3: { const Point3& q = v.at<Point3>(k); o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); break; }
        case LMGPU_POINT2: { const Point2& q = v.at<Point2>(k); o[0] = q.x(); o[1] = q.y(); break; }
        case LMGPU_CAL3_S2: { const Cal3_S2& q = v.at<Cal3_S2>(k); o[0] = q.fx(); o[1] = q.fy(); o[2] = q.skew(); o[3] = q.px(); o[4] = q.py(); break; }
        default: {
          const Camera& c = v.at<Camera>(k);
          packPose3(c.pose(), o);
          o[12] = c.calibration().fx(); o[13] = c.calibration().k1(); o[14] = c.calibration().k2();
        }
      }
    }
    const_cast<lmgpu_adapter::Problem&>(p_).setValues(packed);
  }

  /// `like` supplies what does not travel: the constant principal point of every Cal3Bundler
  Values download(const Values& like) const {
    const std::vector<double> packed = p_.getValues();
    Values out;
    for (size_t s = 0; s < p_.numVariables(); s++) {
      const Key k = p_.keyOfSlot((int)s);
      const double* q = &packed[p_.valueOffset((int)s)];
      switch (p_.typeOfSlot((int)s)) {
        case LMGPU_POSE2: out.insert(k, Pose2(q[0], q[1], q[2])); break;
        case LMGPU_POSE3: out.insert(k, unpackPose3(q)); break;
        case LMGPU_POINT3: out.insert(k, Point3(q[0], q[1], q[2])); break;
        case LMGPU_POINT2: out.insert(k, Point2(q[0], q[1])); break;
        case LMGPU_CAL3_S2: out.insert(k, Cal3_S2(q[0], q[1], q[2], q[3], q[4])); break;
        default: {
          const Cal3Bundler& K0 = like.at<Camera>(k).calibration();
          out.insert(k, Camera(unpackPose3(q), Cal3Bundler(q[12], q[13], q[14], K0.px(), K0.py())));
        }
      }
    }
    return out;
  }

  VectorValues toVectorValues(const std::vector<double>& packed) const {
    VectorValues out;
    for (size_t s = 0; s < p_.numVariables(); s++) {
      const int d = lmgpu_adapter::varDim(p_.typeOfSlot((int)s));
      out.insert(p_.keyOfSlot((int)s), Vector(Eigen::Map<const Vector>(packed.data() + p_.deltaOffset((int)s), d)));
    }
    return out;
  }

  /// lmgpu_solve with the reference's exception: IndeterminantLinearSystemException(first frontal key of the failing clique)
  VectorValues solve(double lambda, const LevenbergMarquardtParams* lm) const {
    try {
      const lmgpu_adapter::SolveResult r = lm ? p_.solve(lambda, lm->diagonalDamping, lm->minDiagonal, lm->maxDiagonal) : p_.solve(lambda, false, 0.0, 0.0);
      return toVectorValues(r.delta);
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
  }

  /// SmartProjectionFactor::point() of every smart factor of `graph` as the device left it, by graph index (a TriangulationResult for
  /// every slot of the graph, Degenerate where the slot holds no smart factor; empty for a graph without smart factors); with writeBack the factors' own result_ is set too
  std::vector<TriangulationResult> smartPoints(const NonlinearFactorGraph& graph, bool writeBack) const {
    if (p_.numSmartFactors() <= 0) return {};  // (a graph without smart factors pays nothing for this in its iterate())
    std::vector<TriangulationResult> out(graph.size(), TriangulationResult::Degenerate());
    std::vector<double> pts;
    std::vector<int32_t> st;
    p_.smartPoints(&pts, &st);
    const std::vector<int32_t>& gi = p_.smartGraphIndices();
    for (size_t k = 0; k < gi.size(); k++) {
      out[(size_t)gi[k]] = smartResult(st[k], &pts[3 * k]);
      if (writeBack)
        if (auto sp = std::dynamic_pointer_cast<SmartPoseFactor>(graph[(size_t)gi[k]])) SmartAccess::setResult(*sp, out[(size_t)gi[k]]);
    }
    return out;
  }

  /// the device-resident linearization as the GaussianFactorGraph NonlinearFactorGraph::linearize returns: one JacobianFactor
  /// per factor, already whitened (unit noise model), index-preserving
  GaussianFactorGraph::shared_ptr downloadLinearGraph(const NonlinearFactorGraph& graph) const {
    // (a handle with smart factors keeps Jacobians of its internal factors, not the Hessian factors the reference would return: no graph)
    if (p_.numSmartFactors() > 0) return GaussianFactorGraph::shared_ptr();
    const lmgpu_adapter::Problem::LinearGraph lg = p_.jacobians();  // one device copy per factor bucket
    auto out = std::make_shared<GaussianFactorGraph>();
    out->reserve(graph.size());
    size_t next = 0;
    for (size_t i = 0; i < graph.size(); i++) {
      if (!graph[i]) { out->push_back(GaussianFactor::shared_ptr()); continue; }
      if (next >= lg.graphIndex.size() || (size_t)lg.graphIndex[next] != i) throw std::logic_error("lmgpu adapter: linear graph does not match the nonlinear graph");
      const int rows = lg.rows[next], cols = lg.cols[next];
      Eigen::Map<const Matrix> M(lg.data.data() + lg.offsets[next], rows, cols);  // column-major
      next++;
      std::vector<std::pair<Key, Matrix>> terms;
      int c0 = 0;
      for (Key k : graph[i]->keys()) {
        const int d = lmgpu_adapter::varDim(p_.typeOfSlot(p_.slotOf(k)));
        terms.emplace_back(k, M.middleCols(c0, d));
        c0 += d;
      }
      out->push_back(std::make_shared<JacobianFactor>(terms, Vector(M.col(cols - 1))));
    }
    return out;
  }

 private:
  lmgpu_adapter::Problem p_;
};

inline lmgpu_lm_params toC(const LevenbergMarquardtParams& p) {  // gtsam/nonlinear/LevenbergMarquardtParams.h:35-157
  return lmgpu_lm_params{(int32_t)p.maxIterations, p.relativeErrorTol, p.absoluteErrorTol, p.errorTol, p.lambdaInitial, p.lambdaFactor,
                         p.lambdaUpperBound, p.lambdaLowerBound, p.minModelFidelity, p.diagonalDamping ? 1 : 0, p.useFixedLambdaFactor ? 1 : 0,
                         p.minDiagonal, p.maxDiagonal};
}

/// NonlinearOptimizer::solve's dispatch (gtsam/nonlinear/NonlinearOptimizer.cpp:154-173) as far as it is bound: isIterative() with
/// PCGSolverParameters and a Dummy or BlockJacobi preconditioner -> lmgpu_pcg_params (returns true); every other iterative parameter type
/// (SubgraphSolverParameters, another preconditioner, none) throws std::invalid_argument -- no silent fallback to Cholesky.
inline bool toPcg(const NonlinearOptimizerParams& p, lmgpu_pcg_params* out) {
  if (!p.isIterative()) return false;
  auto pcg = std::dynamic_pointer_cast<PCGSolverParameters>(p.iterativeParams);
  if (!pcg) throw std::invalid_argument("lmgpu adapter: the iterative linear solver is bound for PCGSolverParameters only");
  int32_t pre;
  if (std::dynamic_pointer_cast<DummyPreconditionerParameters>(pcg->preconditioner))
    pre = LMGPU_PRECOND_DUMMY;
  else if (std::dynamic_pointer_cast<BlockJacobiPreconditionerParameters>(pcg->preconditioner))
    pre = LMGPU_PRECOND_BLOCK_JACOBI;
  else
    throw std::invalid_argument("lmgpu adapter: PCG is bound with the Dummy or BlockJacobi preconditioner only");
  const size_t lim = (size_t)1 << 28;
  if (pcg->minIterations > lim || pcg->maxIterations > lim || pcg->reset > lim || pcg->reset == 0)
    throw std::invalid_argument("lmgpu adapter: PCG iteration counts out of range (reset >= 1, counts <= 2^28)");
  *out = lmgpu_pcg_params{pre, (int32_t)pcg->minIterations, (int32_t)pcg->maxIterations, (int32_t)pcg->reset, pcg->epsilon_rel,
                          pcg->epsilon_abs};
  return true;
}

/// the lmgpu_pcg_params of `p` as a Device argument (nullptr: the direct solver); `buf` holds them
inline const lmgpu_pcg_params* pcgOf(const NonlinearOptimizerParams& p, lmgpu_pcg_params* buf) { return toPcg(p, buf) ? buf : nullptr; }

}  // namespace lmgpu_detail

/// drop-in for LevenbergMarquardtOptimizer: same constructor arguments, same optimize() / iterate() / lambda() / values().
/// Unsupported factors, constrained noise, Scalar-scheme or custom m-estimators make the constructor throw
/// std::invalid_argument, so that a caller keeps the stock optimizer explicitly — there is no silent fallback.
/// linearSolverType = Iterative with PCGSolverParameters (Dummy / BlockJacobi preconditioner) runs the device PCG solver; any other
/// iterative parameter type throws std::invalid_argument here as well.
class GpuLevenbergMarquardtOptimizer : public LevenbergMarquardtOptimizer {
 public:
  enum Mode { WholeIterate, Piecewise };

  GpuLevenbergMarquardtOptimizer(const NonlinearFactorGraph& graph, const Values& initial,
                                 const LevenbergMarquardtParams& params = LevenbergMarquardtParams(), int device = 0, Mode mode = WholeIterate)
      : LevenbergMarquardtOptimizer(graph, initial, params),  // fixes params_.ordering (LevenbergMarquardtParams.h:112-117), initial error
        dev_(graph, initial, *params_.ordering, device, lmgpu_detail::pcgOf(params_, &pcg_)), cp_(lmgpu_detail::toC(params_)), mode_(mode) {}

  /// LevenbergMarquardtOptimizer::iterate() (LevenbergMarquardtOptimizer.cpp:273-308)
  GaussianFactorGraph::shared_ptr iterate() override {
    if (mode_ == Piecewise) return LevenbergMarquardtOptimizer::iterate();  // calls linearize() / solve() below
    auto cur = static_cast<const internal::LevenbergMarquardtState*>(state_.get());
    lmgpu_lm_state st{cur->error, cur->lambda, cur->currentFactor, (int32_t)cur->iterations, cur->totalNumberInnerIterations};
    try {
      dev_.problem().iterate(cp_, &st);
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
    state_.reset(new internal::LevenbergMarquardtState(dev_.download(cur->values), st.error, st.lambda, st.currentFactor,
                                                       (unsigned)st.iterations, (unsigned)st.totalNumberInnerIterations));
    (void)dev_.smartPoints(graph_, true);  // the smart factors of the caller's graph answer point() with the device's result
    // the hook's contract (NonlinearOptimizer.h:136, LevenbergMarquardtOptimizer.cpp:281,307; read at tests/testNonlinearOptimizer.cpp:282):
    // the linearization this iteration solved -- lmgpu_iterate leaves it on the device (it linearizes once per outer iteration, before
    // the lambda loop, and the accepted step does not touch the Jacobians).  optimize() below discards the graph like defaultOptimize
    // does (NonlinearOptimizer.cpp:92) and therefore does not fetch it.
    return discardLinear_ ? GaussianFactorGraph::shared_ptr() : dev_.downloadLinearGraph(graph_);
  }

  /// NonlinearOptimizer::optimize() (NonlinearOptimizer.h:98): defaultOptimize() calls iterate() and drops what it returns; skip the download
  const Values& optimize() override {
    discardLinear_ = true;
    try {
      defaultOptimize();
    } catch (...) {
      discardLinear_ = false;
      throw;
    }
    discardLinear_ = false;
    return values();
  }

  /// LevenbergMarquardtOptimizer::linearize() (LevenbergMarquardtOptimizer.h:113): graph_.linearize(state_->values) on the device
  GaussianFactorGraph::shared_ptr linearize() const override {
    if (dev_.problem().numSmartFactors() > 0)  // (the reference's loop would damp and solve the graph this returns; there is none to hand over)
      throw lmgpu_adapter::Error(LMGPU_INVALID, "smart factors: the Piecewise mode is not bound, use WholeIterate");
    dev_.upload(state_->values);
    dev_.problem().linearize();
    return dev_.downloadLinearGraph(graph_);
  }

  /// NonlinearOptimizer::solve() (NonlinearOptimizer.h:129-130).  tryLambda hands over buildDampedSystem(linear) — the
  /// linearization lmgpu_linearize left on the device plus lambda priors — so the damped system is rebuilt on the device from
  /// the state's lambda instead of being parsed out of `damped`.
  VectorValues solve(const GaussianFactorGraph& /*damped*/, const NonlinearOptimizerParams& /*params*/) const override {
    return dev_.solve(static_cast<const internal::LevenbergMarquardtState*>(state_.get())->lambda, &params_);
  }

  /// the whitened Jacobians of the last linearization as a GaussianFactorGraph (what iterate() returns in the reference)
  GaussianFactorGraph::shared_ptr lastLinearGraph() const { return dev_.downloadLinearGraph(graph_); }

  /// SmartProjectionFactor::point() of the graph's smart factors by graph index, from the device (also written back after every iterate())
  std::vector<TriangulationResult> gpuSmartPoints() const { return dev_.smartPoints(graph_, false); }

 private:
  lmgpu_pcg_params pcg_{};  // (declared before dev_: the constructor fills it while building dev_)
  mutable lmgpu_detail::Device dev_;
  lmgpu_lm_params cp_;
  Mode mode_;
  bool discardLinear_ = false;
};

/// drop-in for GaussNewtonOptimizer (gtsam/nonlinear/GaussNewtonOptimizer.cpp:44-66): iterate() = lmgpu_gn_iterate
class GpuGaussNewtonOptimizer : public GaussNewtonOptimizer {
 public:
  GpuGaussNewtonOptimizer(const NonlinearFactorGraph& graph, const Values& initial, const GaussNewtonParams& params = GaussNewtonParams(),
                          int device = 0)
      : GaussNewtonOptimizer(graph, initial, params), dev_(graph, initial, *params_.ordering, device, lmgpu_detail::pcgOf(params_, &pcg_)) {}

  GaussianFactorGraph::shared_ptr iterate() override {
    lmgpu_lm_state st{state_->error, 0.0, 0.0, (int32_t)state_->iterations, 0};
    try {
      dev_.problem().gnIterate(&st);
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
    state_.reset(new internal::NonlinearOptimizerState(dev_.download(state_->values), st.error, (unsigned)st.iterations));
    (void)dev_.smartPoints(graph_, true);
    return discardLinear_ ? GaussianFactorGraph::shared_ptr() : dev_.downloadLinearGraph(graph_);  // GaussNewtonOptimizer.cpp:49,65
  }

  std::vector<TriangulationResult> gpuSmartPoints() const { return dev_.smartPoints(graph_, false); }

  const Values& optimize() override {  // see GpuLevenbergMarquardtOptimizer::optimize
    discardLinear_ = true;
    try {
      defaultOptimize();
    } catch (...) {
      discardLinear_ = false;
      throw;
    }
    discardLinear_ = false;
    return values();
  }

  VectorValues solve(const GaussianFactorGraph& /*linear*/, const NonlinearOptimizerParams& /*params*/) const override {
    return dev_.solve(0.0, nullptr);
  }

 private:
  lmgpu_pcg_params pcg_{};  // (declared before dev_: the constructor fills it while building dev_)
  mutable lmgpu_detail::Device dev_;
  bool discardLinear_ = false;
};

/// drop-in for NonlinearConjugateGradientOptimizer (gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h:80-132, .cpp:44-90): the
/// gradient, the direction update, the golden-section line search and the advance run on the device (lmgpu_ncg_iterate /
/// lmgpu_ncg_optimize), one host wait per iteration.  The optimizer eliminates nothing: the ordering only fixes the slot order
/// (params.ordering, else the keys of the Values in their order); linearSolverType = Iterative builds the handle without fronts.
/// The direction method is honoured (the reference's constructor takes it but leaves directionMethod_ at PolakRibiere, .cpp:44-49).
class GpuNonlinearConjugateGradientOptimizer : public NonlinearConjugateGradientOptimizer {
 public:
  GpuNonlinearConjugateGradientOptimizer(const NonlinearFactorGraph& graph, const Values& initial, const Parameters& params = Parameters(),
                                         const DirectionMethod& directionMethod = DirectionMethod::PolakRibiere, int device = 0)
      : NonlinearConjugateGradientOptimizer(graph, initial, params, directionMethod),
        dev_(graph, initial, params.ordering ? *params.ordering : Ordering(initial.keys()), device, lmgpu_detail::pcgOf(params_, &pcg_)),
        method_(directionMethod) {}

  /// NonlinearConjugateGradientOptimizer::iterate() (.cpp:71-80): returns nullptr like the reference's
  GaussianFactorGraph::shared_ptr iterate() override {
    lmgpu_lm_state st{state_->error, 0.0, 0.0, (int32_t)state_->iterations, 0};
    dev_.problem().ncgIterate(toC(), &st);
    state_.reset(new internal::NonlinearOptimizerState(dev_.download(state_->values), st.error, (unsigned)st.iterations));
    return nullptr;
  }

  /// NonlinearConjugateGradientOptimizer::optimize() (.cpp:82-90)
  const Values& optimize() override {
    lmgpu_lm_state st{state_->error, 0.0, 0.0, (int32_t)state_->iterations, 0};
    dev_.problem().ncgOptimize(toC(), &st);
    state_.reset(new internal::NonlinearOptimizerState(dev_.download(state_->values), st.error, (unsigned)st.iterations));
    return state_->values;
  }

 private:
  lmgpu_ncg_params toC() const {
    int32_t m = LMGPU_NCG_POLAK_RIBIERE;
    switch (method_) {
      case DirectionMethod::FletcherReeves: m = LMGPU_NCG_FLETCHER_REEVES; break;
      case DirectionMethod::PolakRibiere: m = LMGPU_NCG_POLAK_RIBIERE; break;
      case DirectionMethod::HestenesStiefel: m = LMGPU_NCG_HESTENES_STIEFEL; break;
      case DirectionMethod::DaiYuan: m = LMGPU_NCG_DAI_YUAN; break;
    }
    return lmgpu_ncg_params{m, 0, (int32_t)params_.maxIterations, params_.relativeErrorTol, params_.absoluteErrorTol, params_.errorTol};
  }

  lmgpu_pcg_params pcg_{};  // (declared before dev_: the constructor fills it while building dev_)
  mutable lmgpu_detail::Device dev_;
  DirectionMethod method_;
};

/// DoglegOptimizer's state type (internal::DoglegState) is private to DoglegOptimizer.cpp:54-62, so a subclass cannot replace
/// state_; the Dogleg binding is therefore a NonlinearOptimizer of its own with the same interface (getDelta(), iterate()).
class GpuDoglegOptimizer : public NonlinearOptimizer {
  struct State : public internal::NonlinearOptimizerState {
    double delta;
    State(const Values& v, double e, double d, unsigned it = 0) : internal::NonlinearOptimizerState(v, e, it), delta(d) {}
  };

 public:
  GpuDoglegOptimizer(const NonlinearFactorGraph& graph, const Values& initial, const DoglegParams& params = DoglegParams(), int device = 0)
      : NonlinearOptimizer(graph, std::unique_ptr<internal::NonlinearOptimizerState>(new State(initial, graph.error(initial), params.deltaInitial))),
        params_(params) {
    if (params_.isIterative())  // DoglegOptimizer.cpp:108-110 throws in iterate(); refused before anything is built here
      throw std::invalid_argument("Dogleg is not currently compatible with the linear conjugate gradient solver");
    if (!params_.ordering) params_.ordering = Ordering::Create(params_.orderingType, graph);  // DoglegOptimizer.cpp:127-131
    dev_.reset(new lmgpu_detail::Device(graph, initial, *params_.ordering, device));
  }
  double getDelta() const { return static_cast<const State*>(state_.get())->delta; }

  GaussianFactorGraph::shared_ptr iterate() override {  // DoglegOptimizer.cpp:84-126
    lmgpu_lm_state st{state_->error, getDelta(), 0.0, (int32_t)state_->iterations, 0};
    try {
      dev_->problem().dlIterate(&st);  // trust radius travels in lambda (lmgpu.h)
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
    state_.reset(new State(dev_->download(state_->values), st.error, st.lambda, (unsigned)st.iterations));
    return discardLinear_ ? GaussianFactorGraph::shared_ptr() : dev_->downloadLinearGraph(graph_);  // DoglegOptimizer.cpp:87,122
  }

  const Values& optimize() override {  // see GpuLevenbergMarquardtOptimizer::optimize
    discardLinear_ = true;
    try {
      defaultOptimize();
    } catch (...) {
      discardLinear_ = false;
      throw;
    }
    discardLinear_ = false;
    return values();
  }

 protected:
  const NonlinearOptimizerParams& _params() const override { return params_; }
  DoglegParams params_;
  std::unique_ptr<lmgpu_detail::Device> dev_;
  bool discardLinear_ = false;
};

/// What GpuMarginals::jointMarginalCovariance returns: the reference's JointMarginal (Marginals.h:141-191) has a protected constructor
/// with `friend class Marginals`, so this is a small class of the same shape -- at(i, j), operator()(i, j), fullMatrix() -- with the
/// blocks ordered by Key as there.
class GpuJointMarginal {
 public:
  GpuJointMarginal(const KeyVector& keys, const std::vector<size_t>& dims, const Matrix& full) : keys_(keys), full_(full) {
    size_t o = 0;
    for (size_t q = 0; q < keys.size(); q++) {
      range_[keys[q]] = std::make_pair(o, dims[q]);
      o += dims[q];
    }
  }
  /// JointMarginal::at(iVariable, jVariable): the block of the two variables
  Matrix at(Key iVariable, Key jVariable) const {
    const std::pair<size_t, size_t>&a = range_.at(iVariable), &b = range_.at(jVariable);
    return full_.block(a.first, b.first, a.second, b.second);
  }
  Matrix operator()(Key iVariable, Key jVariable) const { return at(iVariable, jVariable); }
  /// JointMarginal::fullMatrix(): all blocks, ordered by Key
  const Matrix& fullMatrix() const { return full_; }
  const KeyVector& keys() const { return keys_; }

 private:
  KeyVector keys_;
  Matrix full_;
  std::map<Key, std::pair<size_t, size_t>> range_;  // key -> (first scalar, dimension)
};

/// Marginals(graph, solution, ordering) with the covariances of MANY variables from one factorization (gtsam/nonlinear/Marginals.h:
/// the constructor linearizes at the solution and eliminates, Marginals.cpp:28-43; marginalCovariance :124-127, marginalInformation
/// :109-121).  lmgpu_marginals_factor keeps the Bayes tree on the device; each query walks the variable's path to the root
/// (lmgpu_marginal_covariances).  Cholesky only, like the reference's default; an indeterminate system throws from the constructor as
/// the reference's does.  Joint marginals and single cross-covariances come from the same factorization
/// (lmgpu_joint_marginal_covariances, lmgpu_marginal_cross_covariances: the source's path, then each target's branch).
class GpuMarginals {
 public:
  GpuMarginals(const NonlinearFactorGraph& graph, const Values& solution, const Ordering& ordering, int device = 0)
      : dev_(new lmgpu_detail::Device(graph, solution, ordering, device)) {
    try {
      dev_->problem().marginalsFactor();
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
  }

  /// Marginals::marginalCovariance(variable)
  Matrix marginalCovariance(Key variable) const { return marginalCovariances(KeyVector{variable}).front(); }
  /// Marginals::marginalInformation(variable)
  Matrix marginalInformation(Key variable) const { return marginalCovariance(variable).inverse(); }
  /// the covariances of `variables`, in their order: one launch per chunk of requests, one workgroup per variable
  std::vector<Matrix> marginalCovariances(const KeyVector& variables) const {
    lmgpu_adapter::Problem& p = dev_->problem();
    std::vector<int32_t> slots;
    slots.reserve(variables.size());
    for (Key k : variables) slots.push_back(p.slotOf(k));
    std::vector<double> packed;
    try {
      packed = p.marginalCovariances(slots);
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
    std::vector<Matrix> out;
    out.reserve(slots.size());
    size_t o = 0;
    for (int32_t s : slots) {
      const int d = lmgpu_adapter::varDim(p.typeOfSlot(s));
      out.push_back(Eigen::Map<const Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>>(packed.data() + o, d, d));
      o += (size_t)d * d;
    }
    return out;
  }
  /// Marginals::jointMarginalCovariance(variables) (Marginals.cpp:130-137): distinct variables, blocks ordered by Key
  GpuJointMarginal jointMarginalCovariance(const KeyVector& variables) const {
    lmgpu_adapter::Problem& p = dev_->problem();
    KeyVector keys(variables);
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> slots;
    std::vector<size_t> dims;
    size_t D = 0;
    for (Key k : keys) {
      slots.push_back(p.slotOf(k));
      dims.push_back((size_t)lmgpu_adapter::varDim(p.typeOfSlot(slots.back())));
      D += dims.back();
    }
    std::vector<double> packed;
    try {
      packed = p.jointMarginalCovariance(slots);
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
    return GpuJointMarginal(keys, dims, Eigen::Map<const Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>>(packed.data(), D, D));
  }
  /// Marginals::jointMarginalInformation(variables) (Marginals.cpp:145): here the inverse of the joint covariance
  GpuJointMarginal jointMarginalInformation(const KeyVector& variables) const {
    const GpuJointMarginal cov = jointMarginalCovariance(variables);
    std::vector<size_t> dims;
    for (Key k : cov.keys()) dims.push_back((size_t)cov.at(k, k).rows());
    return GpuJointMarginal(cov.keys(), dims, cov.fullMatrix().inverse());
  }
  /// Sigma[i, j], dim_i x dim_j: the path of j is walked, then the branch of i below the junction of the two paths
  Matrix crossCovariance(Key i, Key j) const {
    lmgpu_adapter::Problem& p = dev_->problem();
    const int32_t si = p.slotOf(i), sj = p.slotOf(j);
    std::vector<double> packed;
    try {
      packed = p.marginalCrossCovariances(std::vector<int32_t>{si}, std::vector<int32_t>{sj});
    } catch (const lmgpu_adapter::Indeterminate& e) {
      throw IndeterminantLinearSystemException(e.key);
    }
    return Eigen::Map<const Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>>(
        packed.data(), lmgpu_adapter::varDim(p.typeOfSlot(si)), lmgpu_adapter::varDim(p.typeOfSlot(sj)));
  }
  lmgpu_marginals_stats stats() const { return dev_->problem().marginalsStats(); }

 private:
  std::unique_ptr<lmgpu_detail::Device> dev_;
};

/// ISAM2 on the device (lmgpu_isam2_*): the same update() / calculateEstimate() calls as gtsam::ISAM2 (gtsam/nonlinear/ISAM2.h:146-260)
/// for the parameter subset the C ABI binds (Gauss-Newton or Dogleg optimisation params, relinearization threshold as a double or per Symbol
/// character, partial relinearization check, Cholesky).  Not a
/// subclass: ISAM2 is a BayesTree<ISAM2Clique> whose cliques live on the host; here the tree lives on the device and only the
/// estimate comes back.  The constrained COLAMD of recalculate() stays on this side: the callback below is the body of
/// Ordering::ColamdConstrained (gtsam/inference/Ordering.cpp:86-108) on the arrays the library hands over.
class GpuISAM2 {
 public:
  explicit GpuISAM2(const ISAM2Params& params = ISAM2Params(), int device = 0) {
    if (params.factorization != ISAM2Params::CHOLESKY || !params.cacheLinearizedFactors)
      throw std::invalid_argument("GpuISAM2: parameter set not bound (Cholesky, cached linear factors)");
    const bool byChar = std::holds_alternative<FastMap<char, Vector>>(params.relinearizeThreshold);
    const ISAM2DoglegParams* dl = std::get_if<ISAM2DoglegParams>(&params.optimizationParams);
    lmgpu_isam2_params p{byChar ? 0.1 : std::get<double>(params.relinearizeThreshold), params.relinearizeSkip, params.enableRelinearization ? 1 : 0,
                         dl ? dl->wildfireThreshold : std::get<ISAM2GaussNewtonParams>(params.optimizationParams).wildfireThreshold};
    lmgpu_config cfg{device, 0, 1, 0};
    if (lmgpu_isam2_create(&cfg, &p, &GpuISAM2::Ccolamd, nullptr, &h_) != LMGPU_OK) {
      const std::string why = h_ ? lmgpu_isam2_last_error(h_) : "lmgpu_isam2_create failed";
      if (h_) lmgpu_isam2_destroy(h_);
      throw std::runtime_error(why);
    }
    if (dl) check(lmgpu_isam2_set_dogleg(h_, dl->initialDelta, dl->wildfireThreshold, (int32_t)dl->adaptationMode));  // ISAM2Params.h:68-110
    if (byChar) {  // ISAM2Params::relinearizeThreshold as FastMap<char, Vector> (ISAM2Params.h:139-141)
      std::string chrs;
      std::vector<int32_t> dims;
      std::vector<double> values;
      for (const auto& cv : std::get<FastMap<char, Vector>>(params.relinearizeThreshold)) {
        chrs.push_back(cv.first);
        dims.push_back((int32_t)cv.second.size());
        values.insert(values.end(), cv.second.data(), cv.second.data() + cv.second.size());
      }
      check(lmgpu_isam2_set_relinearize_thresholds(h_, (int32_t)dims.size(), chrs.data(), dims.data(), values.data()));
    }
    if (params.enablePartialRelinearizationCheck) check(lmgpu_isam2_set_partial_relinearization_check(h_, 1));
    if (params.evaluateNonlinearError) check(lmgpu_isam2_set_evaluate_nonlinear_error(h_, 1));
    if (params.findUnusedFactorSlots) check(lmgpu_isam2_set_find_unused_factor_slots(h_, 1));
  }
  ~GpuISAM2() { if (h_) lmgpu_isam2_destroy(h_); }
  GpuISAM2(const GpuISAM2&) = delete;
  GpuISAM2& operator=(const GpuISAM2&) = delete;

  /// ISAM2::update(newFactors, newTheta, removeFactorIndices, constrainedKeys, noRelinKeys, extraReelimKeys, force_relinearize)
  /// (ISAM2.h:146-156, ISAM2.cpp:400-416)
  lmgpu_isam2_result update(const NonlinearFactorGraph& newFactors = NonlinearFactorGraph(), const Values& newTheta = Values(),
                            const FactorIndices& removeFactorIndices = FactorIndices(),
                            const std::optional<FastMap<Key, int>>& constrainedKeys = {}, const std::optional<FastList<Key>>& noRelinKeys = {},
                            const std::optional<FastList<Key>>& extraReelimKeys = {}, bool force_relinearize = false) {
    ISAM2UpdateParams params;
    params.constrainedKeys = constrainedKeys;
    params.extraReelimKeys = extraReelimKeys;
    params.force_relinearize = force_relinearize;
    params.noRelinKeys = noRelinKeys;
    params.removeFactorIndices = removeFactorIndices;
    return update(newFactors, newTheta, params);
  }

  /// ISAM2::update(newFactors, newTheta, const ISAM2UpdateParams&) (ISAM2.h:176-186, ISAM2.cpp:419-480).  The new factors take the
  /// indices ISAM2Result::newFactorsIndices would name: size() .. of the factor list, or its empty slots first with findUnusedFactorSlots.
  lmgpu_isam2_result update(const NonlinearFactorGraph& newFactors, const Values& newTheta, const ISAM2UpdateParams& up) {
    if (up.newAffectedKeys) throw std::invalid_argument("GpuISAM2: newAffectedKeys (smart factors) is not bound");
    std::vector<uint64_t> keys;
    std::vector<int32_t> types;
    std::vector<double> packed;
    for (const auto& kv : newTheta) {
      const int32_t t = lmgpu_detail::variableType(kv.value);
      keys.push_back(kv.key);
      types.push_back(t);
      double v[15];
      packOne(newTheta, kv.key, t, v);
      packed.insert(packed.end(), v, v + lmgpu_adapter::varStore(t));
      if (all_.exists(kv.key)) all_.erase(kv.key);  // a key that left the system (unusedKeys) may come back
      all_.insert(kv.key, kv.value);  // keeps what does not travel (Cal3Bundler's principal point) and the types for download
    }
    check(lmgpu_isam2_add_variables(h_, (int32_t)keys.size(), keys.data(), types.data(), packed.data()));
    for (size_t i = 0; i < newFactors.size(); i++) {
      if (!newFactors[i]) continue;
      auto nm = std::dynamic_pointer_cast<NoiseModelFactor>(newFactors[i]);
      int32_t type;
      std::vector<double> meas;
      if (!nm || !lmgpu_detail::extractFactor(newFactors[i], all_, &type, &meas)) throw std::invalid_argument("GpuISAM2: factor type not bound");
      const lmgpu_detail::Noise nz = lmgpu_detail::extractNoise(nm->noiseModel());
      std::vector<uint64_t> fk(nm->keys().begin(), nm->keys().end());
      check(lmgpu_isam2_add_factors_robust(h_, type, 1, fk.data(), meas.data(), nz.kind, nz.data.empty() ? nullptr : nz.data.data(), nz.robust, nz.robustK));
    }
    std::vector<uint64_t> rm(up.removeFactorIndices.begin(), up.removeFactorIndices.end()), ck, nr, ex;
    std::vector<int32_t> cg;
    if (up.constrainedKeys)
      for (const auto& kg : *up.constrainedKeys) {
        ck.push_back(kg.first);
        cg.push_back(kg.second);
      }
    if (up.noRelinKeys) nr.assign(up.noRelinKeys->begin(), up.noRelinKeys->end());
    if (up.extraReelimKeys) ex.assign(up.extraReelimKeys->begin(), up.extraReelimKeys->end());
    const lmgpu_isam2_update_params p{(int32_t)rm.size(), rm.data(), up.constrainedKeys ? 1 : 0, (int32_t)ck.size(), ck.data(), cg.data(),
                                      (int32_t)nr.size(), nr.data(), (int32_t)ex.size(), ex.data(), up.force_relinearize ? 1 : 0,
                                      up.forceFullSolve ? 1 : 0};
    lmgpu_isam2_result r{};
    check(lmgpu_isam2_update_with(h_, &p, &r));
    return r;
  }

  /// ISAM2::marginalizeLeaves(leafKeys, marginalFactorsIndices, deletedFactorsIndices) (ISAM2.h:198-222, ISAM2.cpp:487-720).  The leaf
  /// keys must have been ordered first (constrainedKeys of the update before, as IncrementalFixedLagSmoother does).  A key that is not a
  /// leaf throws std::runtime_error BEFORE anything changes (the reference checks it in debug builds only).
  void marginalizeLeaves(const FastList<Key>& leafKeys, FactorIndices* marginalFactorsIndices = nullptr, FactorIndices* deletedFactorsIndices = nullptr) {
    const std::vector<uint64_t> keys(leafKeys.begin(), leafKeys.end());
    int32_t nm = 0, nd = 0;
    check(lmgpu_isam2_marginalize_leaves(h_, (int32_t)keys.size(), keys.data(), &nm, &nd));
    std::vector<uint64_t> mi((size_t)std::max(1, nm)), di((size_t)std::max(1, nd));
    check(lmgpu_isam2_get_marginalize_result(h_, mi.data(), di.data()));
    if (marginalFactorsIndices) marginalFactorsIndices->assign(mi.begin(), mi.begin() + nm);
    if (deletedFactorsIndices) deletedFactorsIndices->assign(di.begin(), di.begin() + nd);
    for (Key k : leafKeys)
      if (all_.exists(k)) all_.erase(k);
  }
  /// ISAM2::getFixedVariables() (ISAM2.h:259)
  KeySet getFixedVariables() const {
    std::vector<uint64_t> k((size_t)std::max(1, lmgpu_isam2_get_fixed_variables(h_, nullptr)));
    const int n = lmgpu_isam2_get_fixed_variables(h_, k.data());
    return KeySet(k.begin(), k.begin() + n);
  }

  /// ISAM2::marginalCovariance(key) (ISAM2.h:253-257)
  Matrix marginalCovariance(Key key) const {
    if (!all_.exists(key)) throw std::out_of_range("GpuISAM2::marginalCovariance: unknown key");
    const int d = (int)all_.at(key).dim();
    Matrix cov(d, d);  // symmetric: the row-major block the library writes reads the same column-major
    check(lmgpu_isam2_marginal_covariance(h_, key, cov.data()));
    return cov;
  }
  /// the covariances of `variables`, in their order, from the present Bayes tree: one launch per chunk of requests, one workgroup per
  /// variable (lmgpu_isam2_marginal_covariances).  Like marginalCovariance: the covariance at the linearization point.
  std::vector<Matrix> marginalCovariances(const KeyVector& variables) const {
    std::vector<uint64_t> keys(variables.begin(), variables.end());
    size_t total = 0;
    for (Key k : variables) total += dimOf(k) * dimOf(k);
    std::vector<double> packed(std::max<size_t>(total, 1));
    check(lmgpu_isam2_marginal_covariances(h_, (int32_t)keys.size(), keys.data(), packed.data()));
    std::vector<Matrix> out;
    out.reserve(keys.size());
    size_t o = 0;
    for (Key k : variables) {
      const size_t d = dimOf(k);
      out.push_back(Eigen::Map<const Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>>(packed.data() + o, d, d));
      o += d * d;
    }
    return out;
  }
  /// the joint marginal of distinct variables as BayesTree::joint / Marginals::jointMarginalCovariance shape it (blocks ordered by
  /// Key), without refactoring the graph: every block from the present tree (lmgpu_isam2_joint_marginal_covariances), exactly symmetric
  GpuJointMarginal jointMarginalCovariance(const KeyVector& variables) const {
    KeyVector sorted(variables);
    std::sort(sorted.begin(), sorted.end());
    std::vector<uint64_t> keys(sorted.begin(), sorted.end());
    std::vector<size_t> dims;
    size_t D = 0;
    for (Key k : sorted) {
      dims.push_back(dimOf(k));
      D += dims.back();
    }
    const int32_t begin[2] = {0, (int32_t)keys.size()};
    std::vector<double> packed(std::max<size_t>(D * D, 1));
    check(lmgpu_isam2_joint_marginal_covariances(h_, 1, begin, keys.data(), packed.data()));
    return GpuJointMarginal(sorted, dims, Eigen::Map<const Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>>(packed.data(), D, D));
  }
  /// Sigma[i, j], dim_i x dim_j: the path of j is walked, then the branch of i below the junction of the two paths
  Matrix crossCovariance(Key i, Key j) const {
    const size_t di = dimOf(i), dj = dimOf(j);
    const uint64_t ki = i, kj = j;
    std::vector<double> packed(di * dj);
    check(lmgpu_isam2_cross_covariances(h_, 1, &ki, &kj, packed.data()));
    return Eigen::Map<const Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>>(packed.data(), di, dj);
  }
  lmgpu_marginals_stats marginalsStats() const {
    lmgpu_marginals_stats st;
    check(lmgpu_isam2_get_marginals_stats(h_, &st));
    return st;
  }

  /// ISAM2Result::errorBefore / errorAfter of the last update (with ISAM2Params::evaluateNonlinearError)
  std::pair<double, double> errors() const {
    double before = 0, after = 0;
    check(lmgpu_isam2_get_errors(h_, &before, &after));
    return {before, after};
  }
  /// getFactorsUnsafe().error(calculateEstimate())
  double error() const {
    double e = 0;
    check(lmgpu_isam2_error(h_, 0, &e));
    return e;
  }

  /// ISAM2Result::unusedKeys of the last update
  KeySet unusedKeys() const {
    std::vector<uint64_t> k((size_t)std::max(1, lmgpu_isam2_get_unused_keys(h_, nullptr)));
    const int n = lmgpu_isam2_get_unused_keys(h_, k.data());
    return KeySet(k.begin(), k.begin() + n);
  }

  Values calculateEstimate() const { return download(0); }
  /// ISAM2::calculateEstimate<VALUE>(Key) (ISAM2.h:231-236, ISAM2.cpp:757-760): only this variable is retracted and downloaded
  template <class VALUE>
  VALUE calculateEstimate(Key key) const {
    int32_t t = -1;
    double q[15];
    check(lmgpu_isam2_get_value(h_, 0, key, &t, q));
    Values one;
    unpackOne(key, t, q, &one);
    return one.at<VALUE>(key);
  }
  Values calculateBestEstimate() const { return download(1); }
  Values getLinearizationPoint() const { return download(2); }

 private:
  static int Ccolamd(void*, int32_t n_rows, int32_t n_cols, const int32_t* col_ptr, const int32_t* row_idx, const int32_t* cmember, int32_t* perm_out) {
    const size_t Alen = ccolamd_recommended(col_ptr[n_cols], n_rows, n_cols);
    std::vector<int> A(Alen), p(col_ptr, col_ptr + n_cols + 1), cm(cmember, cmember + n_cols);
    std::copy(row_idx, row_idx + col_ptr[n_cols], A.begin());
    double knobs[CCOLAMD_KNOBS];
    ccolamd_set_defaults(knobs);
    knobs[CCOLAMD_DENSE_ROW] = -1;
    knobs[CCOLAMD_DENSE_COL] = -1;
    int stats[CCOLAMD_STATS];
    if (ccolamd(n_rows, n_cols, (int)Alen, A.data(), p.data(), knobs, stats, cm.data()) != 1) return 0;
    std::copy(p.begin(), p.begin() + n_cols, perm_out);
    return 1;
  }
  void check(int rc) const {
    if (rc == LMGPU_OK) return;
    if (rc == LMGPU_INDETERMINATE) throw IndeterminantLinearSystemException(lmgpu_isam2_last_failed_key(h_));
    throw std::runtime_error(lmgpu_isam2_last_error(h_));
  }
  /// scalars of a variable this object was given (the library refuses one that has left the tree since)
  size_t dimOf(Key key) const {
    if (!all_.exists(key)) throw std::out_of_range("GpuISAM2: unknown key");
    return all_.at(key).dim();
  }
  static void packOne(const Values& v, Key k, int32_t t, double* o) {
    switch (t) {
      case LMGPU_POSE2: { const Pose2& q = v.at<Pose2>(k); o[0] = q.x(); o[1] = q.y(); o[2] = q.theta(); break; }
      case LMGPU_POSE3: lmgpu_detail::packPose3(v.at<Pose3>(k), o); break;
      case LMGPU_POINT3: { const Point3& q = v.at<Point3>(k); o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); break; }
      case LMGPU_POINT2: { const Point2& q = v.at<Point2>(k); o[0] = q.x(); o[1] = q.y(); break; }
        case LMGPU_CAL3_S2: { const Cal3_S2& q = v.at<Cal3_S2>(k); o[0] = q.fx(); o[1] = q.fy(); o[2] = q.skew(); o[3] = q.px(); o[4] = q.py(); break; }
      default: {
        const lmgpu_detail::Camera& c = v.at<lmgpu_detail::Camera>(k);
        lmgpu_detail::packPose3(c.pose(), o);
        o[12] = c.calibration().fx(); o[13] = c.calibration().k1(); o[14] = c.calibration().k2();
      }
    }
  }
  void unpackOne(Key k, int32_t t, const double* q, Values* out) const {
    switch (t) {
      case LMGPU_POSE2: out->insert(k, Pose2(q[0], q[1], q[2])); break;
      case LMGPU_POSE3: out->insert(k, lmgpu_detail::unpackPose3(q)); break;
      case LMGPU_POINT3: out->insert(k, Point3(q[0], q[1], q[2])); break;
      case LMGPU_POINT2: out->insert(k, Point2(q[0], q[1])); break;
      case LMGPU_CAL3_S2: out->insert(k, Cal3_S2(q[0], q[1], q[2], q[3], q[4])); break;
      default: {
        const Cal3Bundler& K0 = all_.at<lmgpu_detail::Camera>(k).calibration();
        out->insert(k, lmgpu_detail::Camera(lmgpu_detail::unpackPose3(q), Cal3Bundler(q[12], q[13], q[14], K0.px(), K0.py())));
      }
    }
  }
  Values download(int which) const {
    const int n = lmgpu_isam2_num_variables(h_);
    std::vector<uint64_t> keys((size_t)n);
    std::vector<int32_t> types((size_t)n);
    check(lmgpu_isam2_get_values(h_, 2, keys.data(), types.data(), nullptr));
    size_t tot = 0;
    for (int32_t t : types) tot += (size_t)lmgpu_adapter::varStore(t);
    std::vector<double> packed(tot);
    check(lmgpu_isam2_get_values(h_, which, nullptr, nullptr, packed.data()));
    Values out;
    const double* q = packed.data();
    for (int i = 0; i < n; i++) {
      const Key k = keys[(size_t)i];
      unpackOne(k, types[(size_t)i], q, &out);
      q += lmgpu_adapter::varStore(types[(size_t)i]);
    }
    return out;
  }

  lmgpu_isam2* h_ = nullptr;
  Values all_;  // every variable ever added, at its initial value
};

/// InitializePose3::initialize(graph, givenGuess, useGradient) (gtsam/slam/InitializePose3.h:85-92, InitializePose3.cpp:296-319) on the
/// device: call gtsam::GpuInitializePose3::initialize where the program called InitializePose3::initialize.  The pose graph is extracted
/// by the library (BetweenFactor<Pose3> kept, PriorFactor<Pose3> tied to kAnchorKey, everything else dropped: InitializePose.h:36-52);
/// the relaxation, the projection onto SO(3) / the gradient iteration and the Gauss-Newton step run behind lmgpu_init_pose3_*.
/// `ordering`: elimination order of the pose keys (default: ascending keys, Ordering::Natural); the anchor is placed last unless listed.
class GpuInitializePose3 {
 public:
  static Values initialize(const NonlinearFactorGraph& graph, const Values& givenGuess, bool useGradient = false, const Ordering* ordering = nullptr,
                           int device = 0) {
    Session s(graph, ordering, device);
    std::vector<double> guess;
    if (useGradient) guess = s.packGuess(givenGuess);
    std::vector<double> poses(s.keys.size() * 12);
    s.check(lmgpu_init_pose3_initialize(s.ip, useGradient ? guess.data() : nullptr, useGradient ? 1 : 0, poses.data()));
    Values out;
    for (size_t i = 0; i < s.keys.size(); i++) out.insert(s.keys[i], lmgpu_detail::unpackPose3(&poses[12 * i]));
    return out;
  }
  static Values initialize(const NonlinearFactorGraph& graph) { return initialize(graph, Values(), false); }

  /// initializeOrientations (InitializePose3.cpp:278-285): the chordal rotations as Rot3
  static Values initializeOrientations(const NonlinearFactorGraph& graph, const Ordering* ordering = nullptr, int device = 0) {
    Session s(graph, ordering, device);
    std::vector<double> R(s.keys.size() * 9);
    s.check(lmgpu_init_pose3_orientations_chordal(s.ip, R.data()));
    return s.rotations(R);
  }

  /// computeOrientationsGradient (:117-218) on the graph's extracted pose graph
  static Values computeOrientationsGradient(const NonlinearFactorGraph& graph, const Values& givenGuess, size_t maxIter = 10000,
                                            bool setRefFrame = true, const Ordering* ordering = nullptr, int device = 0) {
    Session s(graph, ordering, device);
    const std::vector<double> guess = s.packGuess(givenGuess);
    std::vector<double> R(s.keys.size() * 9);
    s.check(lmgpu_init_pose3_orientations_gradient(s.ip, guess.data(), static_cast<int32_t>(maxIter), setRefFrame ? 1 : 0, R.data(), nullptr, nullptr));
    return s.rotations(R);
  }

 private:
  struct Session {
    lmgpu_init_pose3* ip = nullptr;
    KeyVector keys;  // result order: the ordering without the anchor
    Session(const NonlinearFactorGraph& graph, const Ordering* ordering, int device) {
      lmgpu_config cfg{device, 0, 1, 0};
      if (lmgpu_init_pose3_create(&cfg, &ip) != LMGPU_OK) throw std::runtime_error("lmgpu_init_pose3_create failed");
      KeySet seen;
      for (size_t i = 0; i < graph.size(); i++) {
        const auto& f = graph[i];
        if (!f) continue;
        const bool between = static_cast<bool>(std::dynamic_pointer_cast<BetweenFactor<Pose3>>(f));
        const bool prior = static_cast<bool>(std::dynamic_pointer_cast<PriorFactor<Pose3>>(f));
        if (!between && !prior) continue;  // buildPoseGraph drops everything else
        int32_t type = 0;
        std::vector<double> m;
        lmgpu_detail::extractFactor(f, Values(), &type, &m);
        const lmgpu_detail::Noise nz = lmgpu_detail::extractNoise(std::static_pointer_cast<NoiseModelFactor>(f)->noiseModel());
        if (nz.robust != LMGPU_ROBUST_NONE) throw std::invalid_argument("GpuInitializePose3: robust noise models are not bound");
        const int32_t gi = static_cast<int32_t>(i);
        std::vector<uint64_t> k(f->keys().begin(), f->keys().end());
        for (uint64_t key : k) seen.insert(key);
        check(lmgpu_init_pose3_add_factors(ip, type, 1, &gi, k.data(), m.data(), nz.kind, nz.data.empty() ? nullptr : nz.data.data()));
      }
      std::vector<uint64_t> order;
      if (ordering) order.assign(ordering->begin(), ordering->end());
      else order.assign(seen.begin(), seen.end());
      if (order.empty()) order.push_back(LMGPU_INIT_POSE3_ANCHOR_KEY);  // let the library refuse the empty graph
      check(lmgpu_init_pose3_finalize(ip, static_cast<int32_t>(order.size()), order.data()));
      for (uint64_t key : order)
        if (key != LMGPU_INIT_POSE3_ANCHOR_KEY) keys.push_back(key);
    }
    ~Session() { lmgpu_init_pose3_destroy(ip); }
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    void check(int rc) const {
      if (rc == LMGPU_OK) return;
      if (rc == LMGPU_INDETERMINATE) throw IndeterminantLinearSystemException(keys.empty() ? Key(0) : keys.front());
      throw std::invalid_argument(std::string("GpuInitializePose3: ") + lmgpu_init_pose3_last_error(ip));
    }
    std::vector<double> packGuess(const Values& givenGuess) const {
      std::vector<double> g(keys.size() * 9);
      for (size_t i = 0; i < keys.size(); i++) {
        const Matrix3 R = givenGuess.at<Pose3>(keys[i]).rotation().matrix();
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) g[9 * i + 3 * r + c] = R(r, c);
      }
      return g;
    }
    Values rotations(const std::vector<double>& R) const {
      Values out;
      for (size_t i = 0; i < keys.size(); i++) {
        Matrix3 M;
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) M(r, c) = R[9 * i + 3 * r + c];
        out.insert(keys[i], Rot3(M));
      }
      return out;
    }
  };
};

/// TranslationRecovery (gtsam/sfm/TranslationRecovery.h) on the device: construct a gtsam::GpuTranslationRecovery where the program constructed
/// a TranslationRecovery and call run the same way.  The graph (TranslationFactor per edge, the two priors or the BetweenFactor<Point3>s),
/// the merging of nodes joined by zero-direction edges, the initial values and the Levenberg-Marquardt solve run behind
/// lmgpu_translation_recovery_*.  Deviations, as documented in lmgpu.h: the random initial values come from a generator owned by this
/// object (seed 42; seed() resets it), a merged set is represented by its smallest key, the BilinearAngleTranslationFactor form is refused.
/// `ordering`: elimination order over the keys of the measurements (default: first appearance).
class GpuTranslationRecovery {
 public:
  using KeyPair = std::pair<Key, Key>;
  using TranslationEdges = std::vector<BinaryMeasurement<Unit3>>;

  explicit GpuTranslationRecovery(const LevenbergMarquardtParams& lmParams = LevenbergMarquardtParams(), bool use_bilinear_translation_factor = false,
                                  int device = 0)
      : lmParams_(lmParams), device_(device) {
    if (use_bilinear_translation_factor)
      throw std::invalid_argument("GpuTranslationRecovery: use_bilinear_translation_factor needs a 1-D variable type (not bound)");
    lmgpu_pcg_params pcg;
    if (lmgpu_detail::toPcg(lmParams, &pcg)) throw std::invalid_argument("GpuTranslationRecovery: solves with the direct solver (PCG is refused)");
  }

  void seed(uint32_t s) { seed_ = s; }

  /// TranslationRecovery::run (TranslationRecovery.cpp:191-228)
  Values run(const TranslationEdges& relativeTranslations, const double scale = 1.0,
             const std::vector<BinaryMeasurement<Point3>>& betweenTranslations = {}, const Values& initialValues = Values(),
             const Ordering* ordering = nullptr) const {
    Session s(device_);
    s.check(lmgpu_translation_recovery_seed(s.tr, seed_));
    for (size_t i = 0; i < relativeTranslations.size(); i++) {
      const auto& e = relativeTranslations[i];
      const Point3 z = e.measured().point3();
      s.add(lmgpu_translation_recovery_add_directions, i, e.key1(), e.key2(), z, e.noiseModel());
    }
    for (size_t i = 0; i < betweenTranslations.size(); i++) {
      const auto& e = betweenTranslations[i];
      s.add(lmgpu_translation_recovery_add_betweens, i, e.key1(), e.key2(), e.measured(), e.noiseModel());
    }
    std::vector<uint64_t> ikeys, order;
    std::vector<double> ivals;
    for (const Key k : initialValues.keys()) {
      const Point3 p = initialValues.at<Point3>(k);
      ikeys.push_back(k);
      ivals.insert(ivals.end(), {p.x(), p.y(), p.z()});
    }
    if (ordering) order.assign(ordering->begin(), ordering->end());
    s.check(lmgpu_translation_recovery_finalize(s.tr, scale, static_cast<int32_t>(ikeys.size()), ikeys.data(), ivals.data(),
                                                static_cast<int32_t>(order.size()), order.data()));
    const lmgpu_lm_params p = lmgpu_detail::toC(lmParams_);
    lmgpu_lm_state st;
    s.check(lmgpu_translation_recovery_run(s.tr, &p, &st));
    const int n = lmgpu_translation_recovery_num_keys(s.tr);
    std::vector<uint64_t> keys(static_cast<size_t>(n));
    std::vector<double> out(3 * static_cast<size_t>(n));
    lmgpu_translation_recovery_get_keys(s.tr, keys.data(), nullptr);
    s.check(lmgpu_translation_recovery_get(s.tr, out.data()));
    Values result;
    for (size_t i = 0; i < keys.size(); i++) result.insert<Point3>(keys[i], Point3(out[3 * i], out[3 * i + 1], out[3 * i + 2]));
    return result;
  }

 private:
  struct Session {
    lmgpu_translation_recovery* tr = nullptr;
    explicit Session(int device) {
      lmgpu_config cfg{device, 0, 1, 0};
      if (lmgpu_translation_recovery_create(&cfg, &tr) != LMGPU_OK) throw std::runtime_error("lmgpu_translation_recovery_create failed");
    }
    ~Session() { lmgpu_translation_recovery_destroy(tr); }
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    void check(int rc) const {
      if (rc == LMGPU_OK) return;
      const std::string msg = std::string("GpuTranslationRecovery: ") + lmgpu_translation_recovery_last_error(tr);
      if (rc == LMGPU_INDETERMINATE) {  // the first frontal variable of the failing front, like the optimizers' adapters
        lmgpu_handle* h = lmgpu_translation_recovery_handle(tr);
        const int n = lmgpu_translation_recovery_get_slots(tr, nullptr);
        std::vector<uint64_t> slots(n > 0 ? static_cast<size_t>(n) : 0);
        if (n > 0) lmgpu_translation_recovery_get_slots(tr, slots.data());
        const int slot = h ? lmgpu_last_failed_slot(h) : -1;
        throw IndeterminantLinearSystemException(slot >= 0 && slot < n ? Key(slots[static_cast<size_t>(slot)]) : Key(0));
      }
      if (rc == LMGPU_INVALID) throw std::invalid_argument(msg);
      throw std::runtime_error(msg);  // LMGPU_HIP_ERROR: the device, not the caller's input
    }
    template <class ADD>
    void add(ADD fn, size_t i, Key k1, Key k2, const Point3& z, const SharedNoiseModel& model) const {
      const lmgpu_detail::Noise nz = lmgpu_detail::extractNoise(model);  // throws on a constrained model
      const int32_t index = static_cast<int32_t>(i);
      const uint64_t keys[2] = {k1, k2};
      const double m[3] = {z.x(), z.y(), z.z()};
      check(fn(tr, 1, &index, keys, m, nz.kind, nz.data.empty() ? nullptr : nz.data.data(), nz.robust, nz.robustK));
    }
  };
  LevenbergMarquardtParams lmParams_;
  int device_;
  uint32_t seed_ = 42;
};

/// MFAS (gtsam/sfm/MFAS.h) on the device: computeOrdering / computeOutlierWeights for one projection direction or one map of edge
/// weights, and outlierWeightSums for many directions at once (what 1dSfM thresholds).  Ties go to the lowest key and an unordered pair
/// given twice is refused (lmgpu.h).
class GpuMFAS {
 public:
  using KeyPair = std::pair<Key, Key>;
  using TranslationEdges = std::vector<BinaryMeasurement<Unit3>>;

  GpuMFAS(const TranslationEdges& relativeTranslations, const Unit3& projectionDirection, int device = 0) : device_(device) {
    for (const auto& e : relativeTranslations) {
      pairs_.emplace_back(e.key1(), e.key2());
      const Point3 z = e.measured().point3();
      meas_.insert(meas_.end(), {z.x(), z.y(), z.z()});
    }
    const Point3 d = projectionDirection.point3();
    dirs_ = {d.x(), d.y(), d.z()};
  }
  explicit GpuMFAS(const std::map<KeyPair, double>& edgeWeights, int device = 0) : device_(device) {
    for (const auto& kw : edgeWeights) {
      pairs_.push_back(kw.first);
      weights_.push_back(kw.second);
    }
  }

  KeyVector computeOrdering() const {
    run();
    return KeyVector(order_.begin(), order_.end());
  }
  std::map<KeyPair, double> computeOutlierWeights() const {
    run();
    std::map<KeyPair, double> out;
    for (size_t e = 0; e < pairs_.size(); e++) out[pairs_[e]] = wout_[e];
    return out;
  }

  /// the per-edge sum of the outlier weights over `directions`, in the order of relativeTranslations
  static std::vector<double> outlierWeightSums(const TranslationEdges& relativeTranslations, const std::vector<Unit3>& directions, int device = 0) {
    GpuMFAS m(relativeTranslations, directions.empty() ? Unit3() : directions.front(), device);
    m.dirs_.clear();
    for (const Unit3& u : directions) {
      const Point3 d = u.point3();
      m.dirs_.insert(m.dirs_.end(), {d.x(), d.y(), d.z()});
    }
    std::vector<double> sum(m.pairs_.size());
    m.call(nullptr, nullptr, sum.data());
    return sum;
  }

 private:
  void call(uint64_t* order, double* wout, double* sum) const {
    std::vector<uint64_t> keys;
    for (const KeyPair& p : pairs_) keys.insert(keys.end(), {p.first, p.second});
    const bool given = !weights_.empty();
    const int32_t D = given ? 1 : static_cast<int32_t>(dirs_.size() / 3);
    const int rc = lmgpu_mfas_outlier_weights(device_, static_cast<int32_t>(pairs_.size()), keys.data(), given ? nullptr : meas_.data(), D,
                                              given ? nullptr : dirs_.data(), given ? weights_.data() : nullptr, order, wout, sum, nullptr);
    if (rc == LMGPU_INVALID) throw std::invalid_argument(std::string("GpuMFAS: ") + lmgpu_mfas_last_error());
    if (rc != LMGPU_OK) throw std::runtime_error(std::string("GpuMFAS: ") + lmgpu_mfas_last_error());
  }
  void run() const {
    if (!wout_.empty() || pairs_.empty()) return;
    KeySet nodes;
    for (const KeyPair& p : pairs_) {
      nodes.insert(p.first);
      nodes.insert(p.second);
    }
    order_.resize(nodes.size());
    wout_.resize(pairs_.size());
    call(order_.data(), wout_.data(), nullptr);
  }
  int device_;
  std::vector<KeyPair> pairs_;
  std::vector<double> meas_, dirs_, weights_;
  mutable std::vector<uint64_t> order_;
  mutable std::vector<double> wout_;
};

/// triangulateSafe(cameras, measured, params) (gtsam/geometry/triangulation.h:701-758) on the device, for CameraSet<PinholeCamera<Cal3Bundler>>
/// and CameraSet<PinholeCamera<Cal3_S2>>: call gtsam::gpuTriangulateSafe where the program called triangulateSafe.  The batched overload
/// triangulates landmark i from cameras[i] / measured[i] in one lmgpu_triangulate_batch call (one lane per landmark).
/// params.noiseModel: null, Unit or Isotropic; params.useLOST is refused (std::invalid_argument).  Where Cal3Bundler::calibrate does not
/// converge the reference lets a std::runtime_error escape triangulateSafe; so does this (status LMGPU_TRI_CALIBRATE_FAILED of the library).
namespace lmgpu_detail {

inline int32_t addCamera(lmgpu_adapter::TriangulationBatch* b, const PinholeCamera<Cal3Bundler>& c) {
  double pose[12];
  packPose3(c.pose(), pose);
  const Cal3Bundler& K = c.calibration();
  return b->addBundlerCamera(pose, K.fx(), K.k1(), K.k2(), K.px(), K.py());
}
inline int32_t addCamera(lmgpu_adapter::TriangulationBatch* b, const PinholeCamera<Cal3_S2>& c) {
  double pose[12];
  packPose3(c.pose(), pose);
  const Cal3_S2& K = c.calibration();
  return b->addS2Camera(pose, K.fx(), K.fy(), K.skew(), K.px(), K.py());
}
inline int32_t cameraModelOf(const Cal3Bundler*) { return 0; }
inline int32_t cameraModelOf(const Cal3_S2*) { return 1; }

inline lmgpu_triangulation_params toC(const TriangulationParameters& p) {  // triangulation.h:562-609
  if (p.useLOST) throw std::invalid_argument("gpuTriangulateSafe: useLOST is not bound");
  double inv_sigma = 0.0;
  if (p.noiseModel) {
    const auto iso = std::dynamic_pointer_cast<noiseModel::Isotropic>(p.noiseModel);
    if (!iso || iso->dim() != 2) throw std::invalid_argument("gpuTriangulateSafe: the noise model must be Unit or Isotropic of dimension 2");
    inv_sigma = 1.0 / iso->sigma();
  }
  return lmgpu_triangulation_params{p.rankTolerance, p.enableEPI ? 1 : 0, 0, p.landmarkDistanceThreshold, p.dynamicOutlierRejectionThreshold, inv_sigma};
}

inline TriangulationResult toTriangulationResult(int32_t status, const double* p) {
  switch (status) {
    case LMGPU_TRI_VALID: return TriangulationResult(Point3(p[0], p[1], p[2]));
    case LMGPU_TRI_DEGENERATE: return TriangulationResult::Degenerate();
    case LMGPU_TRI_BEHIND_CAMERA: return TriangulationResult::BehindCamera();
    case LMGPU_TRI_OUTLIER: return TriangulationResult::Outlier();
    case LMGPU_TRI_FAR_POINT: return TriangulationResult::FarPoint();
    default: throw std::runtime_error("Cal3Bundler::calibrate fails to converge. need a better initialization");
  }
}

}  // namespace lmgpu_detail

template <class CALIBRATION>
std::vector<TriangulationResult> gpuTriangulateSafe(const std::vector<CameraSet<PinholeCamera<CALIBRATION>>>& cameras,
                                                    const std::vector<Point2Vector>& measured, const TriangulationParameters& params,
                                                    int device = 0) {
  if (cameras.size() != measured.size()) throw std::invalid_argument("gpuTriangulateSafe: one measurement vector per camera set");
  lmgpu_adapter::TriangulationBatch batch(lmgpu_detail::cameraModelOf(static_cast<const CALIBRATION*>(nullptr)));
  for (size_t i = 0; i < cameras.size(); i++) {
    if (cameras[i].size() != measured[i].size()) throw std::invalid_argument("gpuTriangulateSafe: one measurement per camera");
    for (size_t k = 0; k < cameras[i].size(); k++) {
      const int32_t cam = lmgpu_detail::addCamera(&batch, cameras[i][k]);
      batch.addObservation(cam, measured[i][k].x(), measured[i][k].y());
    }
    batch.endLandmark();
  }
  std::vector<double> points;
  std::vector<int32_t> status;
  batch.run(device, lmgpu_detail::toC(params), &points, &status);
  std::vector<TriangulationResult> out;
  out.reserve(status.size());
  for (size_t i = 0; i < status.size(); i++) out.push_back(lmgpu_detail::toTriangulationResult(status[i], &points[3 * i]));
  return out;
}

template <class CALIBRATION>
TriangulationResult gpuTriangulateSafe(const CameraSet<PinholeCamera<CALIBRATION>>& cameras, const Point2Vector& measured,
                                       const TriangulationParameters& params, int device = 0) {
  return gpuTriangulateSafe<CALIBRATION>(std::vector<CameraSet<PinholeCamera<CALIBRATION>>>{cameras}, std::vector<Point2Vector>{measured}, params,
                                         device)[0];
}

}  // namespace gtsam
