/* lmgpu.h — C ABI of the MI355X-native Levenberg-Marquardt inner loop.
 *
 * Drop-in boundary for GTSAM's LM hot path (citations relative to the reference tree):
 *   - LevenbergMarquardtOptimizer::iterate()      gtsam/nonlinear/LevenbergMarquardtOptimizer.h:103, .cpp:273-308
 *   - LevenbergMarquardtOptimizer::linearize()    gtsam/nonlinear/LevenbergMarquardtOptimizer.h:113
 *   - NonlinearOptimizer::solve()                 gtsam/nonlinear/NonlinearOptimizer.h:129-130, .cpp:132-178
 *   - NonlinearFactorGraph::error()/linearize()   gtsam/nonlinear/NonlinearFactorGraph.cpp:170-179, 239-278
 *   - GaussianFactorGraph::optimize()             gtsam/linear/GaussianFactorGraph.cpp:316-319
 * The reference has no FFI of its own: its extension points are C++ virtuals.  INTEGRATION.md shows the
 * thin C++ adapter (a LevenbergMarquardtOptimizer subclass) that binds these entry points.
 *
 * Conventions: plain C, opaque handle, caller-owned host pointers with explicit counts, int status return,
 * no exceptions across the boundary.  One HIP stream per handle; a handle is not thread-safe; handles are
 * independent.  All arithmetic is IEEE double.  The library REQUIRES a HIP device: there is no CPU fallback.
 *
 * Variable order: lmgpu_set_variables() receives the variables in ELIMINATION order (the Ordering of
 * NonlinearOptimizerParams::ordering, gtsam/nonlinear/NonlinearOptimizerParams.h:47); the position in that
 * list is the variable's "slot".  Every packed per-variable vector crossing this boundary (values, delta,
 * hessian diagonal) is the concatenation over slots 0..n-1.
 */
#ifndef LMGPU_H
#define LMGPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lmgpu_handle lmgpu_handle;

enum lmgpu_status {
  LMGPU_OK = 0,
  LMGPU_INDETERMINATE = 1, /* IndeterminantLinearSystemException (gtsam/linear/linearExceptions.h); see lmgpu_last_failed_slot */
  LMGPU_INVALID = 2,       /* invalid argument / call order */
  LMGPU_HIP_ERROR = 3      /* HIP or RCCL runtime failure; see lmgpu_last_error */
};

/* Variable types.  dim = tangent dimension, store = doubles per packed value.
 *   POSE2       dim 3  store 3   (x, y, theta)                                   gtsam/geometry/Pose2.h
 *   POSE3       dim 6  store 12  (R row-major 9, t 3)   tangent (omega, v)       gtsam/geometry/Pose3.h
 *   POINT3      dim 3  store 3
 *   CAM_BUNDLER dim 9  store 15  (R 9, t 3, f, k1, k2)  PinholeCamera<Cal3Bundler>; tangent (omega, v, f, k1, k2).
 *               The constant principal point (u0, v0) of Cal3Bundler is folded into the measurement by the host
 *               (z' = z - (u0, v0)); Cal3Bundler::retract keeps it constant (gtsam/geometry/Cal3Bundler.h:134-136).
 *   POINT2      dim 2  store 2                           planar landmark (gtsam/geometry/Point2.h), vector retract
 *   CAL3_S2     dim 5  store 5   (fx, fy, s, u0, v0)     Cal3_S2 as a VARIABLE (gtsam/geometry/Cal3_S2.h:106-119: vector retract / local)
 *   VEC9        dim 9  store 9   nine scalars, vector retract: the relaxed rotation of the chordal initialisation, the 3x3 matrix
 *               column-major as in VectorValues of InitializePose3::buildLinearOrientationGraph (gtsam/slam/InitializePose3.cpp:37-71, 84)
 */
enum lmgpu_var_type {
  LMGPU_POSE2 = 0,
  LMGPU_POSE3 = 1,
  LMGPU_POINT3 = 2,
  LMGPU_CAM_BUNDLER = 3,
  LMGPU_POINT2 = 4,
  LMGPU_CAL3_S2 = 5,
  LMGPU_VEC9 = 6,
  LMGPU_NUM_VAR_TYPES = 7
};

/* Factor types ("buckets" are keyed by (factor type, noise kind) = fixed block shape).
 *   type             arity rows  measurement doubles
 *   SFM              2     2     2   z                         GeneralSFMFactor<PinholeCamera<Cal3Bundler>,Point3>  gtsam/slam/GeneralSFMFactor.h:141-177
 *   BETWEEN_POSE2    2     3     3   (x,y,theta)               BetweenFactor<Pose2>   gtsam/slam/BetweenFactor.h:111-124
 *   BETWEEN_POSE3    2     6     12  (R row-major, t)          BetweenFactor<Pose3>
 *   PRIOR_POSE2      1     3     3                             PriorFactor<Pose2>     gtsam/nonlinear/PriorFactor.h:98-102
 *   PRIOR_POSE3      1     6     12
 *   PRIOR_POINT3     1     3     3
 *   PRIOR_CAM        1     9     15  (R, t, f, k1, k2)         PriorFactor<PinholeCamera<Cal3Bundler>>
 *   PROJECTION       2     2     7   (z, fx, fy, s, u0, v0)    GenericProjectionFactor<Pose3,Point3,Cal3_S2>  gtsam/slam/ProjectionFactor.h:138-165
 *   PROJECTION_BPS   2     2     19  (z, K, body_P_sensor R t) the same with body_P_sensor (ProjectionFactor.h:142-149: camera =
 *                                                              pose.compose(body_P_sensor), H1 chained with AdjointMap(body_P_sensor^-1))
 *   BEARING_RANGE_2D 2     2     2   (bearing angle, range)    BearingRangeFactor<Pose2,Point2>  gtsam/sam/BearingRangeFactor.h:33-77:
 *                                                              error = (wrap(bearing - measured), range - measured) with Pose2::bearing /
 *                                                              Pose2::range and their Jacobians, gtsam/geometry/Pose2.cpp:283-330
 *   SFM2             3     2     2   z                         GeneralSFMFactor2<Cal3_S2> (Pose3, Point3, Cal3_S2)  gtsam/slam/GeneralSFMFactor.h:208-262:
 *                                                              PinholeCamera<Cal3_S2>(pose, K).project(point, H1, H2, H3) - z; a point behind
 *                                                              the camera gives zero error and zero Jacobians (:251-260)
 *   PRIOR_CAL3_S2    1     5     5   (fx, fy, s, u0, v0)       PriorFactor<Cal3_S2>
 *   CHORDAL_BETWEEN  2     9     9   Rij row-major             the JacobianFactor [-I9 | M9 | b = 0], M9 = blockdiag(Rij, Rij, Rij), of
 *                                                              InitializePose3::buildLinearOrientationGraph (gtsam/slam/InitializePose3.cpp:56-62)
 *                                                              on two VEC9: error = M9 x2 - x1.  Its Isotropic::Precision(9, p) is DIAG
 *                                                              noise with nine times sqrt(p); p = 0 is allowed (a factor of zero rows)
 *   PRIOR_VEC9       1     9     9   b                         the JacobianFactor [I9 | b] (the anchor's prior, :65-69): error = x - b
 * Keys of a factor: `arity` per factor, in the reference's key order.
 */
enum lmgpu_factor_type {
  LMGPU_F_SFM = 0,
  LMGPU_F_BETWEEN_POSE2 = 1,
  LMGPU_F_BETWEEN_POSE3 = 2,
  LMGPU_F_PRIOR_POSE2 = 3,
  LMGPU_F_PRIOR_POSE3 = 4,
  LMGPU_F_PRIOR_POINT3 = 5,
  LMGPU_F_PRIOR_CAM = 6,
  LMGPU_F_PROJECTION = 7,
  LMGPU_F_PROJECTION_BPS = 8,
  LMGPU_F_BEARING_RANGE_2D = 9,
  LMGPU_F_SFM2 = 10,
  LMGPU_F_PRIOR_CAL3_S2 = 11,
  LMGPU_F_CHORDAL_BETWEEN = 12,
  LMGPU_F_PRIOR_VEC9 = 13,
  LMGPU_NUM_FACTOR_TYPES = 14
};

/* Noise models (gtsam/linear/NoiseModel.cpp).  Per-factor noise data, `rows` = factor rows:
 *   UNIT   0 doubles
 *   DIAG   rows doubles: INVERSE sigmas (Isotropic = all equal)          whiten: v .* invsigma   (:314-332, :653-665)
 *   GAUSS  rows*rows doubles: sqrt information R, row-major              whiten: R v             (:160-186)
 */
enum lmgpu_noise_kind { LMGPU_N_UNIT = 0, LMGPU_N_DIAG = 2, LMGPU_N_GAUSS = 3 };

#define LMGPU_FLAG_SPLIT_ROOT 1
typedef struct lmgpu_config {
  int32_t device;     /* HIP device ordinal */
  int32_t rank;       /* this process' rank among the cooperating handles (0 if single) */
  int32_t world_size; /* number of cooperating ranks (1 if single) */
  int32_t flags;      /* bit 0 (LMGPU_FLAG_SPLIT_ROOT, testing aid): take the multi-rank data path for the HBM fronts (partial
                         assembly in its own buffer, chunked all-reduce on the communication stream, fold-in before each panel)
                         even with world_size == 1, so that a one-rank RCCL communicator exercises it on a single GPU */
} lmgpu_config;

/* LevenbergMarquardtParams subset honoured by lmgpu_iterate / lmgpu_optimize
 * (gtsam/nonlinear/LevenbergMarquardtParams.h:35-157; defaults = SetLegacyDefaults :69-82). */
typedef struct lmgpu_lm_params {
  int32_t maxIterations;
  double relativeErrorTol, absoluteErrorTol, errorTol;
  double lambdaInitial, lambdaFactor, lambdaUpperBound, lambdaLowerBound;
  double minModelFidelity;
  int32_t diagonalDamping, useFixedLambdaFactor;
  double minDiagonal, maxDiagonal;
} lmgpu_lm_params;

/* LevenbergMarquardtState (gtsam/nonlinear/internal/LevenbergMarquardtState.h:42-68) */
typedef struct lmgpu_lm_state {
  double error;
  double lambda;
  double currentFactor;
  int32_t iterations;
  int32_t totalNumberInnerIterations;
} lmgpu_lm_state;

/* per-phase device time of the last lmgpu_iterate, milliseconds (HIP events on the handle's stream) */
typedef struct lmgpu_timings {
  double linearize_ms, eliminate_ms, backsub_ms, linear_error_ms, retract_error_ms, total_ms;
  int32_t inner_iterations;
} lmgpu_timings;

/* ---- lifetime ---- */
int lmgpu_create(const lmgpu_config* cfg, lmgpu_handle** out);
int lmgpu_destroy(lmgpu_handle* h);
const char* lmgpu_last_error(const lmgpu_handle* h);
int lmgpu_last_failed_slot(const lmgpu_handle* h); /* slot of the first frontal variable of the failing front */

/* ---- structure (once per graph + ordering; replaces the symbolic work eliminateMultifrontal redoes per solve,
 *      gtsam/inference/EliminateableFactorGraph-inst.h:123-146) ---- */
int lmgpu_set_variables(lmgpu_handle* h, int32_t n_vars, const uint64_t* keys, const int32_t* types);
/* graph_index[i] = index of factor i in the NonlinearFactorGraph (defines VariableIndex order and error-sum order);
 * var_slots: n x arity slots; meas: n x measurement doubles; noise: n x noise doubles (NULL for UNIT). */
int lmgpu_add_factor_bucket(lmgpu_handle* h, int32_t factor_type, int32_t n, const int32_t* graph_index, const int32_t* var_slots,
                            const double* meas, int32_t noise_kind, const double* noise);
/* The same with a noiseModel::Robust wrapped around the Gaussian model of every factor of the bucket
 * (gtsam/linear/NoiseModel.h:663-760): linearize multiplies the whitened [A b] of a factor by sqrt(weight(||b||))
 * (Robust::WhitenSystem NoiseModel.cpp:705-723 -> mEstimator::Base::reweight, Block scheme, LossFunctions.cpp:61-76) and the
 * factor's error is loss(||whitened error||) (NoiseModel.h:717-725).  robust_k = the m-estimator's tuning constant. */
enum lmgpu_robust_kind {
  LMGPU_ROBUST_NONE = 0,
  LMGPU_ROBUST_FAIR = 1,           /* LossFunctions.cpp:146-155 */
  LMGPU_ROBUST_HUBER = 2,          /* :179-191 */
  LMGPU_ROBUST_CAUCHY = 3,         /* :217-224 */
  LMGPU_ROBUST_TUKEY = 4,          /* :250-266 */
  LMGPU_ROBUST_WELSCH = 5,         /* :289-297 */
  LMGPU_ROBUST_GEMAN_MCCLURE = 6,  /* :320-331 */
  LMGPU_ROBUST_DCS = 7,            /* :354-373 */
  LMGPU_ROBUST_L2_WITH_DEAD_ZONE = 8 /* :400-412 */
};
int lmgpu_add_factor_bucket_robust(lmgpu_handle* h, int32_t factor_type, int32_t n, const int32_t* graph_index, const int32_t* var_slots,
                                   const double* meas, int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k);
int lmgpu_finalize_structure(lmgpu_handle* h);

/* ---- values ---- */
int lmgpu_set_values(lmgpu_handle* h, const double* packed_values);
int lmgpu_get_values(lmgpu_handle* h, double* packed_values);
/* device-side snapshot / restore of the values (e.g. keep the initial estimate around to restart an optimisation) */
int lmgpu_save_values(lmgpu_handle* h);
int lmgpu_restore_values(lmgpu_handle* h);
int lmgpu_total_dim(const lmgpu_handle* h);   /* sum of tangent dims */
int lmgpu_total_store(const lmgpu_handle* h); /* doubles in packed values */

/* ---- the hot path, piecewise (what LevenbergMarquardtOptimizer::tryLambda calls) ---- */
int lmgpu_error(lmgpu_handle* h, double* total);  /* NonlinearFactorGraph::error at the current values */
int lmgpu_linearize(lmgpu_handle* h);             /* NonlinearFactorGraph::linearize -> device-resident whitened [A|b] per factor */
/* buildDampedSystem + solve + linear.error(0), linear.error(delta).  delta_packed may be NULL. */
int lmgpu_solve(lmgpu_handle* h, double lambda, int32_t diagonal_damping, double min_diag, double max_diag, double* delta_packed,
                double* lin_err0, double* lin_err1);
int lmgpu_retract(lmgpu_handle* h, const double* delta_packed); /* values <- values.retract(delta); NULL = last solve's delta */
int lmgpu_hessian_diagonal(lmgpu_handle* h, double* diag_packed); /* GaussianFactorGraph::hessianDiagonal */

/* ---- the hot path, whole (drop-in for LevenbergMarquardtOptimizer::iterate / NonlinearOptimizer::optimize) ---- */
int lmgpu_lm_init(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* state_out);
int lmgpu_iterate(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout);
int lmgpu_optimize(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout);

/* GaussNewtonOptimizer::iterate (gtsam/nonlinear/GaussNewtonOptimizer.cpp:44-66) on the same device-resident graph:
 * linearize, solve the undamped system, retract, error of the new values; state->error / iterations are updated, lambda
 * is not used.  LMGPU_INDETERMINATE where the reference throws IndeterminantLinearSystemException.
 * lmgpu_gn_optimize = NonlinearOptimizer::defaultOptimize (NonlinearOptimizer.cpp:62-117) around it; of `p` only
 * maxIterations and the three error tolerances are read (NonlinearOptimizerParams). */
int lmgpu_gn_iterate(lmgpu_handle* h, lmgpu_lm_state* inout);
int lmgpu_gn_optimize(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout);

/* DoglegOptimizer::iterate (gtsam/nonlinear/DoglegOptimizer.cpp:84-126, multifrontal elimination, ONE_STEP_PER_ITERATION as there;
 * DoglegOptimizerImpl.h:139-254, DoglegOptimizerImpl.cpp:26-91): undamped solve, steepest-descent point from the Bayes tree
 * (GaussianFactorGraph::optimizeGradientSearch, GaussianFactorGraph.cpp:381-406), dogleg point inside the trust region, gain
 * ratio rho = (f(x) - f(x + dx_d)) / (M(0) - M(dx_d)) with M the Bayes tree's error, radius update.  The trust radius travels in
 * state->lambda (initialise it to DoglegParams::deltaInitial, default 1.0; state->error as for LM).  Single-rank. */
int lmgpu_dl_iterate(lmgpu_handle* h, lmgpu_lm_state* inout);
int lmgpu_dl_optimize(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout);
int lmgpu_get_timings(const lmgpu_handle* h, lmgpu_timings* out);

/* Read-only tap on the two products DoglegOptimizer takes with the Bayes tree of the last solve, read as a GaussianFactorGraph of
 * unit-noise Jacobian factors [R S | d], one per clique (gtsam/linear/GaussianBayesTree.cpp:73-92): gradient_packed (if not NULL) =
 * - sum_c [R S]^T d (GaussianFactorGraph::gradientAtZero, GaussianFactorGraph.cpp:369-378); *sq_norm (if x_packed and sq_norm are not
 * NULL) = sum_c ||[R S] x - alpha d||^2.  Vectors are packed by slot like lmgpu_solve's delta_packed.  Needs a finalized single-rank
 * handle of the direct solver that has solved (else LMGPU_INVALID); the step, the values and the LM / Dogleg state are not touched. */
int lmgpu_bt_products(lmgpu_handle* h, const double* x_packed, double alpha, double* sq_norm, double* gradient_packed);

/* ---- linear solver: NonlinearOptimizerParams::linearSolverType (gtsam/nonlinear/NonlinearOptimizerParams.h; dispatch
 *      NonlinearOptimizer.cpp:154-173).  LMGPU_SOLVER_PCG = Iterative with PCGSolverParameters (gtsam/linear/PCGSolver.h:36-50):
 *      preconditionedConjugateGradient (gtsam/linear/ConjugateGradientSolver.h:109-171) on A = sum J^T J + lambda D, b = -gradientAtZero
 *      (GaussianFactorGraphSystem, PCGSolver.cpp:69-145), from x = 0 (IterativeSolver.cpp:92-102).  Preconditioners
 *      (Preconditioner.cpp:80-177): DUMMY = identity; BLOCK_JACOBI = per variable L = chol(H_jj) of the DAMPED graph's
 *      hessianBlockDiagonal, left L^-1 x, right L^-T x.  Deviation: a diagonal block that is not positive definite returns
 *      LMGPU_INDETERMINATE with lmgpu_last_failed_slot = that variable (the reference carries Eigen's failed LLT on silently).
 *      Reaching maxIterations is not an error (the estimate so far is the step).  lmgpu_solve, lmgpu_iterate, lmgpu_optimize,
 *      lmgpu_gn_iterate and lmgpu_gn_optimize honour the selection; lmgpu_dl_* return LMGPU_INVALID under PCG (the reference throws,
 *      DoglegOptimizer.cpp:108-113); so does world_size > 1.  ISAM2 is not affected.
 *      Selected BEFORE lmgpu_finalize_structure, PCG skips the symbolic analysis and all front memory: the handle has no fronts
 *      (lmgpu_num_fronts 0; lmgpu_get_front, the marginal covariances and switching back to Cholesky return LMGPU_INVALID).
 *      A handle finalized for Cholesky may switch to PCG and back.  Time of a PCG solve is booked as eliminate_ms (backsub_ms 0); its
 *      launches carry no lmgpu_set_kernel_timing events (no category of lmgpu_kernel_category fits them, and LMGPU_KT_NUM stays as it
 *      is): their device time is in lmgpu_get_pcg_stats (precond_ms, iterate_ms), per kernel with rocprofv3. */
enum lmgpu_linear_solver { LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY = 0, LMGPU_SOLVER_PCG = 1 };
enum lmgpu_preconditioner { LMGPU_PRECOND_DUMMY = 0, LMGPU_PRECOND_BLOCK_JACOBI = 1 };
/* ConjugateGradientParameters (ConjugateGradientSolver.h:34-50; defaults min 1, max 500, reset 501, eps_rel 1e-3, eps_abs 1e-3) */
typedef struct lmgpu_pcg_params {
  int32_t preconditioner, minIterations, maxIterations, reset; /* reset >= 1: every reset-th iteration recomputes r = b - A x */
  double epsilon_rel, epsilon_abs;
} lmgpu_pcg_params;
/* pcg may be NULL for LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY */
int lmgpu_set_linear_solver(lmgpu_handle* h, int32_t solver, const lmgpu_pcg_params* pcg);
/* of the last PCG solve: iterations = loop bodies executed; host_waits = host synchronisations of the solve (one per 16 iterations
 * queued + one at the end); gamma0 = |L^-1 b|^2, gamma = |r|^2 at exit, threshold = max(eps_abs, eps_rel^2 gamma0);
 * precond_ms = block diagonal + its Cholesky, iterate_ms = the loop (device time, HIP events).  LMGPU_INVALID before the first. */
typedef struct lmgpu_pcg_stats {
  int32_t iterations, host_waits;
  double gamma0, gamma, threshold, precond_ms, iterate_ms;
} lmgpu_pcg_stats;
int lmgpu_get_pcg_stats(const lmgpu_handle* h, lmgpu_pcg_stats* out);

/* ---- GNC: GncOptimizer<GncParams<LevenbergMarquardtParams | GaussNewtonParams>> (gtsam/nonlinear/GncOptimizer.h, GncParams.h) on the
 *      device-resident graph.  Graduated non-convexity is an outer loop around the base optimizer: per outer iteration every factor gets a
 *      weight w_k in [0, 1] from its unweighted error r_k at the last result, and the base optimizer runs again FROM THE INITIAL VALUES on
 *      the graph whose factor k has the information w_k * information_k (makeWeightedGraph :396-416).  Here the weight lives in the factor
 *      kernels: linearize multiplies the whitened [A b] of factor k by sqrt(w_k), the factor's error is w_k * 0.5 ||whitened e||^2, and a
 *      bucket's noiseModel::Robust is ignored while GNC is enabled (the constructor strips it, :63-73).  The graph structure does not
 *      change under reweighting, so the symbolic analysis, the plan and all front memory are reused by every outer iteration; the weight,
 *      error, threshold and known-inlier / known-outlier vectors stay in device memory except in the explicit get / set calls.
 *      For GAUSS noise the reference re-factors w * information into a new R', which differs from sqrt(w) R by an orthogonal factor: a
 *      factor's [A b] is not a parity quantity there; A^T A, A^T b, the error, the step and the values are.
 *      A weight of 0 removes the factor; if that leaves a variable unconstrained the solve returns LMGPU_INDETERMINATE like any singular
 *      system (the reference throws in the same place).
 *      Boundary vectors (weights, thresholds) have graph_size = nfg_.size() entries indexed by the factor's graph index (`graph_index` of
 *      lmgpu_add_factor_bucket); a slot of the graph that holds no factor reads as weight 1 / threshold 1 and takes part in no reduction.
 *      Single rank (world_size > 1: LMGPU_INVALID); Cholesky and PCG alike (the weights act in linearize and error); ISAM2 is not affected.
 *      While enabled, lmgpu_error, lmgpu_linearize, lmgpu_lm_init, lmgpu_iterate, lmgpu_gn_iterate, ... act on the weighted graph with the
 *      current weights; a change of the weights (set_weights, set_known, calculate_weights, enable) invalidates the stored linearization
 *      (lmgpu_solve and lmgpu_get_jacobian(s) refuse until the next lmgpu_linearize); lmgpu_gnc_enable(h, 0, 0) returns the handle to exactly its behaviour without GNC.  Every other lmgpu_gnc_* call
 *      on a handle without GNC enabled returns LMGPU_INVALID. */
enum lmgpu_gnc_loss { LMGPU_GNC_GM = 0, LMGPU_GNC_TLS = 1 };    /* GncLossType, GncParams.h:36-39 */
enum lmgpu_gnc_base { LMGPU_GNC_BASE_LM = 0, LMGPU_GNC_BASE_GN = 1 };
typedef struct lmgpu_gnc_params { /* GncParams.h:66-81; defaults TLS, 100, 1.4, 1e-5, 1e-4 */
  int32_t lossType, maxIterations, baseOptimizer;
  double muStep, relativeCostTol, weightsTol;
} lmgpu_gnc_params;
typedef struct lmgpu_gnc_result {
  int32_t iterations;            /* `iter` at the exit of the loop GncOptimizer.h:218-257 */
  int32_t stop;                  /* 0 maxIterations, 1 cost, 2 weights, 3 mu, 4 mu <= 0 at initialisation, 5 nothing unknown */
  double mu, cost, prev_cost;
  int32_t base_iterations_total; /* sum of the base optimizer's iterations over all its runs */
} lmgpu_gnc_result;
/* Chi2inv (GncOptimizer.h:38-40): the alpha quantile of the chi-square distribution with `dofs` degrees of freedom, MATLAB's chi2inv.
 * Host code, no device: regularised incomplete gamma function + Newton inside a bisection bracket.  NaN for alpha outside [0, 1). */
double lmgpu_chi2inv(double alpha, int32_t dofs);
/* on != 0: the constructor's state (GncOptimizer.h:100-106): allocate the weight, threshold and mask vectors; weights 1; thresholds
 * 0.5 * chi2inv(0.99, rows of the factor); no known inliers / outliers.  graph_size = nfg_.size() (> every graph_index; 0: the largest
 * graph_index + 1).  on == 0: drop them.  After lmgpu_finalize_structure. */
int lmgpu_gnc_enable(lmgpu_handle* h, int32_t on, int32_t graph_size);
/* setInlierCostThresholds(Vector) (:123-125; n must equal graph_size, :142-149 style check) or, with barcSq == NULL,
 * setInlierCostThresholdsAtProbability(alpha) (:130-137) */
int lmgpu_gnc_set_inlier_cost_thresholds(lmgpu_handle* h, int32_t n, const double* barcSq, double alpha);
/* GncParams::knownInliers / knownOutliers (GncParams.h:78-81) with the constructor's checks (GncOptimizer.h:75-99): an index in both
 * lists or outside the graph is LMGPU_INVALID.  Resets the weights to initializeWeightsFromKnownInliersAndOutliers (:174-180). */
int lmgpu_gnc_set_known(lmgpu_handle* h, int32_t n_in, const uint64_t* inliers, int32_t n_out, const uint64_t* outliers);
int lmgpu_gnc_set_weights(lmgpu_handle* h, int32_t n, const double* w); /* setWeights :142-149: n != graph_size is LMGPU_INVALID */
int lmgpu_gnc_get_weights(lmgpu_handle* h, int32_t n, double* w);       /* getWeights :161 */
int lmgpu_gnc_get_inlier_cost_thresholds(lmgpu_handle* h, int32_t n, double* barcSq); /* getInlierCostThresholds :164 */
/* initializeMu (:272-314) with the factor errors at the handle's CURRENT values (the reference evaluates at state_) */
int lmgpu_gnc_initialize_mu(lmgpu_handle* h, int32_t lossType, double* mu);
/* weights_ = calculateWeights(current values, mu) (:419-469) */
int lmgpu_gnc_calculate_weights(lmgpu_handle* h, int32_t lossType, double mu);
/* GncOptimizer::optimize() (:183-269).  state_ = the handle's values at the call (kept with lmgpu_save_values, which this call
 * overwrites).  initializeMu at state_; base optimizer from state_ on the graph with the current weights; prev_cost = its final error;
 * the two early exits (mu <= 0, nothing unknown); then per outer iteration: calculateWeights at the result, values back to state_, base
 * optimizer with a FRESH state (lmgpu_lm_init: lambda back to lambdaInitial), cost = its final error, checkConvergence (cost, then
 * weights, then mu; :389-393), updateMu.  On return the handle's values are the result, lmgpu_gnc_get_weights the last weights,
 * *base_state_out (may be NULL) the state of the last base optimizer run.  A failing base optimizer's status is returned as it is.
 * `base` = its parameters; for LMGPU_GNC_BASE_GN only maxIterations and the three tolerances are read.
 * Host synchronisations per outer iteration beyond the base optimizer's own (its constructor's error evaluation and its loop): NONE --
 * the weight update is queued in front of the base optimizer and the one scalar checkWeightsConvergence needs (max |w - round(w)|)
 * arrives under the base optimizer's first wait.  Before the loop: one (initializeMu's scalar) + the copy of lmgpu_save_values. */
int lmgpu_gnc_optimize(lmgpu_handle* h, const lmgpu_gnc_params* params, const lmgpu_lm_params* base, lmgpu_lm_state* base_state_out,
                       lmgpu_gnc_result* out);
/* per outer iteration of the last lmgpu_gnc_optimize, 6 doubles: mu used, cost, max |w - round(w)|, device ms of the weight update (error
 * kernels + weights + reduction, HIP events), host wall-clock ms of the base optimizer run (it starts the moment the weight update is
 * queued, without a wait, so it CONTAINS the weight update's device time of the column before), its iterations.  Returns the number of outer iterations
 * recorded (rows6 may be NULL; at most max_rows rows are written). */
int lmgpu_gnc_get_trace(const lmgpu_handle* h, int32_t max_rows, double* rows6);

/* ---- NonlinearConjugateGradientOptimizer (gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h, .cpp) on the device-resident graph:
 *      the one optimizer that needs no factorisation.  It works on a handle finalized for Cholesky or under LMGPU_SOLVER_PCG alike (the
 *      selection is not read) and on every factor type, robust noise included: it uses the linearize and error launches that exist.
 *        System::error    = graph.error                                        (.cpp:51-54)        lmgpu_error
 *        System::gradient = graph.linearize(values)->gradientAtZero()          (.cpp:37-42, 56-60) lmgpu_gradient: -sum_f A_f^T b_f of the
 *                           whitened, robust-reweighted [A b] of lmgpu_linearize, per scalar in a fixed order (bitwise reproducible)
 *        System::advance  = values.retract(alpha * g)                          (.cpp:62-69)
 *        lineSearch       golden section on [-1 / |direction|, 0], tau = 1e-5  (.h:135-181)
 *        nonlinearConjugateGradient                                            (.h:195-289): early exit error <= errorTol; one gradient-
 *                           descent step before the loop that is not counted; beta by enum lmgpu_ncg_direction: FletcherReeves .h:28-36,
 *                           PolakRibiere :38-47, HestenesStiefel :49-59, DaiYuan :61-70; or direction = gradient with gradient_descent;
 *                           direction = gradient + beta * direction; loop while ++iteration < maxIterations && !checkConvergence
 *      The bracket of the line search lives in device memory and each trial (scaled retract, error, one-thread update rule) reads its
 *      step there: per NCG iteration the host queues linearize, gradient, direction update, 40 trials (every kernel of a trial behind the exit
 *      test returns at once), the final advance and its error, and waits ONCE; a search that needs more trials costs one wait per further 44,
 *      and one that has not met the exit test after 128 trials returns LMGPU_HIP_ERROR with a message (the reference would still loop).
 *      Refused with LMGPU_INVALID and a message: a handle with GNC enabled, a handle with a communicator (multi-rank), a call before
 *      lmgpu_set_values.  ISAM2 is not affected.
 *   lmgpu_gradient          gradientAtZero at the current values, lmgpu_total_dim doubles, tangent-packed by slot
 *   lmgpu_ncg_line_search   lineSearch from the current values along dir_packed (NULL: the gradient at the current values); the handle's
 *                           values are left unchanged.  *trials = error evaluations of the search.
 *                           A search that has not met the exit test after 128 evaluations returns LMGPU_HIP_ERROR after three waits;
 *                           lmgpu_last_error names |direction| and the bracket, *alpha and *trials are not written, the values are
 *                           unchanged and the handle stays usable.  This happens when the minimiser of the bracket is step 0 AND the error
 *                           resolves ever smaller steps (values at 0 moved along the direction), and for an all-zero direction
 *                           (|direction| = 0: the bracket is [-inf, 0], every step and every error NaN).  An ascent direction on
 *                           ordinary values does end, with an alpha of no effect: once the steps fall below the spacing of the values
 *                           the errors tie, the tie moves maxStep off 0 and the exit test is met (about 100 evaluations).
 *   lmgpu_ncg_iterate       NonlinearConjugateGradientOptimizer::iterate (.cpp:71-80): nonlinearConjugateGradient with singleIteration, i.e.
 *                           a gradient-descent step and ONE conjugate step, started over at every call; state: error, iterations + 1
 *   lmgpu_ncg_optimize      optimize (.cpp:82-90): the full loop; state: error, iterations = the loop's count
 *   lmgpu_ncg_get_trace     per line search of the last of the three calls above, 4 doubles: alpha, beta (0 where the direction is the
 *                           gradient), error after the advance (lmgpu_ncg_line_search: the best error the search saw), trials.  Row 0 of
 *                           an iterate / optimize is the uncounted gradient-descent step.  Returns the number of rows recorded.
 *   lmgpu_ncg_host_waits    host synchronisations of the last of those calls (the constructor-style error evaluation included) */
enum lmgpu_ncg_direction {
  LMGPU_NCG_FLETCHER_REEVES = 0,
  LMGPU_NCG_POLAK_RIBIERE = 1, /* the reference's default */
  LMGPU_NCG_HESTENES_STIEFEL = 2,
  LMGPU_NCG_DAI_YUAN = 3
};
typedef struct lmgpu_ncg_params { /* NonlinearOptimizerParams defaults: 100, 1e-5, 1e-5, 0 */
  int32_t direction_method, gradient_descent, max_iterations;
  double relative_error_tol, absolute_error_tol, error_tol;
} lmgpu_ncg_params;
int lmgpu_gradient(lmgpu_handle* h, double* g_packed);
int lmgpu_ncg_line_search(lmgpu_handle* h, const double* dir_packed, double* alpha, int32_t* trials);
int lmgpu_ncg_iterate(lmgpu_handle* h, const lmgpu_ncg_params* p, lmgpu_lm_state* inout);
int lmgpu_ncg_optimize(lmgpu_handle* h, const lmgpu_ncg_params* p, lmgpu_lm_state* inout);
int lmgpu_ncg_get_trace(const lmgpu_handle* h, int32_t max_rows, double* rows4);
int lmgpu_ncg_host_waits(const lmgpu_handle* h);

/* ---- InitializePose3 (gtsam/slam/InitializePose3.h, InitializePose3.cpp, InitializePose.h): initial estimate of a 3D pose graph on the
 *      device -- chordal relaxation or the Tron-Vidal gradient iteration for the rotations, then one Gauss-Newton step for the poses.
 *      An lmgpu_init_pose3 owns two lmgpu_handles over the same slots: the ORIENTATION handle (VEC9 variables, CHORDAL_BETWEEN factors,
 *      the anchor's PRIOR_VEC9; zero values, so the step of its lambda = 0 solve IS the relaxed solution) and the POSE handle (POSE3
 *      variables, the extracted pose graph + the anchor's Unit(6) prior).  Rotations cross the boundary as n x 9 doubles, row-major 3x3,
 *      poses as n x 12 (lmgpu.h POSE3 packing), both in the order of the `ordering` given to lmgpu_init_pose3_finalize with the anchor
 *      left out.  The rotations of the last orientation call stay in device memory: lmgpu_init_pose3_compute_poses(R = NULL) reads them
 *      there, so lmgpu_init_pose3_initialize moves nothing but its result through the host.
 *   lmgpu_init_pose3_add_factors   initialize::buildPoseGraph<Pose3> (InitializePose.h:36-52): LMGPU_F_BETWEEN_POSE3 factors are kept,
 *        LMGPU_F_PRIOR_POSE3 factors become between factors from LMGPU_INIT_POSE3_ANCHOR_KEY (kAnchorKey, :30), every other factor type
 *        is dropped silently.  keys: n x arity Keys; meas / noise as in lmgpu_add_factor_bucket; graph_index = the factor's index in the
 *        caller's NonlinearFactorGraph: the extracted graph keeps that order (createSymbolicGraph's factorId, InitializePose3.cpp:221-253).
 *        rotationPrecision p (:48-51) = first entry of noiseModel->whitenInPlace(e1): UNIT 1, DIAG invsigma[0] (so Isotropic 1 / sigma),
 *        GAUSS R[0][0] of the square-root information.
 *   lmgpu_init_pose3_finalize      ordering = the pose keys in elimination order (a boundary input like everywhere in this library); it
 *        may contain the anchor key to place it, otherwise the anchor is eliminated last.  Refused with LMGPU_INVALID BEFORE anything is
 *        built: no Pose3 between factor, a key of `ordering` without a factor in the extracted graph, a factor key missing from
 *        `ordering`, duplicate keys.  The object stays usable for further lmgpu_init_pose3_add_factors / another finalize.
 *   lmgpu_init_pose3_orientations_chordal   computeOrientationsChordal (:102-114): linear solve at lambda = 0 (the linear solver selected
 *        with lmgpu_set_linear_solver on the orientation handle: Cholesky or PCG), then normalizeRelaxedRotations (:75-92) as one kernel,
 *        one thread per pose, on the solve's step vector in device memory: SO3::ClosestTo (gtsam/geometry/SO3.cpp:202-208) of the
 *        transposed relaxed matrix by a one-sided Jacobi SVD in FP64.  LMGPU_INDETERMINATE where GaussianFactorGraph::optimize throws.
 *   lmgpu_init_pose3_closest_rotations      the same kernel on n caller-supplied relaxed 9-vectors (normalizeRelaxedRotations on its own)
 *   lmgpu_init_pose3_orientations_gradient  computeOrientationsGradient (:117-218) with gradientTron (:256-275): guess_R = the rotations of
 *        givenGuess (one per pose), maxIter (the reference's default: 10000), setRefFrame.  One thread per node, CSR adjacency in
 *        factor-index order, two rotation buffers, max-norm by block partials (no floating-point atomics).  The stop rule
 *        `it > 20 && maxGrad < 5e-3` is evaluated on the device at the head of the next iteration's kernel, which then does nothing:
 *        the host looks at the loop state once per 128 queued iterations, and the result is that of the reference's stopping iteration.
 *        *iterations = loop bodies executed, *max_grad = maxGrad of the last one.  Needs at least one prior (the reference's
 *        adjEdgesMap.at(kAnchorKey) throws without): LMGPU_INVALID otherwise.
 *   lmgpu_init_pose3_compute_poses          initialize::computePoses<Pose3> (InitializePose.h:57-97): poses (R, 0), anchor at the identity
 *        with a Unit(6) prior, GaussNewtonOptimizer with maxIterations = 1 (single_iter != 0) or NonlinearOptimizerParams' defaults;
 *        gn_state_out (may be NULL) = the optimizer's final state.  R = NULL: the rotations of the last orientation call.
 *   lmgpu_init_pose3_initialize             InitializePose3::initialize(graph, givenGuess, useGradient) (:296-314); guess_R may be NULL
 *        for use_gradient == 0.
 *   lmgpu_init_pose3_handle                 which = 0 orientation, 1 pose handle (owned by the object; for the parity taps, lmgpu_error,
 *        lmgpu_set_linear_solver, lmgpu_get_pcg_stats).  Slots = positions in lmgpu_init_pose3_get_slots' key list. */
#define LMGPU_INIT_POSE3_ANCHOR_KEY 99999999ull
typedef struct lmgpu_init_pose3 lmgpu_init_pose3;
int lmgpu_init_pose3_create(const lmgpu_config* cfg, lmgpu_init_pose3** out);
int lmgpu_init_pose3_destroy(lmgpu_init_pose3* ip);
const char* lmgpu_init_pose3_last_error(const lmgpu_init_pose3* ip);
int lmgpu_init_pose3_add_factors(lmgpu_init_pose3* ip, int32_t factor_type, int32_t n, const int32_t* graph_index, const uint64_t* keys,
                                 const double* meas, int32_t noise_kind, const double* noise);
int lmgpu_init_pose3_finalize(lmgpu_init_pose3* ip, int32_t n_order, const uint64_t* ordering);
int lmgpu_init_pose3_num_poses(const lmgpu_init_pose3* ip);   /* keys of the extracted graph without the anchor; -1 before finalize */
int lmgpu_init_pose3_num_factors(const lmgpu_init_pose3* ip); /* factors of the extracted pose graph (anchor priors not counted) */
int lmgpu_init_pose3_get_slots(const lmgpu_init_pose3* ip, uint64_t* keys_out); /* the handles' variables by slot, anchor included; returns their number */
lmgpu_handle* lmgpu_init_pose3_handle(lmgpu_init_pose3* ip, int32_t which);
int lmgpu_init_pose3_orientations_chordal(lmgpu_init_pose3* ip, double* R_out);
int lmgpu_init_pose3_closest_rotations(int32_t device, int32_t n, const double* relaxed9, double* R_out);
int lmgpu_init_pose3_orientations_gradient(lmgpu_init_pose3* ip, const double* guess_R, int32_t max_iter, int32_t set_ref_frame, double* R_out,
                                           int32_t* iterations, double* max_grad);
int lmgpu_init_pose3_compute_poses(lmgpu_init_pose3* ip, const double* R, int32_t single_iter, double* poses_out, lmgpu_lm_state* gn_state_out);
int lmgpu_init_pose3_initialize(lmgpu_init_pose3* ip, const double* guess_R, int32_t use_gradient, double* poses_out);

/* ---- TranslationRecovery (gtsam/sfm/TranslationRecovery.{h,cpp}, TranslationFactor.h): positions from relative translation DIRECTIONS ----
 * A session object like lmgpu_init_pose3: it owns one inner lmgpu_handle whose variables are all LMGPU_POINT3.  Its two factor kinds,
 * TranslationFactor (e = normalize(Tb - Ta) - z) and BetweenFactor<Point3> (e = (Tb - Ta) - z), are INTERNAL rows of the library's
 * factor-type table: lmgpu_factor_type keeps its 14 entries and every lmgpu_add_factor_bucket* / ISAM2 / init_pose3 entry point keeps
 * refusing type >= LMGPU_NUM_FACTOR_TYPES.  Coincident translations (Tb == Ta) of a TranslationFactor are OUTSIDE THE CONTRACT: the
 * reference's normalize has no guard for them and neither has the kernel (the error and the Jacobian are then not finite).
 *   create          cfg->world_size > 1 is refused (multi-rank is out of scope).  cfg->device < 0: the host logic only (finalize, get_keys,
 *                   get_initial work; run returns LMGPU_HIP_ERROR).
 *   add_directions  n edges (keys[2 i], keys[2 i + 1]) with measured unit direction dirs[3 i ..] and one noise model: noise_kind / noise as
 *                   in lmgpu_add_factor_bucket (3 inverse sigmas, or R row-major 3 x 3), robust_kind / robust_k as in
 *                   lmgpu_add_factor_bucket_robust.  index[i] = the edge's position in the caller's list of relativeTranslations: the
 *                   calls group edges by noise model, the list order decides "the first edge" and the order of first appearance.
 *   add_betweens    the same for betweenTranslations (meas = the Point3 measurement).
 *   set_prior_sigma addPrior's priorNoiseModel = Isotropic(3, sigma); default 0.01.
 *   seed            the session's 32-bit Mersenne Twister (seeded 42 at create).  DEVIATION: the reference's generator is process-wide.
 *   finalize        TranslationRecovery::run up to the optimizer (:191-223):
 *                   - nodes joined by an edge whose measured direction is (0, 0, 0) -- every component within 1e-9 of zero, the default
 *                     tolerance of Unit3::equals -- are merged; the representative of a set is its
 *                     SMALLEST key (DEVIATION from DSFMap's root; the results are the same); edges inside a set are dropped;
 *                   - graph: one TranslationFactor per remaining direction edge, PRIOR_POINT3 at 0 on the first remaining edge's key1, then
 *                     without betweens PRIOR_POINT3 at scale * z on its key2 with that edge's model, else one BetweenFactor<Point3> each.
 *                     Without a remaining direction edge the graph is EMPTY (addPrior returns at once, :125-126) and run returns the
 *                     initial values;
 *                   - initial values: init_keys / init_vals (n_init x 3) where given, else three draws per node in initializeRandomly's
 *                     order of first appearance, each coordinate 2 ((x1 + x2 2^32) / 2^64) - 1 from two consecutive 32-bit draws; no
 *                     remaining edge but zero-direction edges: every representative at the origin (:218-223);
 *                   - ordering (n_order keys, a boundary input over the ORIGINAL keys; non-representatives are ignored; n_order = 0:
 *                     first appearance).  LMGPU_INVALID, nothing changed: duplicate index, duplicate key in the ordering, a variable
 *                     missing from it, a merged set without any remaining edge (the reference throws there), a key that appears only
 *                     in between-translations whose two ends are the same node (the reference returns no value for it).  A failure
 *                     while the inner handle is built leaves the session unfinalized; the generator advances only on success.
 *   run             lmgpu_optimize on the inner handle from the initial values with the caller's LM parameters, direct solver (PCG selected
 *                   on the inner handle: LMGPU_INVALID); merged-away nodes then receive their representative's value.
 *   get_keys        every key of the input by first appearance with its representative; get = the result in that order (n x 3);
 *                   get_slots = the inner handle's variables by slot; get_initial = their initial values (slots x 3).
 *   handle          the inner handle (owned by the session; NULL for an empty graph) for the parity taps: graph index i < m is direction
 *                   edge i of the m remaining ones, m the origin prior, then the scale prior or the betweens. */
typedef struct lmgpu_translation_recovery lmgpu_translation_recovery;
int lmgpu_translation_recovery_create(const lmgpu_config* cfg, lmgpu_translation_recovery** out);
int lmgpu_translation_recovery_destroy(lmgpu_translation_recovery* tr);
const char* lmgpu_translation_recovery_last_error(const lmgpu_translation_recovery* tr);
int lmgpu_translation_recovery_seed(lmgpu_translation_recovery* tr, uint32_t seed);
int lmgpu_translation_recovery_set_prior_sigma(lmgpu_translation_recovery* tr, double sigma);
int lmgpu_translation_recovery_add_directions(lmgpu_translation_recovery* tr, int32_t n, const int32_t* index, const uint64_t* keys, const double* dirs,
                                              int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k);
int lmgpu_translation_recovery_add_betweens(lmgpu_translation_recovery* tr, int32_t n, const int32_t* index, const uint64_t* keys, const double* meas,
                                            int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k);
int lmgpu_translation_recovery_finalize(lmgpu_translation_recovery* tr, double scale, int32_t n_init, const uint64_t* init_keys, const double* init_vals,
                                        int32_t n_order, const uint64_t* ordering);
int lmgpu_translation_recovery_num_keys(const lmgpu_translation_recovery* tr);    /* -1 before finalize */
int lmgpu_translation_recovery_num_factors(const lmgpu_translation_recovery* tr); /* of the inner graph, priors included */
int lmgpu_translation_recovery_get_keys(const lmgpu_translation_recovery* tr, uint64_t* keys_out, uint64_t* representative_out);
int lmgpu_translation_recovery_get_slots(const lmgpu_translation_recovery* tr, uint64_t* keys_out);
int lmgpu_translation_recovery_get_initial(const lmgpu_translation_recovery* tr, double* out);
lmgpu_handle* lmgpu_translation_recovery_handle(lmgpu_translation_recovery* tr);
int lmgpu_translation_recovery_run(lmgpu_translation_recovery* tr, const lmgpu_lm_params* p, lmgpu_lm_state* state_out);
int lmgpu_translation_recovery_get(const lmgpu_translation_recovery* tr, double* out);

/* ---- MFAS (gtsam/sfm/MFAS.{h,cpp}): outlier weights of translation directions, D projection directions in one launch ----
 * n_edges edges (keys[2 e], keys[2 e + 1]); EITHER measured (n_edges x 3) with dirs (n_dirs x 3): weight = measured . dir, computed as
 * x dx + y dy + z dz with every product and sum rounded once (no contraction); OR edge_weights (n_dirs x n_edges) as in MFAS(edgeWeights).
 * An edge runs first -> second for weight >= 0, second -> first otherwise.  Outputs (any may be NULL): ordering_out (n_dirs x V keys, V =
 * the number of distinct keys), weights_out (n_dirs x n_edges: |weight| where the edge's destination precedes its source in the
 * ordering, else 0), sum_out (n_edges: the sum over the directions, added in direction order by one thread per edge, bitwise
 * reproducible; what a 1dSfM caller thresholds).
 * TIE RULE (ours): the reference walks an unordered_map, so which of several root nodes (inWeightSum < 1e-8) it takes, and which of
 * several nodes of equal heuristic, is unspecified.  Here the LOWEST KEY wins both.  In/out weight sums are accumulated in edge order.
 * REFUSED (LMGPU_INVALID, lmgpu_mfas_last_error): an unordered pair of nodes given twice (the reference's absWeightOfEdge silently reads
 * one of the two entries), an edge from a node to itself, a non-finite input.
 * One workgroup per direction; the node state lives in LDS up to lmgpu_mfas_lds_node_capacity() nodes, above that in global scratch. */
typedef struct lmgpu_mfas_stats {
  int32_t n_nodes;           /* V */
  int32_t global_state;      /* 1: the node state was kept in global scratch */
  int32_t lds_node_capacity;
  int32_t pad_;
  double kernel_ms;          /* device time of the two launches */
} lmgpu_mfas_stats;
int lmgpu_mfas_outlier_weights(int32_t device, int32_t n_edges, const uint64_t* keys, const double* measured, int32_t n_dirs, const double* dirs,
                               const double* edge_weights, uint64_t* ordering_out, double* weights_out, double* sum_out, lmgpu_mfas_stats* stats);
int lmgpu_mfas_lds_node_capacity(void);
const char* lmgpu_mfas_last_error(void); /* of the calling thread's last lmgpu_mfas_outlier_weights */

/* Per-kernel device time (HIP events on the handle's stream around each launch), accumulated since
 * lmgpu_set_kernel_timing(h, 1).  work[] is the ALGORITHMIC work of the launches in the category:
 * bytes for LINEARIZE (232 B per SFM factor + every camera / point row once) and ALLREDUCE,
 * FP64 flop for PANEL and SYRK (kb * m * (m + 1) per trailing update = the n^3/3 of the dense front, plus kb^3/3 + kb^2 cols of a
 * panel factored in the same launch). */
enum lmgpu_kernel_category {
  LMGPU_KT_LINEARIZE = 0,   /* sfm_linearize_kernel */
  LMGPU_KT_LDS_FRONT = 1,   /* lds_front_kernel (assemble + partial Cholesky of one small front per workgroup) */
  LMGPU_KT_HBM_ASSEMBLE = 2,/* memset + factor / child extend-add / Schur gather + damping of an HBM front */
  LMGPU_KT_PANEL = 3,       /* panel factorisations launched on their own: panel_dataflow_kernel, diag_potrf_kernel + panel_trsm_kernel */
  LMGPU_KT_SYRK = 4,        /* step_kernel = trailing update (v_mfma_f64_16x16x4_f64) + the next panel in the same launch (steps outside a chained launch); syrk_mfma_kernel */
  LMGPU_KT_BACKSUB_HBM = 5,
  LMGPU_KT_BACKSUB_LDS = 6,
  LMGPU_KT_LINEAR_ERROR = 7,
  LMGPU_KT_RETRACT_ERROR = 8,
  LMGPU_KT_ALLREDUCE = 9,
  LMGPU_KT_CHAIN = 10,      /* chain_kernel = all fused steps of a dense front (updates + panel factorisations) as ONE launch */
  LMGPU_KT_NUM = 11
};
/* on: 0 off; 1 every category; 2 only LINEARIZE and CHAIN / SYRK (the roofline kernels; SYRK is the per-step form of CHAIN's work): an event between two launches costs a few
 * microseconds of idle device time, and a throughput measurement should not pay that for the eleven categories it does not report */
int lmgpu_set_kernel_timing(lmgpu_handle* h, int32_t on);
int lmgpu_get_kernel_times(const lmgpu_handle* h, double* ms /*[LMGPU_KT_NUM]*/, double* work /*[LMGPU_KT_NUM]*/, int64_t* launches /*[LMGPU_KT_NUM]*/);

/* ---- parity taps ---- */
/* whitened Jacobian of graph factor `graph_index`, column-major rows x (sum dims + 1) like the reference's
 * VerticalBlockMatrix ([A1 A2 b]); out may be NULL to query the shape. */
int lmgpu_get_jacobian(lmgpu_handle* h, int32_t graph_index, double* out, int32_t* rows, int32_t* cols);
/* The whole linearization in one call: what LevenbergMarquardtOptimizer::iterate() RETURNS (the GaussianFactorGraph of
 * gtsam/nonlinear/NonlinearOptimizer.h:136, LevenbergMarquardtOptimizer.cpp:281,307; read by tests/testNonlinearOptimizer.cpp:282).
 * Every factor's whitened [A1 .. Ak b] back to back in ascending graph-index order (index-preserving like
 * NonlinearFactorGraph::linearize), column-major rows[i] x cols[i] at out + offsets[i]; offsets has *n_out + 1 entries.
 * Any output may be NULL (out == NULL: shapes only, no device needed).  One device copy per factor bucket. */
int lmgpu_get_jacobians(lmgpu_handle* h, int32_t* n_out, int32_t* graph_index, int32_t* rows, int32_t* cols, int64_t* offsets, double* out);
int lmgpu_num_fronts(const lmgpu_handle* h); /* 0 on a handle finalized under LMGPU_SOLVER_PCG */
/* info8: n_keys, n_frontal_keys, nf (rows of [R S d]), n (cols), parent front (-1 root), class (0 = LDS front, 1 = HBM front),
 *        owner rank (-1 = replicated on every rank), level (0 = leaf) */
int lmgpu_front_info(const lmgpu_handle* h, int32_t front, int32_t* info8);
/* Structure only (answerable on a device = -1 handle): how many of the plan's gather-leaf launches (one per size bin of a tree level) eliminate
 * their leaves four to a wave, one lane per factor (every leaf of the bin: nf <= 4, factors unary on the leaf's variables or binary to one
 * separator variable of at most 9 columns, at most 4 rows, no separator variable shared by two factors of the leaf); -1 before finalize. */
int lmgpu_leaf_group_launches(const lmgpu_handle* h);
/* Structure only (also on a device = -1 handle): how many tree levels' plain back-substitution launch takes lds_backsub_group_kernel (every
 * LDS front of the level has nf <= 4: four fronts per wave, 16 lanes each); *wide (may be NULL): how many of them its <4, 9> instantiation
 * (a front of nf = 4, or a separator wider than 96 columns).  -1 before finalize. */
int lmgpu_backsub_group_launches(const lmgpu_handle* h, int32_t* wide);
/* Parity tap (tests): the (rhs, rhs) corner scalar b'b - d'd that a gather leaf hands to its parent's Schur gather, after a solve.
 * LMGPU_INVALID for a front that is not a gather leaf. */
int lmgpu_get_leaf_corner(lmgpu_handle* h, int32_t front, double* corner);
/* slots: the front's variables in Scatter order (gtsam/linear/Scatter.cpp:39-73); RSd: column-major nf x n */
int lmgpu_get_front(lmgpu_handle* h, int32_t front, int32_t* slots, double* RSd_colmajor);

/* ---- multi-GPU (points/subtrees sharded over ranks; separator contributions summed with RCCL over xGMI) ---- */
/* rank 0 fills id[128] (ncclUniqueId bytes); the caller broadcasts it; every rank then calls lmgpu_comm_init. */
int lmgpu_comm_unique_id(char id128[128]);
int lmgpu_comm_init(lmgpu_handle* h, const char id128[128]);

/* Marginals(graph, values).marginalCovariance(variable)  (gtsam/nonlinear/Marginals.cpp:28-33 constructor: linearize at the
 * solution and eliminate into a Bayes tree; :124-127 marginalCovariance = inverse of the marginal information :109-121):
 * the dim x dim covariance (row-major) of the variable in `slot` at the handle's current values, i.e. its diagonal block of
 * (A^T A)^-1.  Computed with the path's own two kernels: per column one elimination (lambda = 0) + back-substitution of the
 * linearized system whose gradient is replaced by a unit vector.  The stored linearization is consumed (the next
 * lmgpu_solve needs lmgpu_linearize again).  LMGPU_INDETERMINATE where the reference throws
 * IndeterminantLinearSystemException (singular information matrix).  One GPU only (world_size == 1). */
int lmgpu_marginal_covariance(lmgpu_handle* h, int32_t slot, double* cov /* dim x dim */);
/* Marginals::jointMarginalCovariance(variables) (gtsam/nonlinear/Marginals.cpp:130-137): the blocks of (A^T A)^-1 for the
 * variables in `slots` (distinct), as one D x D row-major matrix, D = sum of their dims, block order = order of `slots`
 * (the reference's JointMarginal::fullMatrix orders the blocks by Key; the caller chooses here).  Cost: D unit-gradient solves. */
int lmgpu_joint_marginal_covariance(lmgpu_handle* h, int32_t nslots, const int32_t* slots, double* cov /* D x D */);

/* ---- marginal covariances of MANY variables from one factorization.  Marginals' constructor factors once and every
 *      marginalCovariance(key) is answered from the Bayes tree (Marginals.cpp:28-43, :124-127).  lmgpu_marginals_factor linearizes at the
 *      current values and eliminates undamped (lambda = 0); the fronts' [R S d] stay on the device.  A query then walks, per variable, the
 *      path from the front it is frontal in to its root -- R^T y = e up the path, R x = y down again -- with one workgroup per variable,
 *      all of its columns together, one launch and one download per chunk of requests.  The factorization is marked stale by everything
 *      that overwrites the fronts or moves the values (lmgpu_set_values, lmgpu_retract, lmgpu_restore_values, lmgpu_linearize, lmgpu_solve,
 *      every *_iterate and *_optimize, the two calls above) and rebuilt by the next query.  After lmgpu_marginals_factor the handle is in
 *      the state lmgpu_linearize + lmgpu_solve(lambda = 0) leave.  Refused with LMGPU_INVALID like lmgpu_joint_marginal_covariance: smart
 *      factors, a handle finalized under PCG, world_size > 1.  The two calls above keep their own route (one solve per column); joint
 *      marginals from this factorization: lmgpu_joint_marginal_covariances below. ---- */
int lmgpu_marginals_factor(lmgpu_handle* h);
/* the dim x dim blocks (row-major, symmetric) of the n variables in `slots`, back to back in the order of `slots`.  Duplicates are
 * allowed; n == 0 is LMGPU_OK; a slot out of range is LMGPU_INVALID and nothing is written.  A variable's block is bitwise the same
 * whatever else the request holds.  LMGPU_INDETERMINATE when a block comes out non-finite (lmgpu_last_failed_slot: the first such
 * variable) or the factorization fails. */
int lmgpu_marginal_covariances(lmgpu_handle* h, int32_t n, const int32_t* slots, double* cov_packed);
/* the fronts of the variable's path, from the front it is frontal in to its root, into fronts_out[0 .. cap); returns the path length
 * (-1: refused).  Structure only: answers on a device = -1 handle. */
int lmgpu_marginals_path(const lmgpu_handle* h, int32_t slot, int32_t* fronts_out, int32_t cap);
/* the path tables of one front: *poff = position of its first frontal scalar in a path's work vector (0 for a root, the parent's
 * poff + the parent's frontal dimension otherwise), spos[0 .. cap) = the positions of its separator scalars, each inside the frontal
 * range of an ancestor.  Returns the number of separator scalars (-1: refused).  Structure only. */
int lmgpu_marginals_front_offsets(const lmgpu_handle* h, int32_t front, int32_t* poff, int32_t* spos, int32_t cap);
/* scratch_bytes: byte budget of the buffer that holds the work vectors too long for LDS; a request is cut into chunks (one launch each)
 * so that a chunk's vectors fit it; a single vector that does not is refused (default 64 MiB).  lds_doubles: the longest work vector
 * (doubles) kept in LDS (default 6144).  0 keeps a value. */
int lmgpu_set_marginals_params(lmgpu_handle* h, int64_t scratch_bytes, int32_t lds_doubles);
/* counted over the handle's life: launches and chunks of marginal_path_kernel, factorizations done for it, variables whose work vector
 * lay in LDS / in scratch, cliques on the longest path walked; lds_capacity (doubles) and scratch_bytes are the parameters in force. */
/* cross walks (below): launches and chunks of marginal_cross_kernel, cross_walks = workgroups = walks of a source's path,
 * cross_targets = blocks written, workgroups whose work vector lay in LDS / in scratch, longest_union = cliques on the longest source
 * path + branch walked by one workgroup, cross_cap = targets per workgroup in force. */
typedef struct lmgpu_marginals_stats {
  int64_t launches, chunks, factorizations, vars_lds, vars_scratch, scratch_bytes;
  int32_t longest_path, lds_capacity;
  int64_t cross_launches, cross_chunks, cross_walks, cross_targets, cross_lds, cross_scratch;
  int32_t longest_union, cross_cap;
} lmgpu_marginals_stats;
int lmgpu_get_marginals_stats(lmgpu_handle* h, lmgpu_marginals_stats* out);

/* ---- cross-covariances and joint marginals from the same factorization (Marginals::jointMarginalCovariance,
 *      Marginals.cpp:130-137, answered from the Bayes tree).  Sigma[:, j] is x with R^T y = e_j, R x = y: y lives on j's path, and x at a
 *      variable i needs only the fronts of i's path, which it shares with j's from their junction (the deepest front on both) to the root.
 *      One workgroup walks the path of a SOURCE j up and down, then, per TARGET i, descends i's branch below the junction and writes the
 *      dim_i x dim_j block.  One launch and one download per chunk.  Refusals, staleness and the LDS / scratch rules are those of
 *      lmgpu_marginal_covariances; lmgpu_set_marginals_params applies.  A block's bits depend on the pair (i, j) and the factorization
 *      alone; the block of (i, i) is bitwise lmgpu_marginal_covariances' block of i. ---- */
/* block q = Sigma[slots_i[q], slots_j[q]], dim_i x dim_j row-major (the columns are those of j, the source), back to back in the order
 * of the pairs.  Pairs with equal j share a walk wherever they stand in the list.  A pair across two trees of a forest: exact zeros.
 * n == 0 is LMGPU_OK; a slot out of range is LMGPU_INVALID and nothing is written.  LMGPU_INDETERMINATE when a block comes out non-finite
 * (lmgpu_last_failed_slot: the source of the first such workgroup) or the factorization fails. */
int lmgpu_marginal_cross_covariances(lmgpu_handle* h, int32_t n, const int32_t* slots_i, const int32_t* slots_j, double* out_packed);
/* n_sets joint marginals: set q holds slots[set_begin[q] .. set_begin[q + 1]) (distinct: a slot twice in one set is LMGPU_INVALID) and
 * gets its D_q x D_q row-major matrix, blocks in the order of its slots as lmgpu_joint_marginal_covariance lays them out, the matrices
 * back to back.  Exactly symmetric: an off-diagonal block is computed once, from the variable of the pair with the shorter path (fewer
 * scalars; ties: the smaller slot) as the source, and mirrored; a diagonal block is the (i, i) block above. */
int lmgpu_joint_marginal_covariances(lmgpu_handle* h, int32_t n_sets, const int32_t* set_begin /* n_sets + 1 */, const int32_t* slots,
                                     double* cov_packed);
/* the junction of two variables' paths: the deepest front on both (-1: different trees of a forest, or refused).  Structure only. */
int lmgpu_marginals_junction(const lmgpu_handle* h, int32_t slot_i, int32_t slot_j);
/* development switch: targets of one source that one workgroup serves after its walk of the source's path (a source with more is split
 * over several workgroups, each repeating the walk).  0 restores the built-in rule: one target per workgroup until the request holds
 * more than 1024 pairs, then pairs / 1024 rounded up, 16 at most (lmgpu_marginals_stats.cross_cap reports that maximum).  Results do
 * not depend on it. */
int lmgpu_set_marginals_cross_cap(lmgpu_handle* h, int32_t targets_per_workgroup);

/* Host-only self-test (no GPU work): the ticket order the library gives the chained factorisation launch of a dense front
 * with n columns (nf frontal) for the steps i0 .. i0 + nsteps - 1 (tile rows beyond far_pct percent scheduled late; far_pct + 1000: the
 * default schedule, whose update tiles apply two steps per pass) is a permutation of all logical workgroups in which every
 * in-launch dependency points to an earlier ticket.  0 = valid.  No reference counterpart (the reference factors a front with
 * one Eigen LLT call, gtsam/base/cholesky.cpp:108-159); it exists so that the CPU test-suite can check the scheduler. */
int lmgpu_selftest_chain_schedule(int n, int nf, int i0, int nsteps, int far_pct);

/* Host-only self-test (no GPU work, no handle): the launches that factor one dense front of n columns (nf frontal) on the per-front
 * path, in execution order.  mode: 0 single rank, 1 row chunks summed on the host (in-process group), 2 row chunks behind events
 * (RCCL); forms: bit 0 LMGPU_PANEL_2L, 1 LMGPU_NO_FUSE, 2 LMGPU_NO_CHAIN, 3 LMGPU_NO_TAIL.  Four int32 per record into `out`:
 * kind (0 dataflow panel, 1 two-launch panel, 2 chained launch, 3 fused step, 4 quadrant update, 5 tile update, 6 tail, 7 add row
 * chunk, 8 wait for row chunk), outer panel i (-1 for 7, 8), steps of a chained launch, row chunk (7, 8; else -1).  Returns the
 * number of records; negative for refused geometry (n <= 0, nf <= 0, nf > n, unknown mode) or more than max_records records.  No
 * reference counterpart (see lmgpu_selftest_chain_schedule); it is what the elimination runs, so the CPU test-suite can pin it. */
int lmgpu_selftest_dense_schedule(int n, int nf, int mode, unsigned forms, int max_records, int32_t* out);

/* Host-only self-test (no GPU work, no handle): the arithmetic of one Dogleg trial as lmgpu_dl_iterate runs it.  which = 0, the trial
 * point (DoglegOptimizerImpl::ComputeDoglegPoint / ComputeBlend, DoglegOptimizerImpl.cpp:26-91): in = (delta, dx_u . dx_u, dx_n . dx_n,
 * dx_u . dx_n), out = (branch: 0 steepest-descent cut, 1 blend, 2 Newton step; its scalar: the factor on dx_u, tau, 1).  which = 1, the
 * radius update (DoglegOptimizerImpl.h:139-254, ONE_STEP_PER_ITERATION): in = (rho, delta, |dx_d|), out = (new delta, 1 if the trial is
 * repeated with it, 0 if the step is dropped at the radius floor else 1).  Returns 0; -1 for a NULL argument or an unknown `which`. */
int lmgpu_selftest_dogleg_step(int which, const double* in, double* out);

/* Host-only self-test (no GPU work, no handle): the library's one table of factor types, so that the CPU test-suite can hold every
 * copy of it outside the library against it.  out = (arity, rows of the error, measurement doubles, lmgpu_var_type of variable 0, 1, 2;
 * -1 beyond the arity) of a public lmgpu_factor_type.  LMGPU_OK; LMGPU_INVALID outside 0 .. LMGPU_NUM_FACTOR_TYPES - 1 or for NULL. */
int lmgpu_selftest_factor_type(int32_t type, int32_t out[6]);
/* Its sibling for a lmgpu_var_type: out = (tangent dimension, doubles of a packed value).  LMGPU_INVALID for an unknown type or NULL. */
int lmgpu_selftest_var_type(int32_t type, int32_t out[2]);

/* ---- triangulation (gtsam/geometry/triangulation.h, triangulation.cpp): triangulatePoint3 / triangulateSafe for PinholeCamera<Cal3Bundler>
 *      and PinholeCamera<Cal3_S2>, batched over landmarks on the device -- one lane per landmark, one launch per degree bin over the
 *      landmarks sorted by their number of observations, results stored at the landmark's own index.  Each camera carries its own
 *      calibration (as in testTriangulation.cpp, fourPoses_distinct_Ks).  Per landmark, line by line:
 *        triangulatePoint3<CAMERA> (triangulation.h:491-549): fewer than 2 observations is underconstrained; projection matrices
 *          K * pose.inverse()[0:3, :] (PinholeCamera.h:316-318); undistortMeasurements (:252-268): nothing for Cal3_S2, for Cal3Bundler
 *          K_pinhole.uncalibrate(cal.calibrate(z)) with calibrate's fixed-point loop (at most 10 passes, break at
 *          distance2(uncalibrate(pn), pi) <= 1e-5, Cal3Bundler.cpp:93-128); triangulateDLT (triangulation.cpp:27-56, 149-157): rows
 *          x P.row(2) - P.row(0), y P.row(2) - P.row(1); DLT (gtsam/base/Matrix.cpp:556-574): rank = singular values > rankTolerance, a
 *          rank below 3 is underconstrained, else the point is v[0:3] / v[3] of the last right singular vector.  The cheirality check
 *          (transformTo(point).z <= 0 for any camera) runs after the refinement; the library is built to the reference's default
 *          GTSAM_THROW_CHEIRALITY_EXCEPTION = ON.
 *        refinement, enableEPI != 0 (triangulation.cpp:177-195, triangulation.h:153-221): Levenberg-Marquardt on the 3-vector, one
 *          TriangulationFactor per observation: error project(point) - z with the full distorted projection, 2x3 Jacobian; a point behind a
 *          camera contributes the error (2 fx, 2 fx) and a zero Jacobian (TriangulationFactor.h:122-136, PinholeCamera.h:321-323).
 *          lambdaInitial 1, lambdaFactor 10, maxIterations 100, absoluteErrorTol 1, everything else LevenbergMarquardtParams(); control flow as
 *          lmgpu_iterate / lmgpu_optimize.  One noise model for all observations: Unit (noise_inv_sigma 0) or Isotropic (one inverse sigma).
 *        triangulateSafe (triangulation.h:701-758): m < 2 or underconstrained -> DEGENERATE; cheirality failure -> BEHIND_CAMERA, before every
 *          distance check; then per camera in order landmarkDistanceThreshold -> FAR_POINT; after the loop the maximum reprojection error
 *          norm against dynamicOutlierRejectionThreshold -> OUTLIER.  A threshold <= 0 is off.
 *      Deviations: useLOST != 0 is refused with LMGPU_INVALID (LOST is not implemented).  A Cal3Bundler::calibrate that has not converged
 *      after 10 passes gives the extra status LMGPU_TRI_CALIBRATE_FAILED for that point (the reference lets a std::runtime_error escape
 *      triangulateSafe there).  A non-finite result (v[3] == 0) is carried through with IEEE semantics, as the reference's expressions give
 *      it.  The CAM_BUNDLER packing folds the principal point into the measurement (variable types above); the DLT rows
 *      (x - u0) r2 - f r0 are algebraically independent of (u0, v0), and so are the reprojection errors, so the device works with
 *      u0 = v0 = 0 and measurements relative to the principal point.  A robust noise model is out of scope.
 *   lmgpu_triangulate_batch       stand-alone (no handle): upload, launches, download.  camera_model 0 = PinholeCamera<Cal3Bundler>, 15
 *        doubles per camera (the CAM_BUNDLER packing), obs_z relative to the principal point; 1 = PinholeCamera<Cal3_S2>, 17 doubles per
 *        camera (POSE3 packing + fx, fy, s, u0, v0).  obs_offsets[n_points + 1]: CSR index of the observations of each landmark into
 *        obs_cam[] (camera indices) and obs_z[] (2 doubles each).  points_out[3 n_points] is NaN where status_out[n_points] is not VALID.
 *        Refused with LMGPU_INVALID before any device work: a camera index out of range, offsets that decrease (or start below 0), a
 *        negative n_points, an unknown camera_model, useLOST != 0, a NULL array that is needed.  n_points == 0 is LMGPU_OK.
 *   lmgpu_triangulate_landmarks   on a finalized handle with values: every POINT3 variable in slot order (lmgpu_num_points3 of them); its
 *        observations are its LMGPU_F_SFM factors (camera = the CAM_BUNDLER variable's current value) or its LMGPU_F_PROJECTION factors
 *        (camera = the POSE3 variable's current value + the K of the factor's measurement), in graph-index order.  The point -> factor
 *        index is built on the host at the first call and kept; cameras and measurements are read where they lie in device memory, only
 *        the result crosses the host.  write_values != 0 stores the VALID points into the handle's values (the stored linearization is
 *        treated as by lmgpu_set_values); points of any other status keep their value.  points_out / status_out / n_valid may be NULL.
 *        Refused with LMGPU_INVALID and a message before anything runs: a point that has both SFM and PROJECTION factors or a
 *        PROJECTION_BPS / SFM2 factor; GNC enabled; world_size > 1; a call before lmgpu_set_values.  Works on a handle finalized for
 *        Cholesky or for PCG (it needs no fronts).  ISAM2 is not affected.
 *   lmgpu_get_triangulation_stats of the last call on the handle, or with h == NULL of the calling thread's last lmgpu_triangulate_batch:
 *        points per status, the maximum and the sum over the points of the refinement's tryLambda calls (linear solves), device
 *        milliseconds of the launches (HIP events).  LMGPU_INVALID before the first call. */
typedef struct lmgpu_triangulation_params { /* TriangulationParameters, triangulation.h:562-609; defaults 1.0, 0, 0, -1, -1, 0 */
  double rankTolerance;
  int32_t enableEPI, useLOST;
  double landmarkDistanceThreshold, dynamicOutlierRejectionThreshold;
  double noise_inv_sigma; /* 0: Unit; > 0: Isotropic, one inverse sigma (only the refinement reads it) */
} lmgpu_triangulation_params;
enum lmgpu_triangulation_status { /* TriangulationResult::Status, triangulation.h:631 */
  LMGPU_TRI_VALID = 0,
  LMGPU_TRI_DEGENERATE = 1,
  LMGPU_TRI_BEHIND_CAMERA = 2,
  LMGPU_TRI_OUTLIER = 3,
  LMGPU_TRI_FAR_POINT = 4,
  LMGPU_TRI_CALIBRATE_FAILED = 5
};
typedef struct lmgpu_triangulation_stats {
  int32_t n_points;
  int32_t n_status[6]; /* indexed by lmgpu_triangulation_status */
  int32_t max_iterations;
  int64_t sum_iterations;
  double device_ms;
} lmgpu_triangulation_stats;
int lmgpu_triangulate_batch(int32_t device, int32_t camera_model, int32_t n_cams, const double* cams, int32_t n_points,
                            const int32_t* obs_offsets, const int32_t* obs_cam, const double* obs_z, const lmgpu_triangulation_params* params,
                            double* points_out, int32_t* status_out);
int lmgpu_triangulate_landmarks(lmgpu_handle* h, const lmgpu_triangulation_params* params, int32_t write_values, double* points_out,
                                int32_t* status_out, int32_t* n_valid);
int lmgpu_num_points3(const lmgpu_handle* h); /* POINT3 variables of the handle; -1 before finalize */
int lmgpu_get_triangulation_stats(const lmgpu_handle* h, lmgpu_triangulation_stats* out);

/* ---- smart projection factors: SmartProjectionPoseFactor<Cal3_S2> (gtsam/slam/SmartProjectionPoseFactor.h:43-152 over SmartProjectionFactor.h
 *      and SmartFactorBase.h; parameters SmartFactorParams.h:31-133) on the batch handle -- one factor per landmark over the m poses that saw
 *      it, the landmark re-triangulated at every linearization and eliminated inside the factor, so that the optimizer sees poses only.
 *      A factor: m >= 1 observations (POSE3 slot, z) with distinct slots, one Cal3_S2 (K5 = fx, fy, s, u0, v0), one Isotropic(2, sigma) noise
 *      model (SmartFactorBase.h:109-115 refuses any other), one lmgpu_smart_params.
 *        member triangulateSafe (SmartProjectionFactor.h:127-184), at the head of EVERY linearization and EVERY error evaluation: m < 2 is
 *          DEGENERATE and leaves the cache alone; else re-triangulate iff the cache is empty or a camera pose is not
 *          Pose3::equals(cached, retriangulationThreshold) (gtsam/geometry/Pose3.cpp:184-186 -> fpEqual, gtsam/base/Vector.cpp:42-77: in
 *          effect |a - b| <= tol on the nine rotation and three translation entries); re-triangulating stores the current poses and
 *          result_ = gtsam::triangulateSafe(cameras, measured, params.triangulation) (the "triangulation" section above).  The result
 *          therefore depends on the history of calls; the library makes them in the reference's order (LevenbergMarquardtOptimizer:
 *          constructor error, per iteration linearize, per trial lambda one error evaluation iff the damped system was solved and its
 *          linearized cost did not rise, LevenbergMarquardtOptimizer.cpp:206-216).  The cache belongs to the handle: lmgpu_set_values,
 *          lmgpu_retract, lmgpu_restore_values keep it; lmgpu_smart_reset empties it (= newly constructed factors).
 *        error (:411-439): valid result: 0.5 sum |(project(point) - z) / sigma|^2 at result_; otherwise 0.
 *        linearize (:198-237), HESSIAN: valid result: the augmented information of CameraSet::SchurComplement(Fs, E, b, 0)
 *          (gtsam/geometry/CameraSet.h:145-216), Fs (2x6) / E (2x3) the PinholePose<Cal3_S2> projection Jacobians at result_, b = -(reprojection
 *          error), all divided by sigma; constant term b'b - b'E (E'E)^-1 E'b.  Otherwise a zero factor on the m keys (ZERO_ON_DEGENERACY).
 *      How it is carried: a factor with m >= 2 is a HIDDEN POINT3 variable in front of the caller's slots with m internal factors; the
 *      existing leaf elimination produces exactly F'(I - E (E'E)^-1 E')F.  The hidden point is never damped, never retracted, and no
 *      part of values, delta, lmgpu_total_dim / lmgpu_total_store or any packed vector at this boundary; slots of this header stay the
 *      caller's.  lmgpu_solve's lin_err0 is the reference's linear.error(0) (constant terms as above).  The front taps (lmgpu_num_fronts,
 *      lmgpu_front_info, lmgpu_get_front) show the internal structure: hidden points as leaf fronts, slots shifted up by the number of hidden
 *      points; they are not parity quantities here.  lmgpu_last_failed_slot is negative for a hidden point.
 *      Deviation: a VALID cached point that a pose moved within retriangulationThreshold puts behind a camera gives that observation
 *      GenericProjectionFactor's throwCheirality = false behaviour (zero Jacobians, error 2 fx); the reference lets CheiralityException escape.
 *      Supported on such a handle: lmgpu_error, lmgpu_linearize, lmgpu_solve / lmgpu_lm_init / lmgpu_iterate / lmgpu_optimize without
 *      diagonal damping, lmgpu_gn_iterate / lmgpu_gn_optimize, lmgpu_retract, lmgpu_set / get / save / restore_values, lmgpu_get_timings, any
 *      other factor bucket beside them.  Refused with LMGPU_INVALID and one message (each needs the Schur complement itself, not the
 *      Jacobians the engine keeps): diagonal damping, lmgpu_hessian_diagonal, PCG, GNC, NCG / lmgpu_gradient, Dogleg, lmgpu_bt_products, the
 *      marginal covariances, lmgpu_get_jacobian(s), lmgpu_triangulate_landmarks.  Not implemented (refused where expressible): the other
 *      linearization and degeneracy modes, body_P_sensor, SmartProjectionRigFactor, Cal3Bundler smart factors, ISAM2 (newAffectedKeys).
 *   lmgpu_add_smart_factors   before lmgpu_finalize_structure, any number of times, each call with its own params.  graph_index[n]: the
 *        factor's index in the NonlinearFactorGraph; obs_offsets[n + 1]: CSR into obs_slots[] (the caller's POSE3 slots) and obs_z[] (2
 *        doubles each); K5[5 n]; inv_sigma[n] = 1 / sigma.  Refused with LMGPU_INVALID and a message before any device work: a mode other
 *        than HESSIAN / ZERO_ON_DEGENERACY, useLOST, a slot that is not POSE3, a slot twice in one factor, a factor without observations,
 *        decreasing offsets, inv_sigma <= 0, world_size > 1.
 *   lmgpu_smart_get_points    SmartProjectionFactor::point() of every factor in the order added: NaN unless VALID, with the status
 *        (lmgpu_triangulation_status); DEGENERATE before the first evaluation.  Either output may be NULL.
 *   lmgpu_smart_get_hessian   parity tap: the augmented information ((6 m + 1)^2, column-major, symmetric) of the factor with this graph
 *        index, built on the host from the device's own F, E, b of the last linearization.  aug_info_colmajor may be NULL (m only).
 *   lmgpu_get_smart_stats     of the last linearize / error evaluation that counts (a dropped speculative one does not): factors
 *        re-triangulated, factors per status, device ms of its triangulation launches and of the last smart linearize launches (HIP events). */
enum lmgpu_smart_linearization_mode { LMGPU_SMART_HESSIAN = 0, LMGPU_SMART_IMPLICIT_SCHUR = 1, LMGPU_SMART_JACOBIAN_Q = 2, LMGPU_SMART_JACOBIAN_SVD = 3 };
enum lmgpu_smart_degeneracy_mode { LMGPU_SMART_IGNORE_DEGENERACY = 0, LMGPU_SMART_ZERO_ON_DEGENERACY = 1, LMGPU_SMART_HANDLE_INFINITY = 2 };
typedef struct lmgpu_smart_params { /* SmartProjectionParams, SmartFactorParams.h:42-133; defaults HESSIAN, IGNORE_DEGENERACY, 1e-5 */
  int32_t linearizationMode, degeneracyMode;
  double retriangulationThreshold;
  lmgpu_triangulation_params triangulation;
} lmgpu_smart_params;
typedef struct lmgpu_smart_stats {
  int32_t n_factors, retriangulations;
  int32_t n_status[6]; /* indexed by lmgpu_triangulation_status */
  double triangulate_ms, linearize_ms;
} lmgpu_smart_stats;
int lmgpu_add_smart_factors(lmgpu_handle* h, int32_t n, const int32_t* graph_index, const int32_t* obs_offsets, const int32_t* obs_slots,
                            const double* obs_z, const double* K5, const double* inv_sigma, const lmgpu_smart_params* params);
int lmgpu_num_smart_factors(const lmgpu_handle* h); /* -1 before finalize */
int lmgpu_smart_get_points(lmgpu_handle* h, double* points3, int32_t* status);
int lmgpu_smart_get_hessian(lmgpu_handle* h, int32_t graph_index, int32_t* m, double* aug_info_colmajor);
int lmgpu_smart_reset(lmgpu_handle* h);
int lmgpu_get_smart_stats(const lmgpu_handle* h, lmgpu_smart_stats* out);

/* ---- ISAM2 (gtsam/nonlinear/ISAM2.h): incremental smoothing on a device-resident Bayes tree (BASELINE config 5) ----
 * ISAM2::update(newFactors, newTheta) (gtsam/nonlinear/ISAM2.cpp:419-480) = lmgpu_isam2_add_variables + lmgpu_isam2_add_factors
 * (the pending input) + lmgpu_isam2_update: add the variables, (every relinearizeSkip-th update) refresh delta, mark and
 * relinearize the variables whose delta exceeds relinearizeThreshold, relinearize the affected factor subset on the device,
 * remove the top of the Bayes tree, re-eliminate it with the cached boundary factors of the orphaned subtrees under a constrained
 * COLAMD ordering (:250-362; batch fallback when >= 65 % of the variables are affected, :156-159), and keep the tree on the device.
 * ISAM2Params honoured: ISAM2GaussNewtonParams::wildfireThreshold, relinearizeThreshold (one double), relinearizeSkip,
 * enableRelinearization (gtsam/nonlinear/ISAM2Params.h:133-246); Cholesky factorisation; cacheLinearizedFactors semantics.
 * ISAM2UpdateParams (gtsam/nonlinear/ISAM2UpdateParams.h:30-90) through lmgpu_isam2_update_with: removeFactorIndices, constrainedKeys,
 * noRelinKeys, extraReelimKeys, force_relinearize, forceFullSolve.
 * relinearizeThreshold as FastMap<char, Vector> and enablePartialRelinearizationCheck: the two setters below.
 * ISAM2DoglegParams: lmgpu_isam2_set_dogleg.
 * Robust noise models: lmgpu_isam2_add_factors_robust.
 * ISAM2::marginalizeLeaves: lmgpu_isam2_marginalize_leaves; ISAM2Params::findUnusedFactorSlots: lmgpu_isam2_set_find_unused_factor_slots.
 * Not bound: QR, newAffectedKeys (smart factors).
 * updateDelta (ISAM2.cpp:701-719) is scheduled by the library: Gauss-Newton mode runs it BEHIND an update's elimination, under the update's
 * one wait, when delta is going to be read before the next elimination anyway (the next update checks relinearization, or the caller read an
 * estimate after the previous update); otherwise where the reference runs it (at the next reader).  Same delta either way; the one visible
 * difference: an indeterminate back-substitution would be returned by that update instead of the next call (the elimination's own pivot
 * test reports such a system first).
 *
 * The fill-reducing ordering is a boundary input like in the batch path, but here it is needed per update: the caller hands over
 * ITS ccolamd (the reference side: the one Ordering::ColamdConstrained calls, gtsam/inference/Ordering.cpp:50-125) as a callback:
 *   int fn(user, n_rows, n_cols, col_ptr[n_cols + 1], row_idx[nnz], cmember[n_cols], perm_out[n_cols]) -> 1 on success,
 * to be run with GTSAM's knobs (CCOLAMD_DENSE_ROW = CCOLAMD_DENSE_COL = -1, Ordering.cpp:94-97); perm_out[j] = the column eliminated j-th. */
typedef struct lmgpu_isam2 lmgpu_isam2;
typedef int (*lmgpu_ccolamd_fn)(void* user, int32_t n_rows, int32_t n_cols, const int32_t* col_ptr, const int32_t* row_idx, const int32_t* cmember,
                                int32_t* perm_out);
typedef struct lmgpu_isam2_params {
  double relinearizeThreshold;  /* default 0.1 */
  int32_t relinearizeSkip;      /* default 10 */
  int32_t enableRelinearization; /* default 1 */
  double wildfireThreshold;     /* ISAM2GaussNewtonParams, default 0.001 */
} lmgpu_isam2_params;
/* ISAM2Result subset (gtsam/nonlinear/ISAM2Result.h:60-93) + whether the batch fallback ran */
typedef struct lmgpu_isam2_result {
  int32_t variablesRelinearized, variablesReeliminated, factorsRecalculated, cliques, batch;
} lmgpu_isam2_result;
int lmgpu_isam2_create(const lmgpu_config* cfg, const lmgpu_isam2_params* params, lmgpu_ccolamd_fn ccolamd, void* user, lmgpu_isam2** out);
int lmgpu_isam2_destroy(lmgpu_isam2* s);
const char* lmgpu_isam2_last_error(const lmgpu_isam2* s);
uint64_t lmgpu_isam2_last_failed_key(const lmgpu_isam2* s); /* LMGPU_INDETERMINATE: first frontal key of the failing clique */
/* ISAM2Params::relinearizeThreshold as FastMap<char, Vector> (gtsam/nonlinear/ISAM2Params.h:139-141, 169-181): n entries, entry i = the
 * Symbol character chrs[i] with dims[i] per-dof thresholds, the vectors back to back in `values`.  A variable is then relinearized
 * when any |delta_i| > threshold_i (strictly; ISAM2-impl.h:266, 375) of its character's vector; an update that meets a variable
 * without a vector of its dimension returns LMGPU_INVALID (the reference throws, :258-262).  n = 0: the scalar threshold again. */
int lmgpu_isam2_set_relinearize_thresholds(lmgpu_isam2* s, int32_t n, const char* chrs, const int32_t* dims, const double* values);
/* ISAM2Params::optimizationParams = ISAM2DoglegParams(initialDelta, wildfireThreshold, adaptationMode) (ISAM2Params.h:68-110) instead of
 * ISAM2GaussNewtonParams: updateDelta becomes one iteration of Powell's dog leg (ISAM2.cpp:739-779; adaptationMode as
 * DoglegOptimizerImpl::TrustRegionAdaptationMode: 0 SEARCH_EACH_ITERATION (the default), 1 SEARCH_REDUCE_ONLY, 2 ONE_STEP_PER_ITERATION).
 * To be called before the first variable is added.  lmgpu_isam2_get_dogleg_delta: the current trust-region radius (doglegDelta_). */
int lmgpu_isam2_set_dogleg(lmgpu_isam2* s, double initialDelta, double wildfireThreshold, int32_t adaptationMode);
double lmgpu_isam2_get_dogleg_delta(const lmgpu_isam2* s);
/* ISAM2Params::evaluateNonlinearError (ISAM2Params.h:200-203): every update also evaluates the nonlinear error of the whole graph at
 * calculateEstimate() after the new factors have been added (ISAM2Result::errorBefore, ISAM2.cpp:444-446) and at its end (errorAfter,
 * :481-483) -- each through calculateEstimate(), i.e. with the back-substitution brought up to date first, like the reference.
 * lmgpu_isam2_get_errors returns the two of the last update; lmgpu_isam2_error is getFactorsUnsafe().error(values) on demand,
 * which = 0 at calculateEstimate(), 2 at the linearization point (the error kernels of the batch path on every factor bucket). */
int lmgpu_isam2_set_evaluate_nonlinear_error(lmgpu_isam2* s, int32_t enable);
int lmgpu_isam2_get_errors(const lmgpu_isam2* s, double* error_before, double* error_after);
int lmgpu_isam2_error(lmgpu_isam2* s, int32_t which, double* out);
/* ISAM2Params::enablePartialRelinearizationCheck (ISAM2Params.h:214-222): the check walks down from the roots and stops below a
 * clique none of whose variables is above its threshold (CheckRelinearizationPartial, ISAM2-impl.h:246-331) */
int lmgpu_isam2_set_partial_relinearization_check(lmgpu_isam2* s, int32_t enable);
/* newTheta of the next update: packed values like lmgpu_set_values (store doubles per type, in the order given) */
int lmgpu_isam2_add_variables(lmgpu_isam2* s, int32_t n, const uint64_t* keys, const int32_t* types, const double* packed_values);
/* newFactors of the next update, appended in call order (= their order in the NonlinearFactorGraph); keys: n x arity Keys */
int lmgpu_isam2_add_factors(lmgpu_isam2* s, int32_t factor_type, int32_t n, const uint64_t* keys, const double* meas, int32_t noise_kind,
                            const double* noise);
/* the same with noiseModel::Robust(mEstimator(robust_k), model) around the Gaussian model of every one of the n factors (lmgpu_robust_kind;
 * gtsam/linear/NoiseModel.h:663-760): relinearization reweights [A b] by sqrt(weight(||b||)) (Robust::WhitenSystem, Block scheme) and
 * evaluateNonlinearError uses the m-estimator's loss, exactly as in the batch path (lmgpu_add_factor_bucket_robust) */
int lmgpu_isam2_add_factors_robust(lmgpu_isam2* s, int32_t factor_type, int32_t n, const uint64_t* keys, const double* meas, int32_t noise_kind,
                                   const double* noise, int32_t robust_kind, double robust_k);
int lmgpu_isam2_update(lmgpu_isam2* s, int32_t force_relinearize, lmgpu_isam2_result* out);
/* ISAM2::update(newFactors, newTheta, const ISAM2UpdateParams&) (gtsam/nonlinear/ISAM2.h:176-186, ISAM2UpdateParams.h:30-90).
 * removeFactorIndices: positions in the factor list (getFactorsUnsafe(); the factors of update k start at lmgpu_isam2_num_factors()
 *   before it); a removed factor leaves an empty slot (indices never shift), removing an empty slot is a no-op, an index beyond the
 *   list (including the factors this very update adds) is LMGPU_INVALID.  A variable that loses its last factor leaves the system
 *   (ISAM2Result::unusedKeys -> ISAM2::removeVariables, ISAM2.cpp:385-398): see lmgpu_isam2_get_unused_keys.
 * constrainedKeys (has_constrained != 0: the optional is engaged, even with n_constrained == 0): key -> group for the constrained
 *   COLAMD call instead of "the observed keys last" (ISAM2.cpp:205-218, 318-340).
 * noRelinKeys: never relinearized by this update; extraReelimKeys: re-eliminated although no new factor touches them;
 * forceFullSolve: wildfire threshold 0 and every variable relinearized (the reference's debugging switch). */
typedef struct lmgpu_isam2_update_params {
  int32_t n_remove;
  const uint64_t* removeFactorIndices;
  int32_t has_constrained, n_constrained;
  const uint64_t* constrainedKeys;
  const int32_t* constrainedGroups;
  int32_t n_no_relin;
  const uint64_t* noRelinKeys;
  int32_t n_extra_reelim;
  const uint64_t* extraReelimKeys;
  int32_t force_relinearize, forceFullSolve;
} lmgpu_isam2_update_params;
int lmgpu_isam2_update_with(lmgpu_isam2* s, const lmgpu_isam2_update_params* params, lmgpu_isam2_result* out);
/* ISAM2Result::unusedKeys of the last update, ascending; returns their number (keys_out may be NULL) */
int lmgpu_isam2_get_unused_keys(const lmgpu_isam2* s, uint64_t* keys_out);
/* 1 when slot i of the factor list holds a factor (getFactorsUnsafe().exists(i)) */
int lmgpu_isam2_factor_exists(const lmgpu_isam2* s, int32_t i);
/* ISAM2Params::findUnusedFactorSlots (gtsam/nonlinear/ISAM2Params.h:225): new factors -- of an update and of marginalizeLeaves -- fill the
 * empty slots of the factor list from the front before they extend it (FactorGraph::add_factors, gtsam/inference/FactorGraph-inst.h:109-137). */
int lmgpu_isam2_set_find_unused_factor_slots(lmgpu_isam2* s, int32_t enable);
/* ISAM2::marginalizeLeaves(leafKeys, &marginalFactorsIndices, &deletedFactorsIndices) (gtsam/nonlinear/ISAM2.h:198-222, ISAM2.cpp:487-720):
 * the variables must be leaves of the Bayes tree (the caller orders them first with constrainedKeys, as with the reference: see
 * IncrementalFixedLagSmoother).  The marginal on what they were connected to stays in the factor list as LinearContainerFactors (constant
 * Hessian factors in device memory: they enter later eliminations, are never relinearized and add nothing to the nonlinear error), their
 * keys become fixedVariables_ (lmgpu_isam2_get_fixed_variables, ascending; returns their number), the summarised factors' slots empty.
 * n_marginal_out / n_deleted_out: sizes of the two index lists, read with lmgpu_isam2_get_marginalize_result (either may be NULL).
 * A key that is not a leaf is refused BEFORE anything changes (LMGPU_INVALID, lmgpu_isam2_last_failed_key names the variable that is in
 * the way) -- the reference checks this in debug builds only and leaves the object unusable.
 * lmgpu_isam2_get_marginal_factor: parity tap -- slot i as a marginal factor: its keys, their dimensions and the augmented information
 * matrix ((sum dims + 1)^2, column-major, symmetric); returns the number of keys, -1 when slot i holds no marginal factor. */
int lmgpu_isam2_marginalize_leaves(lmgpu_isam2* s, int32_t n, const uint64_t* leaf_keys, int32_t* n_marginal_out, int32_t* n_deleted_out);
int lmgpu_isam2_get_marginalize_result(const lmgpu_isam2* s, uint64_t* marginal_idx_out, uint64_t* deleted_idx_out);
int lmgpu_isam2_get_fixed_variables(const lmgpu_isam2* s, uint64_t* keys_out);
int lmgpu_isam2_get_marginal_factor(lmgpu_isam2* s, int32_t i, uint64_t* keys_out, int32_t* dims_out, double* info_colmajor);
int lmgpu_isam2_num_variables(const lmgpu_isam2* s); /* live variables = theta_.size() */
int lmgpu_isam2_num_factors(const lmgpu_isam2* s);   /* slots of the factor list, removed ones included */
/* which: 0 = calculateEstimate (ISAM2.cpp:748-754), 1 = calculateBestEstimate (:763-766), 2 = getLinearizationPoint.
 * Variables ascending by Key (the reference's Values order); any of the outputs may be NULL. */
int lmgpu_isam2_get_values(lmgpu_isam2* s, int32_t which, uint64_t* keys_out, int32_t* types_out, double* packed_out);
/* calculateEstimate(Key) (ISAM2.cpp:757-760) for which = 0, the linearization point of one variable for which = 2: only this variable
 * is retracted and downloaded (store doubles of its type, lmgpu.h packings); LMGPU_INVALID for an unknown key */
int lmgpu_isam2_get_value(lmgpu_isam2* s, int32_t which, uint64_t key, int32_t* type_out, double* packed_out);
int lmgpu_isam2_get_delta(lmgpu_isam2* s, double* packed); /* getDelta (:776-779), ascending by Key */
/* ISAM2::marginalCovariance(key) (gtsam/nonlinear/ISAM2.h:253-257: the inverse of BayesTree::marginalFactor(key)'s information; the
 * linearization point's covariance block of the variable, dim x dim): two triangular solves per column, on the device, along the path
 * from the variable's clique to its root.  LMGPU_INVALID for a variable that is not in the tree. */
int lmgpu_isam2_marginal_covariance(lmgpu_isam2* s, uint64_t key, double* cov);
/* ---- marginals of MANY variables, cross-covariances and joint marginals from the tree the last update left on the device (DESIGN section
 *      19; BayesTree::joint, gtsam/inference/BayesTree.h:181-187, without refactoring the graph).  Nothing is re-linearized or re-eliminated:
 *      the blocks are blocks of (R^T R)^-1 of the PRESENT tree, i.e. the covariance at the LINEARIZATION POINT, which is what
 *      ISAM2::marginalCovariance gives.  The walk is lmgpu_marginal_covariances' / lmgpu_marginal_cross_covariances' (above): one
 *      workgroup per source variable, up its path with R^T y = e, down again with R x = y, then down each target's branch below the
 *      junction; the work vector holds the frontal scalars of the walked path only (LDS, or a slice of the scratch buffer).  One launch,
 *      one download and one wait per chunk of requests.  Packing is that of the batch entries: row-major blocks back to back in request
 *      order; a cross block is Sigma[i, j], dim_i x dim_j, the columns those of j, the source; a joint matrix is D_q x D_q with the blocks in
 *      the order of the set's keys.  Duplicates are allowed in the first two calls, a key twice in one joint set is LMGPU_INVALID; n == 0
 *      is LMGPU_OK.  LMGPU_INVALID, nothing written, the handle usable afterwards: a key that is not in the Bayes tree (never added, gone
 *      with its last factor, marginalized), a NULL array that is needed, n < 0, set_begin that decreases or starts below 0, a single work
 *      vector beyond scratch_bytes.  LMGPU_INDETERMINATE: a non-finite block (lmgpu_isam2_last_failed_key: the source of the first such
 *      workgroup).  LMGPU_HIP_ERROR for n > 0 on a handle without a device.
 *      A block's bits depend on its pair and the tree alone -- not on the rest of the request, its order, the chunking, LDS or scratch
 *      placement, or targets_per_workgroup; the (i, i) cross block is bitwise the marginal_covariances block of i; a joint matrix is exactly
 *      symmetric (an off-diagonal block is computed once, from the variable of the pair with the shorter path -- fewer scalars; ties: the
 *      smaller key -- as the source, and mirrored); a pair across two trees of a forest gives exact zeros.
 *      lmgpu_isam2_marginal_covariance above keeps its own route. ---- */
int lmgpu_isam2_marginal_covariances(lmgpu_isam2* s, int32_t n, const uint64_t* keys, double* cov_packed);
int lmgpu_isam2_cross_covariances(lmgpu_isam2* s, int32_t n, const uint64_t* keys_i, const uint64_t* keys_j, double* out_packed);
int lmgpu_isam2_joint_marginal_covariances(lmgpu_isam2* s, int32_t n_sets, const int32_t* set_begin /* n_sets + 1 */, const uint64_t* keys,
                                           double* cov_packed);
/* structure taps (no device needed), cliques named by their first frontal key.  path: the cliques from the one `key` is frontal in to its
 * root into first_frontal_keys_out[0 .. cap) (may be NULL); returns the path length, -1 refused.  junction: the deepest clique on both
 * paths; returns 1 (and the clique), 0 when the keys lie in two trees of a forest, -1 refused. */
int lmgpu_isam2_marginals_path(lmgpu_isam2* s, uint64_t key, uint64_t* first_frontal_keys_out, int32_t cap);
int lmgpu_isam2_marginals_junction(lmgpu_isam2* s, uint64_t key_i, uint64_t key_j, uint64_t* first_frontal_key_out);
/* as lmgpu_set_marginals_params + lmgpu_set_marginals_cross_cap (defaults 64 MiB, 6144 doubles, the built-in rule); 0 keeps a value.
 * Results do not depend on any of the three. */
int lmgpu_isam2_set_marginals_params(lmgpu_isam2* s, int64_t scratch_bytes, int32_t lds_doubles, int32_t targets_per_workgroup);
/* lmgpu_marginals_stats over the handle's life: launches / chunks / vars_* / longest_path count lmgpu_isam2_marginal_covariances, the
 * cross_* fields the other two calls; factorizations stays 0 */
int lmgpu_isam2_get_marginals_stats(lmgpu_isam2* s, lmgpu_marginals_stats* out);
/* parity taps: the Bayes tree depth-first from the roots (children in order).  lmgpu_isam2_num_cliques takes the snapshot the
 * other two index; info5: n_keys, n_frontal_keys, nf, n, parent (index in the snapshot, -1 root); RSd column-major nf x n */
int lmgpu_isam2_num_cliques(lmgpu_isam2* s);
int lmgpu_isam2_clique_info(const lmgpu_isam2* s, int32_t i, int32_t* info5);
int lmgpu_isam2_get_clique(lmgpu_isam2* s, int32_t i, uint64_t* keys, double* RSd_colmajor);

#ifdef LMGPU_TEST_HOOKS
/* TEST HOOKS -- exported by liblmgpu_test.so only (csrc/Makefile builds it with -DLMGPU_TEST_HOOKS); the product library has none of them.
 * In-process stand-in for the RCCL communicator: W handles created by W threads of ONE process on one
 * device sum their buffers through a host rendezvous, at exactly the call sites where the RCCL path all-reduces.
 * Lets the sharded LM loop run end to end on a single GPU.  Every rank must drive its handle from its own thread. */
typedef struct lmgpu_local_group lmgpu_local_group;
int lmgpu_local_group_create(int32_t world_size, lmgpu_local_group** out);
int lmgpu_local_group_destroy(lmgpu_local_group* g);
int lmgpu_comm_init_local(lmgpu_handle* h, lmgpu_local_group* g);
/* The launch tables finalize built, as digests: one record per table that is uploaded and per piece of the host launch metadata (the
 * level work lists in the parts the build phases fill, gather ranges, merged segments, block-solve runs, pool layout, solve-form
 * flags) -- its name (32 bytes, zero-terminated), its number of entries and the FNV-1a of its fields.  Available on structure-only
 * handles too.  Writes at most `max` records; returns the number of records the handle has, or -1 before finalize. */
int lmgpu_debug_table_digest(lmgpu_handle* h, int32_t max, char* names32, uint64_t* counts, uint64_t* fnv1a);
/* The kernels of the nonlinear conjugate gradient optimizer (csrc/kernels_ncg.hpp) on caller data, launched as lmgpu_ncg_* launches them
 * (the same block counts: the grid rule is one function both call).  They need a device and no graph; every call allocates, runs on a
 * stream of its own, waits and frees.  lmgpu_debug_ncg_ctl is the device's line-search record field for field. */
typedef struct lmgpu_debug_ncg_ctl {
  double minStep, maxStep, newStep, newError, step, alpha, error, beta, dnorm;
  int32_t done, trials, flag, first;
} lmgpu_debug_ncg_ctl;
/* method 0..3 (LMGPU_NCG_*): the dot-product partials of (g, gp, dir), beta, dir = g + beta * dir, then the head of the line search.
 * method -1: dir = src and its squared-norm partials instead (beta = 0), src = g (alias 0; gp is not read) or src = dir itself (alias 1: g is
 * uploaded and not read).  dir (n doubles) is read and overwritten.  parts5: 5 x 256 doubles, the block partials of g.g, g.(g - gp),
 * gp.gp, dir.(g - gp) and of the new dir.dir; every entry is preset to NaN, so an entry at or beyond *npart_out (and all of the first four
 * rows under method -1) reads as NaN.  ctl_out: the record after ncg_ls_begin_kernel, preset to all-ones bytes before the first kernel. */
int lmgpu_debug_ncg_direction(int32_t device, int32_t n, int32_t method, int32_t alias, const double* g, const double* gp, double* dir,
                              double* parts5, int32_t* npart_out, lmgpu_debug_ncg_ctl* ctl_out);
/* ncg_ls_control_kernel k times on one stream from the record *ctl_in, launch i reading errors[i]; records_out[i] = the record after
 * launch i.  final != 0: ncg_final_kernel afterwards, reading errors[k], its record in records_out[k]. */
int lmgpu_debug_ncg_ls_control(int32_t device, const lmgpu_debug_ncg_ctl* ctl_in, int32_t k, const double* errors, int32_t final,
                               lmgpu_debug_ncg_ctl* records_out);
/* out2[0]: ncg_reduce_stage1 / 2 over buf[0 .. n) with the skip flag set to `skip` (skip < 0: no flag at all); out2[1]: the product's
 * reduce_to over the same buffer.  Both destinations hold `sentinel` before. */
int lmgpu_debug_ncg_reduce(int32_t device, int32_t n, const double* buf, int32_t skip, double sentinel, double* out2);
#endif

/* ---- micro-benchmarks used by bench.py for roofline peaks (device-only, no graph needed) ---- */
int lmgpu_peak_mfma_f64(int32_t device, int32_t iters, double* tflops);
/* the same loop with n_acc (4, 8, or 16 = the 4 x 4 accumulators and 4 + 4 operand registers of the update tile's 64x64 wave tile, two
 * workgroups per CU) independent accumulators, measured after ~1 s of back-to-back launches, together with the shader
 * clock the chip HOLDS under that load (in-kernel s_memtime / s_memrealtime stamps) and the resulting flop per clock and SIMD:
 * 32 = one v_mfma_f64_16x16x4_f64 per 64 cycles, the issue rate behind the 78.6 TFLOP/s datasheet figure at 2.4 GHz */
int lmgpu_peak_mfma_f64_clock(int32_t device, int32_t iters, int32_t n_acc, double* tflops, double* sclk_mhz, double* flop_per_clk_simd);
int lmgpu_peak_hbm_copy(int32_t device, int64_t bytes, int32_t iters, double* gbps);

#ifdef __cplusplus
}
#endif
#endif /* LMGPU_H */
