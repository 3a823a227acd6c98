// NonlinearConjugateGradientOptimizer on the device (gtsam/nonlinear/NonlinearConjugateGradientOptimizer.h, .cpp): host side of the
// lmgpu_ncg_* group and lmgpu_gradient.  Included by lmgpu.hip after the handle's own entry points.  The optimizer needs no
// factorisation: it runs on a handle finalized for Cholesky or for PCG alike, on the existing linearize / error launches of every
// factor type plus the kernels of kernels_ncg.hpp.  Per NCG iteration the host queues linearize, the gradient gather, the direction
// update, the whole golden-section line search and the final advance with its error, and waits ONCE for the record (alpha, error,
// trials); a line search that has not finished within the first queue of trials costs one more wait per further queue.
#pragma once

#include "kernels_ncg.hpp"

// Trials of one line search.  The bracket starts as [-1 / |d|, 0] and loses the factor 1 / phi = 0.618 per trial; the search stops
// once (maxStep - minStep) < tau (|testStep| + |newStep|), tau = 1e-5 (.h:143, 155).  With the minimiser at -r / |d| the right-hand
// side is about 2 tau r / |d|, so the search ends after n = 1 + ceil(log(2 tau r) / log(0.618)) evaluations: 24 for r = 1 (the widest
// bracket relative to the step), 29 for r = 0.1, 39 for r = 1e-3.  NCG_TRIALS_FIRST trials are queued before the host looks (every
// kernel of a trial behind `done` returns at once on the flag: a surplus trial costs its launches only); if `done` is not set it queues NCG_TRIALS_MORE at a time up to NCG_MAX_TRIALS = 128 (r down to 1e-22), then reports an error: the reference
// would still be looping there (a minimiser AT 0 never meets its exit test).
#define NCG_TRIALS_FIRST 40
#define NCG_TRIALS_MORE 44
#define NCG_MAX_TRIALS 128

struct NcgState {
  double *g[2] = {nullptr, nullptr}, *dir = nullptr, *part = nullptr, *part_dd = nullptr;  // g[cur_g] = currentGradient, the other prevGradient
  int cur_g = 0;
  lmgpu::NcgCtl* ctl = nullptr;
  lmgpu::NcgCtl* h_ctl = nullptr;  // pinned
  std::vector<double> trace;       // per line search of the last run: alpha, beta, error, trials
  int host_waits = 0;              // host synchronisations of the last run
};

static void ncg_release(lmgpu_handle* h) {
  NcgState* s = h->ncg;
  if (!s) return;
  void* ptrs[] = {s->g[0], s->g[1], s->dir, s->part, s->part_dd, s->ctl};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (s->h_ctl) (void)hipHostFree(s->h_ctl);
  delete s;
  h->ncg = nullptr;
}

namespace {

int ncg_allocate(lmgpu_handle* h) {
  NcgState* s = h->ncg;
  const size_t nb = std::max(1, h->ntot) * sizeof(double);
  HIPCHECK(hipMalloc((void**)&s->g[0], nb));
  HIPCHECK(hipMalloc((void**)&s->g[1], nb));
  HIPCHECK(hipMalloc((void**)&s->dir, nb));
  HIPCHECK(hipMalloc((void**)&s->part, 4 * NCG_MAXPART * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&s->part_dd, NCG_MAXPART * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&s->ctl, sizeof(NcgCtl)));
  HIPCHECK(hipMemset(s->ctl, 0, sizeof(NcgCtl)));
  HIPCHECK(hipHostMalloc((void**)&s->h_ctl, sizeof(NcgCtl), hipHostMallocDefault));
  return LMGPU_OK;
}

// h->ncg is either complete or null: a failed allocation releases what it got, and the next call tries again
int ncg_ensure(lmgpu_handle* h) {
  if (h->ncg) return LMGPU_OK;
  h->ncg = new NcgState();
  const int rc = ncg_allocate(h);
  if (rc) ncg_release(h);
  return rc;
}

// the device's copy of the tangent dimensions (var_tangent_dim, used by the scaled retract) is the host's table
static_assert(kNumVarTypes == 7 && sizeof(kVarDim) / sizeof(kVarDim[0]) == 7, "var_tangent_dim covers seven variable types");
static_assert(var_tangent_dim(0) == kVarDim[0] && var_tangent_dim(1) == kVarDim[1] && var_tangent_dim(2) == kVarDim[2] &&
                  var_tangent_dim(3) == kVarDim[3] && var_tangent_dim(4) == kVarDim[4] && var_tangent_dim(5) == kVarDim[5] &&
                  var_tangent_dim(6) == kVarDim[6],
              "var_tangent_dim (kernels_factors.hpp) and kVarDim (factor_types.hpp) disagree");

// the three states the group refuses
int ncg_check(lmgpu_handle* h, const char* who) {
  if (smart_refused(h, who)) return LMGPU_INVALID;
  if (!h->finalized || !h->have_values) {
    h->err = std::string(who) + ": refused (no values: lmgpu_finalize_structure and lmgpu_set_values come first)";
    return LMGPU_INVALID;
  }
  if (h->gnc_on) {
    h->err = std::string(who) + ": refused (GNC is enabled on this handle; nonlinear conjugate gradient under GNC is not bound)";
    return LMGPU_INVALID;
  }
  if (h->cfg.world_size > 1 || h->comm || h->lgroup) {
    h->err = std::string(who) + ": refused (multi-rank handle; nonlinear conjugate gradient is single-rank)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  return ncg_ensure(h);
}

// blocks of the direction kernels over ntot scalars = block partials per dot product; the kernels stride beyond NCG_MAXPART blocks
int ncg_grid(int ntot) { return std::min(NCG_MAXPART, std::max(1, (ntot + 255) / 256)); }
// blocks of ncg_reduce_stage1 over n error terms: reduce_to's rule (lmgpu.hip), so that the partial sums are the same
int ncg_reduce_grid(int n) { return std::min(256, std::max(1, (n + 255) / 256)); }

// System::gradient at the current values -> g[cur_g] (queued)
int ncg_enqueue_gradient(lmgpu_handle* h) {
  NcgState* s = h->ncg;
  int rc = do_linearize(h);
  if (rc) return rc;
  hipLaunchKernelGGL(ncg_gradient_kernel, dim3(std::max(1, (h->ntot + 255) / 256)), dim3(256), 0, h->stream, h->ntot, (const int32_t*)h->d_scalar_var,
                     (const int32_t*)h->d_scalar_col, (const int32_t*)h->d_vi_ptr, (const int32_t*)h->d_vi_fac, (const int8_t*)h->d_vi_pos,
                     (const FacDesc*)h->d_fd, (const double*)h->pool, s->g[s->cur_g]);
  HIPCHECK(hipGetLastError());
  return LMGPU_OK;
}

// direction = src (queued), with the partials of its squared norm
int ncg_enqueue_set_direction(lmgpu_handle* h, const double* src) {
  NcgState* s = h->ncg;
  hipLaunchKernelGGL(ncg_set_direction_kernel, dim3(ncg_grid(h->ntot)), dim3(256), 0, h->stream, h->ntot, src, s->dir, s->part_dd, s->ctl);
  HIPCHECK(hipGetLastError());
  return LMGPU_OK;
}

// beta and direction = currentGradient + beta * direction (queued)
int ncg_enqueue_direction(lmgpu_handle* h, int method) {
  NcgState* s = h->ncg;
  const int g = ncg_grid(h->ntot);
  hipLaunchKernelGGL(ncg_dots_kernel, dim3(g), dim3(256), 0, h->stream, h->ntot, (const double*)s->g[s->cur_g], (const double*)s->g[s->cur_g ^ 1],
                     (const double*)s->dir, s->part);
  hipLaunchKernelGGL(ncg_direction_kernel, dim3(g), dim3(256), 0, h->stream, h->ntot, method, (const double*)s->part, g,
                     (const double*)s->g[s->cur_g], s->dir, s->part_dd, s->ctl);
  HIPCHECK(hipGetLastError());
  return LMGPU_OK;
}

void ncg_launch_retract(lmgpu_handle* h, int final) {
  NcgState* s = h->ncg;
  for (int t = 0; t < kNumVarTypes; t++) {
    const int n = h->plan.type_count[t];
    if (n == 0) continue;
    hipLaunchKernelGGL(ncg_retract_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, t, n, (const double*)h->vals[h->cur][t],
                       h->vals[h->cur ^ 1][t], (const int32_t*)h->type_xoff[t], (const double*)s->dir, (const NcgCtl*)s->ctl, final);
  }
}

// lineSearch(system, current values, direction) along s->dir, whose squared-norm partials are in part_dd; advance != 0: then
// values[cur ^ 1] = advance(values[cur], alpha, direction) and its error.  One wait when the search ends within the first queue.
// On LMGPU_OK the record is in s->h_ctl; the caller flips h->cur.
int ncg_line_search(lmgpu_handle* h, int advance) {
  NcgState* s = h->ncg;
  hipLaunchKernelGGL(ncg_ls_begin_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)s->part_dd, ncg_grid(h->ntot), s->ctl);
  int queued = 0;
  while (true) {
    const int more = queued == 0 ? NCG_TRIALS_FIRST : std::min(NCG_TRIALS_MORE, NCG_MAX_TRIALS - queued);
    const int32_t* done = &s->ctl->done;
    const int rg = ncg_reduce_grid(h->n_counted);
    for (int k = 0; k < more; k++) {
      ncg_launch_retract(h, 0);
      h->err_skip = done;  // the error launches of a trial behind the exit test return at once too
      const int rc = launch_factors<false>(h, h->cur ^ 1);
      h->err_skip = nullptr;
      if (rc) return rc;
      hipLaunchKernelGGL(ncg_reduce_stage1, dim3(rg), dim3(256), 0, h->stream, (const double*)h->ebuf0, h->n_counted, h->partial, done);
      hipLaunchKernelGGL(ncg_reduce_stage2, dim3(1), dim3(256), 0, h->stream, (const double*)h->partial, rg, h->dscal, done);
      hipLaunchKernelGGL(ncg_ls_control_kernel, dim3(1), dim3(64), 0, h->stream, (const double*)h->dscal, s->ctl);
    }
    queued += more;
    if (advance) {
      ncg_launch_retract(h, 1);
      const int rc = launch_factors<false>(h, h->cur ^ 1);
      if (rc) return rc;
      reduce_to(h, h->ebuf0, h->n_counted, h->dscal);
      hipLaunchKernelGGL(ncg_final_kernel, dim3(1), dim3(64), 0, h->stream, (const double*)h->dscal, s->ctl);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(s->h_ctl, s->ctl, sizeof(NcgCtl), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    s->host_waits += 1;
    if (s->h_ctl->done) break;
    if (queued >= NCG_MAX_TRIALS) {
      char buf[256];
      std::snprintf(buf, sizeof(buf),
                    "nonlinear conjugate gradient: the line search has not met its exit test after %d trials (|direction| = %g, bracket [%g, %g])",
                    queued, s->h_ctl->dnorm, s->h_ctl->minStep, s->h_ctl->maxStep);
      h->err = buf;
      return LMGPU_HIP_ERROR;
    }
  }
  const double row[4] = {s->h_ctl->alpha, s->h_ctl->beta, advance ? s->h_ctl->error : s->h_ctl->newError, (double)s->h_ctl->trials};
  s->trace.insert(s->trace.end(), row, row + 4);
  return LMGPU_OK;
}

// nonlinearConjugateGradient (.h:195-289) from the handle's current values; returns the iteration count, the final error in *err_out
int ncg_run(lmgpu_handle* h, const lmgpu_ncg_params* p, bool singleIteration, int* iterations_out, double* err_out) {
  NcgState* s = h->ncg;
  s->trace.clear();
  s->host_waits = 0;
  int iteration = 0;
  // check if we're already close enough (:205-213)
  double currentError = 0;
  int rc = compute_error(h, h->cur, &currentError);
  if (rc) return rc;
  s->host_waits += 1;
  *iterations_out = 0;
  *err_out = currentError;
  if (currentError <= p->error_tol) return LMGPU_OK;
  // currentGradient = system.gradient(currentValues), direction = currentGradient; one step of gradient descent (:215-224)
  if ((rc = ncg_enqueue_gradient(h))) return rc;
  if ((rc = ncg_enqueue_set_direction(h, s->g[s->cur_g]))) return rc;
  if ((rc = ncg_line_search(h, 1))) return rc;
  h->cur ^= 1;
  h->linearized = h->marg_valid = false;
  double prevError = currentError;
  currentError = s->h_ctl->error;
  do {
    if (p->gradient_descent) {  // direction = system.gradient(currentValues) (:232-233)
      if ((rc = ncg_enqueue_gradient(h))) return rc;
      if ((rc = ncg_enqueue_set_direction(h, s->g[s->cur_g]))) return rc;
    } else {  // prevGradient = currentGradient; currentGradient = system.gradient(currentValues); beta; direction (:235-257)
      s->cur_g ^= 1;
      if ((rc = ncg_enqueue_gradient(h))) return rc;
      if ((rc = ncg_enqueue_direction(h, p->direction_method))) return rc;
    }
    if ((rc = ncg_line_search(h, 1))) return rc;  // alpha = lineSearch(...); currentValues = advance(prevValues, alpha, direction) (:260-266)
    h->cur ^= 1;
    h->linearized = h->marg_valid = false;
    prevError = currentError;
    currentError = s->h_ctl->error;
    *err_out = currentError;
  } while (++iteration < p->max_iterations && !singleIteration &&
           !check_convergence(p->relative_error_tol, p->absolute_error_tol, p->error_tol, prevError, currentError));
  *iterations_out = iteration;
  *err_out = currentError;
  return LMGPU_OK;
}

int ncg_check_params(lmgpu_handle* h, const lmgpu_ncg_params* p, const char* who) {
  if (!p) {
    h->err = std::string(who) + ": refused (!params)";
    return LMGPU_INVALID;
  }
  if (p->direction_method < LMGPU_NCG_FLETCHER_REEVES || p->direction_method > LMGPU_NCG_DAI_YUAN) {
    h->err = std::string(who) + ": Invalid directionMethod";  // the reference throws (.h:252-254)
    return LMGPU_INVALID;
  }
  return LMGPU_OK;
}

}  // namespace

extern "C" {

int lmgpu_gradient(lmgpu_handle* h, double* g_packed) {
  if (!h) return LMGPU_INVALID;
  if (!g_packed) {
    h->err = "lmgpu_gradient: refused (!g_packed)";
    return LMGPU_INVALID;
  }
  int rc = ncg_check(h, "lmgpu_gradient");
  if (rc) return rc;
  NcgState* s = h->ncg;
  if ((rc = ncg_enqueue_gradient(h))) return rc;
  HIPCHECK(hipMemcpyAsync(g_packed, s->g[s->cur_g], h->ntot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->kt.resolve();
  return LMGPU_OK;
}

int lmgpu_ncg_line_search(lmgpu_handle* h, const double* dir_packed, double* alpha, int32_t* trials) {
  if (!h) return LMGPU_INVALID;
  int rc = ncg_check(h, "lmgpu_ncg_line_search");
  if (rc) return rc;
  NcgState* s = h->ncg;
  s->trace.clear();
  s->host_waits = 0;
  if (dir_packed) {
    HIPCHECK(hipMemcpyAsync(s->dir, dir_packed, h->ntot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = ncg_enqueue_set_direction(h, s->dir))) return rc;
  } else {
    if ((rc = ncg_enqueue_gradient(h))) return rc;
    if ((rc = ncg_enqueue_set_direction(h, s->g[s->cur_g]))) return rc;
  }
  if ((rc = ncg_line_search(h, 0))) return rc;  // trial values went to the other value buffer: the handle's values are untouched
  h->kt.resolve();
  if (alpha) *alpha = s->h_ctl->alpha;
  if (trials) *trials = s->h_ctl->trials;
  return LMGPU_OK;
}

int lmgpu_ncg_iterate(lmgpu_handle* h, const lmgpu_ncg_params* p, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  int rc = ncg_check(h, "lmgpu_ncg_iterate");
  if (rc) return rc;
  if ((rc = ncg_check_params(h, p, "lmgpu_ncg_iterate"))) return rc;
  if (inout) h->lm = *inout;
  // NonlinearConjugateGradientOptimizer::iterate (.cpp:71-80): singleIteration = true; State(newValues, error, iterations + 1)
  int it = 0;
  double err = h->lm.error;
  rc = ncg_run(h, p, true, &it, &err);
  h->kt.resolve();
  if (rc == LMGPU_OK) {
    h->lm.error = err;
    h->lm.iterations += 1;
  }
  if (inout) *inout = h->lm;
  return rc;
}

int lmgpu_ncg_optimize(lmgpu_handle* h, const lmgpu_ncg_params* p, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  int rc = ncg_check(h, "lmgpu_ncg_optimize");
  if (rc) return rc;
  if ((rc = ncg_check_params(h, p, "lmgpu_ncg_optimize"))) return rc;
  if (inout) h->lm = *inout;
  // NonlinearConjugateGradientOptimizer::optimize (.cpp:82-90): State(newValues, error, iterations)
  int it = 0;
  double err = h->lm.error;
  rc = ncg_run(h, p, false, &it, &err);
  h->kt.resolve();
  if (rc == LMGPU_OK) {
    h->lm.error = err;
    h->lm.iterations = it;
  }
  if (inout) *inout = h->lm;
  return rc;
}

int lmgpu_ncg_get_trace(const lmgpu_handle* h, int32_t max_rows, double* rows4) {
  if (!h || !h->ncg) return 0;
  const int n = (int)(h->ncg->trace.size() / 4);
  if (rows4)
    for (int i = 0; i < std::min(n, (int)max_rows) * 4; i++) rows4[i] = h->ncg->trace[i];
  return n;
}

int lmgpu_ncg_host_waits(const lmgpu_handle* h) { return (h && h->ncg) ? h->ncg->host_waits : 0; }

}  // extern "C"

#ifdef LMGPU_TEST_HOOKS
// ---- TEST HOOKS (liblmgpu_test.so only; include/lmgpu.h): the kernels of kernels_ncg.hpp on caller data, launched with the shapes and
//      the grid rules of the path above (ncg_grid, ncg_reduce_grid, reduce_to).  They need a device and no graph.
namespace {

static_assert(sizeof(lmgpu_debug_ncg_ctl) == sizeof(NcgCtl) && offsetof(lmgpu_debug_ncg_ctl, step) == offsetof(NcgCtl, step) &&
                  offsetof(lmgpu_debug_ncg_ctl, alpha) == offsetof(NcgCtl, alpha) && offsetof(lmgpu_debug_ncg_ctl, error) == offsetof(NcgCtl, error) &&
                  offsetof(lmgpu_debug_ncg_ctl, beta) == offsetof(NcgCtl, beta) && offsetof(lmgpu_debug_ncg_ctl, dnorm) == offsetof(NcgCtl, dnorm) &&
                  offsetof(lmgpu_debug_ncg_ctl, done) == offsetof(NcgCtl, done) && offsetof(lmgpu_debug_ncg_ctl, trials) == offsetof(NcgCtl, trials) &&
                  offsetof(lmgpu_debug_ncg_ctl, flag) == offsetof(NcgCtl, flag) && offsetof(lmgpu_debug_ncg_ctl, first) == offsetof(NcgCtl, first),
              "lmgpu_debug_ncg_ctl (lmgpu.h) is NcgCtl (kernels_ncg.hpp) field for field");

// device memory and the stream of one hook call
struct NcgDebugMem {
  std::vector<void*> dev;
  hipStream_t stream = nullptr;
  ~NcgDebugMem() {
    for (void* p : dev) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
  }
  template <typename T>
  T* alloc(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T)) != hipSuccess) return nullptr;
    dev.push_back(p);
    return (T*)p;
  }
};

#define NCG_DEBUG_CHECK(expr)                           \
  do {                                                  \
    if ((expr) != hipSuccess) return LMGPU_HIP_ERROR;   \
  } while (0)

}  // namespace

extern "C" {

int lmgpu_debug_ncg_direction(int32_t device, int32_t n, int32_t method, int32_t alias, const double* g, const double* gp, double* dir,
                              double* parts5, int32_t* npart_out, lmgpu_debug_ncg_ctl* ctl_out) {
  if (n < 1 || method < -1 || method > LMGPU_NCG_DAI_YUAN || !g || !dir || !parts5 || !npart_out || !ctl_out || (method >= 0 && !gp))
    return LMGPU_INVALID;
  NCG_DEBUG_CHECK(hipSetDevice(device));
  NcgDebugMem m;
  NCG_DEBUG_CHECK(hipStreamCreate(&m.stream));
  double *dg = m.alloc<double>(n), *dgp = m.alloc<double>(n), *ddir = m.alloc<double>(n), *dpart = m.alloc<double>(5 * NCG_MAXPART);
  NcgCtl* dctl = m.alloc<NcgCtl>(1);
  if (!dg || !dgp || !ddir || !dpart || !dctl) return LMGPU_HIP_ERROR;
  const size_t nb = (size_t)n * sizeof(double);
  NCG_DEBUG_CHECK(hipMemcpyAsync(dg, g, nb, hipMemcpyHostToDevice, m.stream));
  if (method >= 0) NCG_DEBUG_CHECK(hipMemcpyAsync(dgp, gp, nb, hipMemcpyHostToDevice, m.stream));
  NCG_DEBUG_CHECK(hipMemcpyAsync(ddir, dir, nb, hipMemcpyHostToDevice, m.stream));
  NCG_DEBUG_CHECK(hipMemsetAsync(dpart, 0xFF, 5 * NCG_MAXPART * sizeof(double), m.stream));  // a partial nobody wrote reads as NaN
  NCG_DEBUG_CHECK(hipMemsetAsync(dctl, 0xFF, sizeof(NcgCtl), m.stream));
  const int grid = ncg_grid(n);
  double* dpart_dd = dpart + 4 * NCG_MAXPART;
  if (method < 0) {
    hipLaunchKernelGGL(ncg_set_direction_kernel, dim3(grid), dim3(256), 0, m.stream, n, alias ? (const double*)ddir : (const double*)dg, ddir, dpart_dd,
                       dctl);
  } else {
    hipLaunchKernelGGL(ncg_dots_kernel, dim3(grid), dim3(256), 0, m.stream, n, (const double*)dg, (const double*)dgp, (const double*)ddir, dpart);
    hipLaunchKernelGGL(ncg_direction_kernel, dim3(grid), dim3(256), 0, m.stream, n, method, (const double*)dpart, grid, (const double*)dg, ddir,
                       dpart_dd, dctl);
  }
  hipLaunchKernelGGL(ncg_ls_begin_kernel, dim3(1), dim3(256), 0, m.stream, (const double*)dpart_dd, grid, dctl);
  NCG_DEBUG_CHECK(hipGetLastError());
  NCG_DEBUG_CHECK(hipMemcpyAsync(dir, ddir, nb, hipMemcpyDeviceToHost, m.stream));
  NCG_DEBUG_CHECK(hipMemcpyAsync(parts5, dpart, 5 * NCG_MAXPART * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  NCG_DEBUG_CHECK(hipMemcpyAsync(ctl_out, dctl, sizeof(NcgCtl), hipMemcpyDeviceToHost, m.stream));
  NCG_DEBUG_CHECK(hipStreamSynchronize(m.stream));
  *npart_out = grid;
  return LMGPU_OK;
}

int lmgpu_debug_ncg_ls_control(int32_t device, const lmgpu_debug_ncg_ctl* ctl_in, int32_t k, const double* errors, int32_t final,
                               lmgpu_debug_ncg_ctl* records_out) {
  if (!ctl_in || k < 0 || k > 4096 || !errors || !records_out || (k == 0 && !final)) return LMGPU_INVALID;
  NCG_DEBUG_CHECK(hipSetDevice(device));
  NcgDebugMem m;
  NCG_DEBUG_CHECK(hipStreamCreate(&m.stream));
  const int nrec = k + (final ? 1 : 0);
  double* derr = m.alloc<double>(nrec);
  NcgCtl *dctl = m.alloc<NcgCtl>(1), *drec = m.alloc<NcgCtl>(nrec);
  if (!derr || !dctl || !drec) return LMGPU_HIP_ERROR;
  NCG_DEBUG_CHECK(hipMemcpyAsync(derr, errors, nrec * sizeof(double), hipMemcpyHostToDevice, m.stream));
  NCG_DEBUG_CHECK(hipMemcpyAsync(dctl, ctl_in, sizeof(NcgCtl), hipMemcpyHostToDevice, m.stream));
  for (int i = 0; i < nrec; i++) {
    if (i < k)
      hipLaunchKernelGGL(ncg_ls_control_kernel, dim3(1), dim3(64), 0, m.stream, (const double*)(derr + i), dctl);
    else
      hipLaunchKernelGGL(ncg_final_kernel, dim3(1), dim3(64), 0, m.stream, (const double*)(derr + i), dctl);
    NCG_DEBUG_CHECK(hipMemcpyAsync(drec + i, dctl, sizeof(NcgCtl), hipMemcpyDeviceToDevice, m.stream));
  }
  NCG_DEBUG_CHECK(hipGetLastError());
  NCG_DEBUG_CHECK(hipMemcpyAsync(records_out, drec, nrec * sizeof(NcgCtl), hipMemcpyDeviceToHost, m.stream));
  NCG_DEBUG_CHECK(hipStreamSynchronize(m.stream));
  return LMGPU_OK;
}

int lmgpu_debug_ncg_reduce(int32_t device, int32_t n, const double* buf, int32_t skip, double sentinel, double* out2) {
  if (n < 1 || !buf || !out2) return LMGPU_INVALID;
  NCG_DEBUG_CHECK(hipSetDevice(device));
  NcgDebugMem m;
  NCG_DEBUG_CHECK(hipStreamCreate(&m.stream));
  double *dbuf = m.alloc<double>(n), *dpartial = m.alloc<double>(2 * 256), *dout = m.alloc<double>(2);
  int32_t* dskip = m.alloc<int32_t>(1);
  if (!dbuf || !dpartial || !dout || !dskip) return LMGPU_HIP_ERROR;
  const double preset[2] = {sentinel, sentinel};
  const int32_t skip_value = skip < 0 ? 0 : skip;
  NCG_DEBUG_CHECK(hipMemcpyAsync(dbuf, buf, (size_t)n * sizeof(double), hipMemcpyHostToDevice, m.stream));
  NCG_DEBUG_CHECK(hipMemcpyAsync(dout, preset, sizeof(preset), hipMemcpyHostToDevice, m.stream));
  NCG_DEBUG_CHECK(hipMemcpyAsync(dskip, &skip_value, sizeof(int32_t), hipMemcpyHostToDevice, m.stream));
  NCG_DEBUG_CHECK(hipMemsetAsync(dpartial, 0xFF, 2 * 256 * sizeof(double), m.stream));
  const int rg = ncg_reduce_grid(n);
  const int32_t* skip_ptr = skip < 0 ? nullptr : dskip;  // skip < 0: the kernels' form without a flag
  hipLaunchKernelGGL(ncg_reduce_stage1, dim3(rg), dim3(256), 0, m.stream, (const double*)dbuf, n, dpartial, skip_ptr);
  hipLaunchKernelGGL(ncg_reduce_stage2, dim3(1), dim3(256), 0, m.stream, (const double*)dpartial, rg, dout, skip_ptr);
  reduce_to(nullptr, dbuf, n, dout + 1, m.stream, dpartial + 256);  // stream and scratch given: the handle is not read
  NCG_DEBUG_CHECK(hipGetLastError());
  NCG_DEBUG_CHECK(hipMemcpyAsync(out2, dout, 2 * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  NCG_DEBUG_CHECK(hipStreamSynchronize(m.stream));
  return LMGPU_OK;
}

}  // extern "C"
#undef NCG_DEBUG_CHECK
#endif  // LMGPU_TEST_HOOKS
