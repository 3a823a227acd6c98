// liblmgpu — C ABI (include/lmgpu.h) over the HIP engine.  gfx950 only; no CPU fallback: every compute entry
// point fails with LMGPU_HIP_ERROR when no device is bound.
//
// Host-side pieces in this file:
//   * graph intake + symbolic plan (plan.cpp) -> device descriptors
//   * the level-scheduled multifrontal solve (LDS fronts batched per level, HBM fronts blocked on MFMA)
//   * the LM control loop: a restatement of LevenbergMarquardtOptimizer::iterate / tryLambda
//     (gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:121-308) and NonlinearOptimizer::defaultOptimize
//     (gtsam/nonlinear/NonlinearOptimizer.cpp:62-117) that only reads three scalars back per inner iteration.
//   * multi-GPU: the subtrees hanging below the replicated top (HBM) fronts are dealt to the ranks; each rank
//     linearizes / eliminates / back-substitutes its own subtrees; the partial assembly of a replicated top front is summed
//     over the ranks in 256-row chunks (ncclAllReduce on a communication stream, RCCL over xGMI) and folded into the
//     working matrix just before each panel is factored; error scalars with a 3-double all-reduce.
//   * Gauss-Newton and Dogleg on the same device-resident graph / Bayes tree (gn_iterate, dl_iterate).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <limits>
#include <mutex>
#include <string>
#include <map>
#include <vector>

#include "../../include/lmgpu.h"
#include "kernels_dense.hpp"
#include "kernels_potrf.hpp"
#include "kernels_step.hpp"
#include "dense_schedule.hpp"
#include "dogleg_step.hpp"
#include "kernels_batched.hpp"
#include "kernels_level.hpp"
#include "kernels_bayes.hpp"
#include "kernels_schur.hpp"
#include "kernels_pcg.hpp"
#include "kernels_gnc.hpp"
#include "kernels_ncg.hpp"
#include "kernels_marginals.hpp"
#include "kernels_isam2_marginals.hpp"
#include "plan.hpp"

// Development switches (A/B forms of the same arithmetic, cross-checked by tests/test_gpu_lookahead.py): read from the environment by the
// TEST library only (liblmgpu_test.so, -DLMGPU_TEST_HOOKS).  The product library has two: LMGPU_GRAPH (graph replay on / off) and
// LMGPU_ISAM2_TRACE (phase times of the incremental path on stderr).  The batch path's are listed in DevSwitches below.
static const char* dev_switch(const char* name) {
#ifdef LMGPU_TEST_HOOKS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}


using namespace lmgpu;

// Every development switch of the batch path, read ONCE, when the handle is created (read_dev_switches): a test sets them before it
// builds its optimizer.  (ISAM2's LMGPU_ISAM2_* switches are read per call on a live handle: isam2.hpp.)
// Tri-state switches: -1 = unset, the structure decides (build_solve_flags).
struct DevSwitches {
  // ---- dense fronts on the per-front path (dense_schedule.hpp, kernels_potrf.hpp, kernels_step.hpp)
  bool two_launch_panel = false;  // LMGPU_PANEL_2L=1: diag_potrf + panel_trsm for every outer panel (A/B)
  bool no_fuse = false;           // LMGPU_NO_FUSE=1: trailing update and next panel as separate launches (A/B)
  bool no_chain = false;          // LMGPU_NO_CHAIN=1: one launch per fused step instead of one per run of steps (A/B)
  bool no_tail = false;           // LMGPU_NO_TAIL=1: the end of a front as separate update / panel launches (A/B)
  bool tail_scalar = false;       // LMGPU_TAIL_SCALAR=1: front_tail_scalar_kernel, the LDS / scalar-FMA form (cross-check)
  int chain_forms = 0;            // CHAIN_FORM_* bits: LMGPU_CHAIN_FENCED_TILES, LMGPU_CHAIN_PREREAD (kernels_step.hpp)
  bool chain_one_task = true;     // a chained launch as one workgroup per task (the product's form; LMGPU_CHAIN_ONE_TASK=1 says so explicitly) ...
  int chain_grid = 0;             // ... LMGPU_CHAIN_GRID=<n>: as resident workgroups that draw tickets in a loop, n of them (0: min(tasks, resident workgroups)) (A/B)
  bool chain_merge = true;        // LMGPU_NO_MERGE: update tiles one step per pass instead of pairs of steps (chain_schedule)
  int chain_split_pct = 60;       // LMGPU_CHAIN_SPLIT: share of a block's update tasks listed in front of its row-panel workgroups
  int chain_far_pct = 50;         // LMGPU_CHAIN_FAR: tile rows beyond this percentage of the front are scheduled late (chain_schedule)
  bool no_med = false;            // LMGPU_NO_MED: one-panel fronts on the per-front path instead of the batched launches per level
  // ---- Schur-form assembly (kernels_schur.hpp)
  bool no_gather_write = false;   // LMGPU_NO_GATHER_WRITE=1: clear the front and add (A/B)
  bool schur_split_diag = false;  // LMGPU_SCHUR_SPLIT_DIAG: (v, v) and (v, rhs) as pair blocks + schur_factor_kernel (A/B)
  bool schur_unmasked = false;    // LMGPU_SCHUR_UNMASKED: operand loads by every lane instead of only the lanes holding an element
  // ---- LDS fronts (kernels_front.hpp, kernels_leaf.hpp, kernels_level.hpp)
  bool no_wide16 = false;         // LMGPU_NO_WIDE16=1: LDS fronts always with four waves (A/B)
  int wide16_max = 256;           // LMGPU_WIDE16_MAX: launches of at most this many wide LDS fronts take sixteen waves per front
  bool no_leaf_groups = false;    // LMGPU_NO_LEAF_GROUPS: lds_front_kernel<true> where lds_front_group_kernel would run (A/B)
  bool no_leafpack = false;       // LMGPU_NO_LEAFPACK: no packed leaf records (and so no leaf groups): the general descriptor path
  int leaf_group_threads = 256;   // LMGPU_LEAF_GROUP_THREADS=64|128|256: workgroup size of lds_front_group_kernel (A/B)
  int merge_elim = -1;            // LMGPU_MERGE_ELIM=0/1: LDS fronts of consecutive levels in one dataflow launch on the way up
  int fuse_levels = -1;           // LMGPU_FUSE_LEVELS=0/1: a level's LDS fronts and medium fronts in one launch
  int fuse_threads = 0;           // LMGPU_FUSE_THREADS=1024: that launch with sixteen waves where its LDS fronts would take them (0: unset)
  // ---- back-substitution
  int merge_backsub = -1;         // LMGPU_MERGE_BACKSUB=0/1: LDS fronts of consecutive levels in one dataflow launch on the way down
  bool no_backsub_groups = false; // LMGPU_NO_BACKSUB_GROUPS: lds_backsub_kernel (a wave per front) where lds_backsub_group_kernel would run (A/B)
  bool bsd_ticket = false;        // LMGPU_BSD_TICKET=1: the block back-substitution always draws tickets (the path of levels with more blocks than CUs)
  bool no_bsd_runs = false;       // LMGPU_NO_BSD_RUNS: the block-solved fronts level by level instead of a run of levels per launch
  bool no_inv16_reuse = false;    // LMGPU_NO_INV16_REUSE: the dense back-solve inverts its diagonal blocks itself (the fallback form)
  bool backsolve_hop64 = false;   // LMGPU_BACKSOLVE_HOP64: 64-row hops (hbm_backsolve_dataflow2_kernel) in place of the 128-row form
  // ---- PCG
  bool pcg_fused = false;         // LMGPU_PCG_FUSED=1: the forward product recomputed inside the transpose gather (A/B)
  // ---- product library as well (plain getenv)
  int graph = -1;                 // LMGPU_GRAPH=0/1: replay the solve's launch sequence as a graph; unset: deep trees do
};

static DevSwitches read_dev_switches() {
  DevSwitches w;
  auto on = [](const char* name) { return dev_switch(name) != nullptr; };
  auto tri = [](const char* e) { return e ? (atoi(e) != 0 ? 1 : 0) : -1; };
  w.two_launch_panel = on("LMGPU_PANEL_2L");
  w.no_fuse = on("LMGPU_NO_FUSE");
  w.no_chain = on("LMGPU_NO_CHAIN");
  w.no_tail = on("LMGPU_NO_TAIL");
  w.tail_scalar = on("LMGPU_TAIL_SCALAR");
  w.chain_forms = (on("LMGPU_CHAIN_FENCED_TILES") ? CHAIN_FORM_FENCED_TILES : 0) | (on("LMGPU_CHAIN_PREREAD") ? CHAIN_FORM_PREREAD : 0);
  if (const char* e = dev_switch("LMGPU_CHAIN_GRID")) {
    w.chain_one_task = on("LMGPU_CHAIN_ONE_TASK");
    w.chain_grid = std::max(0, atoi(e));
  }
  w.chain_merge = !on("LMGPU_NO_MERGE");
  if (const char* e = dev_switch("LMGPU_CHAIN_SPLIT")) w.chain_split_pct = std::max(0, std::min(100, atoi(e)));
  if (const char* e = dev_switch("LMGPU_CHAIN_FAR")) w.chain_far_pct = std::max(10, std::min(100, atoi(e)));
  w.no_med = on("LMGPU_NO_MED");
  w.no_gather_write = on("LMGPU_NO_GATHER_WRITE");
  w.schur_split_diag = on("LMGPU_SCHUR_SPLIT_DIAG");
  w.schur_unmasked = on("LMGPU_SCHUR_UNMASKED");
  w.no_wide16 = on("LMGPU_NO_WIDE16");
  if (const char* e = dev_switch("LMGPU_WIDE16_MAX")) w.wide16_max = atoi(e);
  w.no_leaf_groups = on("LMGPU_NO_LEAF_GROUPS");
  w.no_leafpack = on("LMGPU_NO_LEAFPACK");
  if (const char* e = dev_switch("LMGPU_LEAF_GROUP_THREADS")) w.leaf_group_threads = atoi(e) == 64 ? 64 : (atoi(e) == 128 ? 128 : 256);
  w.merge_elim = tri(dev_switch("LMGPU_MERGE_ELIM"));
  w.fuse_levels = tri(dev_switch("LMGPU_FUSE_LEVELS"));
  if (const char* e = dev_switch("LMGPU_FUSE_THREADS")) w.fuse_threads = atoi(e) == 1024 ? 1024 : 256;
  w.merge_backsub = tri(dev_switch("LMGPU_MERGE_BACKSUB"));
  w.no_backsub_groups = on("LMGPU_NO_BACKSUB_GROUPS");
  w.bsd_ticket = on("LMGPU_BSD_TICKET");
  w.no_bsd_runs = on("LMGPU_NO_BSD_RUNS");
  w.no_inv16_reuse = on("LMGPU_NO_INV16_REUSE");
  w.backsolve_hop64 = on("LMGPU_BACKSOLVE_HOP64");
  w.pcg_fused = on("LMGPU_PCG_FUSED");
  w.graph = tri(getenv("LMGPU_GRAPH"));
  return w;
}

#define HIPCHECK(expr)                                                                         \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      h->err = std::string(#expr) + ": " + hipGetErrorString(_e);                              \
      return LMGPU_HIP_ERROR;                                                                  \
    }                                                                                          \
  } while (0)
#define NCCLCHECK(expr)                                                                        \
  do {                                                                                         \
    ncclResult_t _r = (expr);                                                                  \
    if (_r != ncclSuccess) {                                                                   \
      h->err = std::string(#expr) + ": " + ncclGetErrorString(_r);                             \
      return LMGPU_HIP_ERROR;                                                                  \
    }                                                                                          \
  } while (0)

namespace {

struct Bucket {
  int type = 0, n = 0, noise_kind = 0;  // n = factors given by the caller
  int robust = 0;                       // lmgpu_robust_kind of the whole bucket (noiseModel::Robust around the Gaussian model)
  double robust_k = 0.0;
  std::vector<int32_t> graph_index, slots;
  std::vector<double> meas, noise;
  int rows = 0, cols = 0;  // Jacobian shape (cols includes b)
  // local (this rank's) part
  int n_loc = 0;
  std::vector<int32_t> loc_of;  // caller idx -> local idx inside the bucket, -1 if not evaluated on this rank
  int64_t joff = 0;             // pool offset of the bucket's local Jacobians
  int32_t* d_vidx = nullptr;
  double* d_meas = nullptr;
  double* d_noise = nullptr;
  int32_t* d_epos = nullptr;
};

struct LevelWork {
  // LDS fronts of this level, grouped by LDS-size bin: [bin_begin[b], bin_begin[b+1]) inside the level's list
  int list_begin = 0, list_count = 0;
  int lds_nf_max = 0;  // largest frontal dimension among the level's LDS fronts
  int lds_ns_max = 0;  // largest separator dimension among them
  int lds_rsd_max = 0; // largest nf x (n | 1) among them: doubles of LDS the workgroup-per-front back-substitution stages
  int bin_begin[16] = {0};
  int bin_srows[16] = {0};  // rows of the front kept in LDS for the bin's launch
  int bin_jcap[16] = {0};   // doubles of Jacobian staging per workgroup (largest front of the bin, 96 .. LDSF_JCAP)
  int64_t pack_off[16] = {0};  // byte offset of the launch's packed leaf records in d_leafpack, and their stride (0: none)
  int pack_stride[16] = {0};
  uint8_t bin_group[16] = {0};  // the bin's launch takes lds_front_group_kernel (kernels_leaf.hpp): 1 = nf <= 3 and binary factors of at most two rows, 2 = the caps
  int bin_group_out[16] = {0}, bin_group_maxfac[16] = {0};  // ... the largest nf x n and the largest number of factors among its leaves
  std::vector<int> hbm;  // HBM fronts of this level
  int small_begin = 0, small_count = 0;  // those with nf <= BSS_MAX_NF, in d_hbm_small: back-substituted in one launch per level
  int bsd_begin = 0, bsd_count = 0;      // their 64-row blocks in d_bsd_table (hbm_backsolve_blocks_kernel: one workgroup per block)
  // "medium" HBM fronts (one outer panel, no gather leaves, not replicated): eliminated with batched launches (kernels_batched.hpp)
  int med_begin = 0, med_count = 0, med_max_fac = 0, med_max_child = 0, med_max_nf = 0, med_max_cols = 0, med_max_n = 0;
  // LDS fronts + medium fronts of the level as ONE launch (level_fused_kernel): its slice of d_level_tasks, the LDS size class of the launch
  int fuse_task_begin = 0, fuse_task_count = 0, fuse_nmax = 0, fuse_jcap = 0, fuse_threads = 0;
};

struct KTimer {
  bool on = false;
  bool dominant_only = false;  // lmgpu_set_kernel_timing(h, 2): only the roofline kernels (LINEARIZE; CHAIN, or SYRK = the per-step form of the same work) carry events
  std::vector<hipEvent_t> pool;
  struct Rec {
    int cat, e0, e1, launches;
  };
  std::vector<Rec> recs;
  int used = 0;
  double ms[LMGPU_KT_NUM] = {0}, work[LMGPU_KT_NUM] = {0};
  long long cnt[LMGPU_KT_NUM] = {0};
  int grab() {
    if (used == (int)pool.size()) {
      hipEvent_t e;
      (void)hipEventCreate(&e);
      pool.push_back(e);
    }
    return used++;
  }
  int begin(int cat, hipStream_t s) {
    if (!on || (dominant_only && cat != LMGPU_KT_LINEARIZE && cat != LMGPU_KT_CHAIN && cat != LMGPU_KT_SYRK)) return -1;
    const int e = grab();
    (void)hipEventRecord(pool[e], s);
    recs.push_back({cat, e, -1, 1});
    return (int)recs.size() - 1;
  }
  // `launches` back-to-back launches of one kernel may share one begin / end pair (an event record between two
  // launches costs ~8 us of idle device time: measured 35 x 11 us on the root's step kernels)
  void end(int r, hipStream_t s, double w = 0, int launches = 1) {
    if (!on || r < 0) return;
    const int e = grab();
    (void)hipEventRecord(pool[e], s);
    recs[r].e1 = e;
    recs[r].launches = launches;
    work[recs[r].cat] += w;
  }
  void resolve() {  // call after the stream is synchronised
    for (const Rec& r : recs) {
      float t = 0;
      if (r.e1 >= 0 && hipEventElapsedTime(&t, pool[r.e0], pool[r.e1]) == hipSuccess) {
        ms[r.cat] += t;
        cnt[r.cat] += r.launches;
      }
    }
    recs.clear();
    used = 0;
  }
  void reset() {
    for (int i = 0; i < LMGPU_KT_NUM; i++) ms[i] = work[i] = 0, cnt[i] = 0;
  }
};

const int kBinN[6] = {24, 48, 72, 96, 120, 139};  // 139^2 * 8 + staging = 162.5 KB <= 160 KiB of LDS per workgroup
const int kNumBins = 12;  // 0..5: LDS fronts by size; 6..11: the same sizes for GATHER leaves (only nf rows in LDS)
const int kLdsLimitN = 139;
const int kLdsFrontExtra = LDSF_EXTRA_BYTES;
const int NB = 64;    // potrf / trsm step
const int NBO = DENSE_NBO;  // outer panel: rows eliminated per trailing update of the HBM front
const int kSyrkLds = 2 * 2 * SYRK_KC * SYRK_LDW * 8;

}  // namespace

#include "front_launch.hpp"  // the front kernels' launchers and the dense-front executor (shared with isam2.hpp)

// In-process stand-in for the RCCL communicator: W handles of ONE process (one thread each) sum their buffers through a
// host rendezvous.  Same call sites and semantics as the ncclAllReduce path; exists so that the sharded LM loop can be
// exercised end to end on a single GPU (two RCCL ranks may not share a device).  Not a performance path.
struct lmgpu_local_group {
  int world = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  long generation = 0;
  std::vector<void*> ptr;
  std::vector<hipStream_t> stream;
  // rendezvous: returns once all ranks are in
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const long g = generation;
    if (++arrived == world) {
      arrived = 0;
      generation++;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return generation != g; });
    }
  }
};

__global__ void local_sum_kernel(double* __restrict__ dst, const double* __restrict__ src, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] += src[i];
}
__global__ void local_min_kernel(int* __restrict__ dst, const int* __restrict__ src) { *dst = min(*dst, *src); }

// damping weights of diagonal damping: w = sqrt(clamp(diag, min, max))^2 -- the square of what the reference's prior carries
// (value.cwiseMax(minDiagonal).cwiseMin(maxDiagonal).cwiseSqrt(), LevenbergMarquardtOptimizer.cpp:294-298; the prior squares it again)
__global__ void clamp_diag_kernel(int n, const double* __restrict__ diag, double* __restrict__ w, double lo, double hi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double s = sqrt(fmin(fmax(diag[i], lo), hi));
  w[i] = s * s;
}

struct NcgState;  // ncg.hpp
static void ncg_release(lmgpu_handle* h);
struct TriState;  // triangulation.hpp
static void tri_release(lmgpu_handle* h);
struct MargState;  // marginals.hpp: parameters, statistics and device buffers of the marginal path walks
static void marg_release(lmgpu_handle* h);
struct SmartState;  // smart.hpp: the smart projection factors of a handle (hidden points, cache, internal factor bucket)
static void smart_release(lmgpu_handle* h);
static int smart_prepare(lmgpu_handle* h);
static int smart_upload(lmgpu_handle* h);
static void smart_enqueue_triangulate(lmgpu_handle* h, int which);
static void smart_commit(lmgpu_handle* h);
static void smart_enqueue_const(lmgpu_handle* h);
static void smart_fix_lin0(lmgpu_handle* h);
static void smart_launch_factors(lmgpu_handle* h, const lmgpu::BucketDev& d, const lmgpu::ValuesDev& vals, bool jac);
static bool smart_refused(lmgpu_handle* h, const char* who);

struct lmgpu_handle {
  lmgpu_config cfg;
  DevSwitches sw;  // the development switches, as read by lmgpu_create
  int device = -1;
  std::string err;
  int failed_slot = -1;
  Plan plan;
  std::vector<Bucket> buckets;
  bool finalized = false, have_values = false, linearized = false, solved = false;
  std::string finalize_err;  // non-empty: lmgpu_finalize_structure failed with this error, and the handle refuses every call but lmgpu_destroy with it
  bool have_jacobians = false;  // the pool holds the [A b] of the last linearization (they outlive `linearized`: an accepted step moves the values, not the Jacobians)
  std::vector<int32_t> graph_index_sorted;  // parallel to plan.factors

  // ---- ownership (multi-GPU).  Everything is "active" and "counted" when world_size == 1.
  std::vector<int> front_owner;      // -1 = replicated on every rank
  std::vector<char> front_active;    // this rank assembles / factors / back-substitutes the front
  std::vector<int32_t> fac_local;    // plan.factors index -> local factor index (-1: not on this rank)
  int nfac = 0;                      // local factors
  int n_counted = 0;                 // local factors [0, n_counted) enter this rank's error sums (each factor counted on one rank)

  // ---- device state
  hipStream_t stream = nullptr;
  double *bs_inv = nullptr, *bs_x = nullptr;  // dataflow back-substitution scratch
  double* inv16 = nullptr;                     // 16 x (16x16) inverses of the current outer panel's diagonal tiles
  // per dense front on the per-front path: its launch schedule (dense_schedule.hpp) and, per DENSE_CHAIN record, the ticket order of
  // that launch as a range of d_chain_tasks.  Built by ensure_dense_schedules before a solve is queued; dense_mode = the communicator
  // they were built for (-1: not built)
  struct DensePlan { std::vector<DenseStep> steps; std::vector<int> task_begin, task_count; };
  std::vector<DensePlan> dense_plans;
  int2* d_chain_tasks = nullptr;
  int dense_mode = -1;
  double* d_lambda = nullptr;   // damping parameter of the solve being queued (device memory: see do_solve_enqueue)
  bool merge_backsub = false;   // LDS fronts of consecutive levels in one dataflow launch (deep trees; LMGPU_MERGE_BACKSUB=0/1)
  // the same on the way up: runs of consecutive levels without dense fronts in between whose LDS fronts go as ONE launch
  // (lds_front_merged_kernel); elim_seg_of[level] = index into elim_segs when the level starts a segment, -2 when it lies inside one
  struct ElimSeg {
    int lvl_lo, lvl_hi, nmax, jcap, threads;
  };
  std::vector<ElimSeg> elim_segs;
  std::vector<int> elim_seg_of;
  bool merge_elim = false;
  FillUpper* d_fill_upper = nullptr;  // the update matrices of the merged launches' fronts (fill_upper_kernel)
  int n_fill_upper = 0;
  bool fuse_levels = false;            // levels with LDS fronts and medium fronts: one launch for both (LMGPU_FUSE_LEVELS=0/1)
  LevelTask* d_level_tasks = nullptr;
  LevelSync* d_level_sync = nullptr;   // one record per medium front (all levels)
  int n_level_sync = 0;
  int32_t *d_bs_parent = nullptr, *d_bs_pos = nullptr;  // per front: parent front if it is an LDS front (else -1); position in d_lists (-1: HBM)
  char* d_leafpack = nullptr;                           // packed descriptors of the LDS fronts (kernels_front.hpp, LEAFPACK_*)
  unsigned int* d_bs_done = nullptr;                    // per front flag + one ticket counter per level
  bool use_graph = false;       // replay the solve's launch sequence as a hipGraph (deep trees; LMGPU_GRAPH=0/1 overrides)
  int eager_solves = 0;
  hipGraphExec_t solve_graph[2] = {nullptr, nullptr};  // [1]: with the extra gradient vector of the marginal solves
  int n_leaf_group_launches = 0;               // gather-leaf bin launches that take lds_front_group_kernel (lmgpu_leaf_group_launches)
  unsigned int* d_pflags = nullptr;            // hand-off flags of panel_dataflow_kernel, PDF_FLAG_WORDS per outer panel
  int pflags_panels = 0;
  unsigned int* bs_flags = nullptr;
  bool pflags_prefilled = false, bs_prefilled = false;  // their clears are entries of the elimination's fill table (ensure_fill_tables)
  double* pool = nullptr;
  size_t pool_doubles = 0;
  double* vals[2][kNumVarTypes] = {};
  double* saved[kNumVarTypes] = {};
  int cur = 0;
  int32_t* type_xoff[kNumVarTypes] = {};
  double *delta = nullptr, *dampw = nullptr, *hdiag = nullptr, *ebuf0 = nullptr, *ebuf1 = nullptr, *partial = nullptr, *dscal = nullptr,
         *ywork = nullptr;
  int* d_status = nullptr;
  double* h_scal = nullptr;  // pinned: [0]=err, [1]=lin0, [2]=lin1
  int* h_status = nullptr;   // pinned
  FacDesc* d_fd = nullptr;
  FrontDesc* d_fronts = nullptr;
  FrontFac* d_ffac = nullptr;
  ChildRef* d_childs = nullptr;
  int32_t *d_cmap = nullptr, *d_fxoff = nullptr, *d_sxoff = nullptr, *d_lists = nullptr;
  FrontTablesDev tabs;  // the same tables as the launchers take them (front_launch.hpp): filled by upload_launch_tables
  int32_t *d_hbm_small = nullptr, *d_f_ld = nullptr, *d_med_list = nullptr;
  MedFront* d_med_fronts = nullptr;     // packed records of the medium fronts, level by level (same order as d_med_list)
  BsdBlock* d_bsd_table = nullptr;      // 64-row blocks of the smaller HBM fronts, per level, each front from its last block to its first
  // runs of consecutive levels that hold nothing but such fronts: their blocks as ONE launch, levels top-down (merged back-substitution only)
  struct BsdRun {
    int lvl_hi, lvl_lo, begin, count;
  };
  std::vector<BsdRun> bsd_runs;
  std::vector<int> bsd_run_of;          // per level: index of the run that starts (top) here, -2 inside a run, -1 none
  BsdBlock* d_bsd_run_table = nullptr;
  // the clears and sentinel fills at the head of an elimination / a back-substitution, one launch each (fill_chunks_kernel)
  FillChunk* d_fill_elim = nullptr;
  FillChunk* d_fill_backsub = nullptr;
  int n_fill_elim = -1, n_fill_backsub = -1;  // (-1: not built yet, ensure_fill_tables)
  double* d_bsd_x = nullptr;            // their published x (64 per block), preset to the all-ones sentinel at the start of a back-substitution
  unsigned int* d_bsd_ticket = nullptr; // one ticket counter per level
  size_t bsd_x_count = 0;
  ZeroRange* d_zero_ranges = nullptr;   // the HBM fronts a solve clears first, when they are many and scattered (zero_ranges_kernel)
  int n_zero_ranges = 0;
  int num_cus = 0;                      // compute units of the device (a grid of at most this many small workgroups is resident at once)
  int chain_resident = 0;               // workgroups of chain_kernel the device holds at once: the grid of a chained launch (chain_grid)
  // deterministic assembly of HBM fronts (kernels_dense.hpp: hbm_assemble_rows_kernel): per front the start of its n + 1 row
  // pointers in d_rowptr (-1: none), the pointers (offsets into d_rowsrc) and the sources
  std::vector<int32_t> row_begin;
  int32_t *d_row_begin = nullptr, *d_rowptr = nullptr;
  RowSrc* d_rowsrc = nullptr;
  int n_lds_fronts = 0;                         // all levels' LDS-class fronts are contiguous in d_lists
  double *bt_ebuf = nullptr, *bt_vec = nullptr;  // Dogleg: per-clique / per-row squared residuals; gradient / zero vector
  int bt_ebuf_len = 0;
  // the gradient as a fixed-order sum: a slot per (clique, column) [per 64-row chunk for HBM fronts], gathered per scalar (built on first use)
  double* bt_part = nullptr;
  int64_t* d_bt_part_off = nullptr;  // per entry of d_lists (LDS-class fronts)
  std::vector<int64_t> bt_hbm_part_off;  // per front id (HBM fronts)
  int32_t *d_bt_ptr = nullptr, *d_bt_idx = nullptr;
  bool bt_gather_built = false;
  double* inv16_med = nullptr;
  std::vector<char> is_med;
  int64_t* d_f_off = nullptr;
  int32_t *d_scalar_var = nullptr, *d_scalar_col = nullptr, *d_vi_ptr = nullptr, *d_vi_fac = nullptr;
  int8_t* d_vi_pos = nullptr;
  // gather-mode (Schur form) assembly of HBM fronts from their leaf children
  struct GatherRange {
    int pblk_begin = 0, pblk_short = 0, pblk_long = 0, vblk_begin = 0, vblk_count = 0, leaf_begin = 0, leaf_count = 0;  // short blocks first
    int vblk_short = 0;  // variable blocks of at most SCHUR_VAR_SHORT leaf and factor entries (they come first; split-diagonal form: 0)
    // write mode: every contribution to the front's upper triangle before the gather comes from the gather itself (all children are
    // gather leaves), so the gather writes its blocks and only the blocks no list covers are cleared: [zero_begin, +zero_count)
    bool write_ok = false;
    int zero_begin = 0, zero_count = 0;
  };
  std::vector<GatherRange> gather;  // per front (only HBM fronts have non-empty ranges)
  GPairBlock* d_gpblk = nullptr;
  GZeroBlock* d_gzero = nullptr;
  int n_hbm_fronts = 0;          // number of HBM-class fronts on this rank (selects the clearing regime in do_eliminate)
  GPairEntry* d_gpent = nullptr;
  GVarBlock* d_gvblk = nullptr;
  GVarEntry* d_gvent = nullptr;
  double* d_gcorner = nullptr;
  std::vector<FrontDesc> h_fronts;
  std::vector<int64_t> f_off;  // HBM fronts: pool offset of the dense front (else -1)
  std::vector<int> f_ld;
  std::vector<int64_t> s_off;  // multi-rank, replicated HBM front: pool offset of this rank's PARTIAL assembly (else -1)
  hipStream_t comm_stream = nullptr;  // chunked all-reduce of the partial assembly, beside the factorisation
  hipEvent_t asm_ev = nullptr;
  std::vector<hipEvent_t> chunk_ev;
  std::vector<LevelWork> levels;
  int ntot = 0, nstore = 0;
  bool dampw_is_ones = false;
  int inv16_owner = -1;  // HBM front whose panels' 16x16 inverses inv16 currently holds
  double* gex = nullptr;         // ntot doubles: extra gradient vector for solves with a prescribed right-hand side (marginals)
  double* gex_active = nullptr;  // == gex while such a solve is being assembled, else nullptr

  // ---- marginal path walks (kernels_marginals.hpp, marginals.hpp).  The tables are built on every handle with fronts (launch_tables.hpp:
  //      build_marginal_tables); a structure-only handle answers lmgpu_marginals_path from them.
  std::vector<int32_t> marg_poff;   // per front: path offset (poff[root] = 0, poff[child] = poff[parent] + nf[parent])
  std::vector<int32_t> marg_depth;  // per front: cliques above it on its path
  std::vector<int32_t> marg_vcol;   // per slot: its first scalar inside the front it is frontal in
  std::vector<int32_t> marg_spos;   // parallel to sxoff: path position of each separator scalar
  int32_t *d_marg_parent = nullptr, *d_marg_poff = nullptr, *d_marg_spos = nullptr;
  bool marg_valid = false;          // the pool's [R S d] are the undamped factorization at the current values (lmgpu_marginals_factor)
  bool marg_factoring = false;      // lmgpu_marginals_factor is queueing its solve: always the direct solver
  MargState* marg = nullptr;

  // ---- LM
  lmgpu_lm_state lm{};
  lmgpu_timings tim{};
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  KTimer kt;

  ncclComm_t comm = nullptr;       // scalars / status / Hessian diagonal: issued on the compute stream only
  ncclComm_t comm_data = nullptr;  // the chunked all-reduce of a replicated front's partial assembly: issued on the communication stream only
                                   // (a communicator of its own, so that no communicator is ever driven from two streams at once)
  lmgpu_local_group* lgroup = nullptr;  // test-only in-process communicator (lmgpu_comm_init_local)

  // ---- PCG (kernels_pcg.hpp; lmgpu_set_linear_solver)
  int solver = LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY;
  lmgpu_pcg_params pcgp{LMGPU_PRECOND_BLOCK_JACOBI, 1, 500, 501, 1e-3, 1e-3};
  bool pcg_structure = false;   // finalized under PCG: no symbolic analysis, no fronts
  bool pcg_ready = false;       // the PCG buffers below exist
  bool pcg_gram_valid = false;  // pcg_H / pcg_rhs hold the blocks of the current linearization
  bool pcg_have_stats = false;
  int pcg_cap = 0;              // iterations pcg_gam / pcg_done can hold
  int32_t* pcg_xoff = nullptr;
  int64_t *pcg_loff = nullptr, *pcg_yoff = nullptr;
  double *pcg_H = nullptr, *pcg_L = nullptr, *pcg_rhs = nullptr, *pcg_r = nullptr, *pcg_p = nullptr, *pcg_q = nullptr, *pcg_y = nullptr,
         *pcg_part = nullptr, *pcg_gam = nullptr;
  int32_t* pcg_done = nullptr;
  PcgCtl* pcg_ctl = nullptr;
  PcgCtl* h_pcg_ctl = nullptr;   // pinned
  int32_t* h_pcg_done = nullptr; // pinned
  hipEvent_t pcg_ev[3] = {nullptr, nullptr, nullptr};
  lmgpu_pcg_stats pcg_stats{};

  // ---- GNC (kernels_gnc.hpp; lmgpu_gnc_*).  Device vectors in local factor order (= the error buffer's), nfac entries each.
  bool gnc_on = false;
  bool gnc_raw = false;          // the next error launches evaluate the UNWEIGHTED graph (r_k for the weight update)
  int gnc_n = 0;                 // nfg_.size(): length of every vector that crosses the boundary
  int gnc_n_in = 0, gnc_n_out = 0;
  double *gnc_w = nullptr, *gnc_b = nullptr, *gnc_part = nullptr, *gnc_scal = nullptr;
  unsigned char* gnc_fixed = nullptr;
  double* h_gnc_scal = nullptr;  // pinned: [0] max |w - round(w)|, [1] mu
  std::vector<int32_t> gnc_pos;  // graph index -> local factor (-1: the slot holds no factor)
  std::vector<unsigned char> gnc_fixed_h;
  std::vector<double> gnc_trace; // per outer iteration: mu, cost, max |w - round(w)|, weight-update ms, base optimizer ms, base iterations
  hipEvent_t gnc_ev[2] = {nullptr, nullptr};

  // ---- nonlinear conjugate gradient (kernels_ncg.hpp, ncg.hpp; lmgpu_ncg_*): allocated at first use
  NcgState* ncg = nullptr;
  TriState* tri = nullptr;  // the cached point -> factor index and result buffers of lmgpu_triangulate_landmarks
  SmartState* smart = nullptr;  // smart projection factors (smart.hpp); null on a handle that has none
  int n_hidden = 0;             // hidden POINT3 variables in front of the caller's slots (one per smart factor with m >= 2); 0 without smart factors
  bool smart_speculative = false;  // the next error launch is tryLambda's speculative one: its cache update waits for smart_commit
  const int32_t* err_skip = nullptr;  // set around the trial launches of a line search: BucketDev::skip of the error launches
#ifdef LMGPU_TEST_HOOKS
  struct DigestRec {  // lmgpu_debug_table_digest (launch_tables.hpp): name, entries and FNV-1a of one launch table, taken by finalize
    char name[32];
    uint64_t count, fnv1a;
  };
  std::vector<DigestRec> table_digest;
#endif
};

namespace {

template <typename T>
int upload(lmgpu_handle* h, T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  if (src.empty()) {
    HIPCHECK(hipMalloc((void**)dst, sizeof(T)));
    return LMGPU_OK;
  }
  HIPCHECK(hipMalloc((void**)dst, src.size() * sizeof(T)));
  HIPCHECK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return LMGPU_OK;
}

int need_device(lmgpu_handle* h) {
  if (h->device < 0) {
    h->err = "no HIP device bound to this handle (structure-only handle); the hot path has no CPU fallback";
    return LMGPU_HIP_ERROR;
  }
  return LMGPU_OK;
}

int need_comm(lmgpu_handle* h) {
  if ((h->cfg.world_size > 1 || (h->cfg.flags & LMGPU_FLAG_SPLIT_ROOT)) && !h->comm && !h->lgroup) {
    h->err = "world_size > 1 but lmgpu_comm_init has not been called";
    return LMGPU_INVALID;
  }
  return LMGPU_OK;
}

ValuesDev values_dev(lmgpu_handle* h, int which) {
  ValuesDev v;
  for (int t = 0; t < kNumVarTypes; t++) v.v[t] = h->vals[which][t];
  return v;
}

BucketDev bucket_dev(lmgpu_handle* h, const Bucket& b) {
  BucketDev d;
  d.type = b.type;
  d.n = b.n_loc;
  d.noise_kind = b.noise_kind;
  d.robust = h->gnc_on ? 0 : b.robust;  // GncOptimizer's constructor strips noiseModel::Robust (GncOptimizer.h:63-73)
  d.rk = b.robust_k;
  d.gw = (h->gnc_on && !h->gnc_raw) ? h->gnc_w : nullptr;
  d.vidx = b.d_vidx;
  d.meas = b.d_meas;
  d.noise = b.d_noise;
  d.J = h->pool + b.joff;
  d.epos = b.d_epos;
  d.sel = nullptr;
  d.skip = h->err_skip;
  return d;
}

// launch the factor kernels of every bucket: JAC -> Jacobians, else per-factor errors into ebuf0
template <bool JAC>
int launch_factors(lmgpu_handle* h, int which) {
  const ValuesDev vals = values_dev(h, which);
  if (h->smart) smart_enqueue_triangulate(h, which);  // SmartProjectionFactor::triangulateSafe at the head of every linearize / error
  for (const Bucket& b : h->buckets) {
    if (b.n_loc == 0) continue;
    const BucketDev d = bucket_dev(h, b);
    hipStream_t s = h->stream;
    if (b.type == LMGPU_F_SFM) {
      const int g256 = (b.n_loc + 255) / 256;
      if (JAC) {
        // algorithmic bytes: 232 B per factor + each variable once (120 B camera, 24 B point)
        const int kt = h->kt.begin(LMGPU_KT_LINEARIZE, s);
        hipLaunchKernelGGL(sfm_linearize_kernel, dim3(g256), dim3(256), 0, s, d, vals);
        h->kt.end(kt, s, 232.0 * b.n_loc + 120.0 * h->plan.type_count[3] + 24.0 * h->plan.type_count[2]);
      } else {
        hipLaunchKernelGGL(sfm_error_kernel, dim3(g256), dim3(256), 0, s, d, vals, h->ebuf0);
      }
    } else if (b.type == kSmartObsType) {
      smart_launch_factors(h, d, vals, JAC);
    } else if (!launch_generic_bucket<JAC>(d, vals, h->ebuf0, s)) {
      h->err = "no factor kernel for factor type " + std::to_string(b.type);
      return LMGPU_INVALID;
    }
  }
  if (JAC && h->smart) smart_enqueue_const(h);
  return LMGPU_OK;
}

void reduce_to(lmgpu_handle* h, const double* buf, int n, double* dst, hipStream_t st = nullptr, double* scratch = nullptr) {
  const int g = std::min(256, std::max(1, (n + 255) / 256));
  if (!st) st = h->stream;
  if (!scratch) scratch = h->partial;
  hipLaunchKernelGGL(reduce_stage1, dim3(g), dim3(256), 0, st, buf, n, scratch);
  hipLaunchKernelGGL(reduce_stage2, dim3(1), dim3(256), 0, st, (const double*)scratch, g, dst);
}

// all-reduce over the ranks: RCCL, or the in-process local group
int allreduce_sum(lmgpu_handle* h, double* buf, size_t count, hipStream_t s) {
  if (h->comm) {
    NCCLCHECK(ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, h->comm, s));
  } else if (h->lgroup) {
    lmgpu_local_group* g = h->lgroup;
    HIPCHECK(hipStreamSynchronize(s));
    g->ptr[h->cfg.rank] = buf;
    g->barrier();
    if (h->cfg.rank == 0) {
      for (int r = 1; r < g->world; r++)
        hipLaunchKernelGGL(local_sum_kernel, dim3(1024), dim3(256), 0, s, buf, (const double*)g->ptr[r], count);
      HIPCHECK(hipStreamSynchronize(s));
      for (int r = 1; r < g->world; r++) HIPCHECK(hipMemcpy(g->ptr[r], buf, count * sizeof(double), hipMemcpyDeviceToDevice));
    }
    g->barrier();
  }
  return LMGPU_OK;
}
int allreduce_min_int(lmgpu_handle* h, int* buf, hipStream_t s) {
  if (h->comm) {
    NCCLCHECK(ncclAllReduce(buf, buf, 1, ncclInt, ncclMin, h->comm, s));
  } else if (h->lgroup) {
    lmgpu_local_group* g = h->lgroup;
    HIPCHECK(hipStreamSynchronize(s));
    g->ptr[h->cfg.rank] = buf;
    g->barrier();
    if (h->cfg.rank == 0) {
      for (int r = 1; r < g->world; r++) hipLaunchKernelGGL(local_min_kernel, dim3(1), dim3(1), 0, s, buf, (const int*)g->ptr[r]);
      HIPCHECK(hipStreamSynchronize(s));
      for (int r = 1; r < g->world; r++) HIPCHECK(hipMemcpy(g->ptr[r], buf, sizeof(int), hipMemcpyDeviceToDevice));
    }
    g->barrier();
  }
  return LMGPU_OK;
}

// sum `count` doubles at dscal+first over the ranks (each factor is counted on exactly one rank)
int allreduce_scalars(lmgpu_handle* h, int first, int count) {
  return allreduce_sum(h, h->dscal + first, count, h->stream);
}

int compute_error(lmgpu_handle* h, int which, double* out) {
  int rc = launch_factors<false>(h, which);
  if (rc) return rc;
  reduce_to(h, h->ebuf0, h->n_counted, h->dscal);
  if ((rc = allreduce_scalars(h, 0, 1))) return rc;
  HIPCHECK(hipMemcpyAsync(h->h_scal, h->dscal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  *out = h->h_scal[0];
  return LMGPU_OK;
}

int do_linearize(lmgpu_handle* h) {
  h->marg_valid = false;
  const int rc = launch_factors<true>(h, h->cur);
  if (rc) return rc;
  HIPCHECK(hipGetLastError());
  h->linearized = true;
  h->have_jacobians = true;
  h->pcg_gram_valid = false;
  return LMGPU_OK;
}

int launch_hessian_diag(lmgpu_handle* h) {
  hipLaunchKernelGGL(hessian_diag_kernel, dim3((h->ntot + 255) / 256), dim3(256), 0, h->stream, h->ntot, h->d_scalar_var, h->d_scalar_col,
                     h->d_vi_ptr, h->d_vi_fac, h->d_vi_pos, h->d_fd, (const double*)h->pool, h->hdiag);
  return allreduce_sum(h, h->hdiag, h->ntot, h->stream);
}

int fill_dampw(lmgpu_handle* h, int diagonal, double min_diag, double max_diag) {
  if (!diagonal) {
    if (!h->dampw_is_ones) {
      std::vector<double> ones(h->ntot, 1.0);
      std::fill(ones.begin(), ones.begin() + 3 * h->n_hidden, 0.0);  // LM never damps the point a smart factor eliminates
      HIPCHECK(hipMemcpyAsync(h->dampw, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPCHECK(hipStreamSynchronize(h->stream));
      h->dampw_is_ones = true;
    }
    return LMGPU_OK;
  }
  // hessianDiagonal, clamped (LevenbergMarquardtOptimizer.cpp:291-298: sqrt then squared by the prior = clamp(diag)); an
  // element-wise kernel on the stream, nothing crosses PCIe
  int rc = launch_hessian_diag(h);
  if (rc) return rc;
  hipLaunchKernelGGL(clamp_diag_kernel, dim3((h->ntot + 255) / 256), dim3(256), 0, h->stream, h->ntot, (const double*)h->hdiag, h->dampw, min_diag, max_diag);
  h->dampw_is_ones = false;
  return LMGPU_OK;
}

// ---- numeric elimination of all (active) fronts, level by level (a10-a13)
// The front's first contribution is its own Schur gather (all children are gather leaves, single rank): no clear, the gather writes.
// Only in the per-front clearing regime (few large HBM fronts); the span memset of general sparse graphs covers everything anyway.
// With several ranks the same holds for the rank's partial-assembly buffer (the working matrix still starts from zero): after the
// all-reduce it holds the sums of the previous solve, which this rank's gather overwrites where it has entries and the list of
// blocks it does not cover clears.
static bool gather_writes(const lmgpu_handle* h, int fi) {
  const lmgpu_handle::GatherRange& G = h->gather[fi];
  if (!(G.write_ok && G.leaf_count > 0 && !h->sw.no_gather_write && h->n_hbm_fronts <= 4)) return false;
  if (h->s_off[fi] < 0) return true;
  return (h->h_fronts[fi].pad & 1) != 0 && (h->comm || h->lgroup);  // the partial-assembly buffer is in use (`split` below)
}

static void add_fill(std::vector<FillChunk>& t, const void* p, size_t bytes, uint32_t value) {
  for (size_t o = 0; o < bytes; o += FILL_CHUNK_BYTES)
    t.push_back(FillChunk{(unsigned long long)(uintptr_t)p + o, (uint32_t)std::min<size_t>(FILL_CHUNK_BYTES, bytes - o), value});
}

// how the assembled rows of HBM front fi reach its working matrix (dense_schedule.hpp): in place, or -- a replicated front with a
// partial-assembly buffer, once a communicator is attached -- in row chunks summed over the ranks
static int dense_mode_of(const lmgpu_handle* h, int fi) {
  const bool replicated = (h->h_fronts[fi].pad & 1) != 0;
  if (h->s_off[fi] < 0 || !replicated || !(h->comm || h->lgroup)) return DENSE_SINGLE;
  return h->comm ? DENSE_SPLIT_EVENTS : DENSE_SPLIT_HOST;
}

// chunk c of a split front = rows [256 c, 256 (c+1)) from the first column of its diagonal block to the end of its last row
static void chunk_range(int n, int ld, int c, size_t& begin, size_t& count) {
  const int r0c = c * NBO, rows = std::min(n, r0c + NBO) - r0c;
  begin = (size_t)r0c * ld + r0c;  // r0c is a multiple of 256: 16-aligned
  count = (size_t)rows * ld - r0c;
}

// chunk c of the partial assembly Asm is complete (summed over the ranks) for everything queued on the main stream after this call
static int wait_chunk(lmgpu_handle* h, double* Asm, int n, int ld, int c) {
  if (h->comm) {
    HIPCHECK(hipStreamWaitEvent(h->stream, h->chunk_ev[c], 0));
    return LMGPU_OK;
  }
  size_t cb, cn;  // in-process group: synchronous
  chunk_range(n, ld, c, cb, cn);
  return allreduce_sum(h, Asm + cb, cn, h->stream);
}

// fold chunk c into the working matrix A (which already carries the trailing updates of earlier panels)
static int add_chunk(lmgpu_handle* h, double* A, double* Asm, int n, int ld, int c) {
  hipStream_t s = h->stream;
  const int ktc = h->kt.begin(LMGPU_KT_ALLREDUCE, s);
  const int rcw = wait_chunk(h, Asm, n, ld, c);
  if (rcw) return rcw;
  size_t cb, cn;
  chunk_range(n, ld, c, cb, cn);
  hipLaunchKernelGGL(local_sum_kernel, dim3(std::min<size_t>(2048, (cn + 255) / 256)), dim3(256), 0, s, A + cb, (const double*)(Asm + cb), cn);
  h->kt.end(ktc, s, (double)cn * 8.0);
  return LMGPU_OK;
}

// Everything the dense fronts of the per-front path need before a solve is queued or captured: their launch schedules, the ticket
// orders of their chained launches (chain_schedule) in device memory, and the chunk events of the split fronts.  Built at the first
// solve, and again when a communicator has been attached since (the split fronts' schedules depend on it).
static int ensure_dense_schedules(lmgpu_handle* h) {
  const int mode = h->comm ? DENSE_SPLIT_EVENTS : h->lgroup ? DENSE_SPLIT_HOST : DENSE_SINGLE;
  if (h->dense_mode == mode) return LMGPU_OK;
  const unsigned forms = (h->sw.two_launch_panel ? DENSE_FORM_TWO_LAUNCH : 0u) | (h->sw.no_fuse ? DENSE_FORM_NO_FUSE : 0u) |
                         (h->sw.no_chain ? DENSE_FORM_NO_CHAIN : 0u) | (h->sw.no_tail ? DENSE_FORM_NO_TAIL : 0u);
  std::vector<int2> tasks;
  h->dense_plans.assign(h->h_fronts.size(), lmgpu_handle::DensePlan());
  for (const LevelWork& L : h->levels)
    for (int fi : L.hbm) {
      if (h->is_med[fi]) continue;
      const FrontDesc& F = h->h_fronts[fi];
      if ((F.nf + NBO - 1) / NBO + 1 > h->pflags_panels) {
        h->err = "panel flag buffer too small";
        return LMGPU_INVALID;
      }
      lmgpu_handle::DensePlan& P = h->dense_plans[fi];
      P.steps = dense_front_schedule(F.n, F.nf, dense_mode_of(h, fi), forms);
      P.task_begin.assign(P.steps.size(), 0);
      P.task_count.assign(P.steps.size(), 0);
      for (size_t r = 0; r < P.steps.size(); r++) {
        if (P.steps[r].kind != DENSE_CHAIN) continue;
        const std::vector<int2> t = chain_schedule(F.n, F.nf, P.steps[r].i, P.steps[r].nsteps, h->sw.chain_far_pct, h->sw.chain_merge, h->sw.chain_split_pct);
        P.task_begin[r] = (int)tasks.size();
        P.task_count[r] = (int)t.size();
        tasks.insert(tasks.end(), t.begin(), t.end());
      }
      if (dense_mode_of(h, fi) != DENSE_SINGLE)
        while ((int)h->chunk_ev.size() < 2 * ((F.n + NBO - 1) / NBO)) {
          hipEvent_t e;
          HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
          h->chunk_ev.push_back(e);
        }
    }
  if (h->d_chain_tasks) HIPCHECK(hipFree(h->d_chain_tasks));
  const int rcu = upload(h, &h->d_chain_tasks, tasks);
  if (rcu) return rcu;
  h->dense_mode = mode;
  return LMGPU_OK;
}

// How an elimination clears the HBM fronts, which their children add to before their own level runs.  EACH: a memset per front (few large
// fronts; a front whose gather writes first is left out).  SPAN: many mid-size fronts (general sparse graphs), one fill over their span
// [lo, hi) of the pool; what lies between them ([R S d] / update storage of LDS fronts, laid out in the same post-order) is rewritten by
// the elimination before it is read.  RANGES: many fronts scattered through the pool, one launch over the list of their ranges.
enum { HBM_CLEAR_EACH, HBM_CLEAR_SPAN, HBM_CLEAR_RANGES };
static int hbm_clear_regime(const lmgpu_handle* h, int64_t* lo_out, int64_t* hi_out) {
  int n_hbm = 0;
  int64_t lo = INT64_MAX, hi = 0, sum = 0;
  for (const LevelWork& L : h->levels)
    for (int fi : L.hbm) {
      const int64_t cnt = (int64_t)h->h_fronts[fi].n * h->f_ld[fi] * (h->s_off[fi] >= 0 ? 2 : 1);
      n_hbm++;
      sum += cnt;
      lo = std::min(lo, h->f_off[fi]);
      hi = std::max(hi, h->f_off[fi] + cnt);
    }
  *lo_out = lo;
  *hi_out = hi;
  return n_hbm <= 4 ? HBM_CLEAR_EACH : (hi - lo <= 2 * sum ? HBM_CLEAR_SPAN : HBM_CLEAR_RANGES);
}

// deep trees: the LDS fronts of consecutive levels without HBM fronts in between are back-substituted as ONE dataflow launch
static bool backsub_merged(const lmgpu_handle* h) {
  return h->merge_backsub && h->cfg.world_size == 1 && !(h->cfg.flags & LMGPU_FLAG_SPLIT_ROOT);
}

// The clears and sentinel fills at the head of an elimination and of a back-substitution (one fill_chunks_kernel launch each) and the
// ranges of HBM_CLEAR_RANGES, in device memory.  They hold device addresses, so they are built at the first solve and not by finalize:
// before anything is queued or captured, like the dense schedules above.
static int ensure_fill_tables(lmgpu_handle* h) {
  int64_t lo, hi;
  const int regime = hbm_clear_regime(h, &lo, &hi);
  if (h->n_fill_elim < 0) {
    std::vector<FillChunk> fills;
    add_fill(fills, h->d_status, sizeof(int), 0x7f7f7f7fu);
    add_fill(fills, h->d_status + 1, sizeof(int), 0u);  // [1]: a dataflow hand-off timed out (1 + front id)
    if (h->merge_elim || h->fuse_levels)  // one ticket counter per level (shared with the back-substitution, which clears them again)
      add_fill(fills, h->d_bs_done, (size_t)(h->h_fronts.size() + h->levels.size() + 1) * sizeof(unsigned int), 0u);
    if (h->fuse_levels) add_fill(fills, h->d_level_sync, (size_t)h->n_level_sync * sizeof(LevelSync), 0u);
    if (regime == HBM_CLEAR_SPAN) add_fill(fills, h->pool + lo, (size_t)(hi - lo) * sizeof(double), 0u);
    // The hand-off flags of the per-front dense path (d_pflags) and the flags and sentinels of the dataflow back-substitution of a
    // front of more than BSS_MAX_NF rows (bs_flags, bs_x) are touched by that front's own launches only.  When ONE front of a solve
    // uses them (a root behind point leaves), their clears ride in this launch instead of a memset command each in front of the
    // front; with several such fronts every front clears the buffers in front of its own launches, as before.  do_eliminate and
    // do_backsub only ever run as the pair of solve_sequence (eager or replayed, gex or not), so the head of the elimination is in
    // front of every use.
    int n_plan = 0, n_wide = 0, plan_fi = -1, wide_fi = -1;
    for (const LevelWork& L : h->levels)
      for (int fi : L.hbm) {
        if (!h->is_med[fi]) n_plan++, plan_fi = fi;
        if (h->h_fronts[fi].nf > BSS_MAX_NF) n_wide++, wide_fi = fi;
      }
    h->pflags_prefilled = n_plan == 1;
    h->bs_prefilled = n_wide == 1;
    if (h->pflags_prefilled)
      add_fill(fills, h->d_pflags, (size_t)((h->h_fronts[plan_fi].nf + NBO - 1) / NBO + 1) * PDF_FLAG_WORDS * sizeof(unsigned int), 0u);
    if (h->bs_prefilled) {  // (sized for the 64-row and the 128-row form alike: the flags of the former, the whole blocks of the latter)
      const int nf = h->h_fronts[wide_fi].nf;
      add_fill(fills, h->bs_flags, (size_t)((nf + NB - 1) / NB + 1) * sizeof(unsigned int), 0u);
      add_fill(fills, h->bs_x, (size_t)((nf + BSW_NB - 1) / BSW_NB) * BSW_NB * sizeof(double), 0xffffffffu);  // "not published yet"
    }
    h->n_fill_elim = (int)fills.size();
    const int rcu = upload(h, &h->d_fill_elim, fills);
    if (rcu) return rcu;
  }
  if (regime == HBM_CLEAR_RANGES && !h->d_zero_ranges) {  // (f_ld and the pool offsets are multiples of 16)
    std::vector<ZeroRange> zr;
    for (const LevelWork& L : h->levels)
      for (int fi : L.hbm) {
        const bool gw = gather_writes(h, fi);
        const int64_t cnt = (int64_t)h->h_fronts[fi].n * h->f_ld[fi];
        if (!gw || h->s_off[fi] >= 0) zr.push_back(ZeroRange{h->f_off[fi], cnt});
        if (!gw && h->s_off[fi] >= 0) zr.push_back(ZeroRange{h->s_off[fi], cnt});
      }
    h->n_zero_ranges = (int)zr.size();
    const int rcu = upload(h, &h->d_zero_ranges, zr);
    if (rcu) return rcu;
  }
  if (h->n_fill_backsub < 0) {
    std::vector<FillChunk> fills;
    if (backsub_merged(h)) {
      add_fill(fills, h->d_bs_done, (size_t)(h->h_fronts.size() + h->levels.size() + 1) * sizeof(unsigned int), 0u);  // (the ticket counters)
      add_fill(fills, h->delta, h->ntot * sizeof(double), 0xffffffffu);  // "not published yet": merged launches hand x over through delta itself
    }
    if (h->bsd_x_count > 0) {
      add_fill(fills, h->d_bsd_x, h->bsd_x_count * sizeof(double), 0xffffffffu);  // "not published yet"
      add_fill(fills, h->d_bsd_ticket, h->levels.size() * sizeof(unsigned int), 0u);
    }
    h->n_fill_backsub = (int)fills.size();
    if (!fills.empty()) {
      const int rcu = upload(h, &h->d_fill_backsub, fills);
      if (rcu) return rcu;
    }
  }
  return LMGPU_OK;
}

// the clears: the HBM fronts (hbm_clear_regime), the status words and the counters of the merged and fused launches
static int eliminate_clears(lmgpu_handle* h) {
  hipStream_t s = h->stream;
  const int kt0 = h->kt.begin(LMGPU_KT_HBM_ASSEMBLE, s);
  int64_t lo, hi;
  const int regime = hbm_clear_regime(h, &lo, &hi);
  if (regime == HBM_CLEAR_RANGES && h->n_zero_ranges > 0)
    hipLaunchKernelGGL(zero_ranges_kernel, dim3(16, h->n_zero_ranges), dim3(256), 0, s, (const ZeroRange*)h->d_zero_ranges, h->pool);
  if (regime == HBM_CLEAR_EACH)
    for (const LevelWork& L : h->levels)
      for (int fi : L.hbm) {
        // gather_writes: the upper triangle of the buffer the front is assembled into is written by the gather and a list of
        // uncovered blocks -- the front itself on one rank, the partial-assembly buffer with several
        const bool gw = gather_writes(h, fi);
        const size_t bytes = (size_t)h->h_fronts[fi].n * h->f_ld[fi] * sizeof(double);
        if (!gw || h->s_off[fi] >= 0) HIPCHECK(hipMemsetAsync(h->pool + h->f_off[fi], 0, bytes, s));
        if (!gw && h->s_off[fi] >= 0) HIPCHECK(hipMemsetAsync(h->pool + h->s_off[fi], 0, bytes, s));
      }
  hipLaunchKernelGGL(fill_chunks_kernel, dim3(h->n_fill_elim), dim3(256), 0, s, (const FillChunk*)h->d_fill_elim);
  h->kt.end(kt0, s);
  return LMGPU_OK;
}

// the LDS fronts of level L, one launch per size bin
static void eliminate_level_bins(lmgpu_handle* h, const LevelWork& L, const Damping& dmp) {
  hipStream_t s = h->stream;
  for (int b = 0; b < kNumBins; b++) {
    const int cnt = L.bin_begin[b + 1] - L.bin_begin[b];
    if (cnt == 0) continue;
    const int nmax = kBinN[b % 6], jcap = L.bin_jcap[b];
    const char* pack = h->d_leafpack && L.pack_stride[b] ? h->d_leafpack + L.pack_off[b] : nullptr;
    const int kt = h->kt.begin(LMGPU_KT_LDS_FRONT, s);
    if (L.bin_group[b]) {  // every leaf of the bin qualifies (leaf_group_form): four leaves per wave, one lane per factor
      launch_leaf_groups(s, h->pool, h->d_status, dmp, L.bin_group[b], h->d_leafpack + L.pack_off[b], L.pack_stride[b], cnt, jcap, L.bin_group_out[b],
                         L.bin_group_maxfac[b], h->sw.leaf_group_threads, h->d_gcorner);
    } else {
      // (the thread rules of ISAM2's launches differ: is_launch_lds_level, isam2.hpp)
      // gather leaves keep only nf rows: one wave per front (barriers become free, ~2.5x more fronts resident per CU)
      const int threads = (b >= 6 || b % 6 == 0) ? 64 : (b % 6 == 1 ? 128 : 256);
      // a handful of wide fronts (the upper levels of a general sparse tree, where a launch lasts as long as its slowest front and the
      // device is idle): sixteen waves per front -- the rank-4 trailing updates, the extend-add and the emission all scale with them
      const bool wide16 = b >= 3 && b < 6 && cnt <= h->sw.wide16_max && !h->sw.no_wide16;
      launch_lds_fronts(s, h->tabs, h->pool, h->d_status, dmp, wide16 ? LDS_FRONT_WIDE16 : (b < 6 ? LDS_FRONT_PLAIN : LDS_FRONT_GATHER_LEAF),
                        L.list_begin + L.bin_begin[b], cnt, threads, nmax, L.bin_srows[b], jcap, h->d_gcorner, pack, L.pack_stride[b]);
    }
    h->kt.end(kt, s);
  }
}

// The assembly of HBM front fi into the n x ld block at pool offset aoff: the blocks no gather list covers, its children's update
// matrices and own factors by row, its leaf children in Schur form, then -- behind a gather that wrote -- the own factors and the damping.
static void assemble_hbm_front(lmgpu_handle* h, int fi, int64_t aoff, const Damping& dmp) {
  hipStream_t s = h->stream;
  const FrontDesc& F = h->h_fronts[fi];
  const int ld = h->f_ld[fi];
  const bool own_terms = (F.pad & 2) == 0;
  const lmgpu_handle::GatherRange& G = h->gather[fi];
  const bool gwrite = gather_writes(h, fi);
  // the row assembly, when the front has sources for it: whether the launch was made
  auto assemble_rows = [&](bool with_factors, bool damp) {
    if (!(h->row_begin[fi] >= 0 && (F.child_count > 0 || (with_factors && F.fac_count > 0)))) return false;
    launch_assemble_rows(s, h->tabs, h->pool, F, aoff, ld, h->row_begin[fi], with_factors, damp ? &dmp : nullptr);
    return true;
  };
  if (gwrite && G.zero_count > 0)
    hipLaunchKernelGGL(zero_blocks_kernel, dim3(G.zero_count), dim3(128), 0, s, (const GZeroBlock*)(h->d_gzero + G.zero_begin), h->pool, aoff, ld);
  // (the damping rides in the row assembly where there is one; a front without sources here keeps hbm_damp_kernel)
  const bool damp_here = !gwrite && own_terms;
  if (!assemble_rows(own_terms && !gwrite, damp_here) && damp_here) launch_hbm_damp(s, h->tabs, h->pool, F, aoff, ld, dmp);
  // leaf children in Schur form: deterministic gather instead of atomics
  const int schur_masked = h->sw.schur_unmasked ? 0 : 2;  // (operand loads that only the lanes holding an element take part in)
  // (LMGPU_SCHUR_UNMASKED reaches schur_pairs_kernel and the split form's schur_factor_kernel; schur_var_kernel has the masked loads only)
  if (G.pblk_short > 0)
    hipLaunchKernelGGL((schur_pairs_kernel<1>), dim3((G.pblk_short + 7) & ~7), dim3(64), 0, s, (const GPairBlock*)(h->d_gpblk + G.pblk_begin),
                       (const GPairEntry*)h->d_gpent, h->pool, aoff, ld, G.pblk_short, (gwrite ? 1 : 0) | schur_masked);
  if (G.pblk_long > 0)
    hipLaunchKernelGGL((schur_pairs_kernel<4>), dim3((G.pblk_long + 7) & ~7), dim3(256), 0, s,
                       (const GPairBlock*)(h->d_gpblk + G.pblk_begin + G.pblk_short), (const GPairEntry*)h->d_gpent, h->pool, aoff, ld,
                       G.pblk_long, (gwrite ? 1 : 0) | schur_masked);
#ifdef LMGPU_TEST_HOOKS
  if (h->sw.schur_split_diag) {
    if (G.vblk_count > 0)
      hipLaunchKernelGGL(schur_factor_kernel, dim3(G.vblk_count), dim3(64 * SCHUR_FW), 0, s, (const GVarBlock*)(h->d_gvblk + G.vblk_begin),
                         (const GVarEntry*)h->d_gvent, h->pool, aoff, ld, F.n, schur_masked);
    if (G.leaf_count > 0) {  // the (rhs, rhs) corner
      double* scal = h->dscal + 4;
      reduce_to(h, h->d_gcorner + G.leaf_begin, G.leaf_count, scal, s, nullptr);
      hipLaunchKernelGGL(add_scalar_kernel, dim3(1), dim3(1), 0, s, h->pool + aoff + (size_t)(F.n - 1) * ld + F.n - 1, (const double*)scal);
    }
  } else
#endif
  {
    // one workgroup per separator variable writes (adds) its (v, v) and (v, rhs); the last launch carries one more workgroup,
    // which sums the leaves' (rhs, rhs) scalars into the corner
    const int vlong = G.vblk_count - G.vblk_short;
    const int corner_short = (G.leaf_count > 0 && vlong == 0) ? 1 : 0, corner_long = (G.leaf_count > 0 && vlong > 0) ? 1 : 0;
    if (G.vblk_short + corner_short > 0)
      hipLaunchKernelGGL((schur_var_kernel<1>), dim3(G.vblk_short + corner_short), dim3(64), 0, s, (const GVarBlock*)(h->d_gvblk + G.vblk_begin),
                         (const GVarEntry*)h->d_gvent, h->pool, aoff, ld, F.n, G.vblk_short, gwrite ? 1 : 0,
                         (const double*)(h->d_gcorner + G.leaf_begin), G.leaf_count);
    if (vlong + corner_long > 0)
      hipLaunchKernelGGL((schur_var_kernel<SCHUR_VAR_WAVES>), dim3(vlong + corner_long), dim3(64 * SCHUR_VAR_WAVES), 0, s,
                         (const GVarBlock*)(h->d_gvblk + G.vblk_begin + G.vblk_short), (const GVarEntry*)h->d_gvent, h->pool, aoff, ld, F.n, vlong,
                         gwrite ? 1 : 0, (const double*)(h->d_gcorner + G.leaf_begin), G.leaf_count);
  }
  if (gwrite && own_terms) {  // the front's own factors and the damping are added: after the gather has initialised the entries
    // (a gather-write front has no update-matrix children: only its factors are added here, the damping behind them in the same launch)
    if (!(F.fac_count > 0 && assemble_rows(true, true))) launch_hbm_damp(s, h->tabs, h->pool, F, aoff, ld, dmp);
  }
}

// HBM front fi on the per-front path: assembly, the all-reduces of a split front's row chunks, then the front's schedule
// (dense_schedule.hpp, built by ensure_dense_schedules) record by record
static int eliminate_hbm_front(lmgpu_handle* h, int fi, const Damping& dmp) {
  hipStream_t s = h->stream;
  const FrontDesc& F = h->h_fronts[fi];
  const int ld = h->f_ld[fi];
  double* A = h->pool + h->f_off[fi];
  // `split`: the assembled contributions go to a buffer of their own (aoff) and reach the working matrix A (which starts
  // from zero and collects the trailing updates) in 256-row chunks, each just before its panel is factored.
  //   multi-rank   : the chunks are summed over the ranks (RCCL on the communication stream / the in-process group)
  // (gathering the chunks on a second stream beside the factorisation was measured in round 1 -- 13.5 vs 10.4 ms per step: two
  //  resident workgroups of the update kernel hold every VGPR of a SIMD, the gather waves only get in between -- and removed)
  const int mode = dense_mode_of(h, fi);
  const bool split = mode != DENSE_SINGLE;
  const int64_t aoff = split ? h->s_off[fi] : h->f_off[fi];
  double* Asm = h->pool + aoff;

  const int kt = h->kt.begin(LMGPU_KT_HBM_ASSEMBLE, s);
  assemble_hbm_front(h, fi, aoff, dmp);
  h->kt.end(kt, s);
  if (mode == DENSE_SPLIT_EVENTS) {  // RCCL: all chunks queued on the communication stream, one event each
    HIPCHECK(hipEventRecord(h->asm_ev, s));
    HIPCHECK(hipStreamWaitEvent(h->comm_stream, h->asm_ev, 0));
    for (int c = 0; c < (F.n + NBO - 1) / NBO; c++) {
      size_t cb, cn;
      chunk_range(F.n, ld, c, cb, cn);
      NCCLCHECK(ncclAllReduce(Asm + cb, Asm + cb, cn, ncclDouble, ncclSum, h->comm_data ? h->comm_data : h->comm, h->comm_stream));
      HIPCHECK(hipEventRecord(h->chunk_ev[c], h->comm_stream));
    }
  }

  const lmgpu_handle::DensePlan& plan = h->dense_plans[fi];
  h->inv16_owner = fi;  // the per-panel 16x16 inverses now belong to this front (read again by its back-substitution)
  const DenseExec X{s, A, split ? (const double*)Asm : nullptr, ld, F.n, F.nf, F.id, h->d_status, h->inv16, 4096, h->d_pflags, h->pflags_prefilled,
                    h->d_chain_tasks, plan.task_begin.data(), plan.task_count.data(), &h->kt, h->sw.chain_forms, h->sw.tail_scalar,
                    h->chain_resident, h->sw.chain_one_task, h->sw.chain_grid};
  return run_dense_steps(X, plan.steps, [&](int kind, int c) { return kind == DENSE_ADD_CHUNK ? add_chunk(h, A, Asm, F.n, ld, c) : wait_chunk(h, Asm, F.n, ld, c); },
                         &h->err);
}

// The elimination as a list of launches: the clears, then level by level the LDS fronts (merged segment, fused level or bins), the medium
// fronts and the dense fronts.
int do_eliminate(lmgpu_handle* h, double lambda_v, const double* lambda_p) {  // lambda by value (eager) or in device memory (graph replay)
  hipStream_t s = h->stream;
  const Damping dmp{lambda_v, lambda_p, h->dampw, h->gex_active};
  const bool merge_el = h->merge_elim && !h->elim_segs.empty();
  int rc = eliminate_clears(h);
  if (rc) return rc;
  // (Running a level's LDS fronts on a second stream beside its dense fronts -- they only depend on the levels below -- was measured
  //  with the replayed graph: 4.9 vs 2.5 ms per LM iteration on sphere2500; every cross-stream edge of the graph costs more than the
  //  45 us of LDS-front latency it hides.  Not kept.)
  if (merge_el)  // "not published yet" over the update matrices of the merged launches' fronts
    hipLaunchKernelGGL(fill_upper_kernel, dim3(h->n_fill_upper), dim3(256), 0, s, (const FillUpper*)h->d_fill_upper, h->pool);
  for (size_t li = 0; li < h->levels.size(); li++) {
    const LevelWork& L = h->levels[li];
    const int seg = merge_el ? h->elim_seg_of[li] : -1;  // >= 0: a merged segment starts here; -2: the level lies inside one
    const bool fused = h->fuse_levels && L.fuse_task_count > 0;
    const MedLevel ML{(const MedFront*)(h->d_med_fronts + L.med_begin)};
    if (seg >= 0) {  // the LDS fronts of the segment's levels as one launch (no relay: the status word is read back with the solve's scalars)
      const lmgpu_handle::ElimSeg& E = h->elim_segs[seg];
      const int kt = h->kt.begin(LMGPU_KT_LDS_FRONT, s);
      launch_lds_fronts_merged(s, h->tabs, h->pool, h->d_status, dmp, h->levels[E.lvl_lo].list_begin,
                               h->levels[E.lvl_hi].list_begin + h->levels[E.lvl_hi].list_count, E.threads, E.nmax, E.jcap,
                               h->d_bs_done + h->h_fronts.size() + E.lvl_hi, nullptr);
      h->kt.end(kt, s);
    }
    if (fused) {  // the level's LDS fronts and medium fronts in one grid
      const int kt = h->kt.begin(LMGPU_KT_PANEL, s);
      launch_level_fused(s, h->tabs, h->pool, h->d_status, dmp, h->d_level_tasks + L.fuse_task_begin, L.fuse_task_count,
                         h->d_bs_done + h->h_fronts.size() + li, L.fuse_threads, L.fuse_nmax, L.fuse_jcap, ML, h->inv16_med, h->d_level_sync + L.med_begin);
      h->kt.end(kt, s);
    }
    if (seg == -1 && !fused) eliminate_level_bins(h, L, dmp);
    if (L.med_count > 0 && !fused) launch_med_level(s, h->tabs, h->pool, h->d_status, dmp, h->kt, L, ML, h->inv16_med);
    for (int fi : L.hbm)
      if (!h->is_med[fi] && (rc = eliminate_hbm_front(h, fi, dmp))) return rc;
  }
  HIPCHECK(hipGetLastError());
  return LMGPU_OK;
}

// Does this front qualify for lds_front_group_kernel (kernels_leaf.hpp)?  0: no; 1: yes, nf <= 3 and every binary factor of at most two rows; 2: yes.
// A gather leaf ([R S d] stored with ld_rsd = n) with a single-batch packed record (the conditions of the LEAFPACK_* records below, has_xo included), nf <= LEAFGRP_MAXNF,
// not replicated, every factor unary on a frontal variable or binary between one frontal and one separator variable, at most
// LEAFGRP_MAXROWS rows and LEAFGRP_MAXSEP separator columns per factor, and no separator variable shared by two factors (a lane owns
// its factor's separator columns of [R S d]).
static int leaf_group_form(const FrontDesc& F, const FrontFac* ffac, const FacDesc* fd, int jcap) {
  if (F.par_ld != -1 || F.pad != 0 || F.nf < 1 || F.nf > LEAFGRP_MAXNF || F.nf > LEAFPACK_MAXNF || F.ld_rsd != F.n) return 0;
  if (F.fac_count < 1 || F.fac_count > LDSF_MAXB) return 0;
  int form = F.nf <= 3 ? 1 : 2;
  int32_t seen[LDSF_MAXB];
  int nseen = 0;
  for (int k = 0; k < F.fac_count; k++) {
    const FrontFac& ff = ffac[F.fac_begin + k];
    const FacDesc& d = fd[ff.fac];
    if (d.d2 > 0 || d.rows < 1 || d.rows > LEAFGRP_MAXROWS) return 0;
    if (d.d1 == 0) {  // unary: on frontal columns
      if (ff.c0 + d.d0 > F.nf) return 0;
      continue;
    }
    const bool f0 = ff.c0 < F.nf, f1 = ff.c1 < F.nf;
    if (f0 == f1) return 0;  // both frontal, or none
    const int cf = f0 ? ff.c0 : ff.c1, df = f0 ? d.d0 : d.d1, cs = f0 ? ff.c1 : ff.c0, ds = f0 ? d.d1 : d.d0;
    if (cf + df > F.nf || ds > LEAFGRP_MAXSEP || cs + ds > F.n - 1) return 0;
    for (int q = 0; q < nseen; q++)
      if (seen[q] == cs) return 0;
    seen[nseen++] = cs;
    if (d.rows > 2) form = 2;
  }
  if (front_jacobian_doubles(F, ffac, fd) > jcap) return 0;  // no single-batch record
  return form;
}

// the LDS fronts of level l as one launch sized for the level's largest front (merged and fused launches): false when the level has none, too
// many of them (a launch sized for the largest front would cost the small ones their occupancy), or gather leaves
static bool level_lds_class(const lmgpu_handle* h, int l, int* nmax, int* jcap, int* threads) {
  const int kMergeCap = 160;
  const LevelWork& L = h->levels[l];
  if (L.list_count == 0 || L.list_count > kMergeCap || L.bin_begin[kNumBins] != L.bin_begin[6]) return false;
  int top = -1, jc = 96, cnt_top = 0;
  for (int b = 0; b < 6; b++)
    if (L.bin_begin[b + 1] > L.bin_begin[b]) {
      top = b;
      cnt_top = L.bin_begin[b + 1] - L.bin_begin[b];
      jc = std::max(jc, L.bin_jcap[b]);
    }
  *nmax = kBinN[top];
  *jcap = jc;
  const bool wide16 = top >= 3 && cnt_top <= h->sw.wide16_max && !h->sw.no_wide16;
  *threads = wide16 ? 1024 : (top == 0 ? 64 : 256);  // (four waves from 25 columns on: the blocked Cholesky of the LDS body needs them)
  // (ISAM2 sizes its merged launch by a rule of its own: is_launch_merged, isam2.hpp)
  return true;
}

// Which kernel the plain per-level back-substitution launch of level L takes.  0: lds_backsub_kernel / lds_backsub_wide_kernel; 1:
// lds_backsub_group_kernel<3, 6> (every front nf <= 3, separators of at most 96 columns); 2: lds_backsub_group_kernel<LDSBG_MAXNF, 9>.
static int backsub_group_form(const lmgpu_handle* h, const LevelWork& L) {
  if (L.list_count == 0 || L.lds_nf_max > LDSBG_MAXNF || h->sw.no_backsub_groups) return 0;
  return (L.lds_nf_max <= 3 && L.lds_ns_max <= 6 * LEAFGRP_LANES) ? 1 : 2;
}

// ---- back-substitution, top-down (a14)
// the LDS fronts of one level as a launch of their own
static void backsub_lds_level(lmgpu_handle* h, const LevelWork& L) {
  const int group = backsub_group_form(h, L);
  const LdsBacksubForm form = L.lds_nf_max > LDSB_SMALL_NF ? LDS_BACKSUB_WIDE
                              : group == 1                 ? LDS_BACKSUB_GROUP_SMALL
                              : group == 2                 ? LDS_BACKSUB_GROUP
                                                           : LDS_BACKSUB_PLAIN;
  launch_lds_backsub(h->stream, h->tabs, h->pool, h->delta, h->d_status, form, L.list_begin, L.list_count, L.lds_rsd_max);
}

// the LDS fronts of levels lo .. hi (bottom, top) of the merged back-substitution: one level as its own launch, several as ONE dataflow launch
static void backsub_lds_segment(lmgpu_handle* h, int lo, int hi) {
  hipStream_t s = h->stream;
  const int kt = h->kt.begin(LMGPU_KT_BACKSUB_LDS, s);
  if (hi == lo) {
    backsub_lds_level(h, h->levels[hi]);
  } else {
    const int b = h->levels[lo].list_begin, e = h->levels[hi].list_begin + h->levels[hi].list_count;
    int rsdmax = 0;
    for (int l = lo; l <= hi; l++) rsdmax = std::max(rsdmax, h->levels[l].lds_rsd_max);
    const BacksubMergeDev M{h->d_bs_parent, h->d_bs_pos, h->d_bs_done, h->d_bs_done + (int)h->h_fronts.size() + hi};
    launch_lds_backsub(s, h->tabs, h->pool, h->delta, h->d_status, LDS_BACKSUB_MERGED, b, e - b, rsdmax, &M);
  }
  h->kt.end(kt, s);
}

// HBM front fi of more than BSS_MAX_NF rows: y = d - S x_S, then ONE dataflow launch over its row blocks
static int backsolve_hbm_front(lmgpu_handle* h, int fi) {
  hipStream_t s = h->stream;
  const FrontDesc& F = h->h_fronts[fi];
  const int64_t off = h->f_off[fi];
  const int ld = h->f_ld[fi];
  const int kt = h->kt.begin(LMGPU_KT_BACKSUB_HBM, s);
  const bool has_sep = F.n - F.nf - 1 > 0;
  if (has_sep)  // y = d - S x_S (a root reads d in place)
    hipLaunchKernelGGL(hbm_rhs_init_kernel, dim3(F.nf), dim3(64), 0, s, F, off, ld, (const int32_t*)h->d_sxoff, (const double*)h->pool,
                       (const double*)h->delta, h->ywork);
  // ONE dataflow launch: workgroup b waits for x_j (j > b); the inverses of the diagonal blocks are built inside it when the 16 x 16
  // inverses of this front's factorisation are still there (else by a launch of their own in front of it).  128-row blocks with
  // explicit inverses then (hbm_backsolve_wide_kernel); 64-row blocks in the fallback and, test library only, under LMGPU_BACKSOLVE_HOP64
  const bool reuse = h->inv16_owner == fi && !h->sw.no_inv16_reuse;
  const bool wide = reuse && !h->sw.backsolve_hop64;
  const int bw = wide ? BSW_NB : NB, nblk = (F.nf + bw - 1) / bw;
  if (!h->bs_prefilled) {  // (else cleared by the fill launch at the head of the elimination: ensure_fill_tables)
    HIPCHECK(hipMemsetAsync(h->bs_flags, 0, (nblk + 1) * sizeof(unsigned int), s));  // flags + ticket
    HIPCHECK(hipMemsetAsync(h->bs_x, 0xff, (size_t)nblk * bw * sizeof(double), s));  // sentinel: "not published yet"
  }
  if (wide) {
    hipLaunchKernelGGL((hbm_backsolve_wide_kernel<false>), dim3(nblk), dim3(512), 0, s, F, off, ld, (const int32_t*)h->d_fxoff, (const double*)h->pool,
                       (const double*)h->inv16, has_sep ? (const double*)h->ywork : (const double*)nullptr, h->bs_x, h->bs_flags, h->delta,
                       h->d_status, h->bs_inv, (unsigned long long*)nullptr);
#ifdef LMGPU_TEST_HOOKS
  } else if (reuse) {
    hipLaunchKernelGGL((hbm_backsolve_dataflow2_kernel<false>), dim3(nblk), dim3(256), 0, s, F, off, ld, (const int32_t*)h->d_fxoff, (const double*)h->pool,
                       (const double*)h->inv16, has_sep ? (const double*)h->ywork : (const double*)nullptr, h->bs_x, h->bs_flags, h->delta,
                       h->d_status, (unsigned long long*)nullptr);
#endif
  } else {
    if (!has_sep)
      hipLaunchKernelGGL(hbm_rhs_init_kernel, dim3(F.nf), dim3(64), 0, s, F, off, ld, (const int32_t*)h->d_sxoff, (const double*)h->pool,
                         (const double*)h->delta, h->ywork);
    hipLaunchKernelGGL((hbm_invert_diag_kernel<NB>), dim3(nblk), dim3(NB), 0, s, (const double*)(h->pool + off), ld, F.nf, h->bs_inv);
    hipLaunchKernelGGL((hbm_backsolve_dataflow_kernel<NB>), dim3(nblk), dim3(256), 0, s, F, off, ld, (const int32_t*)h->d_fxoff,
                       (const double*)h->pool, (const double*)h->bs_inv, (const double*)h->ywork, h->bs_x, h->bs_flags, h->delta,
                       h->d_status);
  }
  h->kt.end(kt, s);
  return LMGPU_OK;
}

// ---- back-substitution, top-down (a14)
int do_backsub(lmgpu_handle* h) {
  hipStream_t s = h->stream;
  if (h->cfg.world_size > 1) HIPCHECK(hipMemsetAsync(h->delta, 0, h->ntot * sizeof(double), s));
  const bool merge = backsub_merged(h);
  if (h->n_fill_backsub > 0) hipLaunchKernelGGL(fill_chunks_kernel, dim3(h->n_fill_backsub), dim3(256), 0, s, (const FillChunk*)h->d_fill_backsub);
  int seg_hi = -1, seg_lo = -1;  // levels of the pending segment (top, bottom)
  auto flush_segment = [&] {
    if (seg_hi >= 0) backsub_lds_segment(h, seg_lo, seg_hi);
    seg_hi = seg_lo = -1;
  };
  for (int li = (int)h->levels.size() - 1; li >= 0; li--) {
    const LevelWork& L = h->levels[li];
    if (merge && !L.hbm.empty()) flush_segment();  // this level's HBM fronts need every ancestor: finish the pending LDS levels first
    const int brun = (merge && !h->bsd_run_of.empty() && !h->sw.no_bsd_runs) ? h->bsd_run_of[li] : -1;
    if (brun >= 0) {  // this level and the ones below it that hold nothing but block-solved fronts: one launch, separator values awaited by value
      const lmgpu_handle::BsdRun& R = h->bsd_runs[brun];
      const int kt = h->kt.begin(LMGPU_KT_BACKSUB_HBM, s);
      launch_backsolve_blocks(s, h->tabs, h->pool, h->delta, h->d_bsd_x, h->d_status, h->d_bsd_run_table + R.begin, R.count, h->d_bsd_ticket + li, 1);
      h->kt.end(kt, s);
    }
    if (L.bsd_count > 0 && brun == -1) {  // the smaller HBM fronts of the level: one workgroup per 64-row block, one launch
      const int kt = h->kt.begin(LMGPU_KT_BACKSUB_HBM, s);
      launch_backsolve_blocks(s, h->tabs, h->pool, h->delta, h->d_bsd_x, h->d_status, h->d_bsd_table + L.bsd_begin, L.bsd_count,
                              (L.bsd_count <= h->num_cus && !h->sw.bsd_ticket) ? nullptr : h->d_bsd_ticket + li, 0);
      h->kt.end(kt, s);
    }
    for (int fi : L.hbm)
      if (h->h_fronts[fi].nf > BSS_MAX_NF) {  // (the others: done above)
        const int rc = backsolve_hbm_front(h, fi);
        if (rc) return rc;
      }
    if (merge) {  // accumulated; flushed before the next HBM front or at the end
      if (L.list_count > 0) {
        if (seg_hi < 0) seg_hi = li;
        seg_lo = li;
      }
      if (li == 0 || !h->levels[li - 1].hbm.empty()) flush_segment();
    } else if (L.list_count > 0) {
      const int kt = h->kt.begin(LMGPU_KT_BACKSUB_LDS, s);
      backsub_lds_level(h, L);
      h->kt.end(kt, s);
    }
  }
  HIPCHECK(hipGetLastError());
  return LMGPU_OK;
}

// Solve the damped system.  do_solve_enqueue queues everything (eliminate, back-substitute, the two linear errors and the
// copies of the scalars / the status word to pinned host memory) without waiting; do_solve_finish waits for the stream and
// returns LMGPU_OK / LMGPU_INDETERMINATE with the linear errors in h_scal[1], h_scal[2].  tryLambda queues the retraction and
// the new error behind the solve BEFORE it waits (one host round trip per inner iteration instead of two); their result is
// simply not used when the solve failed or the linearised cost went up.
__global__ void set_scalar_kernel(double* p, double v) { *p = v; }


// ---- PCG (kernels_pcg.hpp): buffers at first use (a handle finalized for Cholesky may switch over later)
int pcg_ensure(lmgpu_handle* h) {
  if (h->pcg_ready) return LMGPU_OK;
  const Plan& P = h->plan;
  std::vector<int32_t> xo(P.xoff.begin(), P.xoff.begin() + P.n_vars + 1);
  std::vector<int64_t> loff(P.n_vars);
  int64_t lsz = 0;
  for (int s = 0; s < P.n_vars; s++) {
    loff[s] = lsz;
    lsz += (int64_t)P.dims[s] * P.dims[s];
  }
  std::vector<FacDesc> fd(h->nfac);
  HIPCHECK(hipMemcpy(fd.data(), h->d_fd, fd.size() * sizeof(FacDesc), hipMemcpyDeviceToHost));
  std::vector<int64_t> yoff(h->nfac);
  int64_t ysz = 0;
  for (int f = 0; f < h->nfac; f++) {
    yoff[f] = ysz;
    ysz += fd[f].rows;
  }
  int rc;
  if ((rc = upload(h, &h->pcg_xoff, xo))) return rc;
  if ((rc = upload(h, &h->pcg_loff, loff))) return rc;
  if ((rc = upload(h, &h->pcg_yoff, yoff))) return rc;
  const size_t n = std::max(1, h->ntot);
  HIPCHECK(hipMalloc((void**)&h->pcg_H, std::max<int64_t>(1, lsz) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_L, std::max<int64_t>(1, lsz) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_rhs, n * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_r, n * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_p, n * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_q, n * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_y, std::max<int64_t>(1, ysz) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_part, 3 * PCG_MAXPART * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->pcg_ctl, sizeof(PcgCtl)));
  HIPCHECK(hipHostMalloc((void**)&h->h_pcg_ctl, sizeof(PcgCtl), hipHostMallocDefault));
  HIPCHECK(hipHostMalloc((void**)&h->h_pcg_done, sizeof(int32_t), hipHostMallocDefault));
  for (int i = 0; i < 3; i++) HIPCHECK(hipEventCreate(&h->pcg_ev[i]));
  h->pcg_ready = true;
  return LMGPU_OK;
}

__global__ void pcg_reset_ctl_kernel(PcgCtl* c) {
  c->status = 0x7fffffff;
  c->iters = 0;
}

// One PCG solve into h->delta, then the two linear errors like solve_sequence.  The loop is queued 16 iterations at a time with one
// host wait per chunk (a chunk queued after convergence would do nothing: every kernel of iteration k first reads done[k - 1]).
int pcg_solve_enqueue(lmgpu_handle* h, double lambda) {
  int rc = pcg_ensure(h);
  if (rc) return rc;
  const lmgpu_pcg_params& pp = h->pcgp;
  if (pp.maxIterations + 1 > h->pcg_cap) {
    if (h->pcg_gam) (void)hipFree(h->pcg_gam);
    if (h->pcg_done) (void)hipFree(h->pcg_done);
    h->pcg_gam = nullptr;
    h->pcg_done = nullptr;
    h->pcg_cap = 0;
    HIPCHECK(hipMalloc((void**)&h->pcg_gam, (size_t)(pp.maxIterations + 1) * sizeof(double)));
    HIPCHECK(hipMalloc((void**)&h->pcg_done, (size_t)(pp.maxIterations + 1) * sizeof(int32_t)));
    h->pcg_cap = pp.maxIterations + 1;
  }
  hipStream_t s = h->stream;
  const bool bj = pp.preconditioner == LMGPU_PRECOND_BLOCK_JACOBI;
  const int nv = h->plan.n_vars, ntot = h->ntot, nfac = h->nfac;
  const PcgVars V{nv, h->pcg_xoff, h->pcg_loff};
  const int gs = std::max(1, std::min(PCG_MAXPART, (ntot + 255) / 256));  // scalar kernels (their partials: p . q)
  const int gv = std::max(1, std::min(PCG_MAXPART, (nv + 255) / 256));    // variable kernels (their partials: r . r)
  const int gf = std::max(1, (nfac + 255) / 256);
  double* part_pq = h->pcg_part;
  double* part_rr = h->pcg_part + PCG_MAXPART;
  double* part_rs = h->pcg_part + 2 * PCG_MAXPART;  // r . r of the initial / a reset residual
  const double* L = h->pcg_L;
  double* x = h->delta;
  (void)hipEventRecord(h->ev[1], s);
  (void)hipEventRecord(h->pcg_ev[0], s);
  hipLaunchKernelGGL(pcg_reset_ctl_kernel, dim3(1), dim3(1), 0, s, h->pcg_ctl);
  if (!h->pcg_gram_valid && ntot > 0) {
    hipLaunchKernelGGL(pcg_gram_kernel, dim3((ntot + 255) / 256), dim3(256), 0, s, ntot, (const int32_t*)h->d_scalar_var,
                       (const int32_t*)h->d_scalar_col, (const int32_t*)h->d_vi_ptr, (const int32_t*)h->d_vi_fac, (const int8_t*)h->d_vi_pos,
                       (const FacDesc*)h->d_fd, (const double*)h->pool, V, h->pcg_H, h->pcg_rhs);
    h->pcg_gram_valid = true;
  }
  if (bj) hipLaunchKernelGGL(pcg_chol_kernel, dim3((nv + 255) / 256), dim3(256), 0, s, V, (const double*)h->pcg_H, lambda, (const double*)h->dampw, h->pcg_L, h->pcg_ctl);
  (void)hipEventRecord(h->pcg_ev[1], s);
  if (bj)
    hipLaunchKernelGGL((pcg_precond_kernel<true, true>), dim3(gv), dim3(256), 0, s, V, L, (const double*)h->pcg_rhs, x, h->pcg_r, h->pcg_p, part_rs, (const int32_t*)nullptr, 0);
  else
    hipLaunchKernelGGL((pcg_precond_kernel<true, false>), dim3(gv), dim3(256), 0, s, V, L, (const double*)h->pcg_rhs, x, h->pcg_r, h->pcg_p, part_rs, (const int32_t*)nullptr, 0);
  hipLaunchKernelGGL(pcg_start_kernel, dim3(1), dim3(256), 0, s, (const double*)part_rs, gv, pp.epsilon_rel, pp.epsilon_abs, pp.minIterations,
                     pp.maxIterations, h->pcg_gam, h->pcg_done, h->pcg_ctl);
  int waits = 0;
  const bool fz = h->sw.pcg_fused;
  for (int k = 1; k <= pp.maxIterations;) {
    const int kend = std::min(pp.maxIterations, k + 15);
    for (; k <= kend; k++) {
      const int rs = (k % pp.reset == 0) ? 1 : 0;
      const int32_t* dn = h->pcg_done;
      if (rs) {  // r = L^-1 (b - A x), p = L^-T r, gamma = r . r  (ConjugateGradientSolver.h:149-154)
        if (!fz)
          hipLaunchKernelGGL(pcg_forward_kernel, dim3(gf), dim3(256), 0, s, (const FacDesc*)h->d_fd, nfac, (const int64_t*)h->pcg_yoff,
                             (const double*)h->pool, (const double*)x, h->pcg_y, dn, k);
        hipLaunchKernelGGL((fz ? pcg_transpose_kernel<true, true> : pcg_transpose_kernel<true, false>), dim3(gs), dim3(256), 0, s, ntot, (const int32_t*)h->d_scalar_var, (const int32_t*)h->d_scalar_col,
                           (const int32_t*)h->d_vi_ptr, (const int32_t*)h->d_vi_fac, (const int8_t*)h->d_vi_pos, (const FacDesc*)h->d_fd,
                           (const double*)h->pool, (const int64_t*)h->pcg_yoff, (const double*)h->pcg_y, (const double*)x, lambda,
                           (const double*)h->dampw, (const double*)h->pcg_rhs, h->pcg_q, (double*)nullptr, dn, k);
        if (bj)
          hipLaunchKernelGGL((pcg_precond_kernel<false, true>), dim3(gv), dim3(256), 0, s, V, L, (const double*)h->pcg_q, x, h->pcg_r, h->pcg_p, part_rs, dn, k);
        else
          hipLaunchKernelGGL((pcg_precond_kernel<false, false>), dim3(gv), dim3(256), 0, s, V, L, (const double*)h->pcg_q, x, h->pcg_r, h->pcg_p, part_rs, dn, k);
      }
      // q = A p
      if (!fz)
        hipLaunchKernelGGL(pcg_forward_kernel, dim3(gf), dim3(256), 0, s, (const FacDesc*)h->d_fd, nfac, (const int64_t*)h->pcg_yoff,
                           (const double*)h->pool, (const double*)h->pcg_p, h->pcg_y, dn, k);
      hipLaunchKernelGGL((fz ? pcg_transpose_kernel<false, true> : pcg_transpose_kernel<false, false>), dim3(gs), dim3(256), 0, s, ntot, (const int32_t*)h->d_scalar_var, (const int32_t*)h->d_scalar_col,
                         (const int32_t*)h->d_vi_ptr, (const int32_t*)h->d_vi_fac, (const int8_t*)h->d_vi_pos, (const FacDesc*)h->d_fd,
                         (const double*)h->pool, (const int64_t*)h->pcg_yoff, (const double*)h->pcg_y, (const double*)h->pcg_p, lambda,
                         (const double*)h->dampw, (const double*)h->pcg_rhs, h->pcg_q, part_pq, dn, k);
      if (bj) {
        hipLaunchKernelGGL(pcg_update_kernel<true>, dim3(gv), dim3(256), 0, s, V, L, (const double*)part_pq, gs, (const double*)part_rs, gv,
                           (const double*)h->pcg_gam, (const double*)h->pcg_p, (const double*)h->pcg_q, x, h->pcg_r, part_rr, dn, k, rs);
        hipLaunchKernelGGL(pcg_direction_kernel<true>, dim3(gv), dim3(256), 0, s, V, L, (const double*)part_rr, gv, (const double*)part_rs, gv,
                           h->pcg_gam, (const double*)h->pcg_r, h->pcg_p, h->pcg_done, h->pcg_ctl, k, rs, pp.minIterations, pp.maxIterations);
      } else {
        hipLaunchKernelGGL(pcg_update_kernel<false>, dim3(gv), dim3(256), 0, s, V, L, (const double*)part_pq, gs, (const double*)part_rs, gv,
                           (const double*)h->pcg_gam, (const double*)h->pcg_p, (const double*)h->pcg_q, x, h->pcg_r, part_rr, dn, k, rs);
        hipLaunchKernelGGL(pcg_direction_kernel<false>, dim3(gv), dim3(256), 0, s, V, L, (const double*)part_rr, gv, (const double*)part_rs, gv,
                           h->pcg_gam, (const double*)h->pcg_r, h->pcg_p, h->pcg_done, h->pcg_ctl, k, rs, pp.minIterations, pp.maxIterations);
      }
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(h->h_pcg_done, h->pcg_done + kend, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(&h->h_pcg_ctl->status, &h->pcg_ctl->status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    waits++;
    if (h->h_pcg_ctl->status != 0x7fffffff) break;  // an indefinite diagonal block: the iterations are meaningless
    if (*h->h_pcg_done) break;
  }
  (void)hipEventRecord(h->pcg_ev[2], s);
  (void)hipEventRecord(h->ev[2], s);
  (void)hipEventRecord(h->ev[3], s);  // no back-substitution: backsub_ms = 0
  if (nfac > 0)
    hipLaunchKernelGGL(linear_error_kernel, dim3((nfac + 255) / 256), dim3(256), 0, s, (const FacDesc*)h->d_fd, nfac, (const double*)h->pool,
                       (const double*)x, h->ebuf0, h->ebuf1);
  reduce_to(h, h->ebuf0, h->n_counted, h->dscal + 1);
  reduce_to(h, h->ebuf1, h->n_counted, h->dscal + 2);
  (void)hipEventRecord(h->ev[4], s);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(h->h_scal + 1, h->dscal + 1, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(h->h_pcg_ctl, h->pcg_ctl, sizeof(PcgCtl), hipMemcpyDeviceToHost, s));
  h->pcg_stats.host_waits = waits + 1;  // + the wait of do_solve_finish
  return LMGPU_OK;
}

int pcg_solve_finish(lmgpu_handle* h) {
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->kt.resolve();
  h->solved = true;
  const PcgCtl& c = *h->h_pcg_ctl;
  lmgpu_pcg_stats& st = h->pcg_stats;
  st.iterations = c.iters;
  st.gamma0 = c.gamma0;
  st.gamma = c.gamma;
  st.threshold = c.threshold;
  float ms = 0;
  st.precond_ms = (hipEventElapsedTime(&ms, h->pcg_ev[0], h->pcg_ev[1]) == hipSuccess) ? ms : 0.0;
  st.iterate_ms = (hipEventElapsedTime(&ms, h->pcg_ev[1], h->pcg_ev[2]) == hipSuccess) ? ms : 0.0;
  h->pcg_have_stats = true;
  if (c.status != 0x7fffffff) {
    h->failed_slot = c.status;
    h->err = "PCG: the diagonal block of variable slot " + std::to_string(c.status) + " is not positive definite";
    return LMGPU_INDETERMINATE;
  }
  return LMGPU_OK;
}

// the solver a solve of this handle takes (the marginal covariances always eliminate: they need the direct path's unit-gradient solves)
static bool use_pcg(const lmgpu_handle* h) { return h->solver == LMGPU_SOLVER_PCG && !h->gex_active && !h->marg_factoring; }

// everything of one damped solve that is queued on the stream
int solve_sequence(lmgpu_handle* h, bool phase_events, double lambda_v, const double* lambda_p) {
  hipStream_t s = h->stream;
  int rc = do_eliminate(h, lambda_v, lambda_p);
  if (rc) return rc;
  if (phase_events) (void)hipEventRecord(h->ev[2], s);
  rc = do_backsub(h);
  if (rc) return rc;
  if (phase_events) (void)hipEventRecord(h->ev[3], s);
  const int kt = h->kt.begin(LMGPU_KT_LINEAR_ERROR, s);
  if (h->nfac > 0)
    hipLaunchKernelGGL(linear_error_kernel, dim3((h->nfac + 255) / 256), dim3(256), 0, s, (const FacDesc*)h->d_fd, h->nfac,
                       (const double*)h->pool, (const double*)h->delta, h->ebuf0, h->ebuf1);
  reduce_to(h, h->ebuf0, h->n_counted, h->dscal + 1);
  reduce_to(h, h->ebuf1, h->n_counted, h->dscal + 2);
  h->kt.end(kt, s);
  rc = allreduce_scalars(h, 1, 2);
  if (rc) return rc;
  { const int rcs = allreduce_min_int(h, h->d_status, s); if (rcs) return rcs; }
  return LMGPU_OK;
}

// Deep clique trees (general SLAM graphs: 20-130 levels, several launches per level) are bound by launch latency: 265 launches
// of 3.5 ms total kernel time took 6.8 ms per solve on victoria_park / COLAMD.  The launch sequence of a solve depends only on
// the structure, so after the first (eager) solve it is captured into a hipGraph once and replayed; the only per-solve
// input, lambda, lives in device memory.  Not with kernel timers on (their events sit between the launches), with several
// ranks (collectives and host-side rendezvous inside the sequence), or for shallow trees (nothing to gain; the per-phase
// events of the eager path stay available there).
static bool graph_eligible(const lmgpu_handle* h) {
  return h->use_graph && !h->kt.on && h->cfg.world_size == 1 && !h->comm && !h->lgroup && !(h->cfg.flags & LMGPU_FLAG_SPLIT_ROOT) &&
         h->eager_solves >= 1;
}

int do_solve_enqueue(lmgpu_handle* h, double lambda) {
  h->marg_valid = false;  // the fronts are about to be overwritten
  if (use_pcg(h)) return pcg_solve_enqueue(h, lambda);
  hipStream_t s = h->stream;
  int rc = ensure_dense_schedules(h);  // (both allocate and upload at the first solve: before anything is queued or captured)
  if (!rc) rc = ensure_fill_tables(h);
  if (rc) return rc;
  (void)hipEventRecord(h->ev[1], s);
  if (graph_eligible(h)) {
    hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, s, h->d_lambda, lambda);  // the replay reads lambda from device memory
    hipGraphExec_t& exec = h->solve_graph[h->gex_active ? 1 : 0];
    if (!exec) {
      hipGraph_t graph = nullptr;
      HIPCHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      rc = solve_sequence(h, false, 0.0, h->d_lambda);
      const hipError_t ec = hipStreamEndCapture(s, &graph);
      if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      HIPCHECK(ec);
      HIPCHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      (void)hipGraphDestroy(graph);
    }
    HIPCHECK(hipGraphLaunch(exec, s));
    // no phase boundaries inside a replay: the whole sequence is booked as elimination time
    (void)hipEventRecord(h->ev[2], s);
    (void)hipEventRecord(h->ev[3], s);
  } else {
    rc = solve_sequence(h, true, lambda, nullptr);
    if (rc) return rc;
    h->eager_solves++;
  }
  if (h->smart) smart_fix_lin0(h);
  (void)hipEventRecord(h->ev[4], s);
  HIPCHECK(hipMemcpyAsync(h->h_scal + 1, h->dscal + 1, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(h->h_status, h->d_status, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  return LMGPU_OK;
}

int do_solve_finish(lmgpu_handle* h) {
  if (use_pcg(h)) return pcg_solve_finish(h);
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->kt.resolve();
  h->solved = true;
  if (h->h_status[1] != 0) {  // a bounded spin of an in-launch hand-off ran out: a scheduling / protocol fault, NOT an ill-conditioned system
    h->err = "in-launch dataflow hand-off timed out in front " + std::to_string(h->h_status[1] - 1) + " (spin bound hit)";
    return LMGPU_HIP_ERROR;
  }
  if (*h->h_status < (int)h->h_fronts.size()) {
    const Front& fr = h->plan.fronts[*h->h_status];
    h->failed_slot = fr.vars[0] - h->n_hidden;  // (negative: the hidden point of a smart factor)
    return LMGPU_INDETERMINATE;
  }
  return LMGPU_OK;
}

int do_solve(lmgpu_handle* h, double lambda) {
  const int rc = do_solve_enqueue(h, lambda);
  if (rc) return rc;
  return do_solve_finish(h);
}

int do_retract(lmgpu_handle* h, int from, int to) {
  h->marg_valid = false;
  static_assert(kNumVarTypes <= 7, "RetractMulti holds seven entries");
  RetractMulti rm{};  // the variable types present, one launch (blockIdx.y = entry; retract_body is retract_kernel's)
  int ne = 0, maxn = 0;
  for (int t = 0; t < kNumVarTypes; t++) {
    // the hidden points of smart factors are the first POINT3 variables: never retracted (their value is the cache's, smart.hpp)
    const int skip = t == LMGPU_POINT3 ? h->n_hidden : 0;
    const int n = h->plan.type_count[t] - skip;
    if (n == 0) continue;
    rm.type[ne] = t;
    rm.n[ne] = n;
    rm.cur[ne] = (const double*)h->vals[from][t] + 3 * skip;
    rm.out[ne] = h->vals[to][t] + 3 * skip;
    rm.xoff[ne] = (const int32_t*)h->type_xoff[t] + skip;
    rm.sel[ne] = nullptr;
    maxn = std::max(maxn, n);
    ne++;
  }
  if (ne > 0) hipLaunchKernelGGL(retract_multi_kernel, dim3((maxn + 255) / 256, ne), dim3(256), 0, h->stream, rm, (const double*)h->delta);
  HIPCHECK(hipGetLastError());
  return LMGPU_OK;
}

void accumulate_times(lmgpu_handle* h, bool with_retract) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev[1], h->ev[2]) == hipSuccess) h->tim.eliminate_ms += ms;
  if (hipEventElapsedTime(&ms, h->ev[2], h->ev[3]) == hipSuccess) h->tim.backsub_ms += ms;
  if (hipEventElapsedTime(&ms, h->ev[3], h->ev[4]) == hipSuccess) h->tim.linear_error_ms += ms;
  if (with_retract && hipEventElapsedTime(&ms, h->ev[5], h->ev[6]) == hipSuccess) h->tim.retract_error_ms += ms;
}

// values[cur ^ 1] = retract(values[cur], delta); its nonlinear error into h_scal[0] (queued, no wait)
int enqueue_retract_and_error(lmgpu_handle* h) {
  (void)hipEventRecord(h->ev[5], h->stream);
  const int kt = h->kt.begin(LMGPU_KT_RETRACT_ERROR, h->stream);
  int rc = do_retract(h, h->cur, h->cur ^ 1);
  if (rc) return rc;
  if ((rc = launch_factors<false>(h, h->cur ^ 1))) return rc;
  reduce_to(h, h->ebuf0, h->n_counted, h->dscal);
  h->kt.end(kt, h->stream);
  rc = allreduce_scalars(h, 0, 1);
  if (rc) return rc;
  (void)hipEventRecord(h->ev[6], h->stream);
  HIPCHECK(hipMemcpyAsync(h->h_scal, h->dscal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return LMGPU_OK;
}

// LevenbergMarquardtOptimizer::tryLambda  (gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:121-270)
int try_lambda(lmgpu_handle* h, const lmgpu_lm_params* p, bool* done) {
  lmgpu_lm_state& st = h->lm;
  double modelFidelity = 0.0;
  bool step_is_successful = false, stopSearchingLambda = false;
  double newError = std::numeric_limits<double>::infinity(), costChange = 0.0;
  int rc = do_solve_enqueue(h, st.lambda);
  if (rc) return rc;
  h->smart_speculative = true;
  rc = enqueue_retract_and_error(h);  // speculative: used only if the solve succeeded and the linearised cost did not go up
  h->smart_speculative = false;
  if (rc) return rc;
  rc = do_solve_finish(h);
  if (rc != LMGPU_OK && rc != LMGPU_INDETERMINATE) return rc;
  const bool solved = (rc == LMGPU_OK);
  bool retracted = false;
  if (solved) {
    const double oldLin = h->h_scal[1], newLin = h->h_scal[2];
    const double linearizedCostChange = oldLin - newLin;
    if (linearizedCostChange >= 0) {
      newError = h->h_scal[0];
      retracted = true;
      costChange = st.error - newError;
      if (linearizedCostChange > std::numeric_limits<double>::epsilon() * oldLin) {
        modelFidelity = costChange / linearizedCostChange;
        step_is_successful = modelFidelity > p->minModelFidelity;
      }
      const double minAbsoluteTolerance = p->relativeErrorTol * st.error;
      if (std::abs(costChange) < minAbsoluteTolerance) stopSearchingLambda = true;
    }
  }
  if (retracted && h->smart) smart_commit(h);  // the reference evaluated the error here: its factors' caches moved with it
  accumulate_times(h, retracted);
  h->tim.inner_iterations += 1;
  if (step_is_successful) {
    // decreaseLambda (LevenbergMarquardtState.h:80-93)
    double newLambda = st.lambda, newFactor = st.currentFactor;
    if (p->useFixedLambdaFactor) {
      newLambda /= st.currentFactor;
    } else {
      newLambda *= std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * modelFidelity - 1.0, 3));
      newFactor = 2.0 * st.currentFactor;
    }
    newLambda = std::max(p->lambdaLowerBound, newLambda);
    h->cur ^= 1;
    h->linearized = false;
    st.error = newError;
    st.lambda = newLambda;
    st.currentFactor = newFactor;
    st.iterations += 1;
    st.totalNumberInnerIterations += 1;
    *done = true;
  } else if (!stopSearchingLambda) {
    // increaseLambda (:70-76)
    st.lambda *= st.currentFactor;
    st.totalNumberInnerIterations += 1;
    if (!p->useFixedLambdaFactor) st.currentFactor *= 2.0;
    *done = (st.lambda >= p->lambdaUpperBound);
  } else {
    *done = true;
  }
  return LMGPU_OK;
}

int lm_iterate(lmgpu_handle* h, const lmgpu_lm_params* p) {
  std::memset(&h->tim, 0, sizeof(h->tim));
  (void)hipEventRecord(h->ev[0], h->stream);
  int rc = do_linearize(h);
  if (rc) return rc;
  (void)hipEventRecord(h->ev[7], h->stream);
  rc = fill_dampw(h, p->diagonalDamping, p->minDiagonal, p->maxDiagonal);
  if (rc) return rc;
  bool done = false;
  while (!done) {
    rc = try_lambda(h, p, &done);
    if (rc) return rc;
  }
  HIPCHECK(hipStreamSynchronize(h->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev[0], h->ev[7]) == hipSuccess) h->tim.linearize_ms = ms;
  h->tim.total_ms = h->tim.linearize_ms + h->tim.eliminate_ms + h->tim.backsub_ms + h->tim.linear_error_ms + h->tim.retract_error_ms;
  return LMGPU_OK;
}

// GaussNewtonOptimizer::iterate (gtsam/nonlinear/GaussNewtonOptimizer.cpp:44-66): linearize, solve the UNDAMPED system
// (lambda = 0: nothing is added to the frontal diagonals), retract, error of the new values, iterations + 1.  An
// indeterminate system is returned as LMGPU_INDETERMINATE (the reference lets IndeterminantLinearSystemException escape).
int gn_iterate(lmgpu_handle* h) {
  std::memset(&h->tim, 0, sizeof(h->tim));
  (void)hipEventRecord(h->ev[0], h->stream);
  int rc = do_linearize(h);
  if (rc) return rc;
  (void)hipEventRecord(h->ev[7], h->stream);
  rc = fill_dampw(h, 0, 0.0, 0.0);
  if (rc) return rc;
  rc = do_solve(h, 0.0);
  if (rc) return rc;
  (void)hipEventRecord(h->ev[5], h->stream);
  const int kt = h->kt.begin(LMGPU_KT_RETRACT_ERROR, h->stream);
  rc = do_retract(h, h->cur, h->cur ^ 1);
  if (rc) return rc;
  if ((rc = launch_factors<false>(h, h->cur ^ 1))) return rc;
  reduce_to(h, h->ebuf0, h->n_counted, h->dscal);
  h->kt.end(kt, h->stream);
  rc = allreduce_scalars(h, 0, 1);
  if (rc) return rc;
  (void)hipEventRecord(h->ev[6], h->stream);
  HIPCHECK(hipMemcpyAsync(h->h_scal, h->dscal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->kt.resolve();
  accumulate_times(h, true);
  h->tim.inner_iterations += 1;
  h->cur ^= 1;
  h->linearized = false;
  h->lm.error = h->h_scal[0];
  h->lm.iterations += 1;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev[0], h->ev[7]) == hipSuccess) h->tim.linearize_ms = ms;
  h->tim.total_ms = h->tim.linearize_ms + h->tim.eliminate_ms + h->tim.backsub_ms + h->tim.linear_error_ms + h->tim.retract_error_ms;
  return LMGPU_OK;
}

// ---- Dogleg (gtsam/nonlinear/DoglegOptimizer.cpp:84-126; DoglegOptimizerImpl.h:139-254 with ONE_STEP_PER_ITERATION;
//      DoglegOptimizerImpl.cpp:26-91).  The Bayes tree stays on the device ([R S d] of every front); the three vectors of the
//      dogleg construction (steepest-descent point, Newton point, dogleg point) are blended on the host.
// sum over the cliques of ||[R S] x - alpha d||^2
int bt_forward(lmgpu_handle* h, const double* x, double alpha, double* out) {
  hipStream_t s = h->stream;
  int len = h->n_lds_fronts;
  for (const LevelWork& L : h->levels)
    for (int fi : L.hbm) len += h->h_fronts[fi].nf;
  if (len > h->bt_ebuf_len) {
    if (h->bt_ebuf) (void)hipFree(h->bt_ebuf);
    HIPCHECK(hipMalloc((void**)&h->bt_ebuf, (size_t)len * sizeof(double)));
    h->bt_ebuf_len = len;
  }
  if (h->n_lds_fronts > 0)
    hipLaunchKernelGGL(bt_lds_forward_kernel, dim3((h->n_lds_fronts + 3) / 4), dim3(256), 0, s, (const int32_t*)h->d_lists, h->n_lds_fronts,
                       (const FrontDesc*)h->d_fronts, (const int32_t*)h->d_fxoff, (const int32_t*)h->d_sxoff, (const double*)h->pool, x, alpha,
                       h->bt_ebuf);
  int o = h->n_lds_fronts;
  for (const LevelWork& L : h->levels)
    for (int fi : L.hbm) {
      const FrontDesc& F = h->h_fronts[fi];
      hipLaunchKernelGGL(bt_hbm_forward_kernel, dim3(F.nf), dim3(64), 0, s, F, h->f_off[fi], h->f_ld[fi], (const int32_t*)h->d_fxoff,
                         (const int32_t*)h->d_sxoff, (const double*)h->pool, x, alpha, h->bt_ebuf + o);
      o += F.nf;
    }
  reduce_to(h, h->bt_ebuf, len, h->dscal + 5);
  HIPCHECK(hipMemcpyAsync(h->h_scal + 5, h->dscal + 5, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *out = h->h_scal[5];
  return LMGPU_OK;
}

// the slots of the gradient's terms and, per scalar, the list of slots that belong to it (front order: LDS-class fronts in the order of
// d_lists, then the HBM fronts level by level, chunk by chunk): built once per structure, on the first Dogleg iteration
int bt_build_gather(lmgpu_handle* h) {
  if (h->bt_gather_built) return LMGPU_OK;
  const Plan& P = h->plan;
  std::vector<int32_t> lists((size_t)h->n_lds_fronts);
  HIPCHECK(hipMemcpy(lists.data(), h->d_lists, lists.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int64_t> lds_off(lists.size());
  std::vector<std::vector<int32_t>> slots((size_t)h->ntot);
  int64_t off = 0;
  auto scalar_of = [&](const Front& fr, int j) {  // column j of the front -> index in delta
    size_t k = 0;
    while (k + 1 < fr.vars.size() && fr.col_off[k + 1] <= j) k++;
    return P.xoff[fr.vars[k]] + (j - fr.col_off[k]);
  };
  for (size_t li = 0; li < lists.size(); li++) {
    const Front& fr = P.fronts[lists[li]];
    lds_off[li] = off;
    for (int j = 0; j < fr.n - 1; j++) slots[(size_t)scalar_of(fr, j)].push_back((int32_t)(off + j));
    off += fr.n - 1;
  }
  h->bt_hbm_part_off.assign(P.fronts.size(), -1);
  for (const LevelWork& L : h->levels)
    for (int fi : L.hbm) {
      const Front& fr = P.fronts[fi];
      h->bt_hbm_part_off[fi] = off;
      const int nchunk = (fr.nf + 63) / 64;
      for (int c = 0; c < nchunk; c++)
        for (int j = 64 * c; j < fr.n - 1; j++) slots[(size_t)scalar_of(fr, j)].push_back((int32_t)(off + (int64_t)c * (fr.n - 1) + j));
      off += (int64_t)nchunk * (fr.n - 1);
    }
  if (off >= (int64_t)1 << 31) {
    h->err = "Dogleg: the gradient's slot table exceeds 2^31 entries";
    return LMGPU_INVALID;
  }
  std::vector<int32_t> ptr((size_t)h->ntot + 1, 0), idx;
  for (int x = 0; x < h->ntot; x++) {
    ptr[(size_t)x] = (int32_t)idx.size();
    idx.insert(idx.end(), slots[(size_t)x].begin(), slots[(size_t)x].end());
  }
  ptr[(size_t)h->ntot] = (int32_t)idx.size();
  HIPCHECK(hipMalloc((void**)&h->bt_part, std::max<int64_t>(1, off) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->d_bt_part_off, std::max<size_t>(1, lds_off.size()) * sizeof(int64_t)));
  HIPCHECK(hipMalloc((void**)&h->d_bt_ptr, ptr.size() * sizeof(int32_t)));
  HIPCHECK(hipMalloc((void**)&h->d_bt_idx, std::max<size_t>(1, idx.size()) * sizeof(int32_t)));
  if (!lds_off.empty()) HIPCHECK(hipMemcpy(h->d_bt_part_off, lds_off.data(), lds_off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h->d_bt_ptr, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (!idx.empty()) HIPCHECK(hipMemcpy(h->d_bt_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  h->bt_gather_built = true;
  return LMGPU_OK;
}

// g = - sum over the cliques of [R S]^T d   (into h->bt_vec), every entry a sum in a fixed order
int bt_gradient(lmgpu_handle* h) {
  hipStream_t s = h->stream;
  const int rcb = bt_build_gather(h);
  if (rcb) return rcb;
  if (h->n_lds_fronts > 0)
    hipLaunchKernelGGL(bt_lds_transpose_kernel, dim3((h->n_lds_fronts + 3) / 4), dim3(256), 0, s, (const int32_t*)h->d_lists, h->n_lds_fronts,
                       (const FrontDesc*)h->d_fronts, (const int32_t*)h->d_fxoff, (const int32_t*)h->d_sxoff, (const double*)h->pool,
                       (const int64_t*)h->d_bt_part_off, h->bt_part);
  for (const LevelWork& L : h->levels)
    for (int fi : L.hbm) {
      const FrontDesc& F = h->h_fronts[fi];
      hipLaunchKernelGGL(bt_hbm_transpose_kernel, dim3((F.n - 1 + 255) / 256, (F.nf + 63) / 64), dim3(256), 0, s, F, h->f_off[fi], h->f_ld[fi],
                         (const double*)h->pool, h->bt_part + h->bt_hbm_part_off[fi]);
    }
  hipLaunchKernelGGL(bt_gather_kernel, dim3((h->ntot + 255) / 256), dim3(256), 0, s, (const int32_t*)h->d_bt_ptr, (const int32_t*)h->d_bt_idx,
                     (const double*)h->bt_part, h->ntot, h->bt_vec);
  HIPCHECK(hipGetLastError());
  return LMGPU_OK;
}

int dl_iterate(lmgpu_handle* h) {
  if (h->cfg.world_size > 1) {
    h->err = "Dogleg is single-rank in this round";
    return LMGPU_INVALID;
  }
  if (h->solver == LMGPU_SOLVER_PCG) {  // DoglegOptimizer.cpp:108-113 throws for iterative linear solvers
    h->err = "Dogleg is not compatible with the conjugate gradient solver (it needs the Bayes tree of the direct solver)";
    return LMGPU_INVALID;
  }
  hipStream_t s = h->stream;
  std::memset(&h->tim, 0, sizeof(h->tim));
  if (!h->bt_vec) HIPCHECK(hipMalloc((void**)&h->bt_vec, std::max(1, h->ntot) * sizeof(double)));
  int rc = do_linearize(h);
  if (rc) return rc;
  rc = fill_dampw(h, 0, 0.0, 0.0);
  if (rc) return rc;
  rc = do_solve(h, 0.0);  // undamped Bayes tree; h->delta = Newton point dx_n
  if (rc) return rc;
  const int n = h->ntot;
  std::vector<double> dx_n(n), dx_u(n), dx_d(n);
  HIPCHECK(hipMemcpyAsync(dx_n.data(), h->delta, n * sizeof(double), hipMemcpyDeviceToHost, s));
  rc = bt_gradient(h);
  if (rc) return rc;
  HIPCHECK(hipMemcpyAsync(dx_u.data(), h->bt_vec, n * sizeof(double), hipMemcpyDeviceToHost, s));
  double RgSq = 0, M_error = 0;
  rc = bt_forward(h, h->bt_vec, 0.0, &RgSq);  // synchronises: dx_n / gradient are on the host now
  if (rc) return rc;
  double gg = 0;
  for (int i = 0; i < n; i++) gg += dx_u[i] * dx_u[i];
  const double step = -gg / RgSq;  // GaussianFactorGraph::optimizeGradientSearch, GaussianFactorGraph.cpp:381-406
  for (int i = 0; i < n; i++) dx_u[i] *= step;
  HIPCHECK(hipMemsetAsync(h->bt_vec, 0, n * sizeof(double), s));
  rc = bt_forward(h, h->bt_vec, 1.0, &M_error);
  if (rc) return rc;
  M_error *= 0.5;
  double uu = 0, nn = 0, un = 0;
  for (int i = 0; i < n; i++) {
    uu += dx_u[i] * dx_u[i];
    nn += dx_n[i] * dx_n[i];
    un += dx_u[i] * dx_n[i];
  }
  double delta = h->lm.lambda;  // trust radius
  const double f_error = h->lm.error;
  double new_f = f_error;
  bool stay = true, moved = true;
  while (stay) {
    // ComputeDoglegPoint / ComputeBlend (dogleg_step.hpp)
    const DoglegTrial trial = dogleg_trial_point(delta, uu, nn, un);
    if (trial.branch == DOGLEG_STEEPEST) {
      const double f = trial.scalar;
      for (int i = 0; i < n; i++) dx_d[i] = f * dx_u[i];
    } else if (trial.branch == DOGLEG_BLEND) {
      const double tau = trial.scalar;
      for (int i = 0; i < n; i++) dx_d[i] = (1. - tau) * dx_u[i] + tau * dx_n[i];
    } else {
      dx_d = dx_n;
    }
    HIPCHECK(hipMemcpyAsync(h->delta, dx_d.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    rc = enqueue_retract_and_error(h);  // values[cur ^ 1] = retract(values[cur], dx_d), f(x_d) -> h_scal[0]
    if (rc) return rc;
    double new_M = 0;
    rc = bt_forward(h, h->delta, 1.0, &new_M);  // synchronises
    if (rc) return rc;
    h->kt.resolve();
    new_M *= 0.5;
    new_f = h->h_scal[0];
    h->tim.inner_iterations += 1;
    const double rho = (std::abs(f_error - new_f) < 1e-15 || std::abs(M_error - new_M) < 1e-15) ? 0.5 : (f_error - new_f) / (M_error - new_M);
    double nd = 0;
    if (rho >= 0.75)
      for (int i = 0; i < n; i++) nd += dx_d[i] * dx_d[i];
    const DoglegRadius upd = dogleg_radius_update(rho, delta, std::sqrt(nd));  // (a NaN rho: f increased)
    delta = upd.delta;
    stay = upd.stay;
    moved = upd.moved;
    if (!moved) new_f = f_error;  // dx_d = 0: keep the values, keep the error
  }
  if (moved) {
    h->cur ^= 1;
  } else {
    HIPCHECK(hipMemsetAsync(h->delta, 0, n * sizeof(double), s));
  }
  h->linearized = false;
  h->lm.error = new_f;
  h->lm.lambda = delta;
  h->lm.iterations += 1;
  h->lm.totalNumberInnerIterations += h->tim.inner_iterations;
  HIPCHECK(hipStreamSynchronize(s));
  return LMGPU_OK;
}

// checkConvergence gtsam/nonlinear/NonlinearOptimizer.cpp:182-231
bool check_convergence(double relTol, double absTol, double errTol, double currentError, double newError) {
  if (newError <= errTol) return true;
  const double absoluteDecrease = currentError - newError;
  const double relativeDecrease = absoluteDecrease / currentError;
  return (relTol && (relativeDecrease <= relTol)) || (absoluteDecrease <= absTol);
}

// Deal the subtrees below the replicated top fronts to the ranks.  A front is replicated iff it is an HBM front
// whose ancestors are all replicated (for BAL: the camera root); with no such front every rank does everything.
// Which fronts are REPLICATED (eliminated by every rank from the all-reduced sum of the ranks' partial assemblies) and which rank
// OWNS each of the others.  A subtree goes to one rank as a whole -- its fronts of either class: with a nested-dissection ordering
// (Ordering::Metis, gtsam/inference/Ordering.cpp:211-256) of a graph whose camera blocks are sparse these are the camera
// subtrees below the top separators, dense HBM fronts included -- unless it is too heavy for one rank (more than 1 / world_size
// of the whole elimination: nf n^2 per front as the measure); then its root front is replicated and its children are looked at
// in turn.  The synthetic C4 graph (every camera pair co-visible) has ONE dense root that is all of the work above the point
// leaves: it is replicated and the leaves are dealt out, as in rounds 1-2.
void assign_owners(lmgpu_handle* h) {
  const Plan& P = h->plan;
  const int NF = (int)P.fronts.size(), W = std::max(1, h->cfg.world_size), R = h->cfg.rank;
  h->front_owner.assign(NF, -1);
  h->front_active.assign(NF, 1);
  if (W == 1) return;
  // cost of the subtree below (and including) every front (post-order: children come first)
  std::vector<double> wsub(NF, 0.0);
  double total = 0;
  for (int fi = 0; fi < NF; fi++) {
    const Front& fr = P.fronts[fi];
    wsub[fi] += (double)fr.nf * fr.n * fr.n + 40.0 * (double)fr.factors.size() + 100.0;
    if (fr.parent >= 0) wsub[fr.parent] += wsub[fi]; else total += wsub[fi];
  }
  std::vector<char> rep(NF, 0);
  bool any = false;
  for (int fi = NF - 1; fi >= 0; fi--) {  // parents before children
    const Front& fr = P.fronts[fi];
    rep[fi] = (fr.cls == 1) && (fr.parent < 0 || rep[fr.parent]) && wsub[fi] * W > total;
    any = any || rep[fi];
  }
  if (!any) return;  // nothing to shard: replicate the whole (small) tree
  // the subtrees to deal out: roots = fronts that are not replicated under a replicated parent (or tree roots)
  std::vector<int> tops;
  double top_total = 0, top_max = 0;
  for (int fi = NF - 1; fi >= 0; fi--) {
    const Front& fr = P.fronts[fi];
    if (!rep[fi] && (fr.parent < 0 || rep[fr.parent])) {
      tops.push_back(fi);
      top_total += wsub[fi];
      top_max = std::max(top_max, wsub[fi]);
    }
  }
  std::vector<int> top_owner(NF, -1);
  if (top_max * 4.0 * W > top_total) {
    // a few heavy subtrees: largest first to the rank with the least work so far (ties: the lower rank; stable order of equal weights)
    std::vector<int> order(tops);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return wsub[a] > wsub[b]; });
    std::vector<double> load(W, 0.0);
    for (int fi : order) {
      int best = 0;
      for (int r = 1; r < W; r++)
        if (load[r] < load[best]) best = r;
      top_owner[fi] = best;
      load[best] += wsub[fi];
    }
  } else {
    // many light subtrees (BAL's point leaves): contiguous chunks of about equal cost, in front order
    double cum = 0;
    for (int fi : tops) {
      top_owner[fi] = std::min(W - 1, (int)(cum / top_total * W));
      cum += wsub[fi];
    }
  }
  for (int fi = NF - 1; fi >= 0; fi--) {
    const Front& fr = P.fronts[fi];
    if (rep[fi]) continue;
    h->front_owner[fi] = (fr.parent < 0 || rep[fr.parent]) ? top_owner[fi] : h->front_owner[fr.parent];
  }
  for (int fi = 0; fi < NF; fi++) h->front_active[fi] = rep[fi] || h->front_owner[fi] == R;
}

}  // namespace

// =============================================================================================== C ABI
#include "launch_tables.hpp"  // the host build of the launch tables (finalize_structure_impl)

extern "C" {

int lmgpu_create(const lmgpu_config* cfg, lmgpu_handle** out) {
  if (!cfg || !out) return LMGPU_INVALID;
  lmgpu_handle* h = new lmgpu_handle();
  h->cfg = *cfg;
  if (h->cfg.world_size < 1) h->cfg.world_size = 1;
  h->device = cfg->device;
  h->sw = read_dev_switches();
  *out = h;
  if (h->device >= 0) {
    HIPCHECK(hipSetDevice(h->device));
    {
      hipDeviceProp_t prop;
      HIPCHECK(hipGetDeviceProperties(&prop, h->device));
      h->num_cus = prop.multiProcessorCount;
    }
    HIPCHECK(hipStreamCreate(&h->stream));
    // the chunk all-reduces gate the panels of the factorisation that runs beside them: highest dispatch priority
    {
      int prio_lo = 0, prio_hi = 0;
      HIPCHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
      HIPCHECK(hipStreamCreateWithPriority(&h->comm_stream, hipStreamNonBlocking, prio_hi));
    }
    HIPCHECK(hipEventCreateWithFlags(&h->asm_ev, hipEventDisableTiming));
    for (int i = 0; i < 8; i++) HIPCHECK(hipEventCreate(&h->ev[i]));
    HIPCHECK(hipHostMalloc((void**)&h->h_scal, 8 * sizeof(double), hipHostMallocDefault));
    HIPCHECK(hipHostMalloc((void**)&h->h_status, 2 * sizeof(int), hipHostMallocDefault));
    HIPCHECK(hipMalloc((void**)&h->d_lambda, sizeof(double)));
    HIPCHECK(hipMemset(h->d_lambda, 0, sizeof(double)));
    HIPCHECK(front_kernels_set_attributes());
    HIPCHECK(chain_resident_blocks(h->num_cus, &h->chain_resident));
  }
  return LMGPU_OK;
}

int lmgpu_destroy(lmgpu_handle* h) {
  if (!h) return LMGPU_INVALID;
  if (h->device >= 0) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->comm_data) ncclCommDestroy(h->comm_data);
    if (h->comm) ncclCommDestroy(h->comm);
    auto fr = [](void* p) {
      if (p) (void)hipFree(p);
    };
    fr(h->pool);
    for (int w = 0; w < 2; w++)
      for (int t = 0; t < kNumVarTypes; t++) fr(h->vals[w][t]);
    for (int t = 0; t < kNumVarTypes; t++) fr(h->type_xoff[t]);
    for (int t = 0; t < kNumVarTypes; t++) fr(h->saved[t]);
    fr(h->gex); fr(h->delta); fr(h->dampw); fr(h->hdiag); fr(h->ebuf0); fr(h->ebuf1); fr(h->partial); fr(h->dscal); fr(h->ywork); fr(h->d_status);
    fr(h->d_fd); fr(h->d_fronts); fr(h->d_ffac); fr(h->d_childs); fr(h->d_cmap); fr(h->d_fxoff); fr(h->d_sxoff); fr(h->d_lists); fr(h->d_hbm_small); fr(h->d_med_list); fr(h->d_med_fronts); fr(h->inv16_med); fr(h->bt_ebuf); fr(h->bt_vec); fr(h->bt_part); fr(h->d_bt_part_off); fr(h->d_bt_ptr); fr(h->d_bt_idx); fr(h->d_f_ld); fr(h->d_f_off);
    fr(h->d_scalar_var); fr(h->d_scalar_col); fr(h->d_vi_ptr); fr(h->d_vi_fac); fr(h->d_vi_pos);
    fr(h->pcg_xoff); fr(h->pcg_loff); fr(h->pcg_yoff); fr(h->pcg_H); fr(h->pcg_L); fr(h->pcg_rhs); fr(h->pcg_r); fr(h->pcg_p); fr(h->pcg_q);
    fr(h->pcg_y); fr(h->pcg_part); fr(h->pcg_gam); fr(h->pcg_done); fr(h->pcg_ctl);
    if (h->h_pcg_ctl) (void)hipHostFree(h->h_pcg_ctl);
    if (h->h_pcg_done) (void)hipHostFree(h->h_pcg_done);
    for (int i = 0; i < 3; i++)
      if (h->pcg_ev[i]) (void)hipEventDestroy(h->pcg_ev[i]);
    ncg_release(h);
    fr(h->gnc_w); fr(h->gnc_b); fr(h->gnc_part); fr(h->gnc_scal); fr(h->gnc_fixed);
    if (h->h_gnc_scal) (void)hipHostFree(h->h_gnc_scal);
    for (int i = 0; i < 2; i++)
      if (h->gnc_ev[i]) (void)hipEventDestroy(h->gnc_ev[i]);
    for (Bucket& b : h->buckets) {
      fr(b.d_vidx); fr(b.d_meas); fr(b.d_noise); fr(b.d_epos);
    }
    if (h->h_scal) (void)hipHostFree(h->h_scal);
    if (h->h_status) (void)hipHostFree(h->h_status);
    for (int i = 0; i < 8; i++)
      if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    for (hipEvent_t e : h->kt.pool) (void)hipEventDestroy(e);
    fr(h->bs_inv); fr(h->bs_x); fr(h->bs_flags); fr(h->inv16); fr(h->d_pflags); fr(h->d_bs_parent); fr(h->d_bs_pos); fr(h->d_bs_done); fr(h->d_fill_upper); fr(h->d_level_tasks); fr(h->d_level_sync); fr(h->d_bsd_table); fr(h->d_bsd_run_table); fr(h->d_fill_elim); fr(h->d_fill_backsub); fr(h->d_zero_ranges); fr(h->d_bsd_x); fr(h->d_bsd_ticket); fr(h->d_leafpack); fr(h->d_gzero);
    fr(h->d_chain_tasks);
    fr(h->d_marg_parent); fr(h->d_marg_poff); fr(h->d_marg_spos);
    fr(h->d_gpblk); fr(h->d_gpent); fr(h->d_gvblk); fr(h->d_gvent); fr(h->d_gcorner); fr(h->d_row_begin); fr(h->d_rowptr); fr(h->d_rowsrc);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    for (int g = 0; g < 2; g++)
      if (h->solve_graph[g]) (void)hipGraphExecDestroy(h->solve_graph[g]);
    if (h->d_lambda) (void)hipFree(h->d_lambda);
    if (h->asm_ev) (void)hipEventDestroy(h->asm_ev);
    for (hipEvent_t e : h->chunk_ev) (void)hipEventDestroy(e);
  }
  tri_release(h);  // also on a structure-only handle: its index is host memory
  marg_release(h);
  smart_release(h);
  delete h;
  return LMGPU_OK;
}

const char* lmgpu_last_error(const lmgpu_handle* h) { return !h ? "null handle" : (h->finalize_err.empty() ? h->err : h->finalize_err).c_str(); }
int lmgpu_last_failed_slot(const lmgpu_handle* h) { return h ? h->failed_slot : -1; }

int lmgpu_set_variables(lmgpu_handle* h, int32_t n_vars, const uint64_t* keys, const int32_t* types) {
  if (!h) return LMGPU_INVALID;
  if (n_vars <= 0 || !keys || !types || h->finalized) {
    h->err = "lmgpu_set_variables: refused (n_vars <= 0 || !keys || !types || h->finalized)";
    return LMGPU_INVALID;
  }
  h->plan.n_vars = n_vars;
  h->plan.keys.assign(keys, keys + n_vars);
  h->plan.types.assign(types, types + n_vars);
  for (int i = 0; i < n_vars; i++)
    if (types[i] < 0 || types[i] >= LMGPU_NUM_VAR_TYPES) {
      h->err = "bad variable type";
      return LMGPU_INVALID;
    }
  return LMGPU_OK;
}

int lmgpu_add_factor_bucket(lmgpu_handle* h, int32_t type, int32_t n, const int32_t* graph_index, const int32_t* var_slots, const double* meas,
                            int32_t noise_kind, const double* noise) {
  return lmgpu_add_factor_bucket_robust(h, type, n, graph_index, var_slots, meas, noise_kind, noise, LMGPU_ROBUST_NONE, 0.0);
}

static int add_bucket_of_row(lmgpu_handle* h, int32_t type, int32_t n, const int32_t* graph_index, const int32_t* var_slots, const double* meas,
                             int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k);

int lmgpu_add_factor_bucket_robust(lmgpu_handle* h, int32_t type, int32_t n, const int32_t* graph_index, const int32_t* var_slots,
                                   const double* meas, int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k) {
  if (!h) return LMGPU_INVALID;
  if (h->finalized || type < 0 || type >= LMGPU_NUM_FACTOR_TYPES || n < 0 || h->plan.n_vars == 0) {
    h->err = "lmgpu_add_factor_bucket_robust: refused (h->finalized || type < 0 || type >= LMGPU_NUM_FACTOR_TYPES || n < 0 || h->plan.n_vars == 0)";
    return LMGPU_INVALID;
  }
  return add_bucket_of_row(h, type, n, graph_index, var_slots, meas, noise_kind, noise, robust_kind, robust_k);
}

// A bucket of one of the INTERNAL generic rows of the factor-type table (factor_types.hpp: kTranslationType, kBetweenPoint3Type), for the
// sessions inside the library that own their handle (translation_recovery.hpp).  Not exported: the boundary above keeps refusing them.
static int add_internal_factor_bucket(lmgpu_handle* h, int32_t type, int32_t n, const int32_t* graph_index, const int32_t* var_slots,
                                      const double* meas, int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k) {
  if (!h) return LMGPU_INVALID;
  if (h->finalized || (type != kTranslationType && type != kBetweenPoint3Type) || n < 0 || h->plan.n_vars == 0) {
    h->err = "add_internal_factor_bucket: refused (h->finalized || not an internal generic type || n < 0 || h->plan.n_vars == 0)";
    return LMGPU_INVALID;
  }
  return add_bucket_of_row(h, type, n, graph_index, var_slots, meas, noise_kind, noise, robust_kind, robust_k);
}

// the body shared by the two: `type` is a row of kFactorTypes its caller has admitted
static int add_bucket_of_row(lmgpu_handle* h, int32_t type, int32_t n, const int32_t* graph_index, const int32_t* var_slots, const double* meas,
                             int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k) {
  if (robust_kind < LMGPU_ROBUST_NONE || robust_kind > LMGPU_ROBUST_L2_WITH_DEAD_ZONE || (robust_kind != LMGPU_ROBUST_NONE && !(robust_k > 0.0)))
    return LMGPU_INVALID;
  if (noise_kind != LMGPU_N_UNIT && noise_kind != LMGPU_N_DIAG && noise_kind != LMGPU_N_GAUSS) return LMGPU_INVALID;
  if (n == 0) return LMGPU_OK;
  if (!graph_index || !var_slots || !meas || (noise_kind != LMGPU_N_UNIT && !noise)) return LMGPU_INVALID;
  const BucketShape sh = bucket_shape(type, noise_kind);
  const int ar = sh.ar;
  for (int i = 0; i < n; i++)
    for (int k = 0; k < ar; k++) {
      const int s = var_slots[i * ar + k];
      if (s < 0 || s >= h->plan.n_vars) {
        h->err = "factor references unknown slot";
        return LMGPU_INVALID;
      }
      if (h->plan.types[s] != var_type(type, k)) {
        h->err = "factor/variable type mismatch";
        return LMGPU_INVALID;
      }
    }
  Bucket b;
  b.type = type;
  b.n = n;
  b.noise_kind = noise_kind;
  b.robust = robust_kind;
  b.robust_k = robust_k;
  b.graph_index.assign(graph_index, graph_index + n);
  b.slots.assign(var_slots, var_slots + (size_t)n * ar);
  b.meas.assign(meas, meas + (size_t)n * sh.ml);
  if (sh.nl) b.noise.assign(noise, noise + (size_t)n * sh.nl);
  b.rows = sh.rows;
  b.cols = sh.cols;
  const int bi = (int)h->buckets.size();
  for (int i = 0; i < n; i++) {
    FactorRef f;
    f.bucket = bi;
    f.idx = i;
    for (int k = 0; k < kMaxArity; k++) f.slots[k] = k < ar ? var_slots[i * ar + k] : -1;
    f.graph_index = graph_index[i];
    h->plan.factors.push_back(f);
  }
  h->buckets.push_back(std::move(b));
  return LMGPU_OK;
}

// the device arrays every solver needs: per-bucket inputs, values, the variable -> factor incidence (hessianDiagonal, PCG), vectors
static int finalize_vectors(lmgpu_handle* h) {
  const Plan& P = h->plan;
  const int NFAC = (int)P.factors.size();
  int rc;
  // per-bucket arrays, compacted to this rank's factors
  {
    std::vector<std::vector<int32_t>> epos(h->buckets.size());
    for (size_t bi = 0; bi < h->buckets.size(); bi++) epos[bi].resize(h->buckets[bi].n_loc);
    for (int i = 0; i < NFAC; i++)
      if (h->fac_local[i] >= 0) epos[P.factors[i].bucket][h->buckets[P.factors[i].bucket].loc_of[P.factors[i].idx]] = h->fac_local[i];
    for (size_t bi = 0; bi < h->buckets.size(); bi++) {
      Bucket& b = h->buckets[bi];
      const BucketShape sh = bucket_shape(b.type, b.noise_kind);
      const int ar = sh.ar, ml = sh.ml, nl = sh.nl;
      std::vector<int32_t> vidx((size_t)b.n_loc * ar);
      std::vector<double> meas((size_t)b.n_loc * ml), noise((size_t)b.n_loc * nl);
      for (int i = 0; i < b.n; i++) {
        const int l = b.loc_of[i];
        if (l < 0) continue;
        for (int k = 0; k < ar; k++) vidx[(size_t)l * ar + k] = P.tidx[b.slots[(size_t)i * ar + k]];
        std::memcpy(&meas[(size_t)l * ml], &b.meas[(size_t)i * ml], ml * sizeof(double));
        if (nl) std::memcpy(&noise[(size_t)l * nl], &b.noise[(size_t)i * nl], nl * sizeof(double));
      }
      if ((rc = upload(h, &b.d_vidx, vidx))) return rc;
      if ((rc = upload(h, &b.d_meas, meas))) return rc;
      if (nl && (rc = upload(h, &b.d_noise, noise))) return rc;
      if ((rc = upload(h, &b.d_epos, epos[bi]))) return rc;
    }
  }
  // values, per type
  for (int t = 0; t < kNumVarTypes; t++) {
    const size_t bytes = std::max<size_t>(1, (size_t)P.type_count[t] * kVarStore[t]) * sizeof(double);
    HIPCHECK(hipMalloc((void**)&h->vals[0][t], bytes));
    HIPCHECK(hipMalloc((void**)&h->vals[1][t], bytes));
    std::vector<int32_t> xo(P.type_count[t]);
    for (int s = 0; s < P.n_vars; s++)
      if (P.types[s] == t) xo[P.tidx[s]] = P.xoff[s];
    if ((rc = upload(h, &h->type_xoff[t], xo))) return rc;
  }
  // hessian-diagonal CSR over the factors COUNTED on this rank (summed over ranks by all-reduce)
  {
    std::vector<int32_t> scalar_var(h->ntot), scalar_col(h->ntot), vi_ptr(P.n_vars + 1, 0), vi_fac;
    std::vector<int8_t> vi_pos;
    for (int s = 0; s < P.n_vars; s++)
      for (int d = 0; d < P.dims[s]; d++) {
        scalar_var[P.xoff[s] + d] = s;
        scalar_col[P.xoff[s] + d] = d;
      }
    std::vector<std::vector<std::pair<int32_t, int8_t>>> vi(P.n_vars);
    for (int i = 0; i < NFAC; i++) {
      const int l = h->fac_local[i];
      if (l < 0 || l >= h->n_counted) continue;
      for (int k = 0; k < kMaxArity; k++)
        if (P.factors[i].slots[k] >= 0) vi[P.factors[i].slots[k]].push_back({l, (int8_t)k});
    }
    for (int s = 0; s < P.n_vars; s++) {
      vi_ptr[s] = (int32_t)vi_fac.size();
      for (auto& pr : vi[s]) {
        vi_fac.push_back(pr.first);
        vi_pos.push_back(pr.second);
      }
    }
    vi_ptr[P.n_vars] = (int32_t)vi_fac.size();
    if ((rc = upload(h, &h->d_scalar_var, scalar_var))) return rc;
    if ((rc = upload(h, &h->d_scalar_col, scalar_col))) return rc;
    if ((rc = upload(h, &h->d_vi_ptr, vi_ptr))) return rc;
    if ((rc = upload(h, &h->d_vi_fac, vi_fac))) return rc;
    if ((rc = upload(h, &h->d_vi_pos, vi_pos))) return rc;
  }
  HIPCHECK(hipMalloc((void**)&h->delta, h->ntot * sizeof(double)));
  HIPCHECK(hipMemset(h->delta, 0, h->ntot * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->dampw, h->ntot * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->hdiag, h->ntot * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->ebuf0, std::max(1, h->nfac) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->ebuf1, std::max(1, h->nfac) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->partial, 256 * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->dscal, 8 * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->ywork, std::max(1, P.max_front_n) * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->d_status, 2 * sizeof(int)));
  return LMGPU_OK;
}

// Every hipMalloc, upload and hipMemset of finalize: the pool, the launch tables in a fixed order, the vectors every solver needs, then the
// scratch buffers.  A failure leaves the handle un-finalized (lmgpu_finalize_structure); lmgpu_destroy frees what was allocated.
static int upload_launch_tables(lmgpu_handle* h, const LaunchTables& T) {
  const Plan& P = h->plan;
  int rc;
  HIPCHECK(hipSetDevice(h->device));
  HIPCHECK(hipMalloc((void**)&h->pool, h->pool_doubles * sizeof(double)));
  // once: entries the kernels read but never write (lower triangles inside diagonal tiles, padding columns) must be finite
  HIPCHECK(hipMemset(h->pool, 0, h->pool_doubles * sizeof(double)));
  if (h->pcg_structure) {  // Jacobians, factor descriptors, incidence list and vectors only
    if ((rc = upload(h, &h->d_fd, T.fd))) return rc;
    return finalize_vectors(h);
  }
  if (!T.packs.empty()) {  // (no records: d_leafpack stays null and the launches take the general descriptor path)
    HIPCHECK(hipMalloc((void**)&h->d_leafpack, T.packs.size()));
    HIPCHECK(hipMemcpy(h->d_leafpack, T.packs.data(), T.packs.size(), hipMemcpyHostToDevice));
  }
#define UPLOAD(dst, src) \
  if ((rc = upload(h, &h->dst, src))) return rc
  UPLOAD(d_fd, T.fd); UPLOAD(d_fronts, h->h_fronts); UPLOAD(d_ffac, T.ffac); UPLOAD(d_childs, T.childs);
  UPLOAD(d_cmap, T.cmap); UPLOAD(d_fxoff, T.fxoff); UPLOAD(d_sxoff, T.sxoff); UPLOAD(d_lists, T.lists);
  UPLOAD(d_bs_parent, T.bs_parent); UPLOAD(d_bs_pos, T.bs_pos);
  if (h->merge_elim) UPLOAD(d_fill_upper, T.fill_upper);
  UPLOAD(d_hbm_small, T.small); UPLOAD(d_bsd_table, T.bsd);
  if (!T.bsd_runs_table.empty()) UPLOAD(d_bsd_run_table, T.bsd_runs_table);
  UPLOAD(d_med_list, T.med); UPLOAD(d_f_off, h->f_off); UPLOAD(d_f_ld, h->f_ld); UPLOAD(d_row_begin, h->row_begin);
  UPLOAD(d_med_fronts, T.med_fronts);
  if (!T.level_tasks.empty()) UPLOAD(d_level_tasks, T.level_tasks);
  UPLOAD(d_rowptr, T.rowptr); UPLOAD(d_rowsrc, T.rowsrc); UPLOAD(d_gpblk, T.gpblk); UPLOAD(d_gzero, T.gzero);
  UPLOAD(d_gpent, T.gpent); UPLOAD(d_gvblk, T.gvblk); UPLOAD(d_gvent, T.gvent);
  UPLOAD(d_marg_parent, T.marg_parent); UPLOAD(d_marg_poff, h->marg_poff); UPLOAD(d_marg_spos, h->marg_spos);
#undef UPLOAD
  if ((rc = finalize_vectors(h))) return rc;
  // ---- scratch
  const size_t NF = P.fronts.size(), wide_blocks = (size_t)(T.max_nf + BSW_NB - 1) / BSW_NB;
  // (inverses of the 64 x 64 diagonal blocks in the fallback; the wide form parks M_B there, 128 x 128 per 128-row block)
  HIPCHECK(hipMalloc((void**)&h->bs_inv, wide_blocks * BSW_NB * BSW_NB * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->inv16, (size_t)((P.max_front_n + NBO - 1) / NBO + 2) * 16 * 256 * sizeof(double)));  // 16 blocks per outer panel
  h->pflags_panels = (P.max_front_n + NBO - 1) / NBO + 1;
  HIPCHECK(hipMalloc((void**)&h->d_pflags, (size_t)h->pflags_panels * PDF_FLAG_WORDS * sizeof(unsigned int)));
  // (x of the dataflow back-substitutions: whole 128-row blocks for the wide form, which covers the 64-row blocks of the others)
  HIPCHECK(hipMalloc((void**)&h->bs_x, wide_blocks * BSW_NB * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->bs_flags, (size_t)((T.max_nf + NB - 1) / NB + 1) * sizeof(unsigned int)));
  HIPCHECK(hipMalloc((void**)&h->d_bs_done, (NF + h->levels.size() + 1) * sizeof(unsigned int)));
  if (h->bsd_x_count > 0) {
    HIPCHECK(hipMalloc((void**)&h->d_bsd_x, h->bsd_x_count * sizeof(double)));
    HIPCHECK(hipMalloc((void**)&h->d_bsd_ticket, h->levels.size() * sizeof(unsigned int)));
  }
  if (T.max_med > 0) HIPCHECK(hipMalloc((void**)&h->inv16_med, (size_t)T.max_med * 16 * 256 * sizeof(double)));
  if (!T.level_tasks.empty()) HIPCHECK(hipMalloc((void**)&h->d_level_sync, std::max<size_t>(1, T.med_fronts.size()) * sizeof(LevelSync)));
  HIPCHECK(hipMalloc((void**)&h->d_gcorner, std::max<size_t>(1, (size_t)T.n_gleaf) * sizeof(double)));
  h->tabs = FrontTablesDev{h->d_fronts, h->d_ffac, h->d_fd, h->d_childs, h->d_cmap, h->d_fxoff, h->d_sxoff, h->d_lists, h->d_rowptr, h->d_rowsrc};
  return LMGPU_OK;
}

// The symbolic plan, then the launch tables phase by phase (launch_tables.hpp: host only, on every handle), then -- on a device handle --
// the one upload.
static int finalize_structure_impl(lmgpu_handle* h) {
  h->pcg_structure = h->solver == LMGPU_SOLVER_PCG;  // PCG selected before finalize: no symbolic analysis, no fronts
  std::string e = h->plan.build(kLdsLimitN, !h->pcg_structure);
  if (!e.empty()) {
    h->err = e;
    return LMGPU_INVALID;
  }
  const Plan& P = h->plan;
  const int NFAC = (int)P.factors.size();
  h->ntot = P.xoff[P.n_vars];
  h->nstore = P.voff[P.n_vars];
  for (int i = 1; i < NFAC; i++)
    if (P.factors[i].graph_index == P.factors[i - 1].graph_index) {
      h->err = "duplicate graph_index";
      return LMGPU_INVALID;
    }
  h->graph_index_sorted.resize(NFAC);
  for (int i = 0; i < NFAC; i++) h->graph_index_sorted[i] = P.factors[i].graph_index;

  LaunchTables T;
  build_ownership(h);
  build_pool_layout(h, T);
  int rc = build_front_tables(h, T);
  if (rc) return rc;
  build_level_lists(h, T);
  build_leaf_group_bins(h, T);
  build_elim_segments(h);
  build_solve_flags(h, T);
  build_leaf_packs(h, T);
  build_backsub_tables(h, T);
  build_fused_levels(h, T);
  build_marginal_tables(h, T);
#ifdef LMGPU_TEST_HOOKS
  digest_tables(h, T);
#endif
  return h->device >= 0 ? upload_launch_tables(h, T) : LMGPU_OK;  // (a structure-only handle: symbolic analysis and tables, no compute)
}

int lmgpu_finalize_structure(lmgpu_handle* h) {
  if (!h) return LMGPU_INVALID;
  if (h->finalized || !h->finalize_err.empty()) {
    h->err = h->finalized ? "lmgpu_finalize_structure: refused (h->finalized)" : h->finalize_err;
    return LMGPU_INVALID;
  }
  // smart factors: the hidden points and the internal observation bucket enter the structure first, their device arrays come last
  int rc = h->smart ? smart_prepare(h) : LMGPU_OK;
  if (!rc) rc = finalize_structure_impl(h);
  if (!rc && h->smart && h->device >= 0) rc = smart_upload(h);
  // finalized only once the build and the upload have succeeded; a handle that failed either keeps its error and refuses everything
  // but lmgpu_destroy, which frees what was allocated
  if (rc) h->finalize_err = h->err;
  else h->finalized = true;
  return rc;
}

// (the hidden points of smart factors are no part of any packed vector at the boundary: they are the first 3 * n_hidden scalars inside)
int lmgpu_total_dim(const lmgpu_handle* h) { return (h && h->finalized) ? h->ntot - 3 * h->n_hidden : -1; }
int lmgpu_total_store(const lmgpu_handle* h) { return (h && h->finalized) ? h->nstore - 3 * h->n_hidden : -1; }

int lmgpu_set_values(lmgpu_handle* h, const double* packed) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !packed) {
    h->err = "lmgpu_set_values: refused (!h->finalized || !packed)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  const Plan& P = h->plan;
  for (int t = 0; t < kNumVarTypes; t++) {
    if (P.type_count[t] == 0) continue;
    std::vector<double> buf((size_t)P.type_count[t] * kVarStore[t]);
    for (int s = h->n_hidden; s < P.n_vars; s++)
      if (P.types[s] == t)
        std::memcpy(&buf[(size_t)P.tidx[s] * kVarStore[t]], packed + (P.voff[s] - 3 * h->n_hidden), kVarStore[t] * sizeof(double));
    HIPCHECK(hipMemcpy(h->vals[h->cur][t], buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  h->have_values = true;
  h->marg_valid = false;
  return LMGPU_OK;
}

int lmgpu_get_values(lmgpu_handle* h, double* packed) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !packed || !h->have_values) {
    h->err = "lmgpu_get_values: refused (!h->finalized || !packed || !h->have_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  const Plan& P = h->plan;
  HIPCHECK(hipStreamSynchronize(h->stream));
  for (int t = 0; t < kNumVarTypes; t++) {
    if (P.type_count[t] == 0) continue;
    std::vector<double> buf((size_t)P.type_count[t] * kVarStore[t]);
    HIPCHECK(hipMemcpy(buf.data(), h->vals[h->cur][t], buf.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = h->n_hidden; s < P.n_vars; s++)
      if (P.types[s] == t)
        std::memcpy(packed + (P.voff[s] - 3 * h->n_hidden), &buf[(size_t)P.tidx[s] * kVarStore[t]], kVarStore[t] * sizeof(double));
  }
  return LMGPU_OK;
}

// device-side snapshot of the current values (e.g. the initial estimate) and its restore: device-to-device copies
int lmgpu_save_values(lmgpu_handle* h) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->have_values) {
    h->err = "lmgpu_save_values: refused (!h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  for (int t = 0; t < kNumVarTypes; t++) {
    const size_t bytes = std::max<size_t>(1, (size_t)h->plan.type_count[t] * kVarStore[t]) * sizeof(double);
    if (!h->saved[t]) HIPCHECK(hipMalloc((void**)&h->saved[t], bytes));
    HIPCHECK(hipMemcpyAsync(h->saved[t], h->vals[h->cur][t], bytes, hipMemcpyDeviceToDevice, h->stream));
  }
  HIPCHECK(hipStreamSynchronize(h->stream));
  return LMGPU_OK;
}

int lmgpu_restore_values(lmgpu_handle* h) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->saved[0]) {
    h->err = "lmgpu_restore_values: refused (!h->finalized || !h->saved[0])";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  h->marg_valid = false;
  for (int t = 0; t < kNumVarTypes; t++) {
    if (h->plan.type_count[t] == 0) continue;  // (a type the graph does not have: its buffers are one unused double each, nothing to restore)
    const size_t bytes = (size_t)h->plan.type_count[t] * kVarStore[t] * sizeof(double);
    HIPCHECK(hipMemcpyAsync(h->vals[h->cur][t], h->saved[t], bytes, hipMemcpyDeviceToDevice, h->stream));
  }
  return LMGPU_OK;
}

int lmgpu_error(lmgpu_handle* h, double* total) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !total || !h->have_values) {
    h->err = "lmgpu_error: refused (!h->finalized || !total || !h->have_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  return compute_error(h, h->cur, total);
}

int lmgpu_linearize(lmgpu_handle* h) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->have_values) {
    h->err = "lmgpu_linearize: refused (!h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  rc = do_linearize(h);
  if (rc) return rc;
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->kt.resolve();
  return LMGPU_OK;
}

int lmgpu_solve(lmgpu_handle* h, double lambda, int32_t diagonal_damping, double min_diag, double max_diag, double* delta_packed,
                double* lin_err0, double* lin_err1) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->linearized) {
    h->err = "lmgpu_solve: no linearization to solve (call lmgpu_linearize after lmgpu_finalize_structure / lmgpu_set_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  if (diagonal_damping && smart_refused(h, "lmgpu_solve with diagonal damping")) return LMGPU_INVALID;
  rc = fill_dampw(h, diagonal_damping, min_diag, max_diag);
  if (rc) return rc;
  rc = do_solve(h, lambda);
  if (rc != LMGPU_OK && rc != LMGPU_INDETERMINATE) return rc;
  if (delta_packed)
    HIPCHECK(hipMemcpy(delta_packed, h->delta + 3 * h->n_hidden, (h->ntot - 3 * h->n_hidden) * sizeof(double), hipMemcpyDeviceToHost));
  if (lin_err0) *lin_err0 = h->h_scal[1];
  if (lin_err1) *lin_err1 = h->h_scal[2];
  return rc;
}

// b := 0 in every stored [A b]: the linear system keeps its matrix A^T A and loses its gradient
__global__ __launch_bounds__(256) void zero_rhs_kernel(const FacDesc* __restrict__ fd, int nfac, double* __restrict__ pool) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nfac) return;
  const FacDesc d = fd[f];
  double* b = pool + d.joff + (size_t)(d.d0 + d.d1) * d.rows;
  for (int r = 0; r < d.rows; r++) b[r] = 0.0;
}
__global__ void set_one_kernel(double* p) { *p = 1.0; }

int lmgpu_joint_marginal_covariance(lmgpu_handle* h, int32_t nslots, const int32_t* slots, double* cov) {
  if (!h) return LMGPU_INVALID;
  if (!cov || !slots || nslots < 1 || !h->finalized || !h->have_values) {
    h->err = "lmgpu_joint_marginal_covariance: refused (!cov || !slots || nslots < 1 || !h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "the marginal covariances")) return LMGPU_INVALID;
  for (int a = 0; a < nslots; a++) {
    if (slots[a] < 0 || slots[a] >= h->plan.n_vars) return LMGPU_INVALID;
    for (int b = 0; b < a; b++)
      if (slots[b] == slots[a]) return LMGPU_INVALID;
  }
  if (h->cfg.world_size > 1) {
    h->err = "marginal covariances are computed on one GPU";
    return LMGPU_INVALID;
  }
  if (h->pcg_structure) {
    h->err = "marginal covariances need the fronts of the direct solver; this handle was finalized under PCG";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  // Marginals::Marginals (gtsam/nonlinear/Marginals.cpp:28-43): linearize at the solution, eliminate into a Bayes tree
  // (here: the same two kernels as every LM step, lambda = 0);  marginalCovariance (:124-127) = inverse of the marginal
  // information (:109-121) = the variable's diagonal block of (A^T A)^-1;  jointMarginalCovariance (:130-137) = the blocks of
  // (A^T A)^-1 for several variables.  Column k of those blocks is the variables' part of the solution of  A^T A x = e_k,
  // i.e. one elimination + back-substitution with the gradient replaced by a unit vector.
  if ((rc = do_linearize(h))) return rc;
  hipStream_t s = h->stream;
  if (h->nfac > 0) hipLaunchKernelGGL(zero_rhs_kernel, dim3((h->nfac + 255) / 256), dim3(256), 0, s, (const FacDesc*)h->d_fd, h->nfac, h->pool);
  if (!h->gex) HIPCHECK(hipMalloc((void**)&h->gex, h->ntot * sizeof(double)));
  if ((rc = fill_dampw(h, 0, 0.0, 0.0))) return rc;
  std::vector<int> boff(nslots + 1, 0);  // block offsets inside the joint matrix, in the order of `slots`
  for (int a = 0; a < nslots; a++) boff[a + 1] = boff[a] + h->plan.dims[slots[a]];
  const int D = boff[nslots];
  std::vector<double> col(h->ntot);
  h->gex_active = h->gex;
  for (int a = 0; a < nslots && rc == LMGPU_OK; a++) {
    for (int k = 0; k < h->plan.dims[slots[a]] && rc == LMGPU_OK; k++) {
      HIPCHECK(hipMemsetAsync(h->gex, 0, h->ntot * sizeof(double), s));
      hipLaunchKernelGGL(set_one_kernel, dim3(1), dim3(1), 0, s, h->gex + h->plan.xoff[slots[a]] + k);
      rc = do_solve(h, 0.0);
      if (rc != LMGPU_OK) break;
      for (int b = 0; b < nslots; b++) {
        const int db = h->plan.dims[slots[b]];
        HIPCHECK(hipMemcpy(col.data(), h->delta + h->plan.xoff[slots[b]], db * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < db; i++) cov[(size_t)(boff[b] + i) * D + boff[a] + k] = col[i];
      }
    }
  }
  h->gex_active = nullptr;
  h->linearized = false;  // the stored right-hand sides are gone: the next solve linearizes again
  h->solved = false;
  if (rc != LMGPU_OK) return rc;  // LMGPU_INDETERMINATE like Marginals' IndeterminantLinearSystemException
  for (int i = 0; i < D; i++)
    for (int j = i + 1; j < D; j++) cov[(size_t)i * D + j] = cov[(size_t)j * D + i] = 0.5 * (cov[(size_t)i * D + j] + cov[(size_t)j * D + i]);
  return LMGPU_OK;
}

int lmgpu_marginal_covariance(lmgpu_handle* h, int32_t slot, double* cov) { return lmgpu_joint_marginal_covariance(h, 1, &slot, cov); }

// The stored linearization ([A b] per factor) stays valid across lmgpu_set_values / lmgpu_retract / lmgpu_restore_values, like the
// GaussianFactorGraph the reference's linearize() returned: tryLambda solves it again with a larger lambda after a rejected step
// (LevenbergMarquardtOptimizer.cpp:302-305) whatever happened to the Values in between.
int lmgpu_retract(lmgpu_handle* h, const double* delta_packed) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->have_values) {
    h->err = "lmgpu_retract: refused (!h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  if (delta_packed)
    HIPCHECK(hipMemcpy(h->delta + 3 * h->n_hidden, delta_packed, (h->ntot - 3 * h->n_hidden) * sizeof(double), hipMemcpyHostToDevice));
  rc = do_retract(h, h->cur, h->cur ^ 1);
  if (rc) return rc;
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->cur ^= 1;
  return LMGPU_OK;
}

int lmgpu_hessian_diagonal(lmgpu_handle* h, double* diag) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->linearized || !diag) {
    h->err = "lmgpu_hessian_diagonal: refused (!h->finalized || !h->linearized || !diag)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "lmgpu_hessian_diagonal")) return LMGPU_INVALID;
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  if ((rc = launch_hessian_diag(h))) return rc;
  HIPCHECK(hipMemcpyAsync(diag, h->hdiag, h->ntot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return LMGPU_OK;
}

int lmgpu_lm_init(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* out) {
  if (!h) return LMGPU_INVALID;
  if (!p || !h->finalized || !h->have_values) {
    h->err = "lmgpu_lm_init: refused (!p || !h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  if (p->diagonalDamping && smart_refused(h, "lmgpu_lm_init with diagonalDamping")) return LMGPU_INVALID;
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  // LevenbergMarquardtOptimizer ctor (LevenbergMarquardtOptimizer.cpp:47-63): state(values, graph.error(values), lambdaInitial, lambdaFactor)
  double e = 0;
  rc = compute_error(h, h->cur, &e);
  if (rc) return rc;
  h->lm.error = e;
  h->lm.lambda = p->lambdaInitial;
  h->lm.currentFactor = p->lambdaFactor;
  h->lm.iterations = 0;
  h->lm.totalNumberInnerIterations = 0;
  if (out) *out = h->lm;
  return LMGPU_OK;
}

int lmgpu_iterate(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  if (!p || !h->finalized || !h->have_values) {
    h->err = "lmgpu_iterate: refused (!p || !h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  if (p->diagonalDamping && smart_refused(h, "lmgpu_iterate with diagonalDamping")) return LMGPU_INVALID;
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  if (inout) h->lm = *inout;  // the caller owns the LevenbergMarquardtState (error, lambda, factor, counters)
  rc = lm_iterate(h, p);
  if (inout) *inout = h->lm;
  return rc;
}

int lmgpu_gn_iterate(lmgpu_handle* h, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->have_values) {
    h->err = "lmgpu_gn_iterate: refused (!h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  if (inout) h->lm = *inout;
  rc = gn_iterate(h);
  if (inout) *inout = h->lm;
  return rc;
}
int lmgpu_gn_optimize(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  if (!p || !h->finalized || !h->have_values) {
    h->err = "lmgpu_gn_optimize: refused (!p || !h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  if (inout) h->lm = *inout;
  // NonlinearOptimizer::defaultOptimize (gtsam/nonlinear/NonlinearOptimizer.cpp:62-117) around GaussNewtonOptimizer::iterate
  double currentError = h->lm.error;
  if (!(currentError <= p->errorTol || h->lm.iterations >= p->maxIterations)) {
    double newError = currentError;
    do {
      currentError = newError;
      rc = gn_iterate(h);
      if (rc) break;
      newError = h->lm.error;
    } while (h->lm.iterations < p->maxIterations &&
             !check_convergence(p->relativeErrorTol, p->absoluteErrorTol, p->errorTol, currentError, newError) && std::isfinite(currentError));
  }
  if (inout) *inout = h->lm;
  return rc;
}
int lmgpu_dl_iterate(lmgpu_handle* h, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || !h->have_values) {
    h->err = "lmgpu_dl_iterate: refused (!h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "lmgpu_dl_iterate")) return LMGPU_INVALID;
  int rc = need_device(h);
  if (rc) return rc;
  if (inout) h->lm = *inout;
  rc = dl_iterate(h);
  if (inout) *inout = h->lm;
  return rc;
}
// Read-only tap on the Bayes-tree products of the last solve (bt_gradient, bt_forward): h->delta, the values and the optimizer state
// stay as they are; h->bt_vec is the scratch vector dl_iterate overwrites first thing.
int lmgpu_bt_products(lmgpu_handle* h, const double* x_packed, double alpha, double* sq_norm, double* gradient_packed) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || h->cfg.world_size > 1 || h->solver == LMGPU_SOLVER_PCG || !h->solved) {
    h->err = "lmgpu_bt_products: needs a finalized single-rank handle of the direct solver with a factor in the pool (call lmgpu_solve first)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "lmgpu_bt_products")) return LMGPU_INVALID;
  int rc = need_device(h);
  if (rc) return rc;
  hipStream_t s = h->stream;
  const int n = h->ntot;
  if (!h->bt_vec) HIPCHECK(hipMalloc((void**)&h->bt_vec, std::max(1, n) * sizeof(double)));
  if (gradient_packed) {
    rc = bt_gradient(h);
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(gradient_packed, h->bt_vec, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  if (x_packed && sq_norm) {
    HIPCHECK(hipMemcpyAsync(h->bt_vec, x_packed, n * sizeof(double), hipMemcpyHostToDevice, s));
    rc = bt_forward(h, h->bt_vec, alpha, sq_norm);  // synchronises
    if (rc) return rc;
  }
  return LMGPU_OK;
}
int lmgpu_dl_optimize(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  if (!p || !h->finalized || !h->have_values) {
    h->err = "lmgpu_dl_optimize: refused (!p || !h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "lmgpu_dl_optimize")) return LMGPU_INVALID;
  int rc = need_device(h);
  if (rc) return rc;
  if (h->solver == LMGPU_SOLVER_PCG) {
    h->err = "Dogleg is not compatible with the conjugate gradient solver (it needs the Bayes tree of the direct solver)";
    return LMGPU_INVALID;
  }
  if (inout) h->lm = *inout;
  double currentError = h->lm.error;
  if (!(currentError <= p->errorTol || h->lm.iterations >= p->maxIterations)) {
    double newError = currentError;
    do {
      currentError = newError;
      rc = dl_iterate(h);
      if (rc) break;
      newError = h->lm.error;
    } while (h->lm.iterations < p->maxIterations &&
             !check_convergence(p->relativeErrorTol, p->absoluteErrorTol, p->errorTol, currentError, newError) && std::isfinite(currentError));
  }
  if (inout) *inout = h->lm;
  return rc;
}
int lmgpu_optimize(lmgpu_handle* h, const lmgpu_lm_params* p, lmgpu_lm_state* inout) {
  if (!h) return LMGPU_INVALID;
  if (!p || !h->finalized || !h->have_values) {
    h->err = "lmgpu_optimize: refused (!p || !h->finalized || !h->have_values)";
    return LMGPU_INVALID;
  }
  if (p->diagonalDamping && smart_refused(h, "lmgpu_optimize with diagonalDamping")) return LMGPU_INVALID;
  int rc = need_device(h);
  if (rc) return rc;
  if ((rc = need_comm(h))) return rc;
  // NonlinearOptimizer::defaultOptimize (gtsam/nonlinear/NonlinearOptimizer.cpp:62-117)
  if (inout) h->lm = *inout;  // the caller owns the LevenbergMarquardtState, as in lmgpu_iterate
  double currentError = h->lm.error;
  if (currentError <= p->errorTol || h->lm.iterations >= p->maxIterations) {
    if (inout) *inout = h->lm;
    return LMGPU_OK;
  }
  double newError = currentError;
  do {
    currentError = newError;
    rc = lm_iterate(h, p);
    if (rc) {
      if (inout) *inout = h->lm;  // the state reached so far, also on an error return
      return rc;
    }
    newError = h->lm.error;
  } while (h->lm.iterations < p->maxIterations &&
           !check_convergence(p->relativeErrorTol, p->absoluteErrorTol, p->errorTol, currentError, newError) && std::isfinite(currentError));
  if (inout) *inout = h->lm;
  return LMGPU_OK;
}

int lmgpu_get_timings(const lmgpu_handle* h, lmgpu_timings* out) {
  if (!h || !out) return LMGPU_INVALID;
  *out = h->tim;
  return LMGPU_OK;
}

int lmgpu_set_linear_solver(lmgpu_handle* h, int32_t solver, const lmgpu_pcg_params* pcg) {
  if (!h) return LMGPU_INVALID;
  if (solver == LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY) {
    if (h->pcg_structure) {
      h->err = "lmgpu_set_linear_solver: this handle was finalized under PCG and has no fronts to eliminate";
      return LMGPU_INVALID;
    }
    h->solver = solver;
    return LMGPU_OK;
  }
  if (solver == LMGPU_SOLVER_PCG && smart_refused(h, "LMGPU_SOLVER_PCG")) return LMGPU_INVALID;
  if (solver != LMGPU_SOLVER_PCG || !pcg) {
    h->err = "lmgpu_set_linear_solver: unknown solver, or PCG without parameters (NonlinearOptimizer.cpp:156-158)";
    return LMGPU_INVALID;
  }
  if (h->cfg.world_size > 1 || (h->cfg.flags & LMGPU_FLAG_SPLIT_ROOT)) {
    h->err = "lmgpu_set_linear_solver: PCG is single-rank";
    return LMGPU_INVALID;
  }
  if ((pcg->preconditioner != LMGPU_PRECOND_DUMMY && pcg->preconditioner != LMGPU_PRECOND_BLOCK_JACOBI) || pcg->minIterations < 0 ||
      pcg->maxIterations < 0 || pcg->maxIterations > (1 << 28) || pcg->reset < 1 || !(pcg->epsilon_rel >= 0.0) || !(pcg->epsilon_abs >= 0.0)) {
    h->err = "lmgpu_set_linear_solver: invalid PCG parameters (preconditioner 0 / 1, iterations >= 0, reset >= 1, epsilons >= 0)";
    return LMGPU_INVALID;
  }
  h->solver = solver;
  h->pcgp = *pcg;
  return LMGPU_OK;
}

int lmgpu_get_pcg_stats(const lmgpu_handle* h, lmgpu_pcg_stats* out) {
  if (!h || !out || !h->pcg_have_stats) return LMGPU_INVALID;
  *out = h->pcg_stats;
  return LMGPU_OK;
}

// ---------------------------------------------------------------- GNC (gtsam/nonlinear/GncOptimizer.h, GncParams.h)
namespace {

// regularised lower incomplete gamma P(a, x): series for x < a + 1, Lentz continued fraction of Q otherwise
double gamma_p(double a, double x) {
  if (x <= 0.0) return 0.0;
  const double lg = std::lgamma(a);
  if (x < a + 1.0) {
    double ap = a, sum = 1.0 / a, del = sum;
    for (int n = 0; n < 10000; n++) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
      if (std::fabs(del) < std::fabs(sum) * 1e-17) break;
    }
    return sum * std::exp(-x + a * std::log(x) - lg);
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, hh = d;
  for (int i = 1; i < 10000; i++) {
    const double an = -i * (i - a);
    b += 2.0;
    d = an * d + b;
    if (std::fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    hh *= del;
    if (std::fabs(del - 1.0) < 1e-16) break;
  }
  return 1.0 - std::exp(-x + a * std::log(x) - lg) * hh;
}

int gnc_need(lmgpu_handle* h, const char* who) {
  if (!h->gnc_on) {
    h->err = std::string(who) + ": GNC is not enabled on this handle (lmgpu_gnc_enable)";
    return LMGPU_INVALID;
  }
  return need_device(h);
}

// a boundary vector (graph-index order, gnc_n entries) -> local factor order; slots without a factor are dropped
void gnc_to_local(const lmgpu_handle* h, const double* v, std::vector<double>& loc) {
  loc.assign((size_t)std::max(1, h->nfac), 1.0);
  for (int g = 0; g < h->gnc_n; g++)
    if (h->gnc_pos[g] >= 0) loc[h->gnc_pos[g]] = v[g];
}

int gnc_upload(lmgpu_handle* h, double* dst, const std::vector<double>& loc) {
  HIPCHECK(hipMemcpyAsync(dst, loc.data(), (size_t)h->nfac * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return LMGPU_OK;
}

int gnc_download(lmgpu_handle* h, const double* src, double* out) {
  std::vector<double> loc((size_t)std::max(1, h->nfac));
  HIPCHECK(hipMemcpyAsync(loc.data(), src, (size_t)h->nfac * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  for (int g = 0; g < h->gnc_n; g++) out[g] = h->gnc_pos[g] >= 0 ? loc[h->gnc_pos[g]] : 1.0;
  return LMGPU_OK;
}

// initializeWeightsFromKnownInliersAndOutliers (GncOptimizer.h:174-180): ones, known outliers 0
int gnc_reset_weights(lmgpu_handle* h) {
  std::vector<double> w((size_t)std::max(1, h->nfac), 1.0);
  for (int i = 0; i < h->nfac; i++)
    if (h->gnc_fixed_h[i] == 2) w[i] = 0.0;
  return gnc_upload(h, h->gnc_w, w);
}

int gnc_default_thresholds(lmgpu_handle* h, double alpha) {
  std::vector<double> b((size_t)std::max(1, h->nfac), 1.0);
  std::map<int, double> by_rows;  // rows of a factor -> its threshold (one quantile evaluation per distinct row count)
  for (size_t i = 0; i < h->plan.factors.size(); i++) {
    const int l = h->fac_local[i];
    if (l < 0) continue;
    const int rows = h->buckets[h->plan.factors[i].bucket].rows;
    auto it = by_rows.find(rows);
    if (it == by_rows.end()) it = by_rows.emplace(rows, 0.5 * lmgpu_chi2inv(alpha, rows)).first;  // :134
    b[l] = it->second;
  }
  return gnc_upload(h, h->gnc_b, b);
}

// r_k of every factor at values[which] into ebuf0: the error kernels on the unweighted graph (gw = nullptr, robust ignored)
int gnc_raw_errors(lmgpu_handle* h, int which) {
  h->gnc_raw = true;
  const int rc = launch_factors<false>(h, which);
  h->gnc_raw = false;
  return rc;
}

// calculateWeights at values[cur] (queued): weights into gnc_w, max |w - round(w)| into h_gnc_scal[0]
int gnc_enqueue_weights(lmgpu_handle* h, int loss, double mu) {
  const int rc = gnc_raw_errors(h, h->cur);
  if (rc) return rc;
  const int g = std::min(GNC_MAX_BLOCKS, std::max(1, (h->nfac + 255) / 256));
  hipLaunchKernelGGL(gnc_weights_kernel, dim3(g), dim3(256), 0, h->stream, h->nfac, (const double*)h->ebuf0, (const double*)h->gnc_b,
                     (const unsigned char*)h->gnc_fixed, mu, loss, h->gnc_w, h->gnc_part);
  hipLaunchKernelGGL(gnc_finish_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)h->gnc_part, g, 0, h->gnc_scal);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(h->h_gnc_scal, h->gnc_scal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  h->linearized = h->have_jacobians = h->marg_valid = false;  // the stored [A b] carry the previous weights: no solve and no parity tap reads them
  return LMGPU_OK;
}

// initializeMu at values[cur] (waits for the scalar)
int gnc_init_mu(lmgpu_handle* h, int loss, double* mu) {
  const int rc = gnc_raw_errors(h, h->cur);
  if (rc) return rc;
  const int g = std::min(GNC_MAX_BLOCKS, std::max(1, (h->nfac + 255) / 256));
  hipLaunchKernelGGL(gnc_mu_init_kernel, dim3(g), dim3(256), 0, h->stream, h->nfac, (const double*)h->ebuf0, (const double*)h->gnc_b, loss,
                     h->gnc_part);
  hipLaunchKernelGGL(gnc_finish_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)h->gnc_part, g, loss == LMGPU_GNC_GM ? 0 : 1,
                     h->gnc_scal + 1);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(h->h_gnc_scal + 1, h->gnc_scal + 1, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  *mu = h->h_gnc_scal[1];
  return LMGPU_OK;
}

// BaseOptimizer(graph, values, params).optimize() on the weighted graph at values[cur]: a fresh state, then the optimizer's own loop
int gnc_base_optimize(lmgpu_handle* h, int base, const lmgpu_lm_params* bp) {
  int rc = lmgpu_lm_init(h, bp, nullptr);
  if (rc) return rc;
  return base == LMGPU_GNC_BASE_GN ? lmgpu_gn_optimize(h, bp, nullptr) : lmgpu_optimize(h, bp, nullptr);
}

}  // namespace

double lmgpu_chi2inv(double alpha, int32_t dofs) {
  if (!(alpha >= 0.0) || !(alpha < 1.0) || dofs < 1) return std::numeric_limits<double>::quiet_NaN();
  if (alpha == 0.0) return 0.0;
  const double a = 0.5 * dofs;
  // bracket, then Newton on P(a, x / 2) = alpha inside it (bisection whenever a step leaves the bracket)
  double lo = 0.0, hi = std::max(1.0, (double)dofs);
  while (gamma_p(a, 0.5 * hi) < alpha) hi *= 2.0;
  double x = 0.5 * (lo + hi);
  for (int it = 0; it < 200; it++) {
    const double f = gamma_p(a, 0.5 * x) - alpha;
    if (f > 0) hi = x; else lo = x;
    const double pdf = 0.5 * std::exp(-0.5 * x + (a - 1.0) * std::log(0.5 * x) - std::lgamma(a));
    double xn = pdf > 0 ? x - f / pdf : 0.5 * (lo + hi);
    if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
    if (std::fabs(xn - x) <= 1e-15 * std::fabs(x)) {
      x = xn;
      break;
    }
    x = xn;
  }
  return x;
}

int lmgpu_gnc_enable(lmgpu_handle* h, int32_t on, int32_t graph_size) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized) {
    h->err = "lmgpu_gnc_enable: refused (!h->finalized)";
    return LMGPU_INVALID;
  }
  if (on && smart_refused(h, "lmgpu_gnc_enable")) return LMGPU_INVALID;
  if (on && (h->cfg.world_size > 1 || (h->cfg.flags & LMGPU_FLAG_SPLIT_ROOT))) {
    h->err = "lmgpu_gnc_enable: GNC is single-rank (world_size > 1)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  auto drop = [&]() {
    if (h->gnc_w) (void)hipFree(h->gnc_w);
    if (h->gnc_b) (void)hipFree(h->gnc_b);
    if (h->gnc_part) (void)hipFree(h->gnc_part);
    if (h->gnc_scal) (void)hipFree(h->gnc_scal);
    if (h->gnc_fixed) (void)hipFree(h->gnc_fixed);
    h->gnc_w = h->gnc_b = h->gnc_part = h->gnc_scal = nullptr;
    h->gnc_fixed = nullptr;
  };
  if (!on) {
    HIPCHECK(hipStreamSynchronize(h->stream));
    drop();
    if (h->gnc_on) h->linearized = h->have_jacobians = h->marg_valid = false;
    h->gnc_on = false;
    return LMGPU_OK;
  }
  const int max_gi = h->graph_index_sorted.empty() ? -1 : h->graph_index_sorted.back();
  if (h->plan.factors.size() && h->graph_index_sorted.front() < 0) {
    h->err = "lmgpu_gnc_enable: negative graph_index";
    return LMGPU_INVALID;
  }
  if (graph_size <= 0) graph_size = max_gi + 1;
  if (graph_size <= max_gi) {
    h->err = "lmgpu_gnc_enable: graph_size is smaller than the largest graph_index + 1";
    return LMGPU_INVALID;
  }
  HIPCHECK(hipStreamSynchronize(h->stream));
  drop();
  h->gnc_n = graph_size;
  h->gnc_n_in = h->gnc_n_out = 0;
  h->gnc_pos.assign((size_t)graph_size, -1);
  for (size_t i = 0; i < h->plan.factors.size(); i++) h->gnc_pos[h->graph_index_sorted[i]] = h->fac_local[i];
  h->gnc_fixed_h.assign((size_t)std::max(1, h->nfac), 0);
  const size_t n1 = (size_t)std::max(1, h->nfac);
  HIPCHECK(hipMalloc((void**)&h->gnc_w, n1 * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->gnc_b, n1 * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->gnc_part, GNC_MAX_BLOCKS * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->gnc_scal, 2 * sizeof(double)));
  HIPCHECK(hipMalloc((void**)&h->gnc_fixed, n1));
  HIPCHECK(hipMemset(h->gnc_fixed, 0, n1));
  if (!h->h_gnc_scal) HIPCHECK(hipHostMalloc((void**)&h->h_gnc_scal, 2 * sizeof(double)));
  for (int i = 0; i < 2; i++)
    if (!h->gnc_ev[i]) HIPCHECK(hipEventCreate(&h->gnc_ev[i]));
  if ((rc = gnc_reset_weights(h))) return rc;
  if ((rc = gnc_default_thresholds(h, 0.99))) return rc;  // GncOptimizer.h:104-106
  h->gnc_on = true;
  h->linearized = h->have_jacobians = h->marg_valid = false;
  return LMGPU_OK;
}

int lmgpu_gnc_set_inlier_cost_thresholds(lmgpu_handle* h, int32_t n, const double* barcSq, double alpha) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_set_inlier_cost_thresholds");
  if (rc) return rc;
  if (!barcSq) {
    if (!(alpha > 0.0 && alpha < 1.0)) {
      h->err = "lmgpu_gnc_set_inlier_cost_thresholds: alpha must lie in (0, 1)";
      return LMGPU_INVALID;
    }
    return gnc_default_thresholds(h, alpha);
  }
  if (n != h->gnc_n) {
    h->err = "lmgpu_gnc_set_inlier_cost_thresholds: the number of thresholds does not match the size of the factor graph";
    return LMGPU_INVALID;
  }
  std::vector<double> loc;
  gnc_to_local(h, barcSq, loc);
  return gnc_upload(h, h->gnc_b, loc);
}

int lmgpu_gnc_set_known(lmgpu_handle* h, int32_t n_in, const uint64_t* inliers, int32_t n_out, const uint64_t* outliers) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_set_known");
  if (rc) return rc;
  if (n_in < 0 || n_out < 0 || (n_in && !inliers) || (n_out && !outliers)) {
    h->err = "lmgpu_gnc_set_known: refused (negative count or NULL list)";
    return LMGPU_INVALID;
  }
  std::vector<unsigned char> slot((size_t)h->gnc_n, 0);
  for (int i = 0; i < n_in; i++) {
    if (inliers[i] >= (uint64_t)h->gnc_n) {
      h->err = "lmgpu_gnc_set_known: one or more measurements that are not in the factor graph selected to be known inliers";
      return LMGPU_INVALID;
    }
    slot[inliers[i]] = 1;
  }
  for (int i = 0; i < n_out; i++) {
    if (outliers[i] >= (uint64_t)h->gnc_n) {
      h->err = "lmgpu_gnc_set_known: one or more measurements that are not in the factor graph selected to be known outliers";
      return LMGPU_INVALID;
    }
    if (slot[outliers[i]] == 1) {
      h->err = "lmgpu_gnc_set_known: one or more measurements selected to be BOTH a known inlier and a known outlier";
      return LMGPU_INVALID;
    }
    slot[outliers[i]] = 2;
  }
  std::fill(h->gnc_fixed_h.begin(), h->gnc_fixed_h.end(), 0);
  for (int g = 0; g < h->gnc_n; g++)
    if (h->gnc_pos[g] >= 0) h->gnc_fixed_h[h->gnc_pos[g]] = slot[g];
  h->gnc_n_in = n_in;
  h->gnc_n_out = n_out;
  HIPCHECK(hipMemcpyAsync(h->gnc_fixed, h->gnc_fixed_h.data(), (size_t)std::max(1, h->nfac), hipMemcpyHostToDevice, h->stream));
  h->linearized = h->have_jacobians = h->marg_valid = false;
  return gnc_reset_weights(h);
}

int lmgpu_gnc_set_weights(lmgpu_handle* h, int32_t n, const double* w) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_set_weights");
  if (rc) return rc;
  if (!w || n != h->gnc_n) {
    h->err = "lmgpu_gnc_set_weights: the number of specified weights does not match the size of the factor graph";
    return LMGPU_INVALID;
  }
  h->linearized = h->have_jacobians = h->marg_valid = false;
  std::vector<double> loc;
  gnc_to_local(h, w, loc);
  return gnc_upload(h, h->gnc_w, loc);
}

int lmgpu_gnc_get_weights(lmgpu_handle* h, int32_t n, double* w) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_get_weights");
  if (rc) return rc;
  if (!w || n != h->gnc_n) {
    h->err = "lmgpu_gnc_get_weights: the length does not match the size of the factor graph";
    return LMGPU_INVALID;
  }
  return gnc_download(h, h->gnc_w, w);
}

int lmgpu_gnc_get_inlier_cost_thresholds(lmgpu_handle* h, int32_t n, double* barcSq) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_get_inlier_cost_thresholds");
  if (rc) return rc;
  if (!barcSq || n != h->gnc_n) {
    h->err = "lmgpu_gnc_get_inlier_cost_thresholds: the length does not match the size of the factor graph";
    return LMGPU_INVALID;
  }
  return gnc_download(h, h->gnc_b, barcSq);
}

static int gnc_check_loss(lmgpu_handle* h, int32_t lossType, const char* who) {
  if (lossType != LMGPU_GNC_GM && lossType != LMGPU_GNC_TLS) {
    h->err = std::string(who) + ": called with unknown loss type";
    return LMGPU_INVALID;
  }
  if (!h->have_values) {
    h->err = std::string(who) + ": refused (!h->have_values)";
    return LMGPU_INVALID;
  }
  return LMGPU_OK;
}

int lmgpu_gnc_initialize_mu(lmgpu_handle* h, int32_t lossType, double* mu) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_initialize_mu");
  if (rc) return rc;
  if (!mu) {
    h->err = "lmgpu_gnc_initialize_mu: refused (!mu)";
    return LMGPU_INVALID;
  }
  if ((rc = gnc_check_loss(h, lossType, "lmgpu_gnc_initialize_mu"))) return rc;
  return gnc_init_mu(h, lossType, mu);
}

int lmgpu_gnc_calculate_weights(lmgpu_handle* h, int32_t lossType, double mu) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_calculate_weights");
  if (rc) return rc;
  if ((rc = gnc_check_loss(h, lossType, "lmgpu_gnc_calculate_weights"))) return rc;
  if ((rc = gnc_enqueue_weights(h, lossType, mu))) return rc;
  HIPCHECK(hipStreamSynchronize(h->stream));
  return LMGPU_OK;
}

int lmgpu_gnc_optimize(lmgpu_handle* h, const lmgpu_gnc_params* gp, const lmgpu_lm_params* bp, lmgpu_lm_state* base_state_out,
                       lmgpu_gnc_result* out) {
  if (!h) return LMGPU_INVALID;
  int rc = gnc_need(h, "lmgpu_gnc_optimize");
  if (rc) return rc;
  if (!gp || !bp || !out) {
    h->err = "lmgpu_gnc_optimize: refused (!params || !base || !out)";
    return LMGPU_INVALID;
  }
  if (gp->baseOptimizer != LMGPU_GNC_BASE_LM && gp->baseOptimizer != LMGPU_GNC_BASE_GN) {
    h->err = "lmgpu_gnc_optimize: the base optimizer must be Levenberg-Marquardt or Gauss-Newton (Dogleg is not bound)";
    return LMGPU_INVALID;
  }
  if (gp->maxIterations < 0 || !(gp->muStep > 0.0)) {
    h->err = "lmgpu_gnc_optimize: refused (maxIterations < 0 || !(muStep > 0))";
    return LMGPU_INVALID;
  }
  if ((rc = gnc_check_loss(h, gp->lossType, "lmgpu_gnc_optimize"))) return rc;
  const int loss = gp->lossType;
  std::memset(out, 0, sizeof(*out));
  h->gnc_trace.clear();
  // state_ = the values at the call: every base optimizer starts from them (GncOptimizer.h:184-187, 236-238)
  if ((rc = lmgpu_save_values(h))) return rc;
  double mu = 0.0;
  if ((rc = gnc_init_mu(h, loss, &mu))) return rc;  // :188 -- a function of state_ and barcSq only, so evaluated while the values are state_
  rc = gnc_base_optimize(h, gp->baseOptimizer, bp);  // :184-187
  if (base_state_out) *base_state_out = h->lm;
  out->base_iterations_total = h->lm.iterations;
  if (rc) return rc;
  double prev_cost = h->lm.error, cost = 0.0;  // :189 graph_initial.error(result) = the base optimizer's own final error
  out->mu = mu;
  out->prev_cost = prev_cost;
  const int nrUnknownInOrOut = h->gnc_n - (h->gnc_n_in + h->gnc_n_out);  // :196
  if (mu <= 0 || nrUnknownInOrOut == 0) {                                 // :198-215
    out->stop = mu <= 0 ? 4 : 5;
    return LMGPU_OK;
  }
  int iter = 0, stop = 0;
  for (iter = 0; iter < gp->maxIterations; iter++) {
    (void)hipEventRecord(h->gnc_ev[0], h->stream);
    if ((rc = gnc_enqueue_weights(h, loss, mu))) return rc;  // :232
    (void)hipEventRecord(h->gnc_ev[1], h->stream);
    if ((rc = lmgpu_restore_values(h))) return rc;  // :236-238
    const auto t0 = std::chrono::steady_clock::now();
    rc = gnc_base_optimize(h, gp->baseOptimizer, bp);
    const double base_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (base_state_out) *base_state_out = h->lm;
    out->base_iterations_total += h->lm.iterations;
    if (rc) return rc;
    cost = h->lm.error;  // :241
    const double wdev = h->h_gnc_scal[0];  // its copy was queued before the base optimizer's first wait
    float wms = 0.0f;
    (void)hipEventElapsedTime(&wms, h->gnc_ev[0], h->gnc_ev[1]);
    const double tr[6] = {mu, cost, wdev, (double)wms, base_ms, (double)h->lm.iterations};
    h->gnc_trace.insert(h->gnc_trace.end(), tr, tr + 6);
    // checkConvergence :389-393 = cost :351-359 || weights :362-386 || mu :332-348
    if (std::fabs(cost - prev_cost) / std::max(prev_cost, 1e-7) < gp->relativeCostTol) {
      stop = 1;
      break;
    }
    if (loss == LMGPU_GNC_TLS && !(wdev > gp->weightsTol)) {
      stop = 2;
      break;
    }
    if (loss == LMGPU_GNC_GM && std::fabs(mu - 1.0) < 1e-9) {
      stop = 3;
      break;
    }
    mu = loss == LMGPU_GNC_GM ? std::max(1.0, mu / gp->muStep) : mu * gp->muStep;  // updateMu :317-329
    prev_cost = cost;
  }
  out->iterations = iter;
  out->stop = stop;
  out->mu = mu;
  out->cost = cost;
  out->prev_cost = prev_cost;
  return LMGPU_OK;
}

int lmgpu_gnc_get_trace(const lmgpu_handle* h, int32_t max_rows, double* rows6) {
  if (!h) return -1;
  const int n = (int)(h->gnc_trace.size() / 6);
  if (rows6)
    for (int i = 0; i < std::min(n, (int)max_rows) * 6; i++) rows6[i] = h->gnc_trace[i];
  return n;
}

int lmgpu_set_kernel_timing(lmgpu_handle* h, int32_t on) {
  if (!h) return LMGPU_INVALID;
  h->kt.on = on != 0;
  h->kt.dominant_only = on == 2;
  h->kt.reset();
  return LMGPU_OK;
}

int lmgpu_get_kernel_times(const lmgpu_handle* h, double* ms, double* work, int64_t* launches) {
  if (!h) return LMGPU_INVALID;
  for (int i = 0; i < LMGPU_KT_NUM; i++) {
    if (ms) ms[i] = h->kt.ms[i];
    if (work) work[i] = h->kt.work[i];
    if (launches) launches[i] = h->kt.cnt[i];
  }
  return LMGPU_OK;
}

int lmgpu_get_jacobian(lmgpu_handle* h, int32_t graph_index, double* out, int32_t* rows, int32_t* cols) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized) {
    h->err = "lmgpu_get_jacobian: refused (!h->finalized)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "lmgpu_get_jacobian")) return LMGPU_INVALID;
  auto it = std::lower_bound(h->graph_index_sorted.begin(), h->graph_index_sorted.end(), graph_index);
  if (it == h->graph_index_sorted.end() || *it != graph_index) return LMGPU_INVALID;
  const FactorRef& f = h->plan.factors[it - h->graph_index_sorted.begin()];
  const Bucket& b = h->buckets[f.bucket];
  if (rows) *rows = b.rows;
  if (cols) *cols = b.cols;
  if (out) {
    int rc = need_device(h);
    if (rc) return rc;
    if (!h->have_jacobians || b.loc_of[f.idx] < 0) return LMGPU_INVALID;  // never linearized, or the factor lives on another rank
    HIPCHECK(hipMemcpy(out, h->pool + b.joff + (int64_t)b.loc_of[f.idx] * b.rows * b.cols, (size_t)b.rows * b.cols * sizeof(double),
                       hipMemcpyDeviceToHost));
  }
  return LMGPU_OK;
}

int lmgpu_get_jacobians(lmgpu_handle* h, int32_t* n_out, int32_t* graph_index, int32_t* rows, int32_t* cols, int64_t* offsets, double* out) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized) {
    h->err = "lmgpu_get_jacobians: refused (!h->finalized)";
    return LMGPU_INVALID;
  }
  if (smart_refused(h, "lmgpu_get_jacobians")) return LMGPU_INVALID;
  const int NFAC = (int)h->plan.factors.size();
  if (n_out) *n_out = NFAC;
  int64_t off = 0;
  for (int i = 0; i < NFAC; i++) {  // plan.factors is ascending by graph index
    const FactorRef& f = h->plan.factors[i];
    const Bucket& b = h->buckets[f.bucket];
    if (graph_index) graph_index[i] = f.graph_index;
    if (rows) rows[i] = b.rows;
    if (cols) cols[i] = b.cols;
    if (offsets) offsets[i] = off;
    off += (int64_t)b.rows * b.cols;
  }
  if (offsets) offsets[NFAC] = off;
  if (!out) return LMGPU_OK;
  int rc = need_device(h);
  if (rc) return rc;
  if (!h->have_jacobians) {
    h->err = "lmgpu_get_jacobians: refused (no linearization on the device)";
    return LMGPU_INVALID;
  }
  // one copy per bucket, then the host puts every factor at its place in graph order
  std::vector<std::vector<double>> jb(h->buckets.size());
  for (size_t k = 0; k < h->buckets.size(); k++) {
    const Bucket& b = h->buckets[k];
    jb[k].resize((size_t)b.n_loc * b.rows * b.cols);
    if (b.n_loc) HIPCHECK(hipMemcpy(jb[k].data(), h->pool + b.joff, jb[k].size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  off = 0;
  for (int i = 0; i < NFAC; i++) {
    const FactorRef& f = h->plan.factors[i];
    const Bucket& b = h->buckets[f.bucket];
    const size_t sz = (size_t)b.rows * b.cols;
    if (b.loc_of[f.idx] < 0) {
      h->err = "lmgpu_get_jacobians: a factor lives on another rank";
      return LMGPU_INVALID;
    }
    std::memcpy(out + off, jb[f.bucket].data() + (size_t)b.loc_of[f.idx] * sz, sz * sizeof(double));
    off += (int64_t)sz;
  }
  return LMGPU_OK;
}

int lmgpu_num_fronts(const lmgpu_handle* h) { return (h && h->finalized) ? (int)h->plan.fronts.size() : -1; }

int lmgpu_leaf_group_launches(const lmgpu_handle* h) { return (h && h->finalized) ? h->n_leaf_group_launches : -1; }

int lmgpu_backsub_group_launches(const lmgpu_handle* h, int32_t* wide) {
  if (!h || !h->finalized) return -1;
  int cnt = 0, w = 0;
  for (const LevelWork& L : h->levels) {
    const int form = backsub_group_form(h, L);
    cnt += form != 0;
    w += form == 2;
  }
  if (wide) *wide = w;
  return cnt;
}

int lmgpu_get_leaf_corner(lmgpu_handle* h, int32_t front, double* corner) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || front < 0 || front >= (int)h->plan.fronts.size() || !corner) {
    h->err = "lmgpu_get_leaf_corner: refused (!h->finalized || front < 0 || front >= (int)h->plan.fronts.size() || !corner)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  const FrontDesc& F = h->h_fronts[front];
  if (!h->solved || !h->front_active[front] || F.par_ld != -1 || !h->d_gcorner) return LMGPU_INVALID;  // (gather leaves only)
  HIPCHECK(hipMemcpy(corner, h->d_gcorner + F.par_map, sizeof(double), hipMemcpyDeviceToHost));
  return LMGPU_OK;
}

int lmgpu_front_info(const lmgpu_handle* h, int32_t front, int32_t* info) {
  if (!h || !h->finalized || front < 0 || front >= (int)h->plan.fronts.size() || !info) return LMGPU_INVALID;
  const Front& fr = h->plan.fronts[front];
  info[0] = (int)fr.vars.size();
  info[1] = fr.n_frontal_vars;
  info[2] = fr.nf;
  info[3] = fr.n;
  info[4] = fr.parent;
  info[5] = fr.cls;
  info[6] = h->front_owner[front];
  info[7] = fr.level;
  return LMGPU_OK;
}

int lmgpu_get_front(lmgpu_handle* h, int32_t front, int32_t* slots, double* RSd) {
  if (!h) return LMGPU_INVALID;
  if (!h->finalized || front < 0 || front >= (int)h->plan.fronts.size()) {
    h->err = "lmgpu_get_front: refused (!h->finalized || front < 0 || front >= (int)h->plan.fronts.size())";
    return LMGPU_INVALID;
  }
  const Front& fr = h->plan.fronts[front];
  if (slots) std::memcpy(slots, fr.vars.data(), fr.vars.size() * sizeof(int32_t));
  if (RSd) {
    int rc = need_device(h);
    if (rc) return rc;
    if (!h->solved || !h->front_active[front]) return LMGPU_INVALID;
    const FrontDesc& F = h->h_fronts[front];
    std::vector<double> rows((size_t)F.nf * F.ld_rsd);
    HIPCHECK(hipMemcpy(rows.data(), h->pool + F.rsd_off, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < F.nf; i++)
      for (int j = 0; j < F.n; j++) RSd[(size_t)j * F.nf + i] = (j >= i) ? rows[(size_t)i * F.ld_rsd + j] : 0.0;
  }
  return LMGPU_OK;
}

int lmgpu_comm_unique_id(char id128[128]) {
  ncclUniqueId id;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  if (ncclGetUniqueId(&id) != ncclSuccess) return LMGPU_HIP_ERROR;
  std::memcpy(id128, &id, 128);
  return LMGPU_OK;
}

int lmgpu_comm_init(lmgpu_handle* h, const char id128[128]) {
  if (!h) return LMGPU_INVALID;
  if (!id128) {
    h->err = "lmgpu_comm_init: refused (!id128)";
    return LMGPU_INVALID;
  }
  int rc = need_device(h);
  if (rc) return rc;
  ncclUniqueId id;
  std::memcpy(&id, id128, 128);
  HIPCHECK(hipSetDevice(h->device));
  NCCLCHECK(ncclCommInitRank(&h->comm, h->cfg.world_size, id, h->cfg.rank));
  NCCLCHECK(ncclCommSplit(h->comm, 0, h->cfg.rank, &h->comm_data, nullptr));  // collective: every rank calls it right after the init
  return LMGPU_OK;
}

#ifdef LMGPU_TEST_HOOKS  // in-process stand-in for the communicator: exported by liblmgpu_test.so only
int lmgpu_local_group_create(int32_t world_size, lmgpu_local_group** out) {
  if (!out || world_size < 1) return LMGPU_INVALID;
  lmgpu_local_group* g = new lmgpu_local_group();
  g->world = world_size;
  g->ptr.assign(world_size, nullptr);
  g->stream.assign(world_size, nullptr);
  *out = g;
  return LMGPU_OK;
}
#endif
// Host-only view of the launch schedule of a dense front (dense_schedule.hpp): (kind, i, nsteps, chunk) per record into `out`; returns
// the number of records, negative for refused geometry or when max_records is too small.
int lmgpu_selftest_dense_schedule(int n, int nf, int mode, unsigned forms, int max_records, int32_t* out) {
  const std::vector<DenseStep> steps = dense_front_schedule(n, nf, mode, forms);
  if (steps.empty() || !out || (int)steps.size() > max_records) return -1;
  for (const DenseStep& st : steps) {
    const int32_t rec[4] = {st.kind, st.i, st.nsteps, st.chunk};
    out = std::copy(rec, rec + 4, out);
  }
  return (int)steps.size();
}
// Host-only view of the arithmetic of one Dogleg trial (dogleg_step.hpp).  which = 0: in = (delta, uu, nn, un), out = (branch, scalar);
// which = 1: in = (rho, delta, |dx_d|), out = (new delta, stay, moved).  0, or -1 for a missing argument or an unknown `which`.
int lmgpu_selftest_dogleg_step(int which, const double* in, double* out) {
  if (!in || !out) return -1;
  if (which == 0) {
    const DoglegTrial t = dogleg_trial_point(in[0], in[1], in[2], in[3]);
    out[0] = t.branch;
    out[1] = t.scalar;
    return 0;
  }
  if (which == 1) {
    const DoglegRadius r = dogleg_radius_update(in[0], in[1], in[2]);
    out[0] = r.delta;
    out[1] = r.stay ? 1.0 : 0.0;
    out[2] = r.moved ? 1.0 : 0.0;
    return 0;
  }
  return -1;
}
// Host-only view of the factor-type table (factor_types.hpp): (arity, rows, meas, var0, var1, var2) of a public factor type ...
int lmgpu_selftest_factor_type(int32_t type, int32_t out[6]) {
  if (type < 0 || type >= LMGPU_NUM_FACTOR_TYPES || !out) return LMGPU_INVALID;
  const int32_t rec[6] = {factor_arity(type), kFactorTypes[type].rows, kFactorTypes[type].meas, var_type(type, 0), var_type(type, 1), var_type(type, 2)};
  std::copy(rec, rec + 6, out);
  return LMGPU_OK;
}
// ... and (tangent dimension, stored doubles) of a variable type
int lmgpu_selftest_var_type(int32_t type, int32_t out[2]) {
  if (type < 0 || type >= LMGPU_NUM_VAR_TYPES || !out) return LMGPU_INVALID;
  out[0] = kVarDim[type];
  out[1] = kVarStore[type];
  return LMGPU_OK;
}
// Host-only check of the ticket order of a chained launch (kernels_step.hpp: chain_schedule): every logical workgroup of every
// step exactly once, and every dependency step_body waits for at an earlier ticket.  0 = valid, else the 1-based ticket at fault.
int lmgpu_selftest_chain_schedule(int n, int nf, int i0, int nsteps, int far_pct) {
  if (nsteps < 1 || n <= nf || nf < (i0 + nsteps + 1) * 256 - 255) return -1;
  int split_pct = 60;
  if (far_pct >= 100000) {  // + 100000 x (split_pct + 1): another share of the update tasks in front of the row-panel workgroups
    split_pct = far_pct / 100000 - 1;
    far_pct %= 100000;
  }
  const bool merge2 = far_pct >= 1000;
  if (merge2) far_pct -= 1000;
  const std::vector<int2> tasks = chain_schedule(n, nf, i0, nsteps, far_pct, merge2, split_pct);
  struct Geo { int T, S, nHead, nTA, nd, nTB, ntrsm, grid; };
  std::vector<Geo> g(nsteps);
  std::vector<std::vector<int>> pos(nsteps);
  std::vector<std::vector<char>> pair_tail(nsteps);  // the update tile's task of this step also applied the step before
  long total = 0;
  for (int s = 0; s < nsteps; s++) {
    const int i = i0 + s, m = n - (i + 1) * 256, kbn = std::min(nf, (i + 2) * 256) - (i + 1) * 256;
    if (m <= 0 || kbn <= 0 || kbn % 64) return -1;
    Geo& G = g[s];
    G.T = (m + 127) / 128;
    G.S = (m + 63) / 64;
    G.nHead = 4 * step_head_units(G.S);
    G.nTA = step_ta_workgroups(G.S);
    G.nd = kbn / 64;
    G.nTB = G.T * (G.T + 1) / 2 - (G.T >= 2 ? 2 * G.T - 1 : G.T);
    G.ntrsm = (m - kbn + 63) / 64;
    G.grid = step_grid(m, kbn);
    if (G.grid != G.nTA + G.nd + G.nTB + G.ntrsm) return -1;
    pos[s].assign(G.grid, -1);
    pair_tail[s].assign(G.grid, 0);
    total += G.grid;
  }
  auto tb_index = [&](int s, int ti, int tj) {  // logical workgroup of update tile (ti, tj), ti >= 2
    int off = g[s].nTA + g[s].nd;
    for (int r = 2; r < ti; r++) off += g[s].T - r;
    return off + (tj - ti);
  };
  auto tb_tile = [&](int s, int t, int* ti, int* tj) {
    int rem = t - g[s].nTA - g[s].nd;
    *ti = 2;
    while (rem >= g[s].T - *ti) {
      rem -= g[s].T - *ti;
      (*ti)++;
    }
    *tj = *ti + rem;
  };
  long covered = 0;
  for (size_t k = 0; k < tasks.size(); k++) {
    const bool mg = (tasks[k].x & CHAIN_TASK_MERGED) != 0;
    const int s = tasks[k].x & ~CHAIN_TASK_MERGED, t = tasks[k].y;
    if (s < 0 || s >= nsteps || t < 0 || t >= g[s].grid || pos[s][t] >= 0) return (int)k + 1;
    pos[s][t] = (int)k;
    covered++;
    if (mg) {  // only update tiles pair up, and the pair's first half is the same tile one step earlier
      if (!merge2 || s < 1 || t < g[s].nTA + g[s].nd || t >= g[s].nTA + g[s].nd + g[s].nTB) return (int)k + 1;
      int ti, tj;
      tb_tile(s, t, &ti, &tj);
      const int tp = tb_index(s - 1, ti + 2, tj + 2);
      if (pos[s - 1][tp] >= 0) return (int)k + 1;
      pos[s - 1][tp] = (int)k;
      pair_tail[s][t] = 1;
      covered++;
    }
  }
  if (covered != total) return -2;
  for (int s = 0; s < nsteps; s++) {
    const Geo& G = g[s];
    int last_prev_trsm = -1, last_ta = -1, last_diag = -1;
    if (s > 0)
      for (int t = 0; t < g[s - 1].ntrsm; t++) last_prev_trsm = std::max(last_prev_trsm, pos[s - 1][g[s - 1].nTA + g[s - 1].nd + g[s - 1].nTB + t]);
    for (int t = 0; t < G.nTA; t++) last_ta = std::max(last_ta, pos[s][t]);
    for (int t = 0; t < G.nd; t++) last_diag = std::max(last_diag, pos[s][G.nTA + t]);
    for (int t = 0; t < G.grid; t++) {
      const int me = pos[s][t];
      int ti = -1, tj = -1;  // 128-tile whose entries this workgroup updates (none for the panel roles)
      if (t < G.nTA) {
        int si, sj;
        if (t < G.nHead) {
          const int u = t >> 2;
          sj = (u >= 6) ? 3 : ((u >= 3) ? 2 : (u >= 1 ? 1 : 0));
          si = u - sj * (sj + 1) / 2;
          ti = si >> 1;
          tj = sj >> 1;
        } else {
          ti = (t - G.nHead) & 1;
          tj = 2 + ((t - G.nHead) >> 1);
        }
      } else if (t < G.nTA + G.nd) {
        if (me < last_ta) return me + 1;  // diagonal workgroups read the head tiles
      } else if (t < G.nTA + G.nd + G.nTB) {
        tb_tile(s, t, &ti, &tj);
      } else {
        if (me < last_ta || me < last_diag) return me + 1;  // row-panel workgroups read head tiles and diagonal tiles
      }
      if (ti >= 0 && s > 0) {
        // the finished panel of this step -- for the first half of a pair this is implied by the second half's wait (panels finish in order)
        if (me < last_prev_trsm) return me + 1;
        const int before = pos[s - 1][tb_index(s - 1, ti + 2, tj + 2)];
        if (pair_tail[s][t] ? before != me : me <= before) return me + 1;  // the tile this one continues (or is paired with)
      }
    }
  }
  return 0;
}

#ifdef LMGPU_TEST_HOOKS
int lmgpu_debug_table_digest(lmgpu_handle* h, int32_t max, char* names32, uint64_t* counts, uint64_t* fnv1a) {
  if (!h || !h->finalized) return -1;
  for (int i = 0; i < std::min(max, (int32_t)h->table_digest.size()); i++) {
    std::memcpy(names32 + 32 * i, h->table_digest[i].name, 32);
    counts[i] = h->table_digest[i].count;
    fnv1a[i] = h->table_digest[i].fnv1a;
  }
  return (int)h->table_digest.size();
}
int lmgpu_local_group_destroy(lmgpu_local_group* g) {
  delete g;
  return LMGPU_OK;
}
int lmgpu_comm_init_local(lmgpu_handle* h, lmgpu_local_group* g) {
  if (!h) return LMGPU_INVALID;
  if (!g || g->world != h->cfg.world_size) {
    h->err = "lmgpu_comm_init_local: refused (!g || g->world != h->cfg.world_size)";
    return LMGPU_INVALID;
  }
  h->lgroup = g;
  return LMGPU_OK;
}
#endif

// ---------------------------------------------------------------- peak micro-benchmarks

__global__ __launch_bounds__(256) void peak_mfma_f64_kernel(double* out, int iters) {
  double4_t acc[4];
  for (int i = 0; i < 4; i++) acc[i] = double4_t{0, 0, 0, 0};
  const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0;
  for (int i = 0; i < 4; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

// Diagnostic form of the same loop: NACC independent accumulators per wave and, around the loop, one pair of stamps per workgroup --
// s_memtime (shader-clock cycles) and s_memrealtime (constant 100 MHz) -- written to a buffer nothing else reads
// (MI355X_MICROARCH.md, DVFS give-back item 6): the clock the chip HOLDS under this load = d(memtime) / d(memrealtime) x 100 MHz.
#define PEAK_CLOCK_KERNEL(NAME, NACC)                                                                                   \
__global__ __launch_bounds__(256) void NAME(double* out, unsigned long long* stamps, int iters) { \
  double4_t acc[NACC]; \
  for (int i = 0; i < NACC; i++) acc[i] = double4_t{0, 0, 0, 0}; \
  const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9; \
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime(); \
  __builtin_amdgcn_sched_barrier(0); \
  for (int it = 0; it < iters; it++) { \
_Pragma("unroll") \
    for (int i = 0; i < NACC; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0); \
  } \
  double s = 0; \
  for (int i = 0; i < NACC; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3]; \
  out[blockIdx.x * 256 + threadIdx.x] = s; \
  __builtin_amdgcn_sched_barrier(0); \
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime(); \
  if (threadIdx.x == 0) { \
    stamps[2 * blockIdx.x] = c1 - c0; \
    stamps[2 * blockIdx.x + 1] = r1 - r0; \
  } \
}
PEAK_CLOCK_KERNEL(peak_mfma_f64_clock_kernel4, 4)
PEAK_CLOCK_KERNEL(peak_mfma_f64_clock_kernel8, 8)
// the register shape of the trailing-update tile: 4 x 4 accumulators of a 64x64 wave tile, four A and four B operand registers.
// (Round 3: the 4- and 8-accumulator loops above stop at ~49 TFLOP/s, which round 2 took for the instruction's ceiling; the update tile
// itself runs at 61-69 TFLOP/s once its memory traffic is taken away (tools/syrk4_bench.hip), and so does this loop.)
__global__ __launch_bounds__(256, 2) void peak_mfma_f64_clock_kernel16(double* out, unsigned long long* stamps, int iters) {
  double4_t acc[4][4];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) acc[i][j] = double4_t{0, 0, 0, 0};
  double a[4], b[4];
  for (int i = 0; i < 4; i++) {
    a[i] = 0.25 + threadIdx.x * 1e-3 + i * 0.01;
    b[i] = 0.5 - threadIdx.x * 1e-3 - i * 0.01;
  }
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_sched_barrier(0);
  for (int it = 0; it < iters; it += 4) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) {  // keep the operands changing (a loop-invariant operand set is not what a tile sees)
      a[i] = -a[i];
      b[i] = -b[i];
    }
  }
  double s = 0;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    stamps[2 * blockIdx.x] = c1 - c0;
    stamps[2 * blockIdx.x + 1] = r1 - r0;
  }
}

__global__ __launch_bounds__(256) void peak_copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

int lmgpu_peak_mfma_f64(int32_t device, int32_t iters, double* tflops) {
  if (hipSetDevice(device) != hipSuccess) return LMGPU_HIP_ERROR;
  const int blocks = 256 * 8;
  double* out = nullptr;
  if (hipMalloc((void**)&out, (size_t)blocks * 256 * sizeof(double)) != hipSuccess) return LMGPU_HIP_ERROR;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  hipLaunchKernelGGL(peak_mfma_f64_kernel, dim3(blocks), dim3(256), 0, 0, out, 16);
  (void)hipEventRecord(e0, 0);
  hipLaunchKernelGGL(peak_mfma_f64_kernel, dim3(blocks), dim3(256), 0, 0, out, iters);
  (void)hipEventRecord(e1, 0);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double flops = (double)blocks * 4 /*waves*/ * (double)iters * 4 * 2048.0;
  *tflops = flops / (ms * 1e-3) / 1e12;
  (void)hipFree(out);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return LMGPU_OK;
}

// tflops: the sustained rate of the loop; sclk_mhz: the median in-kernel shader clock while it ran (after ~1 s of back-to-back
// launches so that the power state has settled); flop_per_clk_simd = tflops / (SIMDs x clock): 32 = one v_mfma_f64_16x16x4_f64
// (2048 flop) per 64 cycles and SIMD, the rate the 78.6 TFLOP/s datasheet figure assumes AT 2.4 GHz.
int lmgpu_peak_mfma_f64_clock(int32_t device, int32_t iters, int32_t n_acc, double* tflops, double* sclk_mhz, double* flop_per_clk_simd) {
  if (hipSetDevice(device) != hipSuccess || (n_acc != 4 && n_acc != 8 && n_acc != 16) || !tflops || !sclk_mhz) return LMGPU_HIP_ERROR;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return LMGPU_HIP_ERROR;
  const int cus = prop.multiProcessorCount;
  const int blocks = cus * (n_acc == 16 ? 2 : 8);  // 16 accumulators: two workgroups per CU, the occupancy of the update tile
  double* out = nullptr;
  unsigned long long* stamps = nullptr;
  if (hipMalloc((void**)&out, (size_t)blocks * 256 * sizeof(double)) != hipSuccess) return LMGPU_HIP_ERROR;
  if (hipMalloc((void**)&stamps, (size_t)blocks * 2 * sizeof(unsigned long long)) != hipSuccess) return LMGPU_HIP_ERROR;
  auto launch = [&](int it) {
    if (n_acc == 16) hipLaunchKernelGGL(peak_mfma_f64_clock_kernel16, dim3(blocks), dim3(256), 0, 0, out, stamps, 4 * it);
    else if (n_acc == 4) hipLaunchKernelGGL(peak_mfma_f64_clock_kernel4, dim3(blocks), dim3(256), 0, 0, out, stamps, it);
    else hipLaunchKernelGGL(peak_mfma_f64_clock_kernel8, dim3(blocks), dim3(256), 0, 0, out, stamps, it);
  };
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  launch(iters);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0, 0);
  launch(iters);
  (void)hipEventRecord(e1, 0);
  (void)hipEventSynchronize(e1);
  float ms1 = 0;
  (void)hipEventElapsedTime(&ms1, e0, e1);
  const int reps = std::max(1, std::min(400, (int)(1000.0 / std::max(0.05f, ms1))));  // ~1 s of back-to-back launches
  for (int r = 0; r < reps; r++) launch(iters);
  (void)hipEventRecord(e0, 0);
  launch(iters);
  (void)hipEventRecord(e1, 0);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> h((size_t)blocks * 2);
  (void)hipMemcpy(h.data(), stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  std::vector<double> clk;
  for (int b = 0; b < blocks; b++)
    if (h[2 * b + 1] > 0) clk.push_back((double)h[2 * b] / (double)h[2 * b + 1] * 100.0);
  std::sort(clk.begin(), clk.end());
  *sclk_mhz = clk.empty() ? 0.0 : clk[clk.size() / 2];
  const double flops = (double)blocks * 4 /*waves*/ * (double)iters * n_acc * 2048.0;  // (the 16-accumulator kernel is launched with 4 x iters and steps its loop by 4)
  *tflops = flops / (ms * 1e-3) / 1e12;
  if (flop_per_clk_simd) *flop_per_clk_simd = (*sclk_mhz > 0) ? (*tflops * 1e12) / ((double)cus * 4 * *sclk_mhz * 1e6) : 0.0;
  (void)hipFree(out);
  (void)hipFree(stamps);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return LMGPU_OK;
}

int lmgpu_peak_hbm_copy(int32_t device, int64_t bytes, int32_t iters, double* gbps) {
  if (hipSetDevice(device) != hipSuccess) return LMGPU_HIP_ERROR;
  float4 *a = nullptr, *b = nullptr;
  if (hipMalloc((void**)&a, bytes) != hipSuccess || hipMalloc((void**)&b, bytes) != hipSuccess) return LMGPU_HIP_ERROR;
  (void)hipMemset(a, 1, bytes);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  const size_t n = bytes / 16;
  hipLaunchKernelGGL(peak_copy_kernel, dim3(2048), dim3(256), 0, 0, a, b, n);
  (void)hipEventRecord(e0, 0);
  for (int i = 0; i < iters; i++) hipLaunchKernelGGL(peak_copy_kernel, dim3(2048), dim3(256), 0, 0, a, b, n);
  (void)hipEventRecord(e1, 0);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  *gbps = 2.0 * (double)bytes * iters / (ms * 1e-3) / 1e9;
  (void)hipFree(a);
  (void)hipFree(b);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return LMGPU_OK;
}

}  // extern "C"

#include "isam2.hpp"
#include "init_pose3.hpp"
#include "translation_recovery.hpp"
#include "mfas.hpp"
#include "ncg.hpp"
#include "triangulation.hpp"
#include "marginals.hpp"
#include "isam2_marginals.hpp"  // (after both: ISAM2's handle and staging, the batch route's chunking constants)
#include "smart.hpp"

#ifdef LDSF_STAMPS  // development aid: tools/ldsf_phases.py
extern "C" int lmgpu_debug_ldsf(unsigned long long* out16, int reset) {
  if (reset) {
    unsigned long long z[16] = {0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(lmgpu::ldsf_dbg), z, sizeof(z));
  }
  return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(lmgpu::ldsf_dbg), 16 * sizeof(unsigned long long));
}
#endif
