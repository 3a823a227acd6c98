// Host side of the front kernels' launches, shared by the batch path (do_eliminate / do_backsub in lmgpu.hip) and ISAM2 (isam2.hpp):
// one view of the device tables, one launcher per kernel family, and the executor that runs a dense front's schedule
// (dense_schedule.hpp) record by record.  Host only.  Part of lmgpu.hip's translation unit: included behind the kernel headers and the
// host constants (kLdsLimitN, kSyrkLds, NBO), KTimer and LevelWork.
//
// A launcher is the only place outside kernels_*.hpp that names its kernel in a launch.  WHICH variant, thread count and LDS size a
// launch gets is decided by the caller and handed in: the batch path's bin rules and ISAM2's rules differ, each stays with its caller.
#pragma once

// the tables the front kernels walk, in device memory.  The batch handle fills one at the end of upload_launch_tables; ISAM2 one per
// elimination, from its staging arena (is_stage_front_tables).
struct FrontTablesDev {
  const FrontDesc* fds = nullptr;
  const FrontFac* ffac = nullptr;
  const FacDesc* fd = nullptr;
  const ChildRef* childs = nullptr;
  const int32_t *cmap = nullptr, *fxoff = nullptr, *sxoff = nullptr, *list = nullptr, *rowptr = nullptr;
  const RowSrc* rowsrc = nullptr;
};

// lambda by value (eager) or in device memory (graph replay), the damping weights and the extra gradient vector of a solve with a
// prescribed right-hand side (or null).  ISAM2 eliminates undamped: {0.0, nullptr, ones, nullptr}.
struct Damping {
  double lambda_v;
  const double* lambda_p;
  const double* dampw;
  const double* gex;
};

// largest dynamic LDS size of every front kernel (lmgpu_create, lmgpu_isam2_create); the first error, if any
static hipError_t front_kernels_set_attributes() {
  const int front = kLdsLimitN * kLdsLimitN * 8 + kLdsFrontExtra + 64, backsub = (kLdsLimitN * kLdsLimitN + LDSB_TAIL) * 8;
  const struct {
    const void* fn;
    int bytes;
  } table[] = {{(const void*)lds_front_kernel<false>, front},
               {(const void*)lds_front_kernel<false, 1024>, front},
               {(const void*)lds_front_kernel<true>, front},
               {(const void*)lds_front_merged_kernel<256>, front},
               {(const void*)lds_front_merged_kernel<1024>, front},
               {(const void*)level_fused_kernel<256>, front},
               {(const void*)level_fused_kernel<1024>, front},
               {(const void*)syrk_mfma_kernel, kSyrkLds},
               {(const void*)lds_backsub_wide_kernel, backsub},
               {(const void*)lds_backsub_merged_kernel, backsub},
               {(const void*)diag_potrf_kernel, DIAG_LDS_BYTES},
               {(const void*)panel_dataflow_kernel, PDF_LDS_BYTES},
               {(const void*)step_kernel, STEP_LDS_BYTES},
               {(const void*)chain_kernel, STEP_LDS_BYTES},
#ifdef LMGPU_TEST_HOOKS
               {(const void*)front_tail_scalar_kernel, TAIL_LDS_BYTES},
#endif
               {(const void*)med_diag_potrf_kernel, DIAG_LDS_BYTES}};
  for (const auto& t : table)
    if (hipError_t e = hipFuncSetAttribute(t.fn, hipFuncAttributeMaxDynamicSharedMemorySize, t.bytes); e != hipSuccess) return e;
  return hipSuccess;
}

// workgroups of chain_kernel the device holds at once: what a chained launch in the resident form starts at most (chain_grid,
// kernels_step.hpp).  Behind front_kernels_set_attributes (the kernel's LDS size is above the default limit).  Correctness does not
// depend on the figure.
static hipError_t chain_resident_blocks(int num_cus, int* out) {
  int per_cu = 0;
  if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)chain_kernel, 256, STEP_LDS_BYTES); e != hipSuccess) return e;
  *out = num_cus * std::max(1, per_cu);
  return hipSuccess;
}

// ---- elimination

// the LDS fronts list[first .. first + count), one workgroup each: four waves (or fewer: `threads`), sixteen waves, or the gather-leaf
// form that keeps only nf rows in LDS.  srows: rows of the front kept in LDS; pack: the launch's packed leaf records (or null)
enum LdsFrontForm { LDS_FRONT_PLAIN, LDS_FRONT_WIDE16, LDS_FRONT_GATHER_LEAF };
static void launch_lds_fronts(hipStream_t s, const FrontTablesDev& D, double* pool, int* status, const Damping& dmp, LdsFrontForm form, int first, int count,
                              int threads, int nmax, int srows, int jcap, double* gcorner, const char* pack, int pack_stride) {
  auto* kernel = form == LDS_FRONT_WIDE16 ? lds_front_kernel<false, 1024> : (form == LDS_FRONT_PLAIN ? lds_front_kernel<false> : lds_front_kernel<true>);
  hipLaunchKernelGGL(kernel, dim3(count), dim3(form == LDS_FRONT_WIDE16 ? 1024 : threads), lds_front_bytes(jcap, srows, nmax), s, D.list + first, D.fds, D.ffac,
                     D.fd, D.childs, D.cmap, D.fxoff, pool, dmp.lambda_v, dmp.lambda_p, dmp.dampw, status, nmax, srows, gcorner, jcap, dmp.gex, pack,
                     pack_stride);
}

// the LDS fronts list[begin .. end) of several levels as ONE dataflow launch; threads == 1024 takes the sixteen-wave kernel.
// relay: the host's pinned status word, which the launch's last workgroup writes (or null)
static void launch_lds_fronts_merged(hipStream_t s, const FrontTablesDev& D, double* pool, int* status, const Damping& dmp, int begin, int end, int threads,
                                     int nmax, int jcap, unsigned int* ticket, int* relay) {
  auto* kernel = threads == 1024 ? lds_front_merged_kernel<1024> : lds_front_merged_kernel<256>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(end - begin)), dim3(threads), lds_front_bytes(jcap, nmax, nmax), s, D.list, begin, end, D.fds, D.ffac, D.fd, D.childs,
                     D.cmap, D.fxoff, pool, dmp.lambda_v, dmp.lambda_p, dmp.dampw, status, nmax, jcap, dmp.gex, ticket, relay);
}

// a level's LDS fronts and medium fronts in one grid
static void launch_level_fused(hipStream_t s, const FrontTablesDev& D, double* pool, int* status, const Damping& dmp, const LevelTask* tasks, int ntasks,
                               unsigned int* ticket, int threads, int nmax, int jcap, MedLevel ML, double* inv16_med, LevelSync* sync) {
  const size_t lds = std::max<size_t>(lds_front_bytes(jcap, nmax, nmax), (size_t)DIAG_LDS_BYTES);
  const bool wide = threads == 1024;
  auto* kernel = wide ? level_fused_kernel<1024> : level_fused_kernel<256>;
  hipLaunchKernelGGL(kernel, dim3(ntasks), dim3(wide ? 1024 : 256), lds, s, tasks, ticket, D.list, D.fds, D.ffac, D.fd, D.childs, D.cmap, D.fxoff, pool,
                     dmp.lambda_v, dmp.lambda_p, dmp.dampw, status, nmax, jcap, dmp.gex, ML, D.rowptr, D.rowsrc, inv16_med, sync);
}

// a bin of gather leaves that all qualify (leaf_group_form): four leaves per wave, one lane per factor.  form: 1 = nf <= 3 and binary
// factors of at most two rows, 2 = the caps; group_out / group_maxfac: the largest nf x n and number of factors among the leaves
static void launch_leaf_groups(hipStream_t s, double* pool, int* status, const Damping& dmp, int form, const char* pack, int pack_stride, int count, int jcap,
                               int group_out, int group_maxfac, int group_threads, double* gcorner) {
  auto* gk = form == 1 ? lds_front_group_kernel<2, LEAFGRP_MAXSEP, 3> : lds_front_group_kernel<LEAFGRP_MAXROWS, LEAFGRP_MAXSEP, LEAFGRP_MAXNF>;
  // LDS per leaf: the staged Jacobians and [R S d]; the second over the first where no lane takes a second factor (kernels_leaf.hpp)
  const int out_off = group_maxfac > LEAFGRP_LANES ? jcap : 0;
  const int lds_leaf = (std::max(jcap, out_off + group_out) + 1) & ~1;
  int gthreads = group_threads;  // (halved until the workgroup's leaves fit 64 KB of LDS)
  while (gthreads > 64 && (size_t)(gthreads / LEAFGRP_LANES) * lds_leaf * sizeof(double) > 65536) gthreads >>= 1;
  const int lpw = gthreads / LEAFGRP_LANES;  // leaves per workgroup
  hipLaunchKernelGGL(gk, dim3((count + lpw - 1) / lpw), dim3(gthreads), (size_t)lpw * lds_leaf * sizeof(double), s, pack, pack_stride, count, pool,
                     dmp.lambda_v, dmp.lambda_p, dmp.dampw, status, gcorner, dmp.gex, lds_leaf, out_off);
}

// the medium fronts of level L: six launches for all of them
static void launch_med_level(hipStream_t s, const FrontTablesDev& D, double* pool, int* status, const Damping& dmp, KTimer& kt, const LevelWork& L, MedLevel ML,
                             double* inv16_med) {
  const unsigned cnt = (unsigned)L.med_count;
  int ktm = kt.begin(LMGPU_KT_HBM_ASSEMBLE, s);
  if (L.med_max_fac > 0 || L.med_max_child > 0)
    hipLaunchKernelGGL(med_assemble_rows_kernel, dim3((L.med_max_n + 3) / 4, cnt), dim3(256), 0, s, ML, D.rowptr, D.rowsrc, D.childs, D.cmap, D.ffac, D.fd, pool,
                       D.fxoff, dmp.lambda_v, dmp.lambda_p, dmp.dampw, dmp.gex);
  else  // (the row-owner assembly damps its own rows)
    hipLaunchKernelGGL(med_damp_kernel, dim3((L.med_max_nf + 255) / 256, cnt), dim3(256), 0, s, ML, D.fxoff, pool, dmp.lambda_v, dmp.lambda_p, dmp.dampw,
                       dmp.gex);
  kt.end(ktm, s);
  ktm = kt.begin(LMGPU_KT_PANEL, s);
  hipLaunchKernelGGL(med_diag_potrf_kernel, dim3(cnt), dim3(256), DIAG_LDS_BYTES, s, ML, pool, status, inv16_med);
  if (L.med_max_cols > 0)
    hipLaunchKernelGGL(med_panel_trsm_kernel, dim3((L.med_max_cols + 63) / 64, cnt), dim3(256), 0, s, ML, pool, (const double*)inv16_med);
  kt.end(ktm, s);
  if (L.med_max_cols > 0) {
    const int S = (L.med_max_cols + 63) / 64;
    ktm = kt.begin(LMGPU_KT_SYRK, s);
    hipLaunchKernelGGL(med_syrk_kernel, dim3(4 * S, S, cnt), dim3(256), 0, s, ML, pool);
    kt.end(ktm, s);
  }
}

// own factors and children's update matrices of HBM front F, assembled at pool offset aoff: one wave per row of the front walks that
// row's sources (its n + 1 row pointers start at D.rowptr + row_begin) in a fixed order (no atomics, bitwise reproducible);
// with_factors = false on the ranks that leave the own terms to rank 0.  dmp (or null): the wave that owns a frontal row also adds that
// row's damping term (and gex) behind the row's last source -- what launch_hbm_damp adds behind this launch, the same additions in the
// same order, without the launch.
static void launch_assemble_rows(hipStream_t s, const FrontTablesDev& D, double* pool, const FrontDesc& F, int64_t aoff, int ld, int row_begin, bool with_factors,
                                 const Damping* dmp) {
  if (dmp)
    hipLaunchKernelGGL(hbm_assemble_rows_damp_kernel, dim3((F.n + 3) / 4), dim3(256), 0, s, F, aoff, ld, D.rowptr + row_begin, D.rowsrc, D.childs, D.cmap, D.ffac,
                       D.fd, pool, with_factors ? 1 : 0, D.fxoff, dmp->lambda_v, dmp->lambda_p, dmp->dampw, dmp->gex);
  else
    hipLaunchKernelGGL(hbm_assemble_rows_kernel, dim3((F.n + 3) / 4), dim3(256), 0, s, F, aoff, ld, D.rowptr + row_begin, D.rowsrc, D.childs, D.cmap, D.ffac, D.fd,
                       pool, with_factors ? 1 : 0);
}
static void launch_hbm_damp(hipStream_t s, const FrontTablesDev& D, double* pool, const FrontDesc& F, int64_t aoff, int ld, const Damping& dmp) {
  hipLaunchKernelGGL(hbm_damp_kernel, dim3((F.nf + 255) / 256), dim3(256), 0, s, F, aoff, ld, D.fxoff, pool, dmp.lambda_v, dmp.lambda_p, dmp.dampw, dmp.gex);
}

// ---- the schedule of one dense front (dense_front_schedule), record by record

struct DenseExec {
  hipStream_t s;
  double* A;          // the n x ld working matrix
  const double* Asm;  // a split front's partial assembly, which the fused and chained launches fold in (else null)
  int ld, n, nf, id;
  int* status;
  double* inv16;        // 16 x (16 x 16) inverses of a panel's diagonal tiles: panel i at inv16 + i * inv16_stride
  size_t inv16_stride;  // (0: every panel overwrites the one before; nothing reads them after the front)
  unsigned int* pflags;   // hand-off flags of the dataflow launches, PDF_FLAG_WORDS per panel; null: a schedule without such launches
  bool pflags_prefilled;  // cleared by the caller: no memset in front of panel 0
  const int2* chain_tasks;                   // ticket orders of the DENSE_CHAIN records: record r takes
  const int *task_begin, *task_count;        // chain_tasks[task_begin[r] .. + task_count[r])
  KTimer* kt;                                // (or null)
  int chain_forms;                           // test library: CHAIN_FORM_* bits
  bool tail_scalar;                          // test library: front_tail_scalar_kernel
  int chain_resident;                        // workgroups of chain_kernel the device holds at once (chain_resident_blocks, once per handle)
  bool chain_one_task;                       // chained launches with one workgroup per task: always, but in the test library under LMGPU_CHAIN_GRID
  int chain_grid;                            // test library, resident form: the grid of every chained launch (0: chain_grid decides)
};

// chunk(kind, c): the caller's DENSE_ADD_CHUNK / DENSE_WAIT_CHUNK of row chunk c (split fronts only); non-zero ends the run and is returned
template <typename ChunkFn>
static int run_dense_steps(const DenseExec& X, const std::vector<DenseStep>& steps, ChunkFn&& chunk, std::string* err) {
  hipStream_t s = X.s;
  double* A = X.A;
  const int ld = X.ld, n = X.n, nf = X.nf;
  KTimer off;  // (on = false: begin / end do nothing)
  KTimer& kt = X.kt ? *X.kt : off;
  int kt_run = -1, run_launches = 0;  // one event pair around a run of consecutive fused-step launches
  double run_flop = 0;
  for (size_t r = 0; r < steps.size(); r++) {
    const DenseStep& st = steps[r];
    // panel i = rows [k0, r0), m columns behind it (panel records only)
    const int i = st.i, k0 = i * NBO, kb = std::min(nf, k0 + NBO) - k0, r0 = k0 + kb, m = n - r0;
    // the wait of a fused step that folds its chunk in itself stays inside the run; everything else is timed on its own
    const bool in_run = st.kind == DENSE_STEP_FUSED || (st.kind == DENSE_WAIT_CHUNK && steps[r + 1].kind == DENSE_STEP_FUSED);
    if (!in_run && run_launches > 0) {
      kt.end(kt_run, s, run_flop, run_launches);
      run_launches = 0;
      run_flop = 0;
    }
    switch (st.kind) {
      case DENSE_PANEL_DATAFLOW:
      case DENSE_PANEL_TWO_LAUNCH: {
        if (i == 0 && X.pflags && !X.pflags_prefilled)
          if (hipError_t e = hipMemsetAsync(X.pflags, 0, (size_t)((nf + NBO - 1) / NBO + 1) * PDF_FLAG_WORDS * sizeof(unsigned int), s); e != hipSuccess) {
            *err = std::string("hipMemsetAsync(panel flags): ") + hipGetErrorString(e);
            return LMGPU_HIP_ERROR;
          }
        double* inv16 = X.inv16 + (size_t)i * X.inv16_stride;
        const int ktp = kt.begin(LMGPU_KT_PANEL, s);
        if (st.kind == DENSE_PANEL_DATAFLOW) {
          hipLaunchKernelGGL(panel_dataflow_kernel, dim3(kb / 64 + (m + 63) / 64), dim3(256), PDF_LDS_BYTES, s, A, ld, n, nf, k0, kb, X.id, X.status, inv16,
                             X.pflags + (size_t)i * PDF_FLAG_WORDS);
        } else {
          hipLaunchKernelGGL(diag_potrf_kernel, dim3(1), dim3(256), DIAG_LDS_BYTES, s, A, ld, nf, k0, kb, X.id, X.status, inv16);
          if (m > 0) hipLaunchKernelGGL(panel_trsm_kernel, dim3((m + 63) / 64), dim3(256), 0, s, A, ld, n, k0, kb, (const double*)inv16);
        }
        kt.end(ktp, s, st.flop);
        break;
      }
      case DENSE_CHAIN: {  // (a split front: behind the wait for the last row chunk the launch folds in)
        ChainArgs ca{A, ld, n, nf, i, st.nsteps, X.id, X.status, X.inv16, X.pflags, X.chain_tasks + X.task_begin[r], X.Asm, X.task_count[r],
                     X.chain_one_task ? 1 : 0};
#ifdef LMGPU_TEST_HOOKS
        ca.dev_forms = X.chain_forms;
#endif
        const int ktc = kt.begin(LMGPU_KT_CHAIN, s);
        hipLaunchKernelGGL(chain_kernel, dim3(chain_grid(X.task_count[r], X.chain_resident, X.chain_one_task, X.chain_grid)), dim3(256), STEP_LDS_BYTES, s, ca);
        kt.end(ktc, s, st.flop, 1);
        break;
      }
      case DENSE_STEP_FUSED: {  // (a split front: behind the wait for the chunk of panel i + 1, which its head tiles fold in)
        const int kbn = std::min(nf, r0 + NBO) - r0;
        StepArgs a{A, ld, n, nf, k0, kb, kbn, X.id, X.status, X.inv16 + (size_t)(i + 1) * X.inv16_stride, X.pflags + (size_t)(i + 1) * PDF_FLAG_WORDS, X.Asm};
#ifdef LMGPU_TEST_HOOKS
        a.dev_forms = X.chain_forms;
#endif
        if (run_launches == 0) kt_run = kt.begin(LMGPU_KT_SYRK, s);
        hipLaunchKernelGGL(step_kernel, dim3(step_grid(m, kbn)), dim3(256), STEP_LDS_BYTES, s, a);
        run_launches++;
        run_flop += st.flop;
        break;
      }
      case DENSE_UPDATE_QUADRANTS:
      case DENSE_UPDATE_MFMA: {
        const int kts = kt.begin(LMGPU_KT_SYRK, s);
        if (st.kind == DENSE_UPDATE_QUADRANTS) {
          const int S = (m + 63) / 64;
          hipLaunchKernelGGL(syrk_quadrants_kernel, dim3(4 * S, S), dim3(256), 0, s, A, ld, n, k0, kb, r0);
        } else {
          const int T = (m + 127) / 128;
          hipLaunchKernelGGL(syrk_mfma_kernel, dim3(T, T), dim3(256), kSyrkLds, s, A, ld, n, k0, kb, r0, n);
        }
        kt.end(kts, s, st.flop);
        break;
      }
      case DENSE_TAIL: {
        const int ktt = kt.begin(LMGPU_KT_PANEL, s);
#ifdef LMGPU_TEST_HOOKS
        if (X.tail_scalar)
          hipLaunchKernelGGL(front_tail_scalar_kernel, dim3(1), dim3(256), TAIL_LDS_BYTES, s, A, ld, n, nf, k0, kb, X.id, X.status,
                             X.inv16 + (size_t)(i + 1) * X.inv16_stride);
        else
#endif
        hipLaunchKernelGGL(front_tail_kernel, dim3(1), dim3(256), 0, s, A, ld, n, nf, k0, kb, X.id, X.status, X.inv16 + (size_t)(i + 1) * X.inv16_stride);
        kt.end(ktt, s, st.flop);
        break;
      }
      case DENSE_ADD_CHUNK:
      case DENSE_WAIT_CHUNK: {
        const int rcc = chunk(st.kind, st.chunk);
        if (rcc) return rcc;
        break;
      }
    }
  }
  if (run_launches > 0) kt.end(kt_run, s, run_flop, run_launches);
  return LMGPU_OK;
}

// ---- back-substitution

// one launch over LDS fronts: the fronts list[begin .. begin + count) of one level (wide: a workgroup per front with [R S d] staged in
// LDS; the two group forms: four fronts per wave; plain: a wave per front), or -- merged -- list[begin .. begin + count) of several
// levels as one dataflow launch.  rsd_max: doubles of [R S d] the staging forms hold
enum LdsBacksubForm { LDS_BACKSUB_PLAIN, LDS_BACKSUB_GROUP_SMALL, LDS_BACKSUB_GROUP, LDS_BACKSUB_WIDE, LDS_BACKSUB_MERGED };
struct BacksubMergeDev {  // merged form: per front its LDS parent and list position, the done flags, the launch's ticket counter
  const int32_t *parent, *pos;
  unsigned int *done, *ticket;
};
static void launch_lds_backsub(hipStream_t s, const FrontTablesDev& D, const double* pool, double* delta, int* status, LdsBacksubForm form, int begin, int count,
                               int rsd_max, const BacksubMergeDev* M = nullptr) {
  const size_t lds = (size_t)(rsd_max + LDSB_TAIL) * sizeof(double);
  switch (form) {
    case LDS_BACKSUB_WIDE:
      hipLaunchKernelGGL(lds_backsub_wide_kernel, dim3(count), dim3(256), lds, s, D.list + begin, count, D.fds, D.fxoff, D.sxoff, pool, delta, status);
      break;
    case LDS_BACKSUB_GROUP_SMALL:
    case LDS_BACKSUB_GROUP: {  // every front of the launch: four fronts per wave, 16 lanes each
      auto* gk = form == LDS_BACKSUB_GROUP_SMALL ? lds_backsub_group_kernel<3, 6> : lds_backsub_group_kernel<LDSBG_MAXNF, 9>;
      hipLaunchKernelGGL(gk, dim3((count + 15) / 16), dim3(256), 0, s, D.list + begin, count, D.fds, D.fxoff, D.sxoff, pool, delta, status);
      break;
    }
    case LDS_BACKSUB_PLAIN:
      hipLaunchKernelGGL(lds_backsub_kernel, dim3((count + 3) / 4), dim3(256), 0, s, D.list + begin, count, D.fds, D.fxoff, D.sxoff, pool, delta, status);
      break;
    case LDS_BACKSUB_MERGED:
      hipLaunchKernelGGL(lds_backsub_merged_kernel, dim3(count), dim3(256), lds, s, D.list, begin, begin + count, D.fds, D.fxoff, D.sxoff, pool, delta, status,
                         M->parent, M->pos, M->done, M->ticket);
      break;
  }
}

// the 64-row blocks of the smaller HBM fronts, one workgroup per block: those of one level (ticket: null when every workgroup is
// resident at once), or of a run of levels (poll: separator values awaited by value)
static void launch_backsolve_blocks(hipStream_t s, const FrontTablesDev& D, const double* pool, double* delta, double* xbuf, int* status, const BsdBlock* blocks,
                                    int count, unsigned int* ticket, int poll) {
  hipLaunchKernelGGL(hbm_backsolve_blocks_kernel, dim3(count), dim3(256), 0, s, blocks, ticket, D.fxoff, D.sxoff, pool, delta, xbuf, status, poll);
}
