// Development microbenchmark (not part of the product): times the dense-front kernels on a synthetic SPD matrix and
// (trailing-update tile at several sizes).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../gtsam_personal_amd/csrc tools/microbench.hip -o tools/microbench
// With -DLMGPU_TEST_HOOKS the kernels carry the test library's hand-off forms as well and   microbench <n> <far_pct> <merge> <forms>
// selects them for the chained launch (CHAIN_FORM_* bits of kernels_step.hpp: 1 = tiles published behind a release fence).
//   microbench <n> <far_pct> <merge> <forms> <one_task 0|1> [grid]   the chained launch as resident workgroups that draw tickets in a
// loop (0, the default; grid: forced, else min(tasks, resident workgroups)) or as one workgroup per task (1).  Stamps are per TASK.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

// phase stamps of the diagonal workgroups: flags[512 + 64 b + 2 slot] (two words per 64-bit s_memrealtime: the 100 MHz
// counter shared by all XCDs, so the stamps of different workgroups lie on one time line)
#define PDF_STAMP(flags, b, slot)                                                                  \
  do {                                                                                             \
    if ((b) < 4 && threadIdx.x == 0) {                                                             \
      unsigned long long t_;                                                                       \
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
      *(unsigned long long*)&(flags)[512 + 64 * (b) + 2 * (slot)] = t_;                            \
    }                                                                                              \
  } while (0)
// where the workgroups of a chained launch spend their time: per class (head quadrants, head 64-tiles, diagonal, update tiles, row-panel)
// [count, ticks waiting for inputs, ticks working] + slot-time per 100 us bucket of the launch (100 MHz realtime counter)
// + the publish segment per class: g_pub[3 cls] = workgroups with a stamp, [3 cls + 1] = ticks from thread 0's last C store to the end
// of the publish; g_fence[3 cls] = release fences, [3 cls + 1] = the signaller's ticks inside them (fence + its wait)
__device__ unsigned long long g_prof[16], g_hist[256], g_t0, g_begin[1 << 17], g_waited[1 << 17];
__device__ unsigned long long g_pub[16], g_fence[16], g_stored[1 << 17], g_fence_n[1 << 17], g_fence_t[1 << 17], g_fence_b[1 << 17];
// per TASK (ticket): start (ticket drawn), inputs there, end, and the workgroup that ran it; g_ticket: the workgroup's current ticket
#define PROF_MAX_TASKS (1 << 17)
__device__ unsigned long long g_tb[PROF_MAX_TASKS], g_tw[PROF_MAX_TASKS], g_te[PROF_MAX_TASKS];
__device__ unsigned int g_twg[PROF_MAX_TASKS], g_ticket[1 << 17];
__device__ __forceinline__ unsigned long long prof_now() {
  unsigned long long t_;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
  return t_;
}
#define CHAIN_PROF_BEGIN(ticket)                            \
  do {                                                      \
    if (threadIdx.x == 0) {                                 \
      g_begin[blockIdx.x] = prof_now();                     \
      g_ticket[blockIdx.x] = (unsigned int)(ticket);        \
      g_waited[blockIdx.x] = 0;                             \
      g_stored[blockIdx.x] = 0;                             \
      g_fence_n[blockIdx.x] = 0;                            \
      g_fence_t[blockIdx.x] = 0;                            \
      atomicMin(&g_t0, g_begin[blockIdx.x]);                \
    }                                                       \
  } while (0)
#define CHAIN_PROF_WAITED()                                 \
  do {                                                      \
    if (threadIdx.x == 0) g_waited[blockIdx.x] = prof_now(); \
  } while (0)
#define CHAIN_PROF_STORED()                                 \
  do {                                                      \
    if (threadIdx.x == 0) g_stored[blockIdx.x] = prof_now(); \
  } while (0)
/* inside `if (signaller)`: one thread of the workgroup */
#define PDF_PROF_FENCE_BEGIN() g_fence_b[blockIdx.x] = prof_now()
#define PDF_PROF_FENCE_END()                                   \
  do {                                                         \
    g_fence_t[blockIdx.x] += prof_now() - g_fence_b[blockIdx.x]; \
    g_fence_n[blockIdx.x] += 1;                                \
  } while (0)
#define CHAIN_PROF_END(cls)                                                              \
  do {                                                                                   \
    __syncthreads();                                                                     \
    if (threadIdx.x == 0 && g_begin[blockIdx.x] != 0) { /* chained launches only */      \
      const unsigned long long e_ = prof_now(), b_ = g_begin[blockIdx.x];                \
      g_begin[blockIdx.x] = 0;                                                           \
      const unsigned long long w_ = g_waited[blockIdx.x] ? g_waited[blockIdx.x] : b_;    \
      const unsigned int k_ = g_ticket[blockIdx.x];                                      \
      if (k_ < PROF_MAX_TASKS) {                                                         \
        g_tb[k_] = b_;                                                                   \
        g_tw[k_] = w_;                                                                   \
        g_te[k_] = e_;                                                                   \
        g_twg[k_] = blockIdx.x;                                                          \
      }                                                                                  \
      atomicAdd(&g_prof[3 * (cls)], 1ull);                                               \
      atomicAdd(&g_prof[3 * (cls) + 1], w_ - b_);                                        \
      atomicAdd(&g_prof[3 * (cls) + 2], e_ - w_);                                        \
      if (g_stored[blockIdx.x]) {                                                        \
        atomicAdd(&g_pub[3 * (cls)], 1ull);                                              \
        atomicAdd(&g_pub[3 * (cls) + 1], e_ - g_stored[blockIdx.x]);                     \
      }                                                                                  \
      atomicAdd(&g_fence[3 * (cls)], g_fence_n[blockIdx.x]);                             \
      atomicAdd(&g_fence[3 * (cls) + 1], g_fence_t[blockIdx.x]);                         \
      const unsigned long long t0_ = g_t0;                                               \
      int it_ = 0;                                                                       \
      for (unsigned long long x_ = w_ - t0_; x_ < e_ - t0_ && it_ < 300; it_++) {        \
        const unsigned long long nb_ = (x_ / 10000 + 1) * 10000;                         \
        const unsigned long long y_ = nb_ < e_ - t0_ ? nb_ : e_ - t0_;                   \
        if (x_ / 10000 < 256) atomicAdd(&g_hist[x_ / 10000], y_ - x_);                   \
        x_ = y_;                                                                         \
      }                                                                                  \
    }                                                                                    \
  } while (0)
#include "kernels_dense.hpp"
#include "kernels_potrf.hpp"
#include "kernels_step.hpp"

using namespace lmgpu;

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e = (x);                                                         \
    if (e != hipSuccess) {                                                      \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

static void fill_spd(std::vector<double>& h, int n, int ld) {
  // diagonally dominant SPD: A = 0.01 * (random symmetric) + n * I   (upper triangle used)
  srand(1);
  for (int i = 0; i < n; i++)
    for (int j = i; j < n; j++) h[(size_t)i * ld + j] = (i == j) ? (double)n : 0.01 * ((rand() % 2001) / 1000.0 - 1.0);
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 9001;
  const int ld = (n + 15) & ~15;
  std::vector<double> h((size_t)n * ld + 1024, 0.0);
  fill_spd(h, n, ld);
  double* A;
  CK(hipMalloc((void**)&A, h.size() * sizeof(double)));
  unsigned long long* st;
  CK(hipMalloc((void**)&st, 64 * sizeof(unsigned long long)));
  int* status;
  CK(hipMalloc((void**)&status, sizeof(int)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int kSyrkLds = 2 * 2 * SYRK_KC * SYRK_LDW * 8;
  CK(hipFuncSetAttribute((const void*)syrk_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSyrkLds));
  auto reset = [&]() { CK(hipMemcpy(A, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice)); };
  auto timeit = [&](const char* name, int reps, auto&& fn) {
    float best = 1e30f, tot = 0;
    for (int r = 0; r < reps; r++) {
      reset();
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0, 0));
      fn();
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      best = ms < best ? ms : best;
      tot += ms;
    }
    printf("%-44s best %9.1f us   avg %9.1f us\n", name, best * 1e3, tot / reps * 1e3);
  };
  const bool chain_only = argc > 3;  // microbench <n> <far_pct> <merge 0|1>: only the chained launch
  // 1. one outer panel as a dataflow launch: duration and the phase stamps of the four diagonal workgroups
  if (!chain_only) {
    unsigned int* flags;
    double* inv16;
    CK(hipMalloc((void**)&flags, PDF_FLAG_WORDS * 4));
    CK(hipMalloc((void**)&inv16, 16 * 256 * 8));
    CK(hipFuncSetAttribute((const void*)panel_dataflow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PDF_LDS_BYTES));
    for (int k0 : {0, 4352}) {
      const int cols = n - k0 - 256, grid = 4 + (cols + 63) / 64;
      float best = 1e30f;
      std::vector<unsigned int> hf(PDF_FLAG_WORDS);
      for (int rep = 0; rep < 3; rep++) {
        reset();
        CK(hipMemset(flags, 0, PDF_FLAG_WORDS * 4));
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(panel_dataflow_kernel, dim3(grid), dim3(256), PDF_LDS_BYTES, 0, A, ld, n, n - 1, k0, 256, 0, status, inv16, flags);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        best = ms < best ? ms : best;
      }
      CK(hipMemcpy(hf.data(), flags, PDF_FLAG_WORDS * 4, hipMemcpyDeviceToHost));
      printf("panel_dataflow k0=%d grid=%d: %.1f us\n", k0, grid, best * 1e3);
      auto st = [&](int b, int slot) { return *(unsigned long long*)&hf[512 + 64 * b + 2 * slot]; };
      const char* names[24] = {"start", "w0", "x0", "p0", "u0", "w1", "x1", "p1", "u1", "w2", "x2", "p2", "u2", "w3", "x3", "p3", "u3", "", "", "",
                               "gathered", "potrf", "stored", "published"};
      for (int b = 0; b < 4; b++) {
        printf("  wg %d (us from its own start; the counters of different XCDs are not aligned):", b);
        const unsigned long long t0 = st(b, 0);
        for (int slot = 1; slot < 24; slot++) {
          const unsigned long long t = st(b, slot);
          if (t) printf(" %s=%.1f", names[slot], (double)(long long)(t - t0) / 100.0);  // 100 MHz
        }
        printf("\n");
      }
    }
  }
  // 2. the fused step launch (update with panel at p0 + factorisation of the next panel) with the same stamps
  if (!chain_only) {
    unsigned int* flags;
    double* inv16;
    CK(hipMalloc((void**)&flags, PDF_FLAG_WORDS * 4));
    CK(hipMalloc((void**)&inv16, 16 * 256 * 8));
    CK(hipFuncSetAttribute((const void*)step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, STEP_LDS_BYTES));
    for (int p0 : {0, 4352, 6400}) {
      if (p0 + 512 >= n) continue;
      const int r0 = p0 + 256, m = n - r0, kbn = 256;
      const int grid = step_grid(m, kbn);
      float best = 1e30f;
      std::vector<unsigned int> hf(PDF_FLAG_WORDS);
      for (int rep = 0; rep < 3; rep++) {
        reset();
        CK(hipMemset(flags, 0, PDF_FLAG_WORDS * 4));
        CK(hipDeviceSynchronize());
        StepArgs a{A, ld, n, n - 1, p0, 256, kbn, 0, status, inv16, flags, nullptr};
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(step_kernel, dim3(grid), dim3(256), STEP_LDS_BYTES, 0, a);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        best = ms < best ? ms : best;
      }
      CK(hipMemcpy(hf.data(), flags, PDF_FLAG_WORDS * 4, hipMemcpyDeviceToHost));
      printf("step_kernel p0=%d m=%d grid=%d: %.1f us (%.1f TFLOP/s)\n", p0, m, grid, best * 1e3, 256.0 * m * (m + 1) / (best * 1e-3) / 1e12);
      auto st = [&](int b, int slot) { return *(unsigned long long*)&hf[512 + 64 * b + 2 * slot]; };
      const char* names[24] = {"start", "w0", "x0", "p0", "u0", "w1", "x1", "p1", "u1", "w2", "x2", "p2", "u2", "w3", "x3", "p3", "u3", "", "", "",
                               "gathered", "potrf", "stored", "published"};
      names[0] = "rows ready";
      for (int b = 0; b < 4; b++) {
        printf("  wg %d (us from its own entry):", b);
        const unsigned long long t0 = st(b, 19);
        for (int slot = 0; slot < 24; slot++) {
          if (slot == 19) continue;
          const unsigned long long t = st(b, slot);
          if (t) printf(" %s=%.1f", names[slot], (double)(long long)(t - t0) / 100.0);  // 100 MHz
        }
        printf("\n");
      }
    }
  }
  // 2b. all fused steps of the matrix as ONE chained launch: total time and the time line of the diagonal workgroups per step
  {
    const int np = (n - 1 + 255) / 256;  // nf = n - 1
    unsigned int* flags;
    double* inv16;
    CK(hipMalloc((void**)&flags, (size_t)(np + 2) * PDF_FLAG_WORDS * 4));
    CK(hipMalloc((void**)&inv16, (size_t)(np + 1) * 16 * 256 * 8));
    CK(hipFuncSetAttribute((const void*)chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, STEP_LDS_BYTES));
    CK(hipFuncSetAttribute((const void*)panel_dataflow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PDF_LDS_BYTES));
    auto rows_of = [&](int i) { return std::min(n - 1, (i + 1) * 256) - i * 256; };
    const bool one_task = argc > 5 && atoi(argv[5]) != 0;
    const int forced_grid = argc > 6 ? atoi(argv[6]) : 0;
    int num_cus = 0, per_cu = 0;
    {
      hipDeviceProp_t prop;
      CK(hipGetDeviceProperties(&prop, 0));
      num_cus = prop.multiProcessorCount;
      CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)chain_kernel, 256, STEP_LDS_BYTES));
    }
    const int resident = num_cus * std::max(1, per_cu);
    for (int first : {0, 17}) {
      int nsteps = 0;
      while (first + nsteps + 1 < np && rows_of(first + nsteps) == 256 && rows_of(first + nsteps + 1) % 64 == 0 && n - (first + nsteps + 1) * 256 > 0) nsteps++;
      const std::vector<int2> tasks = chain_schedule(n, n - 1, first, nsteps, argc > 2 ? atoi(argv[2]) : 50, argc > 3 ? atoi(argv[3]) != 0 : true);
      int2* d_tasks;
      CK(hipMalloc((void**)&d_tasks, tasks.size() * sizeof(int2)));
      CK(hipMemcpy(d_tasks, tasks.data(), tasks.size() * sizeof(int2), hipMemcpyHostToDevice));
      ChainArgs ca{A, ld, n, n - 1, first, nsteps, 0, status, inv16, flags, d_tasks, nullptr, (int)tasks.size(), one_task ? 1 : 0};
      if (tasks.size() > PROF_MAX_TASKS) {
        printf("more than %d tasks: no per-task stamps\n", PROF_MAX_TASKS);
        return 1;
      }
      const int grid = chain_grid((int)tasks.size(), resident, one_task, forced_grid);
#ifdef LMGPU_TEST_HOOKS
      ca.dev_forms = argc > 4 ? atoi(argv[4]) : 0;
      printf("hand-off forms %d\n", ca.dev_forms);
#endif
      reset();
      CK(hipMemset(flags, 0, (size_t)(np + 2) * PDF_FLAG_WORDS * 4));
      // panel `first` must be factored for the first step (its trailing data are whatever the matrix holds: timing only)
      hipLaunchKernelGGL(panel_dataflow_kernel, dim3(4 + (n - first * 256 - 256 + 63) / 64), dim3(256), PDF_LDS_BYTES, 0, A, ld, n, n - 1, first * 256, 256,
                         0, status, inv16, flags + (size_t)first * PDF_FLAG_WORDS);
      CK(hipDeviceSynchronize());
      {
        std::vector<unsigned long long> z(256, 0);
        const unsigned long long big = ~0ull;
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z.data(), 16 * 8));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_hist), z.data(), 256 * 8));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_pub), z.data(), 16 * 8));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_fence), z.data(), 16 * 8));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_t0), &big, 8));
      }
      CK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(chain_kernel, dim3(grid), dim3(256), STEP_LDS_BYTES, 0, ca);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      printf("chain_kernel steps %d..%d (%d tasks, %s, grid %d, %d workgroups resident = %d CUs x %d): %.1f us\n", first, first + ca.nsteps - 1,
             (int)tasks.size(), one_task ? "one task per workgroup" : "resident workgroups draw tickets in a loop", grid, resident, num_cus, per_cu, ms * 1e3);
      std::vector<unsigned int> hf((size_t)(np + 2) * PDF_FLAG_WORDS);
      CK(hipMemcpy(hf.data(), flags, hf.size() * 4, hipMemcpyDeviceToHost));
      auto st = [&](int region, int b, int slot) { return *(unsigned long long*)&hf[(size_t)region * PDF_FLAG_WORDS + 512 + 64 * b + 2 * slot]; };
      const unsigned long long t0 = st(first + 1, 0, 19);
      {
        unsigned long long pr[16], hi[256], pb[16], fe[16];
        CK(hipMemcpyFromSymbol(pr, HIP_SYMBOL(g_prof), 16 * 8));
        CK(hipMemcpyFromSymbol(pb, HIP_SYMBOL(g_pub), 16 * 8));
        CK(hipMemcpyFromSymbol(fe, HIP_SYMBOL(g_fence), 16 * 8));
        CK(hipMemcpyFromSymbol(hi, HIP_SYMBOL(g_hist), 256 * 8));
        const char* cn[5] = {"head quadrants", "head 64-tiles", "diagonal", "update tiles", "row-panel"};
        double tot_work = 0;
        for (int c = 0; c < 5; c++) {
          printf("  class %-14s: %6llu workgroups, waiting %9.1f us, working %10.1f us (avg %6.1f us each)\n", cn[c], pr[3 * c], pr[3 * c + 1] / 100.0,
                 pr[3 * c + 2] / 100.0, pr[3 * c] ? pr[3 * c + 2] / 100.0 / pr[3 * c] : 0.0);
          tot_work += pr[3 * c + 2] / 100.0;
        }
        // the publish segment of the tile roles (last C store of thread 0 -> publish done: drain, barrier, [release fence,] flag add) and the
        // release fences of every class (the signaller's time in fence + wait)
        for (int c = 0; c < 5; c++)
          printf("  class %-14s: publish %6llu x avg %5.2f us = %8.1f us of slot-time | release fences %6llu x avg %5.2f us = %8.1f us\n", cn[c], pb[3 * c],
                 pb[3 * c] ? pb[3 * c + 1] / 100.0 / pb[3 * c] : 0.0, pb[3 * c + 1] / 100.0, fe[3 * c], fe[3 * c] ? fe[3 * c + 1] / 100.0 / fe[3 * c] : 0.0,
                 fe[3 * c + 1] / 100.0);
        printf("  slot occupancy (working workgroup-time / (%d slots x launch time)): %.3f\n", resident, tot_work / ((double)resident * ms * 1e3));
        printf("  working slots per 100 us bucket (of %d):", resident);
        for (int b = 0; b < 256 && b * 100.0 < ms * 1e3; b++) printf(" %d", (int)(hi[b] / 10000.0 + 0.5));
        printf("\n");
      }
      {
        // Slot-time per TASK, split at the moment the ticket list is exhausted (the last ticket drawn).  A slot = one of the `resident`
        // workgroup places of the device.  in task = ticket drawn .. end of the task (waiting for inputs + working); between tasks =
        // end of a task .. next ticket drawn by the SAME workgroup (barrier, ticket atomic; resident form only); empty = the rest:
        // no workgroup in the slot, or one that has not drawn its first ticket yet (one-task form: the turnover of the slot).
        const size_t nt = tasks.size();
        std::vector<unsigned long long> tb(nt), tw(nt), te(nt);
        std::vector<unsigned int> twg(nt);
        CK(hipMemcpyFromSymbol(tb.data(), HIP_SYMBOL(g_tb), nt * 8));
        CK(hipMemcpyFromSymbol(tw.data(), HIP_SYMBOL(g_tw), nt * 8));
        CK(hipMemcpyFromSymbol(te.data(), HIP_SYMBOL(g_te), nt * 8));
        CK(hipMemcpyFromSymbol(twg.data(), HIP_SYMBOL(g_twg), nt * 4));
        unsigned long long k0 = ~0ull, kx = 0, kend = 0;
        for (size_t k = 0; k < nt; k++) k0 = std::min(k0, tb[k]), kx = std::max(kx, tb[k]), kend = std::max(kend, te[k]);
        auto part = [](unsigned long long a, unsigned long long b, unsigned long long lo, unsigned long long hi) {
          const unsigned long long x = std::max(a, lo), y = std::min(b, hi);
          return y > x ? (double)(y - x) : 0.0;
        };
        double wait[2] = {0, 0}, work[2] = {0, 0}, gap[2] = {0, 0};
        for (size_t k = 0; k < nt; k++) {
          wait[0] += part(tb[k], tw[k], k0, kx), wait[1] += part(tb[k], tw[k], kx, kend);
          work[0] += part(tw[k], te[k], k0, kx), work[1] += part(tw[k], te[k], kx, kend);
        }
        std::vector<size_t> order(nt);
        for (size_t k = 0; k < nt; k++) order[k] = k;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return twg[a] != twg[b] ? twg[a] < twg[b] : tb[a] < tb[b]; });
        size_t ngaps = 0;
        for (size_t q = 1; q < nt; q++)
          if (twg[order[q]] == twg[order[q - 1]]) {
            gap[0] += part(te[order[q - 1]], tb[order[q]], k0, kx), gap[1] += part(te[order[q - 1]], tb[order[q]], kx, kend);
            ngaps++;
          }
        printf("  ticket list exhausted at %.1f us of %.1f us (first ticket drawn = 0)\n", (kx - k0) / 100.0, (kend - k0) / 100.0);
        for (int h = 0; h < 2; h++) {
          const double total = (double)resident * (double)(h ? kend - kx : kx - k0);
          const double empty = total - wait[h] - work[h] - gap[h];
          printf("  slot-time %s the list is exhausted: %10.1f ms = working %9.1f + waiting %8.1f + between tasks %7.1f + empty %8.1f ms (empty %.1f %%)\n",
                 h ? "AFTER " : "BEFORE", total / 1e5, work[h] / 1e5, wait[h] / 1e5, gap[h] / 1e5, empty / 1e5, total > 0 ? 100.0 * empty / total : 0.0);
        }
        printf("  between tasks of one workgroup: %zu hand-overs, avg %.2f us; empty slot-time before exhaustion per task: %.2f us\n", ngaps,
               ngaps ? (gap[0] + gap[1]) / 100.0 / ngaps : 0.0, ((double)resident * (double)(kx - k0) - wait[0] - work[0] - gap[0]) / 100.0 / nt);
      }
      {  // cadence of the whole chain: when panel s + 1 was complete (last diagonal workgroup published), and the flop done by then
        double prev = 0, flop_acc = 0;
        for (int sidx = 0; sidx < ca.nsteps; sidx++) {
          const int reg = first + sidx + 1;
          const double t = (double)(long long)(st(reg, 3, 23) - t0) / 100.0;
          const double m = n - (first + sidx + 1) * 256;
          flop_acc += 256.0 * m * (m + 1);
          printf("  cadence step %2d m=%5d: panel done at %8.1f us (+%6.1f)   updates of steps <= this one: %6.1f GF = %6.1f us at 44.8 TF\n", first + sidx,
                 (int)m, t, t - prev, flop_acc / 1e9, flop_acc / 44.8e12 * 1e6);
          prev = t;
        }
      }
      for (int sidx = std::max(0, ca.nsteps - 12); sidx < ca.nsteps; sidx++) {
        const int reg = first + sidx + 1;
        auto us = [&](int b, int slot) { return (double)(long long)(st(reg, b, slot) - t0) / 100.0; };
        printf("  step %2d (m=%4d): wg0 entry %.1f rows %.1f gathered %.1f potrf %.1f pub %.1f | wg1 w0 %.1f potrf %.1f pub %.1f | wg2 pub %.1f | wg3 pub %.1f\n",
               first + sidx, n - (first + sidx + 1) * 256, us(0, 19), us(0, 0), us(0, 20), us(0, 21), us(0, 23), us(1, 1), us(1, 21), us(1, 23), us(2, 23),
               us(3, 23));
      }
    }
  }
  if (chain_only) return 0;
  // 3. strip updates (K = 64, <= 192 rows) and big updates (K = 256) at several trailing sizes
  for (int r0 : {64, 4160, 8256}) {
    char nm[128];
    const int r1 = r0 + 192;
    snprintf(nm, sizeof nm, "syrk strip K=64 rows [%d,%d) cols..n", r0, r1);
    timeit(nm, 5, [&]() {
      const int Tr = (r1 - r0 + 127) / 128, Tc = (n - r0 + 127) / 128;
      hipLaunchKernelGGL(syrk_mfma_kernel, dim3(Tc, Tr), dim3(256), kSyrkLds, 0, A, ld, n, r0 - 64, 64, r0, r1);
    });
  }
  for (int r0 : {256, 2304, 4352, 6400, 8448}) {
    char nm[128];
    snprintf(nm, sizeof nm, "syrk big K=256 rows [%d,n)", r0);
    const double m = n - r0;
    float best = 1e30f;
    for (int r = 0; r < 3; r++) {
      reset();
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0, 0));
      const int T = (n - r0 + 127) / 128;
      hipLaunchKernelGGL(syrk_mfma_kernel, dim3(T, T), dim3(256), kSyrkLds, 0, A, ld, n, r0 - 256, 256, r0, n);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      best = ms < best ? ms : best;
    }
    printf("%-44s best %9.1f us   %6.1f TFLOP/s\n", nm, best * 1e3, 256.0 * m * (m + 1) / (best * 1e-3) / 1e12);
  }
  CK(hipGetLastError());
  return 0;
}
