// (no argument) Latency of hbm_backsolve_blocks_kernel on ONE front, the way the upper levels of a SLAM clique tree run it (a few workgroups on an
// otherwise idle device); checked against a plain CPU back-substitution.  profiles/r02/backsolve_bench.txt has the history.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Igtsam_personal_amd/csrc -o tools/backsolve_bench tools/backsolve_bench.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define LMGPU_TEST_HOOKS  // both hop widths of the root back-substitution
#include "kernels_dense.hpp"
using namespace lmgpu;

// `backsolve_bench hops [nf]`: the dependent chain of the root's dataflow back-substitution, hop by hop.  A synthetic root of nf
// (default 9000, the C4 root: n = 9001) frontal columns, the 64-row form (hbm_backsolve_dataflow2_kernel) and the 128-row form
// (hbm_backsolve_wide_kernel) with in-kernel stamps of the 100 MHz clock: per block the time from the neighbour's publish to its own
// (the hop), from the arrival of the neighbour's x to its own publish (the part of the hop that is this kernel's code), and the head
// of the launch in front of the first publish.  profiles/r06/ has the records.
static int hops_main(int nf) {
  const int n = nf + 1, ld = (n + 15) & ~15;
  std::vector<double> A((size_t)nf * ld, 0.0);
  unsigned long long st = 88172645463325252ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st % 2000001) / 1e6 - 1.0; };
  for (int i = 0; i < nf; i++) {
    for (int j = i; j < n; j++) A[(size_t)i * ld + j] = 1e-4 * rnd();
    A[(size_t)i * ld + i] = 2.0 + rnd() * 0.5;
    A[(size_t)i * ld + n - 1] = rnd();
  }
  std::vector<double> x(nf);
  for (int i = nf - 1; i >= 0; i--) {
    double s = A[(size_t)i * ld + n - 1];
    for (int j = i + 1; j < nf; j++) s -= A[(size_t)i * ld + j] * x[j];
    x[i] = s / A[(size_t)i * ld + i];
  }
  // the 16 x 16 inverses of the diagonal tiles, as the factorisation leaves them: block t at inv16 + 256 t, row-major, identity-padded
  const int nb16 = (nf + 15) / 16, npanel = (nf + 255) / 256;
  std::vector<double> inv16((size_t)(npanel + 2) * 4096, 0.0);
  for (int t = 0; t < nb16; t++) {
    double R[16][16], X[16][16];
    for (int i = 0; i < 16; i++)
      for (int j = 0; j < 16; j++) {
        const int gi = 16 * t + i, gj = 16 * t + j;
        R[i][j] = (gi < nf && gj < nf && j >= i) ? A[(size_t)gi * ld + gj] : (i == j ? 1.0 : 0.0);
      }
    for (int j = 0; j < 16; j++)
      for (int i = 15; i >= 0; i--) {
        double s = (i == j) ? 1.0 : 0.0;
        for (int k = i + 1; k < 16; k++) s -= R[i][k] * X[k][j];
        X[i][j] = s / R[i][i];
      }
    for (int i = 0; i < 16; i++)
      for (int j = 0; j < 16; j++) inv16[(size_t)t * 256 + i * 16 + j] = X[i][j];
  }
  FrontDesc F{};
  F.n = n; F.nf = nf; F.fx_begin = 0; F.sx_begin = 0; F.id = 0;
  std::vector<int32_t> fx(nf);
  for (int i = 0; i < nf; i++) fx[i] = i;
  const int nblk64 = (nf + 63) / 64, nblk128 = (nf + 127) / 128;
  double *dA, *dI, *dx, *dd, *dpark; int32_t* dfx; unsigned int* dflags; int* dst; unsigned long long* dstamp;
  (void)hipMalloc((void**)&dA, A.size() * 8); (void)hipMalloc((void**)&dI, inv16.size() * 8); (void)hipMalloc((void**)&dx, (size_t)nblk128 * 128 * 8);
  (void)hipMalloc((void**)&dd, (size_t)n * 8); (void)hipMalloc((void**)&dfx, (size_t)nf * 4); (void)hipMalloc((void**)&dflags, (size_t)(nblk64 + 1) * 4);
  (void)hipMalloc((void**)&dpark, (size_t)nblk128 * 128 * 128 * 8);
  (void)hipMalloc((void**)&dst, 8); (void)hipMalloc((void**)&dstamp, (size_t)nblk64 * 3 * 8);
  const int st0[2] = {0x7f7f7f7f, 0};
  (void)hipMemcpy(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(dI, inv16.data(), inv16.size() * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(dfx, fx.data(), (size_t)nf * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(dst, st0, 8, hipMemcpyHostToDevice);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int width : {64, 128}) {
    const int nblk = width == 64 ? nblk64 : nblk128;
    auto launch = [&](bool stamp) {
      (void)hipMemsetAsync(dflags, 0, (size_t)(nblk + 1) * 4, 0);
      (void)hipMemsetAsync(dx, 0xff, (size_t)nblk * width * 8, 0);
      const double* noy = nullptr;
      if (width == 64) {
        if (stamp) hipLaunchKernelGGL((hbm_backsolve_dataflow2_kernel<true>), dim3(nblk), dim3(256), 0, 0, F, (int64_t)0, ld, dfx, dA, dI, noy, dx, dflags, dd, dst, dstamp);
        else hipLaunchKernelGGL((hbm_backsolve_dataflow2_kernel<false>), dim3(nblk), dim3(256), 0, 0, F, (int64_t)0, ld, dfx, dA, dI, noy, dx, dflags, dd, dst, dstamp);
      } else {
        if (stamp) hipLaunchKernelGGL((hbm_backsolve_wide_kernel<true>), dim3(nblk), dim3(512), 0, 0, F, (int64_t)0, ld, dfx, dA, dI, noy, dx, dflags, dd, dst, dpark, dstamp);
        else hipLaunchKernelGGL((hbm_backsolve_wide_kernel<false>), dim3(nblk), dim3(512), 0, 0, F, (int64_t)0, ld, dfx, dA, dI, noy, dx, dflags, dd, dst, dpark, dstamp);
      }
    };
    (void)hipMemset(dd, 0, (size_t)n * 8);
    launch(false);
    if (hipDeviceSynchronize() != hipSuccess) { std::printf("width %d: launch failed: %s\n", width, hipGetErrorString(hipGetLastError())); return 1; }
    std::vector<double> out(n);
    int stat[2];
    (void)hipMemcpy(out.data(), dd, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(stat, dst, 8, hipMemcpyDeviceToHost);
    double err = 0, xmax = 0;
    for (int i = 0; i < nf; i++) { err = std::max(err, std::abs(out[i] - x[i])); xmax = std::max(xmax, std::abs(x[i])); }
    std::printf("== %d-row hops: nf %d, %d blocks = %d hops; max |x - ref| %.2e (max |x| %.2e); status %d / %d\n", width, nf, nblk, nblk - 1, err, xmax, stat[0], stat[1]);
    if (stat[1] != 0 || !(err < 1e-9)) { std::printf("width %d: WRONG RESULT, no timing\n", width); return 1; }
    for (int w = 0; w < 3; w++) launch(false);
    float ms = 0;
    (void)hipEventRecord(e0, 0);
    for (int w = 0; w < 20; w++) launch(false);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    std::printf("   %.1f us per launch incl. the two memsets (20 launches back to back, no stamps)\n", 1e3 * ms / 20);
    std::vector<unsigned long long> sp((size_t)nblk * 3);
    for (int rep = 0; rep < 3; rep++) {  // stamped launches, each ONE launch on an idle device
      launch(true);
      (void)hipDeviceSynchronize();
      (void)hipMemcpy(sp.data(), dstamp, sp.size() * 8, hipMemcpyDeviceToHost);
      unsigned long long first = ~0ull;
      for (int b = 0; b < nblk; b++) first = std::min(first, sp[3 * b]);
      std::vector<double> hop, own;
      for (int b = nblk - 2; b >= 0; b--) {
        hop.push_back(0.01 * (double)(long long)(sp[3 * b + 2] - sp[3 * (b + 1) + 2]));
        own.push_back(0.01 * (double)(long long)(sp[3 * b + 2] - sp[3 * b + 1]));
      }
      auto stats = [](std::vector<double> v, double& mean, double& med, double& lo, double& hi) {
        std::sort(v.begin(), v.end());
        mean = 0;
        for (double t : v) mean += t;
        mean /= (double)v.size(); med = v[v.size() / 2]; lo = v.front(); hi = v.back();
      };
      double m, md, lo, hi, om, omd, olo, ohi;
      stats(hop, m, md, lo, hi);
      stats(own, om, omd, olo, ohi);
      const double head = 0.01 * (double)(long long)(sp[3 * (nblk - 1) + 2] - first), total = 0.01 * (double)(long long)(sp[2] - first);
      std::printf("   stamped launch %d: head %.2f us, first start to last publish %.2f us; hop (publish to publish) mean %.3f median %.3f min %.3f max %.3f us;"
                  " arrival to publish mean %.3f median %.3f max %.3f us\n", rep, head, total, m, md, lo, hi, om, omd, ohi);
      if (rep == 2) {
        std::printf("   block: hop us / arrival-to-publish us (launch 2, from the last block down)\n");
        for (size_t i = 0; i < hop.size(); i++) std::printf("   %3d: %.2f / %.2f%s", nblk - 2 - (int)i, hop[i], own[i], (i % 6 == 5 || i + 1 == hop.size()) ? "\n" : "");
      }
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "hops") return hops_main(argc > 2 ? atoi(argv[2]) : 9000);
  for (auto sz : {std::pair<int, int>{330, 331}, {228, 517}, {114, 421}, {30, 199}, {546, 547}}) {
    const int nf = sz.first, n = sz.second, ns = n - nf - 1, ld = (n + 15) & ~15;
    std::vector<double> A((size_t)nf * ld, 0.0), delta(n, 0.0);
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st % 2000001) / 1e6 - 1.0; };
    for (int i = 0; i < nf; i++) {
      for (int j = i; j < n; j++) A[(size_t)i * ld + j] = 0.05 * rnd();
      A[(size_t)i * ld + i] = 2.0 + rnd() * 0.5;
    }
    for (int j = 0; j < ns; j++) delta[nf + j] = rnd();
    // CPU reference
    std::vector<double> x(nf);
    for (int i = nf - 1; i >= 0; i--) {
      double s = A[(size_t)i * ld + n - 1];
      for (int j = 0; j < ns; j++) s -= A[(size_t)i * ld + nf + j] * delta[nf + j];
      for (int j = i + 1; j < nf; j++) s -= A[(size_t)i * ld + j] * x[j];
      x[i] = s / A[(size_t)i * ld + i];
    }
    FrontDesc F{};
    F.n = n; F.nf = nf; F.fx_begin = 0; F.sx_begin = 0; F.id = 0;
    std::vector<int32_t> fx(nf), sx(std::max(ns, 1));
    for (int i = 0; i < nf; i++) fx[i] = i;
    for (int j = 0; j < ns; j++) sx[j] = nf + j;
    double *dA, *dd; int32_t *dl, *dfx, *dsx, *dld; int64_t* doff; FrontDesc* dF; int* dst;
    (void)hipMalloc((void**)&dA, A.size() * 8); (void)hipMalloc((void**)&dd, n * 8);
    (void)hipMalloc((void**)&dl, 4); (void)hipMalloc((void**)&dfx, nf * 4); (void)hipMalloc((void**)&dsx, sx.size() * 4);
    (void)hipMalloc((void**)&dld, 4); (void)hipMalloc((void**)&doff, 8); (void)hipMalloc((void**)&dF, sizeof(F)); (void)hipMalloc((void**)&dst, 8);
    const int32_t zero = 0; const int64_t zero64 = 0; const int big = 0x7f7f7f7f;
    (void)hipMemcpy(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dd, delta.data(), n * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dl, &zero, 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dfx, fx.data(), nf * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dsx, sx.data(), sx.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dld, &ld, 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(doff, &zero64, 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dF, &F, sizeof(F), hipMemcpyHostToDevice);
    (void)hipMemcpy(dst, &big, 4, hipMemcpyHostToDevice);
    std::vector<double> out(n);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    float ms = 0;
    {  // the same front, one workgroup per 64-row block
      const int nblk = (nf + 63) / 64;
      std::vector<BsdBlock> tab;
      for (int b = nblk - 1; b >= 0; b--) tab.push_back(BsdBlock{0, ld, n, nf, 0, 0, 0, b, 0});
      BsdBlock* dtab; unsigned int* dtick; double* dx;
      (void)hipMalloc((void**)&dtab, tab.size() * sizeof(BsdBlock)); (void)hipMalloc((void**)&dtick, 4); (void)hipMalloc((void**)&dx, nblk * 64 * 8);
      (void)hipMemcpy(dtab, tab.data(), tab.size() * sizeof(BsdBlock), hipMemcpyHostToDevice);
      (void)hipMemcpy(dd, delta.data(), n * 8, hipMemcpyHostToDevice);
      auto launch2 = [&]() {
        (void)hipMemsetAsync(dtick, 0, 4, 0);
        (void)hipMemsetAsync(dx, 0xff, nblk * 64 * 8, 0);
        hipLaunchKernelGGL(hbm_backsolve_blocks_kernel, dim3(nblk), dim3(256), 0, 0, dtab, (unsigned int*)nullptr, dfx, dsx, dA, dd, dx, dst);
      };
      launch2();
      (void)hipDeviceSynchronize();
      (void)hipMemcpy(out.data(), dd, n * 8, hipMemcpyDeviceToHost);
      double err2 = 0;
      for (int i = 0; i < nf; i++) err2 = std::max(err2, std::abs(out[i] - x[i]));
      for (int w = 0; w < 5; w++) launch2();
      (void)hipEventRecord(e0, 0);
      for (int w = 0; w < 50; w++) launch2();
      (void)hipEventRecord(e1, 0);
      (void)hipEventSynchronize(e1);
      (void)hipEventElapsedTime(&ms, e0, e1);
      float ms0 = 0;
      (void)hipEventRecord(e0, 0);
      for (int w = 0; w < 50; w++) { (void)hipMemsetAsync(dtick, 0, 4, 0); (void)hipMemsetAsync(dx, 0xff, nblk * 64 * 8, 0); }
      (void)hipEventRecord(e1, 0);
      (void)hipEventSynchronize(e1);
      (void)hipEventElapsedTime(&ms0, e0, e1);
      std::printf("nf %4d n %4d: max |x - ref| %.2e   %.1f us per launch incl. the two memsets (%.1f us for those alone)\n", nf, n, err2, 1e3 * ms / 50, 1e3 * ms0 / 50);
    }
  }
  return 0;
}
