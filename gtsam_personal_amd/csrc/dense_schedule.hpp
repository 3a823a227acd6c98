// The launch schedule of one dense (HBM-class) front on the per-front path: which kernel takes which outer panel, decided once from
// the front's shape (host only, no HIP call; run_dense_steps in front_launch.hpp runs the records in order, for the batch path and for
// ISAM2's wide cliques).  Pinned without a device by
// tests/test_dense_schedule.py through lmgpu_selftest_dense_schedule.
//
// Blocked right-looking partial Cholesky, outer panels of DENSE_NBO = 256 rows.  Panel 0 is one dataflow launch
// (panel_dataflow_kernel); after that ONE launch per outer panel i (step_kernel): trailing update with panel i + factorisation of
// panel i+1 beside/behind it (look-ahead inside the launch, kernels_step.hpp); runs of such steps with full panels go as one chained
// launch (chain_kernel).  A panel whose row count is not a multiple of 64 (the last one) takes the two-launch form diag_potrf_kernel +
// panel_trsm_kernel.
#pragma once
#include <algorithm>
#include <vector>

#include "kernels_potrf.hpp"  // PDF_MAX_COLTILES, PDF_MAX_CHAIN_T, TAIL_MAX_KP, TAIL_MAX_M

namespace lmgpu {

const int DENSE_NBO = 256;  // outer panel: rows eliminated per trailing update; row chunk of the multi-rank assembly

enum DenseKind {
  DENSE_PANEL_DATAFLOW = 0,  // panel i as block-column workgroups with flag hand-offs
  DENSE_PANEL_TWO_LAUNCH,    // panel i as diag_potrf, then panel_trsm when columns follow it
  DENSE_CHAIN,               // steps i .. i + nsteps - 1 in one chained launch
  DENSE_STEP_FUSED,          // update with panel i + factorisation of panel i + 1 in one launch
  DENSE_UPDATE_QUADRANTS,    // update with panel i alone, one workgroup per 32 x 32 quadrant (at most 1024 columns)
  DENSE_UPDATE_MFMA,         // update with panel i alone, 128 x 128 tiles
  DENSE_TAIL,                // the end of the front in one small launch: update with panel i, the last panel, what follows it
  DENSE_ADD_CHUNK,           // multi-rank: row chunk `chunk` is summed over the ranks and added to the working matrix
  DENSE_WAIT_CHUNK           // multi-rank: row chunk `chunk` is summed over the ranks (the launch behind it folds it in itself)
};
// how the assembled rows reach the working matrix
enum DenseMode {
  DENSE_SINGLE = 0,     // assembled in place
  DENSE_SPLIT_HOST,     // in 256-row chunks, each summed over the ranks on the host between two launches (in-process group)
  DENSE_SPLIT_EVENTS    // in 256-row chunks, each with an event on the communication stream (RCCL)
};
enum : unsigned { DENSE_FORM_TWO_LAUNCH = 1, DENSE_FORM_NO_FUSE = 2, DENSE_FORM_NO_CHAIN = 4, DENSE_FORM_NO_TAIL = 8 };  // the A/B switches

struct DenseStep {
  int kind, i, nsteps, chunk;  // i: outer panel (-1 for chunk records); nsteps: DENSE_CHAIN only; chunk: chunk records only (else -1)
  double flop;                 // algorithmic flop the launch books
};

// n columns (right-hand side included), nf frontal columns.  Empty for nonsense geometry.
inline std::vector<DenseStep> dense_front_schedule(int n, int nf, int mode, unsigned forms) {
  std::vector<DenseStep> out;
  if (n <= 0 || nf <= 0 || nf > n || mode < DENSE_SINGLE || mode > DENSE_SPLIT_EVENTS) return out;
  const int NBO = DENSE_NBO;
  const int np = (nf + NBO - 1) / NBO, nchunks = (n + NBO - 1) / NBO;
  const bool split = mode != DENSE_SINGLE, chain_split = mode == DENSE_SPLIT_EVENTS;
  auto rows_of = [&](int i) { return std::min(nf, (i + 1) * NBO) - i * NBO; };
  auto dataflow_ok = [&](int i) { return rows_of(i) % 64 == 0 && !(forms & DENSE_FORM_TWO_LAUNCH) && (n - i * NBO + 63) / 64 <= PDF_MAX_COLTILES; };
  auto panel_flop = [&](int i) {
    const double kb = rows_of(i), cols = n - i * NBO - kb;
    return kb * kb * kb / 3.0 + kb * kb * cols;
  };
  // algorithmic flop of the update with panel i: 2 x kb x (upper-triangle entries of the m x m trailing matrix)
  auto upd_flop = [&](int i) {
    const double kb = rows_of(i), m = n - i * NBO - kb;
    return 2.0 * kb * (m * (m + 1) / 2.0);
  };
  auto panel = [&](int i) { out.push_back({dataflow_ok(i) ? DENSE_PANEL_DATAFLOW : DENSE_PANEL_TWO_LAUNCH, i, 0, -1, panel_flop(i)}); };
  // chunk c = rows [256 c, 256 (c + 1)); `add`: a kernel folds it into the working matrix, else the launch behind the record does
  auto chunk = [&](int c, bool add) {
    if (split && c < nchunks) out.push_back({add ? DENSE_ADD_CHUNK : DENSE_WAIT_CHUNK, -1, 0, c, 0.0});
  };
  // a step that can be fused with the factorisation of the next panel; consecutive ones with full panels go as ONE launch
  auto fusable = [&](int i) { return i + 1 < np && dataflow_ok(i + 1) && !(forms & DENSE_FORM_NO_FUSE) && n - i * NBO - rows_of(i) > 0; };
  // multi-rank (RCCL): the steps still go as chained launches -- their head tiles fold the all-reduced row chunks in -- but in
  // SEGMENTS of 1, 1, 2, 4, 8, ... steps, each launched behind a stream wait for the event of the last chunk it touches: no
  // workgroup ever waits for the network inside a launch (nothing to deadlock on), the first panels start after two chunks, and
  // the communication stream gets further ahead with every segment (one launch per step cost 6.9 vs 6.2 ms for the C4 root in
  // round 1).  The in-process test communicator sums on the host between the launches and keeps the per-step form.
  auto chainable = [&](int i) {
    return fusable(i) && (!split || chain_split) && !(forms & DENSE_FORM_NO_CHAIN) && rows_of(i) == NBO && (n - (i + 1) * NBO + 127) / 128 <= PDF_MAX_CHAIN_T;
  };
  chunk(0, true);
  panel(0);
  for (int i = 0; i < np; i++) {
    const int kb = rows_of(i), r0 = i * NBO + kb, m = n - r0;
    if (m <= 0) break;
    if (chainable(i) && chainable(i + 1)) {  // the run of chainable steps starting here: one launch, or a few segment launches
      int run = 0;
      while (chainable(i + run)) run++;
      for (int at = i, seg = 1, nseg = 0; at < i + run;) {
        int nsteps = chain_split ? std::min(seg, i + run - at) : run;
        if (chain_split && i + run - (at + nsteps) == 1) nsteps++;  // no one-step remainder
        double flop = 0;
        for (int q = at; q < at + nsteps; q++) flop += upd_flop(q) + panel_flop(q + 1);
        chunk(at + nsteps, false);  // every row chunk the segment folds in (at + 1 .. at + nsteps) is summed over the ranks
        out.push_back({DENSE_CHAIN, at, nsteps, -1, flop});
        at += nsteps;
        if (++nseg >= 2) seg *= 2;
      }
      i += run - 1;
      continue;
    }
    // the end of the front as one small launch: update with panel i, factor the last (partial) panel, update what follows
    if (!split && !(forms & DENSE_FORM_NO_TAIL) && i + 2 == np && kb <= TAIL_MAX_KP && m <= TAIL_MAX_M && rows_of(i + 1) < 64) {
      out.push_back({DENSE_TAIL, i, 0, -1, upd_flop(i) + panel_flop(i + 1)});
      break;
    }
    const bool fuse = fusable(i);
    // rows of panel i+1 (and, for i = np-1, of the separator part): a fused step folds them in itself (its 64x64 head tiles
    // cover exactly those rows), otherwise an add kernel does
    const bool fold_in_step = split && fuse && r0 == (i + 1) * NBO;
    chunk(i + 1, !fold_in_step);
    if (fuse) {
      out.push_back({DENSE_STEP_FUSED, i, 0, -1, upd_flop(i) + panel_flop(i + 1)});
    } else {
      // a few tiles: one workgroup per 32 x 32 quadrant (each 128-tile is K / 4 x 16 dependent MFMAs on one CU)
      out.push_back({m <= 1024 ? DENSE_UPDATE_QUADRANTS : DENSE_UPDATE_MFMA, i, 0, -1, upd_flop(i)});
      if (i + 1 < np) panel(i + 1);
    }
  }
  for (int c = np + 1; c < nchunks; c++) chunk(c, true);  // separator rows beyond the chunk after the last panel
  return out;
}

}  // namespace lmgpu
