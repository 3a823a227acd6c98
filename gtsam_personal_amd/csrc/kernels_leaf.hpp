// Gather leaves in lane groups: FOUR small leaf fronts per wave, one lane per factor, no barrier per factor.
// A BAL point is a 3-row front of ~94 columns with ten 2 x 13 Jacobians: lds_front_kernel<true> spends a whole one-wave workgroup, 5.5 KB
// of LDS and a barrier per factor on about 1 kFLOP, and the launch is as long as that leaf's latency times the number of resident rounds
// (DESIGN round 8).  Here a group of 16 lanes takes one leaf:
//   the group copies the leaf's Jacobians to LDS as one flat, coalesced stream (the record says where they are and whether they lie back
//     to back) -- a lane that fetched its own factor from memory touched a cache line of its own per load and the launch was bound by the
//     number of lines, not bytes (0.52 ms where the generic kernel takes 0.29; DESIGN round 8);
//   lane f takes factor f (and f + 16) of the packed record (LEAFPACK_*) from there: its frontal block, its separator block and b;
//   the frontal block, the frontal right-hand side and the (rhs, rhs) corner are sums over the group in a FIXED order (a lane's two
//     factors in record order, then a four-stage butterfly inside the 16-lane row: every lane ends with the same bits);
//   every lane damps and factors the same nf x nf block (sqrt and divide, as the generic gather body; pivot rules of lds_front_body);
//   every lane solves ITS separator columns against it and puts them into the leaf's [R S d] in LDS: no separator variable is shared by
//     two factors of the leaf (the host checks, lmgpu.hip leaf_group_form), so every column is written exactly once, no zero-fill;
//   the group copies [R S d] out as one flat stream, and once more transposed ([S d] at u_off).
// Outputs exactly as lds_front_body<GATHER = true>: [R S d] at rsd_off (strictly-lower part of R zero), the transposed [S d] at u_off,
// the corner at gcorner[par_map], atomicMin(status, id) on a failed pivot or pivot-exponent test.
// The same lane groups serve the way down: lds_backsub_group_kernel at the end of this file.
#pragma once

namespace lmgpu {

// what a bin launch must satisfy for this kernel (checked per front on the host, once)
#define LEAFGRP_MAXNF 4     // frontal scalars of the leaf
#define LEAFGRP_MAXROWS 4   // rows of a factor
#define LEAFGRP_MAXSEP 9    // columns of a factor's separator variable
#define LEAFGRP_LANES 16    // lanes per leaf; a leaf takes its factors in rounds of 16 (at most LDSF_MAXB = 32 of them)

template <int CTRL>
__device__ __forceinline__ double leafgrp_dpp(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// sum over the 16 lanes of a DPP row, the same bits in every lane: neighbours, pairs (quad_perm), the other quad (row_half_mirror), the other
// half (row_mirror).  Each stage adds two values that both partners hold, in either order: addition commutes, so the partners agree.
__device__ __forceinline__ double leafgrp_sum16(double v) {
  v += leafgrp_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += leafgrp_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += leafgrp_dpp<0x141>(v);  // row_half_mirror
  v += leafgrp_dpp<0x140>(v);  // row_mirror
  return v;
}

// one factor of a leaf in a lane's registers: the frontal block spread over the leaf's (at most NFM) frontal columns, the separator block, b.
// Rows MR .. LEAFGRP_MAXROWS - 1 (in the two-row instantiation only unary factors have them: BAL's 3-row prior on a point) only feed the
// frontal sums: they are loaded in the same batch and are dead once added (leafgrp_load).
template <int MR, int DS, int NFM>
struct LeafGrpFac {
  double af[MR][NFM];            // zero outside the factor's rows and its frontal variable's columns
  double b[MR];
  double as[MR][DS];             // binary factors: the separator variable's block (rows < MR: the host picks the instantiation)
  int cs, ds;                    // front column and width of the separator block (ds = 0: unary, or a lane without a factor)
};
// loads factor f of the record into G (WITH_SEP: its separator block too) and adds its share of the frontal block (upper triangle), of the
// frontal right-hand side and of the corner to H, g, cc: per entry the rows in ascending order, as the generic body sums them
template <int MR, int DS, int NFM, bool WITH_SEP, bool FIRST>
__device__ __forceinline__ void leafgrp_load(LeafGrpFac<MR, DS, NFM>& G, const LFac* __restrict__ lf, int f, int nfac, int nf, const double* stage,
                                             double (&H)[NFM][NFM], double (&g)[NFM], double& cc) {
  constexpr int NF = NFM, XR = LEAFGRP_MAXROWS - MR;
  const bool act = f < nfac;
  const LFac d = lf[min(f, nfac - 1)];
  const double* J = stage + d.off;  // the factor's [A b], column-major, in the leaf's staging area
  const int m = d.rows;
  const bool f0 = d.c0 < nf;                        // the frontal variable is the factor's first one (unary factors: always)
  const int qf = f0 ? 0 : d.d0, df = f0 ? d.d0 : d.d1, cf = f0 ? d.c0 : d.c1;  // local column, width and front column of the frontal block
  const int qs = f0 ? d.d0 : 0;
  G.ds = (act && d.d1 > 0) ? (f0 ? d.d1 : d.d0) : 0;
  G.cs = f0 ? d.c1 : d.c0;
  const int qb = d.d0 + d.d1;
  double xa[XR > 0 ? XR : 1][NF], xb[XR > 0 ? XR : 1];
#pragma unroll
  for (int r = 0; r < LEAFGRP_MAXROWS; r++) {
#pragma unroll
    for (int I = 0; I < NF; I++) {
      const double v = (act && r < m && I >= cf && I < cf + df) ? J[(qf + I - cf) * m + r] : 0.0;
      if (r < MR)
        G.af[r][I] = v;
      else
        xa[r - MR][I] = v;
    }
    const double v = (act && r < m) ? J[qb * m + r] : 0.0;
    if (r < MR)
      G.b[r] = v;
    else
      xb[r - MR] = v;
  }
  if constexpr (WITH_SEP) {
#pragma unroll
    for (int r = 0; r < MR; r++)
#pragma unroll
      for (int c = 0; c < DS; c++) G.as[r][c] = (r < m && c < G.ds) ? J[(qs + c) * m + r] : 0.0;
  }
#pragma unroll
  for (int I = 0; I < NF; I++) {
#pragma unroll
    for (int Jc = I; Jc <= NF; Jc++) {  // Jc = NF: the right-hand side
      double v = 0.0;
#pragma unroll
      for (int r = 0; r < MR; r++) v += G.af[r][I] * (Jc < NF ? G.af[r][Jc] : G.b[r]);
#pragma unroll
      for (int r = 0; r < XR; r++) v += xa[r][I] * (Jc < NF ? xa[r][Jc] : xb[r]);
      double& dst = Jc < NF ? H[I][Jc] : g[I];
      dst = FIRST ? v : dst + v;
    }
  }
  double v = 0.0;
#pragma unroll
  for (int r = 0; r < MR; r++) v += G.b[r] * G.b[r];
#pragma unroll
  for (int r = 0; r < XR; r++) v += xb[r] * xb[r];
  cc = FIRST ? v : cc + v;
}

// grid: workgroups of one to four waves, 16 lanes per leaf; group g takes the leaf of record g.  Dynamic LDS: `lds_leaf` doubles per leaf:
// the staged Jacobians (at most jcap doubles) and, from `out_off` on, the leaf's nf x n block [R S d].  out_off = 0 where every leaf of the
// launch has at most 16 factors: a lane then holds its only factor in registers before the first output is written over the staging area.
// A second factor per lane is fetched from the staging area after the first one's columns are out, so such a launch keeps both areas.
// Instantiations (the host picks per launch): <2, 9, 3> for leaves of nf <= 3 whose binary factors have at most two rows (BAL's points,
// planar landmarks): 128 VGPR, no spill, no scratch; <4, 9, 4> for the caps: 204 VGPR, two waves per SIMD.  amdgpu_waves_per_eu pins the
// four (two) waves: an edit that needs a 129th register spills visibly instead of losing the fourth wave silently.
template <int MR, int DS, int NFM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NFM <= 3 ? 4 : 2, NFM <= 3 ? 4 : 2))) void lds_front_group_kernel(const char* __restrict__ pack, int pack_stride, int nleaf, double* __restrict__ pool, double lambda_v,
                                                               const double* __restrict__ lambda_p, const double* __restrict__ dampw, int* __restrict__ status,
                                                               double* __restrict__ gcorner, const double* __restrict__ gex, int lds_leaf, int out_off) {
  extern __shared__ double leafgrp_lds[];
  constexpr int NF = NFM;
  const int tid = threadIdx.x, gl = tid & (LEAFGRP_LANES - 1);
  const int leaf = (int)(blockIdx.x * blockDim.x + tid) / LEAFGRP_LANES;
  // (a group without a leaf in the launch's last workgroup works on the last leaf again and stores nothing: the row sums and the
  //  barriers need every lane)
  const bool live = leaf < nleaf;
  const char* pk = pack + (size_t)min(leaf, nleaf - 1) * pack_stride;
  const FrontDesc F = *(const FrontDesc*)pk;
  const int nfac = ((const int*)(pk + LEAFPACK_HDR))[0], tot = ((const int*)(pk + LEAFPACK_HDR))[1], contig = ((const int*)(pk + LEAFPACK_HDR))[2];
  const LFac* lf = (const LFac*)(pk + LEAFPACK_FAC);
  const int n = F.n, nf = F.nf;
  const double lambda = lambda_p ? *lambda_p : lambda_v;
  double dw[NF];
#pragma unroll
  for (int i = 0; i < NF; i++) dw[i] = dampw[((const int*)(pk + LEAFPACK_XO))[min(i, nf - 1)]];
  double* stage = leafgrp_lds + (size_t)(tid / LEAFGRP_LANES) * lds_leaf;
  double* X = stage + out_off;
  // ---- the leaf's Jacobians into LDS: one flat copy where they lie back to back in the pool (factors of one bucket added together),
  //      sixteen loads in flight per lane; factor by factor otherwise
  if (contig) {
    const double* J = pool + lf[0].joff;
    for (int i0 = gl; i0 < tot; i0 += 16 * LEAFGRP_LANES) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; u++) v[u] = J[min(i0 + u * LEAFGRP_LANES, tot - 1)];
#pragma unroll
      for (int u = 0; u < 16; u++)
        if (i0 + u * LEAFGRP_LANES < tot) stage[i0 + u * LEAFGRP_LANES] = v[u];
    }
  } else {
    for (int f = 0; f < nfac; f++) {  // (the group strides inside a factor: neighbouring lanes, neighbouring doubles)
      const LFac d = lf[f];
      const double* J = pool + d.joff;
      for (int i = gl; i < d.sz; i += LEAFGRP_LANES) stage[d.off + i] = J[i];
    }
  }
  __syncthreads();  // (more than needed: a leaf's LDS area is touched by its own 16 lanes only, all of one wave; measured as it stands)
  // ---- own factors: lane f holds factor f; of a second one (a leaf of more than 16 factors) only the frontal share now
  LeafGrpFac<MR, DS, NFM> G;
  double H[NF][NF], g[NF], cc;  // upper triangle of the frontal block, frontal rhs, corner: this lane's share
  leafgrp_load<MR, DS, NFM, true, true>(G, lf, gl, nfac, nf, stage, H, g, cc);
  if (nfac > LEAFGRP_LANES) {
    LeafGrpFac<MR, DS, NFM> G2;
    leafgrp_load<MR, DS, NFM, false, false>(G2, lf, gl + LEAFGRP_LANES, nfac, nf, stage, H, g, cc);
  }
  // ---- the leaf's sums (all 64 lanes take part), damping, the extra gradient term; rows past nf: identity
#pragma unroll
  for (int I = 0; I < NF; I++) {
#pragma unroll
    for (int J = I; J < NF; J++) H[I][J] = leafgrp_sum16(H[I][J]);
    g[I] = leafgrp_sum16(g[I]);
  }
  cc = leafgrp_sum16(cc);
#pragma unroll
  for (int I = 0; I < NF; I++) {
    if (I < nf) {
      H[I][I] += lambda * dw[I];
      if (gex) g[I] += gex[((const int*)(pk + LEAFPACK_XO))[I]];  // extra gradient term (marginal covariances: unit vectors)
    } else {
      H[I][I] = 1.0;
    }
  }
  // ---- Cholesky of the frontal block, every lane the same: R in H, d in g, 1 / R_kk in inv
  bool failed = false;
  double inv[NF];
#pragma unroll
  for (int k = 0; k < NF; k++) {
    double piv = H[k][k];
    if (!(piv > 0.0)) {
      if (piv <= 0.0) failed = true;  // Eigen LLT: pivot <= 0 -> NumericalIssue (NaN passes, like Eigen)
      piv = (piv == piv && piv != 0.0) ? fabs(piv) : 1.0;
    }
    const double r = sqrt(piv);
    inv[k] = 1.0 / r;
    H[k][k] = r;
#pragma unroll
    for (int J = k + 1; J < NF; J++) H[k][J] *= inv[k];
    g[k] *= inv[k];
    cc -= g[k] * g[k];
#pragma unroll
    for (int I = k + 1; I < NF; I++) {
#pragma unroll
      for (int J = I; J < NF; J++) H[I][J] -= H[k][I] * H[k][J];
      g[I] -= H[k][I] * g[k];
    }
  }
  {  // pivot-exponent test, gtsam/base/cholesky.cpp:146-158
    double dlast = H[0][0], dprev = H[0][0];
#pragma unroll
    for (int I = 1; I < NF; I++)
      if (I < nf) {
        dprev = dlast;
        dlast = H[I][I];
      }
    if (nf >= 2) {
      if (!(frexp_exp(dprev) - frexp_exp(dlast) < 12)) failed = true;
    } else {
      if (!(frexp_exp(dlast) > -12)) failed = true;
    }
  }
  if (live && gl == 0) {
    if (failed) atomicMin(status, F.id);
    gcorner[F.par_map] = cc;
  }
  // ---- [R S d] of the leaf in LDS (nf x n, row-major): lane i < nf puts row i of R (strictly-lower part zero) and d_i ...
  if (gl < nf) {
    double row[NF], di = g[0];
#pragma unroll
    for (int J = 0; J < NF; J++) row[J] = H[0][J];
#pragma unroll
    for (int I = 1; I < NF; I++)
      if (gl == I) {
        di = g[I];
#pragma unroll
        for (int J = 0; J < NF; J++) row[J] = J >= I ? H[I][J] : 0.0;
      }
#pragma unroll
    for (int J = 0; J < NF; J++)
      if (J < nf) X[gl * n + J] = row[J];
    X[gl * n + n - 1] = di;
  }
  // ... and every lane its separator columns: S = R^-T (A_F^T A_S), column by column
  auto emit = [&](const LeafGrpFac<MR, DS, NFM>& Q) {
#pragma unroll
    for (int c = 0; c < DS; c++) {
      double s[NF];
#pragma unroll
      for (int I = 0; I < NF; I++) {
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < MR; r++) v += Q.af[r][I] * Q.as[r][c];
        s[I] = v;
      }
#pragma unroll
      for (int k = 0; k < NF; k++) {
        s[k] *= inv[k];
#pragma unroll
        for (int I = k + 1; I < NF; I++) s[I] -= H[k][I] * s[k];
      }
      if (c < Q.ds) {
#pragma unroll
        for (int I = 0; I < NF; I++)
          if (I < nf) X[I * n + Q.cs + c] = s[I];
      }
    }
  };
  emit(G);
  if (nfac > LEAFGRP_LANES) {  // (out_off > 0 in such a launch: the staging area is still whole)
    double H2[NF][NF], g2[NF], c2;  // (the frontal share again: unused)
    leafgrp_load<MR, DS, NFM, true, true>(G, lf, gl + LEAFGRP_LANES, nfac, nf, stage, H2, g2, c2);
    emit(G);
  }
  __syncthreads();  // (as above: the group's own wave would do)
  // ---- out: [R S d] as it lies (ld_rsd = n for an LDS front: the host checks), then [S d] transposed, (n - nf) x nf
  if (live) {
    double* RSd = pool + F.rsd_off;
    double* St = pool + F.u_off;
    const int nx = nf * n, nt = (n - nf) * nf;
    for (int i = gl; i < nx; i += LEAFGRP_LANES) RSd[i] = X[i];
    for (int i = gl; i < nt; i += LEAFGRP_LANES) {
      const int c = nf == 3 ? (int)(((unsigned)i * 43691u) >> 17) : (nf == 1 ? i : i >> (nf >> 1));  // i / nf  (i < 4 x 139; nf = 2, 4: a shift)
      St[i] = X[(i - c * nf) * n + nf + c];
    }
  }
}

// ---- the same layout on the way down: back-substitution of fronts with nf <= LDSBG_MAXNF, FOUR fronts per wave, 16 lanes per front.
// lds_backsub_kernel gives a front a whole wave; a BAL point (3 x 94) fills 90 of its 192 column slots and a launch of 100 000 of them is
// as long as its four dependent round trips (list -> descriptor -> {offsets, rows} -> x_S) times the rounds of resident waves.  Here
// lane j of a group takes separator columns j, j + 16, ... (NQ of them) of every frontal row:
//   ONE batch of unconditional loads on clamped indices: the separator offsets, the row segments of S, d, R, the frontal offset;
//   one gather of delta at those offsets;
//   the row sums in a FIXED order (a lane's columns ascending, then leafgrp_sum16: every lane of the group ends with the same bits);
//   every lane solves the same nf x nf triangle in registers (divides, last row first); lane i < nf stores x_i and checks it for NaN.
// No LDS, no barrier.  Instantiations (the host picks per launch from the level's largest nf and separator): <3, 6> and <4, 9>.
#define LDSBG_MAXNF 4
template <int NFM, int NQ>
__global__ __launch_bounds__(256) void lds_backsub_group_kernel(const int32_t* __restrict__ list, int nlist, const FrontDesc* __restrict__ fronts,
                                                                 const int32_t* __restrict__ fxoff, const int32_t* __restrict__ sxoff,
                                                                 const double* __restrict__ pool, double* __restrict__ delta, int* __restrict__ status) {
  const int tid = threadIdx.x, gl = tid & (LEAFGRP_LANES - 1);
  const int li = (int)(blockIdx.x * blockDim.x + tid) / LEAFGRP_LANES;
  const bool live = li < nlist;  // (a group past the list works on the last front again and stores nothing)
  const FrontDesc F = fronts[list[min(li, nlist - 1)]];
  const int n = F.n, nf = F.nf, ns = n - nf - 1;
  const double* RSd = pool + F.rsd_off;
  // ---- the batch: everything that depends on the descriptor alone
  const int fo = fxoff[F.fx_begin + min(gl, nf - 1)];
  int so[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) so[q] = ns > 0 ? sxoff[F.sx_begin + min(gl + LEAFGRP_LANES * q, ns - 1)] : 0;  // (a front without separator is a root)
  double sv[NFM][NQ], R[NFM][NFM], rhs[NFM];
#pragma unroll
  for (int u = 0; u < NFM; u++) {
    const double* row = RSd + (size_t)min(u, nf - 1) * F.ld_rsd;
#pragma unroll
    for (int q = 0; q < NQ; q++) sv[u][q] = row[nf + max(min(gl + LEAFGRP_LANES * q, ns - 1), 0)];  // (ns = 0: column nf is d)
#pragma unroll
    for (int k = 0; k < NFM; k++) R[u][k] = row[min(k, nf - 1)];
    rhs[u] = row[n - 1];
  }
  // ---- x_S
  double xs[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const double v = delta[so[q]];
    xs[q] = (gl + LEAFGRP_LANES * q < ns) ? v : 0.0;
  }
  // ---- rhs_i = d_i - sum_j S_ij x_S[j]
#pragma unroll
  for (int u = 0; u < NFM; u++) {
    double acc = sv[u][0] * xs[0];
#pragma unroll
    for (int q = 1; q < NQ; q++) acc += sv[u][q] * xs[q];
    rhs[u] -= leafgrp_sum16(acc);
  }
  // ---- R x = rhs, every lane the same
  double x[NFM];
#pragma unroll
  for (int k = NFM - 1; k >= 0; k--) {
    double t = rhs[k];
#pragma unroll
    for (int j = k + 1; j < NFM; j++) t -= (j < nf ? R[k][j] : 0.0) * x[j];
    x[k] = k < nf ? t / R[k][k] : 0.0;
  }
  double xi = x[0];
#pragma unroll
  for (int k = 1; k < NFM; k++) xi = gl == k ? x[k] : xi;
  if (live && gl < nf) {
    delta[fo] = xi;
    if (xi != xi) atomicMin(status, F.id);  // NaN -> IndeterminantLinearSystemException (linearAlgorithms-inst.h:99)
  }
}

}  // namespace lmgpu
