// The launch tables of a finalized handle, built on the host: finalize_structure_impl (lmgpu.hip) runs the phases below in order on EVERY
// handle -- device, structure-only (device = -1), PCG-structure -- and upload_launch_tables then copies a device handle's tables over in
// one place.  Nothing here touches the device: a wrong table is a host bug the CPU tests can see (lmgpu_debug_table_digest, test library).
// What the launch path reads on the host stays on the handle under its name (levels, gather, elim_segs, bsd_runs, h_fronts, f_off, f_ld,
// s_off, row_begin, is_med, fac_local, the solve-form flags); what is only uploaded lives in LaunchTables.
#pragma once

namespace {

struct LaunchTables {
  std::vector<FacDesc> fd;
  std::vector<FrontFac> ffac;
  std::vector<ChildRef> childs;
  std::vector<int32_t> cmap, fxoff, sxoff, lists, rowptr;
  std::vector<RowSrc> rowsrc;
  std::vector<GPairBlock> gpblk;
  std::vector<GPairEntry> gpent;
  std::vector<GVarBlock> gvblk;
  std::vector<GVarEntry> gvent;
  std::vector<GZeroBlock> gzero;
  int n_gleaf = 0;  // gather leaves (one corner scalar each)
  std::vector<char> packs;
  std::vector<int32_t> bs_parent, bs_pos, small, med;
  std::vector<FillUpper> fill_upper;
  std::vector<BsdBlock> bsd, bsd_runs_table;
  std::vector<MedFront> med_fronts;
  std::vector<LevelTask> level_tasks;
  int max_med = 0;  // most medium fronts on one level (sizes inv16_med)
  int max_nf = 1;   // widest frontal part among the HBM fronts (sizes the back-substitution scratch)
  std::vector<int32_t> marg_parent;  // per front: its parent (marginal path walks; poff and spos stay on the handle)
};

// the entries of ONE HBM front's gather lists while its children are walked; sorted and cut into blocks by build_gather_lists
struct GPairTmp { int64_t key; int16_t da, db; GPairEntry ent; };
struct GVarTmp { int32_t pv; int16_t dv; bool leaf; GVarEntry ent; };  // leaf: the leaf's S_v and d; else a factor's A_v and b

// Ownership and local factor numbering.  Reads the plan and the rank (assign_owners); fills front_owner / front_active, fac_local (counted
// factors first), n_counted, nfac and every bucket's loc_of / n_loc.
void build_ownership(lmgpu_handle* h) {
  const Plan& P = h->plan;
  const int NFAC = (int)P.factors.size(), NF = (int)P.fronts.size(), R = h->cfg.rank;
  assign_owners(h);
  std::vector<char> fac_active(NFAC, 0), fac_counted(NFAC, 0);
  for (int fi = 0; fi < NF; fi++) {
    if (!h->front_active[fi]) continue;
    const bool counted = (h->front_owner[fi] == R) || (h->front_owner[fi] < 0 && R == 0);
    for (int32_t f : P.fronts[fi].factors) {
      fac_active[f] = 1;
      fac_counted[f] = counted;
    }
  }
  if (h->pcg_structure) {  // every factor is local and counted (single rank)
    std::fill(fac_active.begin(), fac_active.end(), 1);
    std::fill(fac_counted.begin(), fac_counted.end(), 1);
  }
  h->fac_local.assign(NFAC, -1);
  int nloc = 0;
  for (int i = 0; i < NFAC; i++)
    if (fac_active[i] && fac_counted[i]) h->fac_local[i] = nloc++;
  h->n_counted = nloc;
  for (int i = 0; i < NFAC; i++)
    if (fac_active[i] && !fac_counted[i]) h->fac_local[i] = nloc++;
  h->nfac = nloc;
  for (Bucket& b : h->buckets) {
    b.loc_of.assign(b.n, -1);
    b.n_loc = 0;
  }
  for (int i = 0; i < NFAC; i++)  // factors are sorted by graph index; bucket-local order follows it
    if (fac_active[i]) {
      Bucket& b = h->buckets[P.factors[i].bucket];
      b.loc_of[P.factors[i].idx] = 0;  // mark
    }
  for (Bucket& b : h->buckets)
    for (int i = 0; i < b.n; i++)
      if (b.loc_of[i] == 0) b.loc_of[i] = b.n_loc++;
}

// Pool layout: Jacobians | [R S d] + updates of LDS fronts | dense HBM fronts.  Reads the plan, the ownership and the buckets; fills the
// buckets' joff, T.fd, the layout half of h_fronts (n, nf, id, pad, the offsets and leading dimensions, par_ld of gather leaves), f_off,
// f_ld, s_off, pool_doubles and T.max_nf.
void build_pool_layout(lmgpu_handle* h, LaunchTables& T) {
  const Plan& P = h->plan;
  const int NFAC = (int)P.factors.size(), NF = (int)P.fronts.size(), R = h->cfg.rank;
  int64_t off = 0;
  for (Bucket& b : h->buckets) {
    b.joff = off;
    off += (int64_t)b.n_loc * b.rows * b.cols;
    off = (off + 15) & ~int64_t(15);
  }
  T.fd.resize(h->nfac);
  auto dim = [&](int32_t v) { return (int16_t)(v >= 0 ? P.dims[v] : 0); };  // of a factor's slot; beyond its arity: dimension 0 at offset -1
  auto xoff = [&](int32_t v) { return v >= 0 ? P.xoff[v] : -1; };
  for (int i = 0; i < NFAC; i++) {
    if (h->fac_local[i] < 0) continue;
    const FactorRef& f = P.factors[i];
    const Bucket& b = h->buckets[f.bucket];
    const int32_t* v = f.slots;
    T.fd[h->fac_local[i]] = FacDesc{b.joff + (int64_t)b.loc_of[f.idx] * b.rows * b.cols, xoff(v[0]), xoff(v[1]), (int16_t)b.rows, dim(v[0]), dim(v[1]),
                                    dim(v[2]), xoff(v[2]), 0};
  }
  h->h_fronts.assign(NF, FrontDesc{});
  h->f_off.assign(NF, -1);
  h->f_ld.assign(NF, 0);
  h->s_off.assign(NF, -1);
  for (int fi = 0; fi < NF; fi++) {
    const Front& fr = P.fronts[fi];
    FrontDesc& F = h->h_fronts[fi];
    F.n = fr.n;
    F.nf = fr.nf;
    F.id = fi;
    F.pad = 0;
    if (!h->front_active[fi]) continue;
    if ((h->cfg.world_size > 1 || (h->cfg.flags & LMGPU_FLAG_SPLIT_ROOT)) && h->front_owner[fi] < 0 && fr.cls == 1)
      F.pad = (R == 0) ? 1 : 3;  // replicated; own terms on rank 0 only
    if (fr.cls == 0) {
      F.ld_rsd = fr.n;
      F.rsd_off = off;
      off += (int64_t)fr.nf * fr.n;
      F.ld_u = fr.n - fr.nf;
      F.u_off = off;
      // an LDS front whose parent lives in HBM hands its update over without an update matrix in HBM when it is a leaf (no children) and
      // the Schur gather can read its factors (at most two variables each): the parent GATHERS -[S d]^T [S d] and the factor terms itself
      // (kernels_schur.hpp), par_ld = -1, and the leaf keeps [S d] transposed ((n - nf) x nf: every variable's block contiguous).  Every
      // other front writes its update matrix like any child; the parent's rows collect it in a fixed order.
      bool gather_leaf = fr.parent >= 0 && P.fronts[fr.parent].cls == 1 && fr.children.empty();
      for (int32_t f : fr.factors) gather_leaf = gather_leaf && P.factors[f].slots[2] < 0;
      if (gather_leaf) F.par_ld = -1;
      off += (int64_t)F.ld_u * (gather_leaf ? fr.nf : F.ld_u);
    } else {
      const int ld = (fr.n + 15) & ~15;
      off = (off + 15) & ~int64_t(15);
      h->f_off[fi] = off;
      h->f_ld[fi] = ld;
      F.ld_rsd = ld;
      F.rsd_off = off;
      F.ld_u = ld;
      F.u_off = off + (int64_t)fr.nf * ld + fr.nf;
      off += (int64_t)fr.n * ld;
      // the assembled contributions get a buffer of their own beside the working matrix when they arrive in row chunks while
      // the factorisation is already running: replicated fronts (chunks all-reduced over the ranks)
      if (F.pad & 1) {
        h->s_off[fi] = off;
        off += (int64_t)fr.n * ld;
      }
      T.max_nf = std::max(T.max_nf, (int)fr.nf);
    }
  }
  h->pool_doubles = (size_t)off + 1024;  // slack: the syrk operand DMA may read up to 127 columns past a row end
}

// Gather-mode leaf c of HBM front fi: registers its S blocks and its factors with the parent's lists.  Reads the plan, T.fd and colof
// (the parent's column of every variable); appends to gp / gv, counts the leaf in h->gather[fi] and T.n_gleaf.
int add_gather_leaf(lmgpu_handle* h, LaunchTables& T, int fi, int c, const std::vector<int32_t>& colof, std::vector<GPairTmp>& gp,
                    std::vector<GVarTmp>& gv) {
  const Plan& P = h->plan;
  const Front &fr = P.fronts[fi], &ch = P.fronts[c];
  FrontDesc& CF = h->h_fronts[c];
  lmgpu_handle::GatherRange& G = h->gather[fi];
  const int li = T.n_gleaf++;
  if (G.leaf_count == 0) G.leaf_begin = li;
  G.leaf_count++;
  CF.par_map = li;  // index of its corner scalar
  struct Ent { int pc, lc, d; };
  std::vector<Ent> ents;
  for (size_t k = ch.n_frontal_vars; k < ch.vars.size(); k++) ents.push_back({colof[ch.vars[k]], ch.col_off[k], P.dims[ch.vars[k]]});
  ents.push_back({fr.n - 1, ch.n - 1, 1});
  // (v, v) and (v, rhs) of a separator variable v come from ONE walk of schur_var_kernel over the leaves that see v: a leaf
  // entry in v's list; the pair lists keep the blocks pa < pb < rhs  (split-diagonal form: every block is a pair block)
  if (!h->sw.schur_split_diag)
    for (size_t x = 0; x + 1 < ents.size(); x++) {
      if (ents[x].d + 1 > 16) {
        h->err = "Schur gather: a separator variable of more than 15 dimensions does not fit the 16 x 16 tile of schur_var_kernel";
        return LMGPU_INVALID;
      }
      gv.push_back(GVarTmp{ents[x].pc, (int16_t)ents[x].d, true,
                           GVarEntry{CF.u_off, (int16_t)ch.nf, (int16_t)(ents[x].lc - ch.nf), (int16_t)(ch.n - 1 - ch.nf), 0}});
    }
  for (size_t x = 0; x < ents.size(); x++)
    for (size_t y = x; y < ents.size(); y++) {
      if (x + 1 == ents.size()) continue;  // (rhs, rhs): the corner is a scalar reduction
      if (!h->sw.schur_split_diag && (y == x || y + 1 == ents.size())) continue;
      Ent a = ents[x], b = ents[y];
      if (a.pc > b.pc) std::swap(a, b);
      gp.push_back(GPairTmp{((int64_t)a.pc << 32) | (uint32_t)b.pc, (int16_t)a.d, (int16_t)b.d,
                            GPairEntry{CF.u_off, (int16_t)((a.lc - ch.nf) * ch.nf), (int16_t)((b.lc - ch.nf) * ch.nf), (int16_t)ch.nf, 0}});
    }
  for (int32_t f : ch.factors)
    for (int pos = 0; pos < 2; pos++) {
      const int v = P.factors[f].slots[pos];
      if (v < 0 || P.front_of_var[v] == c) continue;  // frontal in the leaf: no separator contribution
      const FacDesc& fdd = T.fd[h->fac_local[f]];
      gv.push_back(GVarTmp{colof[v], (int16_t)P.dims[v], false,
                           GVarEntry{fdd.joff, fdd.rows, (int16_t)(pos == 0 ? 0 : fdd.d0), (int16_t)(fdd.d0 + fdd.d1), 0}});
    }
  return LMGPU_OK;
}

// Row -> sources of HBM front fi, for the deterministic assembly.  Reads the front's slices of T.childs / T.cmap / T.ffac and T.fd; fills
// row_begin[fi] and appends the front's n + 1 row pointers and its sources to T.rowptr / T.rowsrc.
void build_row_sources(lmgpu_handle* h, LaunchTables& T, int fi) {
  h->row_begin[fi] = append_row_sources(h->h_fronts[fi], T.childs, T.cmap, T.ffac, T.fd, T.rowptr, T.rowsrc);
}

// Gather lists of ONE HBM front from the entries its gather leaves registered.  Reads gp / gv (consumed), the plan's front and
// F.child_count; fills h->gather[fi] and appends to T.gpblk / gpent (pair blocks, the short ones first), T.gvblk / gvent (variable blocks:
// short first, each variable's leaf entries in front of its factor entries) and T.gzero (the blocks no list covers, when the gather may
// be the front's first writer).
void build_gather_lists(lmgpu_handle* h, LaunchTables& T, int fi, std::vector<GPairTmp>& gp, std::vector<GVarTmp>& gv) {
  const Plan& P = h->plan;
  const Front& fr = P.fronts[fi];
  lmgpu_handle::GatherRange& G = h->gather[fi];
  std::stable_sort(gp.begin(), gp.end(), [](const GPairTmp& a, const GPairTmp& b) { return a.key < b.key; });
  G.pblk_begin = (int)T.gpblk.size();
  std::vector<GPairBlock> longs;
  for (size_t i = 0; i < gp.size();) {
    size_t j = i;
    while (j < gp.size() && gp[j].key == gp[i].key) j++;
    const GPairBlock blk{(int32_t)(gp[i].key >> 32), (int32_t)(gp[i].key & 0xffffffff), gp[i].da, gp[i].db, (int32_t)T.gpent.size(), (int32_t)(j - i)};
    if (j - i <= 32) T.gpblk.push_back(blk); else longs.push_back(blk);
    for (size_t e = i; e < j; e++) T.gpent.push_back(gp[e].ent);
    i = j;
  }
  G.pblk_short = (int)T.gpblk.size() - G.pblk_begin;
  G.pblk_long = (int)longs.size();
  T.gpblk.insert(T.gpblk.end(), longs.begin(), longs.end());
  std::stable_sort(gv.begin(), gv.end(), [](const GVarTmp& a, const GVarTmp& b) { return a.pv < b.pv; });
  G.vblk_begin = (int)T.gvblk.size();
  std::vector<GVarBlock> vlongs;
  for (size_t i = 0; i < gv.size();) {
    size_t j = i;
    while (j < gv.size() && gv[j].pv == gv[i].pv) j++;
    // the variable's leaf entries first, then its factor entries, each in leaf (elimination) order
    int nleaf = 0;
    for (size_t e = i; e < j; e++)
      if (gv[e].leaf) nleaf++;
    const GVarBlock blk{gv[i].pv, gv[i].dv, 0, (int32_t)T.gvent.size(), (int32_t)(j - i), nleaf};
    const bool is_short = !h->sw.schur_split_diag && nleaf <= SCHUR_VAR_SHORT && (int)(j - i) - nleaf <= SCHUR_VAR_SHORT;
    if (is_short || h->sw.schur_split_diag) T.gvblk.push_back(blk); else vlongs.push_back(blk);
    for (int pass = 0; pass < 2; pass++)
      for (size_t e = i; e < j; e++)
        if (gv[e].leaf == (pass == 0)) T.gvent.push_back(gv[e].ent);
    i = j;
  }
  G.vblk_short = h->sw.schur_split_diag ? 0 : (int)T.gvblk.size() - G.vblk_begin;
  T.gvblk.insert(T.gvblk.end(), vlongs.begin(), vlongs.end());
  G.vblk_count = (int)T.gvblk.size() - G.vblk_begin;
  if (h->h_fronts[fi].child_count == 0) {  // no child adds to this front before its own level: the gather can be the first writer
    G.write_ok = true;
    G.zero_begin = (int)T.gzero.size();
    struct VB { int c, d; };
    std::vector<VB> vb;
    for (size_t k = 0; k < fr.vars.size(); k++) vb.push_back({fr.col_off[k], P.dims[fr.vars[k]]});
    vb.push_back({fr.n - 1, 1});
    std::vector<int64_t> covered;  // the keys of the blocks some list writes
    covered.reserve(G.pblk_short + G.pblk_long);
    for (int q = 0; q < G.pblk_short + G.pblk_long; q++)
      covered.push_back(((int64_t)T.gpblk[G.pblk_begin + q].pa << 32) | (uint32_t)T.gpblk[G.pblk_begin + q].pb);
    if (!h->sw.schur_split_diag) {  // a variable block covers (v, v) and (v, rhs); the corner workgroup covers (rhs, rhs)
      for (int q = 0; q < G.vblk_count; q++) {
        const int32_t pv = T.gvblk[G.vblk_begin + q].pv;
        covered.push_back(((int64_t)pv << 32) | (uint32_t)pv);
        covered.push_back(((int64_t)pv << 32) | (uint32_t)(fr.n - 1));
      }
      if (G.leaf_count > 0) covered.push_back(((int64_t)(fr.n - 1) << 32) | (uint32_t)(fr.n - 1));
    }
    std::sort(covered.begin(), covered.end());
    for (size_t x = 0; x < vb.size(); x++)
      for (size_t y = x; y < vb.size(); y++) {
        const int64_t key = ((int64_t)vb[x].c << 32) | (uint32_t)vb[y].c;
        if (!std::binary_search(covered.begin(), covered.end(), key)) T.gzero.push_back(GZeroBlock{vb[x].c, vb[y].c, (int16_t)vb[x].d, (int16_t)vb[y].d});
      }
    G.zero_count = (int)T.gzero.size() - G.zero_begin;
  }
  std::vector<GPairTmp>().swap(gp);
  std::vector<GVarTmp>().swap(gv);
}

// Per-front tables, front by front in elimination order.  Reads the plan, the pool layout and T.fd; fills the list half of h_fronts
// (fac / child / fx / sx ranges, par_map), T.ffac, T.childs, T.cmap, T.fxoff, T.sxoff and, through the three functions above, the
// gather lists and the row sources of the HBM fronts (h->gather, h->row_begin).
int build_front_tables(lmgpu_handle* h, LaunchTables& T) {
  const Plan& P = h->plan;
  const int NF = (int)P.fronts.size(), R = h->cfg.rank;
  h->gather.assign(NF, lmgpu_handle::GatherRange());
  h->row_begin.assign(NF, -1);
  std::vector<GPairTmp> gp;
  std::vector<GVarTmp> gv;
  std::vector<int32_t> colof(P.n_vars, -1);
  for (int fi = 0; fi < NF; fi++) {
    if (!h->front_active[fi]) continue;
    const Front& fr = P.fronts[fi];
    FrontDesc& F = h->h_fronts[fi];
    for (size_t k = 0; k < fr.vars.size(); k++) colof[fr.vars[k]] = fr.col_off[k];
    F.fac_begin = (int)T.ffac.size();
    for (int32_t f : fr.factors) {
      const int32_t* v = P.factors[f].slots;
      T.ffac.push_back(FrontFac{h->fac_local[f], colof[v[0]], v[1] >= 0 ? colof[v[1]] : 0, v[2] >= 0 ? colof[v[2]] : 0});
    }
    F.fac_count = (int)T.ffac.size() - F.fac_begin;
    // children present on this rank: map child's separator scalars (+ rhs) to this front's columns
    F.child_begin = (int)T.childs.size();
    for (int32_t c : fr.children) {
      if (!h->front_active[c]) continue;
      // a replicated child of a replicated front is identical on every rank: its update matrix enters the parent's sum over the ranks once
      if ((F.pad & 1) && (h->h_fronts[c].pad & 1) && R != 0) continue;
      const Front& ch = P.fronts[c];
      const FrontDesc& CF = h->h_fronts[c];
      if (CF.par_ld < 0) {  // gather-mode leaf: no update matrix, no column map
        const int rc = add_gather_leaf(h, T, fi, c, colof, gp, gv);
        if (rc) return rc;
        continue;
      }
      // (pad = the child front + 1: merged launches wait for children of their own launch)
      T.childs.push_back(ChildRef{CF.u_off, CF.ld_u, ch.n - ch.nf, (int)T.cmap.size(), c + 1});
      for (size_t k = ch.n_frontal_vars; k < ch.vars.size(); k++)
        for (int d = 0; d < P.dims[ch.vars[k]]; d++) T.cmap.push_back(colof[ch.vars[k]] + d);
      T.cmap.push_back(fr.n - 1);
    }
    F.child_count = (int)T.childs.size() - F.child_begin;
    if (fr.cls == 1 && (F.child_count > 0 || F.fac_count > 0)) build_row_sources(h, T, fi);
    if (!gp.empty() || !gv.empty()) build_gather_lists(h, T, fi, gp, gv);
    F.fx_begin = (int)T.fxoff.size();
    for (int k = 0; k < fr.n_frontal_vars; k++)
      for (int d = 0; d < P.dims[fr.vars[k]]; d++) T.fxoff.push_back(P.xoff[fr.vars[k]] + d);
    F.sx_begin = (int)T.sxoff.size();
    for (size_t k = fr.n_frontal_vars; k < fr.vars.size(); k++)
      for (int d = 0; d < P.dims[fr.vars[k]]; d++) T.sxoff.push_back(P.xoff[fr.vars[k]] + d);
  }
  return LMGPU_OK;
}

// Level work lists (active fronts only).  Reads the plan, h_fronts and T.fd; fills h->levels (hbm, the bins of the LDS fronts with their
// rows, staging capacity and maxima) and T.lists, the LDS fronts level by level and bin by bin.
void build_level_lists(lmgpu_handle* h, LaunchTables& T) {
  const Plan& P = h->plan;
  const int NF = (int)P.fronts.size();
  h->levels.assign(P.n_levels, LevelWork());
  std::vector<std::vector<std::vector<int>>> byLevelBin(P.n_levels, std::vector<std::vector<int>>(kNumBins));
  for (int fi = 0; fi < NF; fi++) {
    if (!h->front_active[fi]) continue;
    const Front& fr = P.fronts[fi];
    if (fr.cls == 1) {
      h->levels[fr.level].hbm.push_back(fi);
    } else {
      int b = 0;
      while (fr.n > kBinN[b]) b++;
      if (h->h_fronts[fi].par_ld < 0) b += 6;  // gather leaf
      byLevelBin[fr.level][b].push_back(fi);
    }
  }
  // narrow levels (the upper part of a general clique tree): every launch is bound by one front's latency, so fronts of
  // different LDS sizes share ONE launch (the largest occupied bin of the group) instead of up to six
  for (int l = 0; l < P.n_levels; l++)
    for (int g0 = 0; g0 < kNumBins; g0 += 6) {
      size_t total = 0;
      int top = -1;
      for (int b = g0; b < g0 + 6; b++) {
        total += byLevelBin[l][b].size();
        if (!byLevelBin[l][b].empty()) top = b;
      }
      if (top < 0 || total > 512) continue;
      for (int b = g0; b < top; b++) {
        byLevelBin[l][top].insert(byLevelBin[l][top].end(), byLevelBin[l][b].begin(), byLevelBin[l][b].end());
        byLevelBin[l][b].clear();
      }
    }
  for (int l = 0; l < P.n_levels; l++) {
    LevelWork& L = h->levels[l];
    L.list_begin = (int)T.lists.size();
    int c = 0;
    for (int b = 0; b < kNumBins; b++) {
      L.bin_begin[b] = c;
      L.bin_srows[b] = kBinN[b % 6];
      if (b >= 6) {
        int mx = 1;
        for (int fi : byLevelBin[l][b]) mx = std::max(mx, P.fronts[fi].nf);
        L.bin_srows[b] = mx;
      }
      int jc = 96;
      for (int fi : byLevelBin[l][b]) {
        int tot = 0;
        for (int32_t f : P.fronts[fi].factors) {
          const FacDesc& d = T.fd[h->fac_local[f]];
          tot += d.rows * (d.d0 + d.d1 + d.d2 + 1);
        }
        jc = std::max(jc, std::min(tot, LDSF_JCAP));
      }
      L.bin_jcap[b] = (jc + 7) & ~7;
      for (int fi : byLevelBin[l][b]) {
        T.lists.push_back(fi);
        L.lds_nf_max = std::max(L.lds_nf_max, (int)P.fronts[fi].nf);
        L.lds_ns_max = std::max(L.lds_ns_max, (int)P.fronts[fi].n - (int)P.fronts[fi].nf - 1);
        L.lds_rsd_max = std::max(L.lds_rsd_max, (int)P.fronts[fi].nf * ((int)P.fronts[fi].n | 1));
      }
      c += (int)byLevelBin[l][b].size();
    }
    L.bin_begin[kNumBins] = c;
    L.list_count = c;
  }
  h->n_lds_fronts = (int)T.lists.size();
}

// Gather-leaf bins whose launch takes lds_front_group_kernel: decided per bin launch, from the structure alone.  Reads the levels'
// bins, T.lists, h_fronts, T.ffac and T.fd; fills bin_group / bin_group_out / bin_group_maxfac of every level and n_leaf_group_launches.
void build_leaf_group_bins(lmgpu_handle* h, const LaunchTables& T) {
  h->n_leaf_group_launches = 0;
  if (h->sw.no_leaf_groups || h->sw.no_leafpack || h->pcg_structure) return;
  for (LevelWork& L : h->levels)
    for (int b = 6; b < kNumBins; b++) {
      const int cnt = L.bin_begin[b + 1] - L.bin_begin[b];
      int form = cnt > 0 ? 1 : 0;
      for (int q = 0; q < cnt && form; q++) {
        const FrontDesc& F = h->h_fronts[T.lists[L.list_begin + L.bin_begin[b] + q]];
        const int f = leaf_group_form(F, T.ffac.data(), T.fd.data(), L.bin_jcap[b]);
        form = f ? std::max(form, f) : 0;
        L.bin_group_out[b] = std::max(L.bin_group_out[b], F.nf * F.n);
        L.bin_group_maxfac[b] = std::max(L.bin_group_maxfac[b], F.fac_count);
      }
      L.bin_group[b] = (uint8_t)form;
      if (form) h->n_leaf_group_launches++;
    }
}

// Merged elimination launches: runs of consecutive levels, each a handful of LDS fronts, with no dense front between them (only the top
// level of a run may hold dense fronts: they are launched after it and nothing in the run depends on them).  Reads the levels
// (level_lds_class); fills elim_segs and elim_seg_of.
void build_elim_segments(lmgpu_handle* h) {
  const int n_levels = (int)h->levels.size();
  h->elim_segs.clear();
  h->elim_seg_of.assign(n_levels, -1);
  int l = 0;
  while (l < n_levels) {
    int nmax, jcap, threads;
    if (!level_lds_class(h, l, &nmax, &jcap, &threads)) {
      l++;
      continue;
    }
    lmgpu_handle::ElimSeg E{l, l, nmax, jcap, threads};
    while (E.lvl_hi + 1 < n_levels && h->levels[E.lvl_hi].hbm.empty()) {
      int n2, j2, t2;
      if (!level_lds_class(h, E.lvl_hi + 1, &n2, &j2, &t2) || (t2 == 1024) != (E.threads == 1024)) break;
      E.lvl_hi++;
      E.nmax = std::max(E.nmax, n2);
      E.jcap = std::max(E.jcap, j2);
      E.threads = std::max(E.threads, t2);
    }
    if (E.lvl_hi > E.lvl_lo) {
      h->elim_seg_of[E.lvl_lo] = (int)h->elim_segs.size();
      for (int q = E.lvl_lo + 1; q <= E.lvl_hi; q++) h->elim_seg_of[q] = -2;
      h->elim_segs.push_back(E);
    }
    l = E.lvl_hi + 1;
  }
}

// Solve-form flags.  Reads the levels, elim_segs, the communicator size and the switches; fills n_hbm_fronts, use_graph, merge_backsub,
// merge_elim, fuse_levels (build_fused_levels takes that one back when no level qualifies) and, for the merged elimination launches,
// T.fill_upper: the update matrices their fronts preset to "not published yet".
void build_solve_flags(lmgpu_handle* h, LaunchTables& T) {
  h->n_hbm_fronts = 0;
  for (const LevelWork& L : h->levels) h->n_hbm_fronts += (int)L.hbm.size();
  // deep trees are launch-bound: replay the solve as a graph (LMGPU_GRAPH=0 / 1 overrides the depth rule)
  const bool deep = (int)h->levels.size() >= 12, one_rank = h->cfg.world_size == 1;
  h->use_graph = deep;
  h->merge_backsub = deep;
  if (h->sw.merge_backsub >= 0) h->merge_backsub = h->sw.merge_backsub != 0;
  h->merge_elim = deep && one_rank;
  if (h->sw.merge_elim >= 0) h->merge_elim = h->sw.merge_elim != 0 && one_rank;
  if (h->elim_segs.empty()) h->merge_elim = false;
  if (h->sw.graph >= 0) h->use_graph = h->sw.graph != 0;
  h->fuse_levels = deep && one_rank;
  if (h->sw.fuse_levels >= 0) h->fuse_levels = h->sw.fuse_levels != 0 && one_rank;
  if (h->merge_elim)
    for (const lmgpu_handle::ElimSeg& E : h->elim_segs)
      for (int q = h->levels[E.lvl_lo].list_begin; q < h->levels[E.lvl_hi].list_begin + h->levels[E.lvl_hi].list_count; q++) {
        const FrontDesc& F = h->h_fronts[T.lists[q]];
        T.fill_upper.push_back(FillUpper{F.u_off, F.n - F.nf, F.ld_u});
      }
  h->n_fill_upper = (int)T.fill_upper.size();
}

// Packed records of the LDS fronts, launch by launch (kernels_front.hpp, LEAFPACK_*): the front's descriptor, a header, its frontal
// offsets and its factors in one 128-byte-aligned record.  Reads the levels' bins, T.lists, h_fronts, T.ffac, T.fd and T.fxoff; fills
// T.packs and every level's pack_off / pack_stride.  LMGPU_NO_LEAFPACK: none.
void build_leaf_packs(lmgpu_handle* h, LaunchTables& T) {
  if (h->sw.no_leafpack) return;
  std::vector<char>& packs = T.packs;
  for (LevelWork& L : h->levels)
    for (int b = 0; b < kNumBins; b++) {
      const int cnt = L.bin_begin[b + 1] - L.bin_begin[b];
      if (cnt == 0) continue;
      const int32_t* list = T.lists.data() + L.list_begin + L.bin_begin[b];
      int maxfac = 0;
      for (int q = 0; q < cnt; q++) maxfac = std::max(maxfac, std::min((int)LDSF_MAXB, h->h_fronts[list[q]].fac_count));
      const int stride = LEAFPACK_FAC + 32 * std::max(1, maxfac);
      packs.resize((packs.size() + 127) & ~size_t(127));
      L.pack_off[b] = (int64_t)packs.size();
      L.pack_stride[b] = stride;
      packs.resize(packs.size() + (size_t)cnt * stride, 0);
      for (int q = 0; q < cnt; q++) {
        const FrontDesc& F = h->h_fronts[list[q]];
        char* rec = packs.data() + L.pack_off[b] + (size_t)q * stride;
        std::memcpy(rec, &F, sizeof(FrontDesc));
        int32_t* hdr = (int32_t*)(rec + LEAFPACK_HDR);
        hdr[0] = hdr[1] = hdr[2] = hdr[3] = 0;
        if (F.fac_count < 1 || F.fac_count > LDSF_MAXB) continue;
        LFac* lf = (LFac*)(rec + LEAFPACK_FAC);
        int o = 0;
        bool contig = true;
        for (int k = 0; k < F.fac_count; k++) {
          const FrontFac& ff = T.ffac[F.fac_begin + k];
          const FacDesc& d = T.fd[ff.fac];
          lf[k] = LFac{d.joff, ff.c0, ff.c1, d.rows, d.d0, d.d1, d.d2, ff.c2, (int16_t)o, (int16_t)(d.rows * (d.d0 + d.d1 + d.d2 + 1))};
          if (k > 0 && lf[k].joff != lf[0].joff + o) contig = false;
          o += lf[k].sz;
        }
        if (o > L.bin_jcap[b]) continue;  // more than one staging batch: the general path
        hdr[0] = F.fac_count;
        hdr[1] = o;
        hdr[2] = contig ? 1 : 0;
        if (F.nf <= LEAFPACK_MAXNF) {
          hdr[3] = 1;
          int32_t* xo = (int32_t*)(rec + LEAFPACK_XO);
          for (int i = 0; i < F.nf; i++) xo[i] = T.fxoff[F.fx_begin + i];
        }
      }
    }
}

// Back-substitution tables.  Reads the plan, the levels, T.lists, h_fronts, f_off and f_ld; fills T.bs_parent / T.bs_pos (merged LDS
// launches: the LDS parent of a front, its place in T.lists), T.small and T.bsd (the HBM fronts of nf <= BSS_MAX_NF per level and
// their 64-row blocks, last block first) with the levels' small_* / bsd_* ranges and bsd_x_count, and the runs of levels that hold
// nothing but such fronts: bsd_runs, bsd_run_of and T.bsd_runs_table.
void build_backsub_tables(lmgpu_handle* h, LaunchTables& T) {
  const Plan& P = h->plan;
  const int NF = (int)P.fronts.size();
  T.bs_parent.assign(NF, -1);
  T.bs_pos.assign(NF, -1);
  for (size_t q = 0; q < T.lists.size(); q++) T.bs_pos[T.lists[q]] = (int32_t)q;
  for (int fi = 0; fi < NF; fi++) {
    const int par = P.fronts[fi].parent;
    if (par >= 0 && P.fronts[par].cls == 0) T.bs_parent[fi] = par;
  }
  for (LevelWork& L : h->levels) {
    L.small_begin = (int)T.small.size();
    for (int fi : L.hbm)
      if (P.fronts[fi].nf <= BSS_MAX_NF) T.small.push_back(fi);
    L.small_count = (int)T.small.size() - L.small_begin;
  }
  int32_t xoff = 0;
  for (LevelWork& L : h->levels) {
    L.bsd_begin = (int)T.bsd.size();
    for (int q = 0; q < L.small_count; q++) {
      const int fi = T.small[L.small_begin + q], nblk = (P.fronts[fi].nf + 63) / 64;
      const FrontDesc& F = h->h_fronts[fi];
      for (int b = nblk - 1; b >= 0; b--) T.bsd.push_back(BsdBlock{h->f_off[fi], h->f_ld[fi], F.n, F.nf, F.fx_begin, F.sx_begin, F.id, b, xoff});
      xoff += 64 * nblk;
    }
    L.bsd_count = (int)T.bsd.size() - L.bsd_begin;
  }
  h->bsd_x_count = (size_t)xoff;
  h->bsd_runs.clear();
  h->bsd_run_of.assign(h->levels.size(), -1);
  // a level can open a run when every HBM front on it is block-solved; the next level down joins when, in addition, none of its
  // fronts hangs below an LDS front of the run's levels (those are solved by the merged LDS launch BEHIND the run's launch)
  auto opens = [&](int l) {
    const LevelWork& L = h->levels[l];
    return L.bsd_count > 0 && L.small_count == (int)L.hbm.size();
  };
  auto joins = [&](int l, int hi) {
    if (!opens(l)) return false;
    for (int fi : h->levels[l].hbm) {
      const int par = P.fronts[fi].parent;
      if (par >= 0 && P.fronts[par].cls != 1 && P.fronts[par].level <= hi) return false;
    }
    return true;
  };
  int l = (int)h->levels.size() - 1;
  while (l >= 0) {
    if (!opens(l)) {
      l--;
      continue;
    }
    int lo = l;
    while (lo - 1 >= 0 && joins(lo - 1, l)) lo--;
    if (lo < l) {
      lmgpu_handle::BsdRun R{l, lo, (int)T.bsd_runs_table.size(), 0};
      for (int q = l; q >= lo; q--)
        T.bsd_runs_table.insert(T.bsd_runs_table.end(), T.bsd.begin() + h->levels[q].bsd_begin, T.bsd.begin() + h->levels[q].bsd_begin + h->levels[q].bsd_count);
      R.count = (int)T.bsd_runs_table.size() - R.begin;
      h->bsd_run_of[l] = (int)h->bsd_runs.size();
      for (int q = l - 1; q >= lo; q--) h->bsd_run_of[q] = -2;
      h->bsd_runs.push_back(R);
    }
    l = lo - 1;
  }
}

// Medium fronts (one outer panel, no gather leaves, not replicated: eliminated with batched launches) and the fused level launches.
// Reads the levels, h_fronts, gather, f_off, f_ld, row_begin, elim_seg_of and the flags; fills is_med, T.med, T.med_fronts, T.max_med, the
// levels' med_* maxima and, per level that takes level_fused_kernel, its fuse_* fields and its slice of T.level_tasks:
// [LDS fronts | assembly rows | diagonal blocks | panel strips | update quadrants].  No such level: fuse_levels goes back to false.
void build_fused_levels(lmgpu_handle* h, LaunchTables& T) {
  const Plan& P = h->plan;
  h->is_med.assign(P.fronts.size(), 0);
  for (LevelWork& L : h->levels) {
    L.med_begin = (int)T.med.size();
    for (int fi : L.hbm) {
      const Front& fr = P.fronts[fi];
      const FrontDesc& F = h->h_fronts[fi];
      const lmgpu_handle::GatherRange& G = h->gather[fi];
      if (fr.nf > NBO || (F.pad & 1) || G.leaf_count > 0 || G.pblk_short + G.pblk_long + G.vblk_count > 0 || h->sw.no_med) continue;
      T.med.push_back(fi);
      T.med_fronts.push_back(MedFront{F, h->f_off[fi], h->f_ld[fi], h->row_begin[fi]});
      h->is_med[fi] = 1;
      L.med_max_fac = std::max(L.med_max_fac, F.fac_count);
      L.med_max_child = std::max(L.med_max_child, F.child_count);
      L.med_max_nf = std::max(L.med_max_nf, fr.nf);
      L.med_max_cols = std::max(L.med_max_cols, fr.n - fr.nf);
      L.med_max_n = std::max(L.med_max_n, (int)fr.n);
    }
    L.med_count = (int)T.med.size() - L.med_begin;
    T.max_med = std::max(T.max_med, L.med_count);
  }
  std::vector<LevelTask>& tasks = T.level_tasks;
  for (size_t l = 0; l < h->levels.size(); l++) {
    LevelWork& L = h->levels[l];
    L.fuse_task_count = 0;
    int nmax, jcap, threads;
    if (!h->fuse_levels || L.med_count == 0 || !(L.med_max_fac > 0 || L.med_max_child > 0)) continue;
    if (h->merge_elim && h->elim_seg_of[l] != -1) continue;  // its LDS fronts belong to a merged launch
    if (!level_lds_class(h, (int)l, &nmax, &jcap, &threads)) continue;
    L.fuse_task_begin = (int)tasks.size();
    L.fuse_nmax = nmax;
    L.fuse_jcap = jcap;
    // four waves per workgroup for every role: with sixteen (what a launch of wide LDS fronts alone takes) the kernel is held to 128 VGPRs and the
    // register Cholesky of the dense fronts' diagonal blocks spills (sphere2500: 1.93 vs 1.87 ms)
    L.fuse_threads = 256;
    if (h->sw.fuse_threads) L.fuse_threads = h->sw.fuse_threads == 1024 && threads == 1024 ? 1024 : 256;
    for (int q = 0; q < L.list_count; q++) tasks.push_back(LevelTask{0, L.list_begin + q, 0, 0});
    for (int m = 0; m < L.med_count; m++) {
      const FrontDesc& F = T.med_fronts[L.med_begin + m].F;
      for (int r = 0; r < F.n; r += 4) tasks.push_back(LevelTask{1, m, r, 0});
    }
    for (int m = 0; m < L.med_count; m++) tasks.push_back(LevelTask{2, m, 0, 0});
    for (int m = 0; m < L.med_count; m++) {
      const FrontDesc& F = T.med_fronts[L.med_begin + m].F;
      for (int st = 0; st * 64 < F.n - F.nf; st++) tasks.push_back(LevelTask{3, m, st, 0});
    }
    for (int m = 0; m < L.med_count; m++) {
      const FrontDesc& F = T.med_fronts[L.med_begin + m].F;
      const int S = (F.n - F.nf + 63) / 64;
      for (int sj = 0; sj < S; sj++)
        for (int si = 0; si <= sj; si++)
          for (int qd = 0; qd < 4; qd++) tasks.push_back(LevelTask{4, m, si | (sj << 8), qd});
    }
    L.fuse_task_count = (int)tasks.size() - L.fuse_task_begin;
  }
  if (tasks.empty()) h->fuse_levels = false;
  else h->n_level_sync = (int)T.med_fronts.size();
}

// Marginal path walks (kernels_marginals.hpp).  Reads the plan and the sx ranges of h_fronts; fills marg_poff (poff[root] = 0, poff[child] =
// poff[parent] + nf[parent]: fronts are in post-order, so a parent is placed before its children when the list is walked backwards),
// marg_depth, marg_vcol (first scalar of every slot inside the front it is frontal in), marg_spos (parallel to T.sxoff: the separator
// scalar's path position = poff of the ancestor it is frontal in + its column there) and T.marg_parent.
void build_marginal_tables(lmgpu_handle* h, LaunchTables& T) {
  const Plan& P = h->plan;
  const int NF = (int)P.fronts.size();
  h->marg_poff.assign(NF, 0);
  h->marg_depth.assign(NF, 0);
  h->marg_vcol.assign(P.n_vars, 0);
  h->marg_spos.assign(T.sxoff.size(), -1);
  T.marg_parent.assign(NF, -1);
  for (int fi = NF - 1; fi >= 0; fi--) {
    const Front& fr = P.fronts[fi];
    T.marg_parent[fi] = fr.parent;
    if (fr.parent >= 0) {
      h->marg_poff[fi] = h->marg_poff[fr.parent] + P.fronts[fr.parent].nf;
      h->marg_depth[fi] = h->marg_depth[fr.parent] + 1;
    }
    for (int k = 0; k < fr.n_frontal_vars; k++) h->marg_vcol[fr.vars[k]] = fr.col_off[k];
  }
  for (int fi = 0; fi < NF; fi++) {
    if (!h->front_active[fi]) continue;
    const Front& fr = P.fronts[fi];
    int32_t* sp = h->marg_spos.data() + h->h_fronts[fi].sx_begin;
    for (size_t k = fr.n_frontal_vars; k < fr.vars.size(); k++) {
      const int32_t v = fr.vars[k];
      for (int d = 0; d < P.dims[v]; d++) *sp++ = h->marg_poff[P.front_of_var[v]] + h->marg_vcol[v] + d;
    }
  }
}

#ifdef LMGPU_TEST_HOOKS
// ---- the digest tap (lmgpu_debug_table_digest): one record (name, entries, FNV-1a) per table of LaunchTables and per piece of the
// handle's launch metadata, taken at the end of the build; the tables themselves are not retained.  Fields are hashed, never padding:
// put() refuses a type whose bytes are not all value.  Tables of device addresses (FillChunk) are not part of it.
struct Fnv1a {
  uint64_t v = 14695981039346656037ull;
  void bytes(const void* p, size_t n) {
    for (size_t i = 0; i < n; i++) v = (v ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  }
  template <typename X>
  void put(const X& x) {
    static_assert(std::has_unique_object_representations_v<X>, "padding is undefined after aggregate initialisation: hash the fields");
    bytes(&x, sizeof(X));
  }
  template <typename X>
  void put(const std::vector<X>& x) {
    static_assert(std::has_unique_object_representations_v<X>, "padding is undefined after aggregate initialisation: hash the fields");
    bytes(x.data(), x.size() * sizeof(X));
  }
};
void digest_rec(lmgpu_handle* h, const char* name, uint64_t count, const Fnv1a& f) {
  lmgpu_handle::DigestRec r{};
  std::strncpy(r.name, name, sizeof(r.name) - 1);
  r.count = count;
  r.fnv1a = f.v;
  h->table_digest.push_back(r);
}
template <typename X>
void digest_vec(lmgpu_handle* h, const char* name, const std::vector<X>& t) {
  Fnv1a f;
  f.put(t);
  digest_rec(h, name, t.size(), f);
}
void digest_int(lmgpu_handle* h, const char* name, int64_t x) {
  Fnv1a f;
  f.put(x);
  digest_rec(h, name, 1, f);
}
// LevelWork, in the parts the phases fill: 0 lists, 1 leaf groups, 2 packs, 3 back-substitution, 4 medium fronts, 5 fused launches
void digest_levels(lmgpu_handle* h, int part) {
  static const char* const names[6] = {"levels.lists", "levels.groups", "levels.packs", "levels.backsub", "levels.med", "levels.fuse"};
  Fnv1a f;
  for (const LevelWork& L : h->levels) {
    if (part == 0) {
      for (int x : {L.list_begin, L.list_count, L.lds_nf_max, L.lds_ns_max, L.lds_rsd_max}) f.put(x);
      f.put(L.bin_begin), f.put(L.bin_srows), f.put(L.bin_jcap);
      f.put((int)L.hbm.size()), f.put(L.hbm);
    }
    if (part == 1) f.put(L.bin_group), f.put(L.bin_group_out), f.put(L.bin_group_maxfac);
    if (part == 2) f.put(L.pack_off), f.put(L.pack_stride);
    if (part == 3)
      for (int x : {L.small_begin, L.small_count, L.bsd_begin, L.bsd_count}) f.put(x);
    if (part == 4)
      for (int x : {L.med_begin, L.med_count, L.med_max_fac, L.med_max_child, L.med_max_nf, L.med_max_cols, L.med_max_n}) f.put(x);
    if (part == 5)
      for (int x : {L.fuse_task_begin, L.fuse_task_count, L.fuse_nmax, L.fuse_jcap, L.fuse_threads}) f.put(x);
  }
  digest_rec(h, names[part], h->levels.size(), f);
}
// ownership, pool layout, per-front metadata, gather ranges and merged elimination segments
void digest_structure(lmgpu_handle* h) {
  Fnv1a f;
  f.put(h->n_counted), f.put(h->nfac), f.put(h->fac_local);
  digest_rec(h, "fac_local", h->fac_local.size(), f);
  Fnv1a fb;
  for (const Bucket& b : h->buckets) fb.put(b.joff), fb.put(b.n_loc);
  digest_rec(h, "buckets", h->buckets.size(), fb);
  digest_int(h, "pool_doubles", (int64_t)h->pool_doubles);
  digest_vec(h, "h_fronts", h->h_fronts);
  digest_vec(h, "f_off", h->f_off);
  digest_vec(h, "f_ld", h->f_ld);
  digest_vec(h, "s_off", h->s_off);
  digest_vec(h, "row_begin", h->row_begin);
  Fnv1a fg;
  for (const lmgpu_handle::GatherRange& G : h->gather)
    for (int x : {G.pblk_begin, G.pblk_short, G.pblk_long, G.vblk_begin, G.vblk_count, G.leaf_begin, G.leaf_count, G.vblk_short, (int)G.write_ok,
                  G.zero_begin, G.zero_count})
      fg.put(x);
  digest_rec(h, "gather", h->gather.size(), fg);
  Fnv1a fe;
  fe.put(h->elim_segs), fe.put(h->elim_seg_of), fe.put(h->n_leaf_group_launches);
  digest_rec(h, "elim_segs", h->elim_segs.size(), fe);
}
// what the phases behind the merged elimination segments leave on the handle
void digest_solve_forms(lmgpu_handle* h) {
  Fnv1a f;
  for (int x : {h->n_hbm_fronts, (int)h->use_graph, (int)h->merge_backsub, (int)h->merge_elim, (int)h->fuse_levels}) f.put(x);
  digest_rec(h, "flags", 5, f);
  Fnv1a fr;
  fr.put(h->bsd_runs), fr.put(h->bsd_run_of), fr.put((int64_t)h->bsd_x_count);
  digest_rec(h, "bsd_runs", h->bsd_runs.size(), fr);
  digest_vec(h, "is_med", h->is_med);
}
void digest_tables(lmgpu_handle* h, const LaunchTables& T) {
  h->table_digest.clear();
  digest_vec(h, "fd", T.fd), digest_vec(h, "ffac", T.ffac), digest_vec(h, "childs", T.childs), digest_vec(h, "cmap", T.cmap);
  digest_vec(h, "fxoff", T.fxoff), digest_vec(h, "sxoff", T.sxoff), digest_vec(h, "lists", T.lists);
  digest_vec(h, "rowptr", T.rowptr), digest_vec(h, "rowsrc", T.rowsrc);
  digest_vec(h, "gpblk", T.gpblk), digest_vec(h, "gpent", T.gpent), digest_vec(h, "gvblk", T.gvblk), digest_vec(h, "gvent", T.gvent);
  digest_vec(h, "gzero", T.gzero), digest_int(h, "n_gleaf", T.n_gleaf);
  digest_vec(h, "packs", T.packs), digest_vec(h, "bs_parent", T.bs_parent), digest_vec(h, "bs_pos", T.bs_pos);
  digest_vec(h, "fill_upper", T.fill_upper), digest_vec(h, "small", T.small), digest_vec(h, "bsd", T.bsd);
  digest_vec(h, "bsd_runs_table", T.bsd_runs_table), digest_vec(h, "med", T.med), digest_vec(h, "med_fronts", T.med_fronts);
  digest_vec(h, "level_tasks", T.level_tasks), digest_int(h, "max_med", T.max_med), digest_int(h, "max_nf", T.max_nf);
  digest_structure(h);
  for (int part = 0; part < 6; part++) digest_levels(h, part);
  digest_solve_forms(h);
}
#endif  // LMGPU_TEST_HOOKS

}  // namespace
