// sdm_chol_build.hip -- host-side symbolic planning of the multifrontal LDL' (sdm_chol.hip): fronts, elimination-tree levels, the
// maps of the assembly and the launch schedule of every level.  No kernel is defined or launched here.
#include "sdm_chol_sched.h"
#include <algorithm>

namespace sdm {

// ============================================================ host analysis
void chol_build(sdm_plan *P, sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const sdm_int *perm,
                sdm_int nsuper, const sdm_int *xsuper, const sdm_int *ADAjc, const sdm_int *ADAir) {
  CholPlan &C = P->chol;
  C.begun = false;                                                   // (a staged factorisation of the previous factor ends here)
  C.m = m; C.nsuper = nsuper; C.nnzL = Ljc[m]; C.nnzADA = ADAjc[m];
  if (C.nnzADA >= (sdm_int)1 << 31) throw std::runtime_error("nnz(ADA) >= 2^31 not supported");
  C.Ljc.assign(Ljc, Ljc + m + 1);
  C.perm.assign(perm, perm + m);
  std::vector<int> snode(m);
  C.sn_first.resize(nsuper); C.sn_ns.resize(nsuper); C.sn_ms.resize(nsuper); C.sn_ld.resize(nsuper);
  C.sn_parent.assign(nsuper, -1); C.sn_level.assign(nsuper, 0);
  C.sn_foff.resize(nsuper); C.sn_xl.resize(nsuper); C.sn_woff.resize(nsuper); C.sn_roff.assign(nsuper, 0);
  C.sn_toff.resize(nsuper);
  int64_t foff = 0, xl = 0, toff = 0;
  C.maxms = 0; C.maxns = 0;
  for (sdm_int s = 0; s < nsuper; s++) {
    sdm_int f = xsuper[s], n = xsuper[s + 1] - f, ms = Ljc[f + 1] - Ljc[f];
    if (n <= 0 || ms < n) throw std::runtime_error("bad supernode partition");
    for (sdm_int j = f; j < f + n; j++) {
      snode[j] = (int)s;
      if (Ljc[j + 1] - Ljc[j] != ms - (j - f)) throw std::runtime_error("L.L columns are not nested within a supernode");
    }
    C.sn_first[s] = (int)f; C.sn_ns[s] = (int)n; C.sn_ms[s] = (int)ms;
    C.sn_foff[s] = foff; C.sn_xl[s] = xl; C.sn_woff[s] = xl; C.sn_toff[s] = toff;
    C.sn_ld[s] = (int)(ms + (ms & 1));                        // even leading dimension: 16-byte aligned row pairs in every column
    foff += (int64_t)C.sn_ld[s] * ms; xl += ms; toff += (int64_t)((n + NB - 1) / NB) * NB * NB;
    C.maxms = std::max(C.maxms, (int)ms); C.maxns = std::max(C.maxns, (int)n);
  }
  C.fsize = foff; C.wsize = xl; C.tsize = toff;
  // compressed subscripts (row list of the first column of every supernode)
  std::vector<int> lindx((size_t)xl);
  for (sdm_int s = 0; s < nsuper; s++) {
    const sdm_int *r = Lir + Ljc[C.sn_first[s]];
    for (int i = 0; i < C.sn_ms[s]; i++) lindx[C.sn_xl[s] + i] = (int)r[i];
  }
  // supernodal etree: parent = supernode of the first row below the block
  for (sdm_int s = 0; s < nsuper; s++)
    if (C.sn_ms[s] > C.sn_ns[s]) C.sn_parent[s] = snode[lindx[C.sn_xl[s] + C.sn_ns[s]]];
  C.childptr.assign(nsuper + 1, 0);
  for (sdm_int s = 0; s < nsuper; s++) if (C.sn_parent[s] >= 0) C.childptr[C.sn_parent[s] + 1]++;
  for (sdm_int s = 0; s < nsuper; s++) C.childptr[s + 1] += C.childptr[s];
  C.childlist.resize(C.childptr[nsuper]);
  { std::vector<int> pos(C.childptr.begin(), C.childptr.end() - 1);
    for (sdm_int s = 0; s < nsuper; s++) if (C.sn_parent[s] >= 0) C.childlist[pos[C.sn_parent[s]]++] = (int)s; }
  // levels (parents have larger indices than children: postordered)
  int nlev = 0;
  for (sdm_int s = 0; s < nsuper; s++) {
    int p = C.sn_parent[s];
    if (p >= 0) { if (p <= s) throw std::runtime_error("supernodes not postordered"); C.sn_level[p] = std::max(C.sn_level[p], C.sn_level[s] + 1); }
    nlev = std::max(nlev, C.sn_level[s] + 1);
  }
  C.nlevels = nlev;
  if (!C.sn_active.empty() && (sdm_int)C.sn_active.size() != nsuper) throw std::runtime_error("active-supernode mask does not match the supernode partition");
  auto active = [&](sdm_int s) { return C.sn_active.empty() || C.sn_active[s] != 0; };
  C.levptr.assign(nlev + 1, 0);
  for (sdm_int s = 0; s < nsuper; s++) if (active(s)) C.levptr[C.sn_level[s] + 1]++;
  for (int l = 0; l < nlev; l++) C.levptr[l + 1] += C.levptr[l];
  C.levlist.resize(C.levptr[nlev]);
  { std::vector<int> pos(C.levptr.begin(), C.levptr.end() - 1);
    for (sdm_int s = 0; s < nsuper; s++) if (active(s)) C.levlist[pos[C.sn_level[s]]++] = (int)s; }
  for (int l = 0; l < nlev; l++)
    std::stable_sort(C.levlist.begin() + C.levptr[l], C.levlist.begin() + C.levptr[l + 1],
                     [&](int a, int b) { return C.sn_ns[a] > C.sn_ns[b]; });
  // relative indices child rows -> parent front rows
  std::vector<int> relidx;
  { std::vector<int> posmap(m, -1);
    for (sdm_int p = 0; p < nsuper; p++) {
      if (C.childptr[p + 1] == C.childptr[p]) continue;
      for (int i = 0; i < C.sn_ms[p]; i++) posmap[lindx[C.sn_xl[p] + i]] = i;
      for (int ci = C.childptr[p]; ci < C.childptr[p + 1]; ci++) {
        int c = C.childlist[ci];
        C.sn_roff[c] = (int64_t)relidx.size();
        for (int i = C.sn_ns[c]; i < C.sn_ms[c]; i++) {
          int q = posmap[lindx[C.sn_xl[c] + i]];
          if (q < 0) throw std::runtime_error("child structure not contained in parent structure");
          relidx.push_back(q);
        }
      }
    }
  }
  // permuteP map (blkchol.c:95-120): L slot -> ADA value index / front offset
  std::vector<int> asm_src((size_t)C.nnzL);
  std::vector<int64_t> asm_dst((size_t)C.nnzL), asm_dstT((size_t)C.nnzL);
  { std::vector<int> rowpos(m, -1);
    for (sdm_int j = 0; j < m; j++) {
      sdm_int jc = perm[j];
      for (sdm_int t = ADAjc[jc]; t < ADAjc[jc + 1]; t++) rowpos[ADAir[t]] = (int)t;
      int s = snode[j]; int c = (int)(j - C.sn_first[s]);
      for (sdm_int t = Ljc[j]; t < Ljc[j + 1]; t++) {
        asm_src[t] = rowpos[perm[Lir[t]]];
        asm_dst[t] = C.sn_foff[s] + (int64_t)c * C.sn_ld[s] + c + (t - Ljc[j]);
        { // transposed copy of the 64x64 diagonal blocks only: DT[panel][row in block][col in block]
          const int64_t rr = c + (t - Ljc[j]); const int pnl = c / NB;
          asm_dstT[t] = (rr < (int64_t)(pnl + 1) * NB && rr < C.sn_ns[s]) ? C.sn_toff[s] + (int64_t)pnl * NB * NB + (rr - (int64_t)pnl * NB) * NB + (c - pnl * NB) : -1;
        }
      }
      for (sdm_int t = ADAjc[jc]; t < ADAjc[jc + 1]; t++) rowpos[ADAir[t]] = -1;
    }
  }
  // factor launch schedule
  int tile_wg_cap = C.tile_wgs_req;                                  // sdm_plan_set_tile_workgroups: tests (a small number makes every workgroup loop)
  if (tile_wg_cap <= 0) {
#ifdef SDM_EMU
    tile_wg_cap = 1 << 20;
#else
    SDM_HIP_CHECK(hipDeviceGetAttribute(&tile_wg_cap, hipDeviceAttributeMultiprocessorCount, P->device));
#endif
  }
  C.launches.clear(); C.lev_first_launch.assign(nlev + 1, 0); C.lev_T.assign(nlev, 1);
  for (int l = 0; l < nlev; l++) {
    C.lev_first_launch[l] = (int)C.launches.size();
    int b = C.levptr[l], e = C.levptr[l + 1];
    if (b == e) continue;                                            // (no active supernode on this level)
    int maxns = C.sn_ns[C.levlist[b]], maxms = 0;
    for (int i = b; i < e; i++) maxms = std::max(maxms, C.sn_ms[C.levlist[i]]);
    C.lev_T[l] = std::max(1, std::min(128, maxms / 16));
    for (int p = 0; p * NB < maxns; p++) {
      LevelLaunch L; L.level = l; L.panel = p; L.nactive = 0; L.maxrows = 0; L.maxtiles = 0; L.lasttiles = 0; L.ride_wgs = 0;
      for (int i = b; i < e; i++) {
        int s = C.levlist[i];
        if (C.sn_ns[s] <= p * NB) break;
        L.nactive++;
        int kb = std::min(NB, C.sn_ns[s] - p * NB);
        int rows = C.sn_ms[s] - (p * NB + kb);
        L.maxrows = std::max(L.maxrows, rows);
        int nt = (rows + TILE - 1) / TILE;
        L.maxtiles = std::max(L.maxtiles, nt * (nt + 1) / 2);
        if (C.sn_ns[s] <= (p + 1) * NB) L.lasttiles = std::max(L.lasttiles, nt * (nt + 1) / 2);
        // workgroups of k_ldl_panel beyond the diagonal-block one (see the kernel): row solves, then pairs of update tiles
        const int nrw = rows > TRSM_ROWS ? (C.sn_ms[s] - (p * NB + NB) + ROWS_BATCH - 1) / ROWS_BATCH : 0;
        int tw = 0;
        if (p > 0) {
          const int ntp = (C.sn_ms[s] - p * NB + TILE - 1) / TILE;            // tile rows of the update of panel p-1
          tw = nrw > 0 ? tile_sched_items(tile_sched(C.sn_ns[s], C.sn_ms[s], p)) : (ntp * (ntp + 1) / 2 - 1 + 1) / 2;
          // big fronts: the tiles are dealt to as many workgroups as the device holds beside the chain and the row solves (one workgroup
          // per compute unit at this launch's LDS footprint, a few compute units left free: a workgroup that finds none starts when the
          // first one has finished); each works through its tiles as a pipeline (panel_role_tiles_stream)
          if (nrw > 0) tw = std::min(tw, std::max(16, (tile_wg_cap - (C.tile_wgs_req > 0 ? 0 : 8)) / (e - b) - 1 - nrw));
        }
        L.ride_wgs = std::max(L.ride_wgs, nrw + tw);
      }
      C.launches.push_back(L);
    }
    // q0: first panel of the level whose diagonal-block launch carries the previous panel's update tiles
    // (maxtiles does not grow with p)
    int q0 = 1 << 30;
    for (int li = C.lev_first_launch[l] + 1; li < (int)C.launches.size(); li++)
      if (C.launches[li - 1].maxtiles <= FUSE_MAX_TILES) { q0 = C.launches[li].panel; break; }
    for (int li = C.lev_first_launch[l]; li < (int)C.launches.size(); li++) C.launches[li].q0 = q0;
  }
  C.lev_first_launch[nlev] = (int)C.launches.size();
  // levels whose fronts are all of the k_ldl_front kind: blocked row solves (MFMA_MIN_ROWS rule of panel_rows), at most
  // FRONT_MAXT tile rows, no partial last panel with rows below it, and few enough workgroups to be resident together
  C.lev_persist.assign(nlev, 0); C.lev_maxT.assign(nlev, 0); C.lev_ntw.assign(nlev, 0);
  std::vector<int> fslot(std::max<sdm_int>(1, C.nsuper), 0);
  int nslot = 0;
  {
    // sdm_plan_set_one_launch_fronts(p, 0): the comparison switch of tests and tools; front_disabled: a launch of this plan timed out
    // before (chol_wait_timeouts) -- the plan stays on the launch-per-panel path across later set_chol calls too, and with no
    // one-launch level follow_decide (sdm_solve_build.hip) plans no inverse behind the factor either
    const bool off = C.front_off_req || C.front_disabled;
    const int maxT_allowed = FRONT_MAXT;
    // k_ldl_front's workgroups wait for each other in both directions (a row workgroup for its tile workgroups and vice
    // versa): they must all be resident, one per compute unit (135 KB of LDS each).  A device -- or a partition of one --
    // with fewer compute units than the level needs keeps the launch-per-panel path.
    int ncu = 0;
#ifdef SDM_EMU
    ncu = 1 << 20;
#else
    SDM_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, P->device));
    if (chol_front_wgs_per_cu() < 1) ncu = 0;                          // (the kernel cannot be resident here: no level takes the one-launch path)
#endif
    const int wg_budget = std::min(224, ncu - ncu / 8);                // leave an eighth of the device to whatever else is running
    for (int l = 0; l < nlev; l++) {
      bool ok = !off;
      int maxT = 0;
      const int nfr = C.levptr[l + 1] - C.levptr[l];
      for (int i = C.levptr[l]; i < C.levptr[l + 1] && ok; i++) {
        const int s = C.levlist[i], ns = C.sn_ns[s], ms = C.sn_ms[s], T = (ms + TILE - 1) / TILE;
        if (ms - std::min(NB, ns) < MFMA_MIN_ROWS || T > maxT_allowed || (ns % NB != 0 && ms != ns)) ok = false;
        maxT = std::max(maxT, T);
      }
      if (!ok || nfr == 0) continue;
      // one row workgroup per tile row and ONE tile workgroup per tile (r, c), c >= 2: only levels that fit the device that way
      // qualify (single fronts of up to 21 tile rows on a whole MI355X).  Tile workgroups that own several tiles were built and
      // measured in round 2 (MAXCUT-4000's front, 63 tile rows: 5.56 ms against 2.26 ms for the 63 panel launches -- a tile
      // update costs ~20 us of a 147 KB workgroup, so with several tiles each they fall far behind the chain) and removed.
      const int pool = FRONT_POOL;
      const int ntiles = (maxT - 1) * (maxT - 2) / 2;
      const int ntw = std::min(ntiles, wg_budget / nfr - maxT);
      if (ntw < 0 || (int64_t)ntw * pool < ntiles) continue;
      C.lev_persist[l] = 1; C.lev_maxT[l] = maxT; C.lev_ntw[l] = ntw;
      for (int i = C.levptr[l]; i < C.levptr[l + 1]; i++) fslot[C.levlist[i]] = nslot++;
    }
  }
  C.front_cnt.alloc((size_t)std::max(1, nslot) * FRONT_CNT);
  C.d_fslot.upload(fslot);
  // upload
  C.d_first.upload(C.sn_first); C.d_ns.upload(C.sn_ns); C.d_ms.upload(C.sn_ms); C.d_ld.upload(C.sn_ld); C.d_parent.upload(C.sn_parent);
  C.d_childptr.upload(C.childptr); C.d_childlist.upload(C.childlist); C.d_levlist.upload(C.levlist);
  C.d_lindx.upload(lindx); C.d_relidx.upload(relidx);
  { std::vector<int> p32(m); for (sdm_int i = 0; i < m; i++) p32[i] = (int)perm[i]; C.d_perm.upload(p32); }
  C.d_foff.upload(C.sn_foff); C.d_xl.upload(C.sn_xl); C.d_woff.upload(C.sn_woff); C.d_roff.upload(C.sn_roff);
  if (C.fsize <= ASM_FULL_MAX) {                                    // inverse map for k_assemble_full
    std::vector<int> fsrc((size_t)C.fsize, -1);
    for (sdm_int t = 0; t < C.nnzL; t++) fsrc[(size_t)asm_dst[t]] = asm_src[t];
    C.d_asm_fsrc.upload(fsrc);
  } else C.d_asm_fsrc.release();
  C.d_asm_src.upload(asm_src); C.d_asm_dst.upload(asm_dst); C.d_asm_dstT.upload(asm_dstT); C.d_toff.upload(C.sn_toff);
  C.frontsT.alloc((size_t)C.tsize);
  { std::vector<int64_t> l64(C.Ljc.begin(), C.Ljc.end()); C.d_Ljc.upload(l64); }
  C.fronts.alloc((size_t)C.fsize + 128);                          // + padding: k_sinv128 reads up to 63 rows past a partial block
  C.wvec.alloc((size_t)C.wsize); C.colbuf.alloc((size_t)C.wsize + (size_t)nsuper);
  C.d.alloc(m); C.dsolve.alloc(m); C.lb.alloc(m); C.pivval.alloc(m); C.pivstat.alloc(m); C.ub.alloc(3); C.upd_cnt.alloc((size_t)std::max<sdm_int>(1, C.nsuper)); C.diag_cnt.alloc((size_t)std::max<sdm_int>(1, C.nsuper));
  P->ada_val.alloc((size_t)C.nnzADA); P->absd.alloc(m); P->lpr.alloc((size_t)C.nnzL);
  P->rhs.alloc(m); P->y.alloc(m); P->ywork.alloc(m);
  P->has_chol = true; P->factored = false;
  solve_build(P);
}

}  // namespace sdm
