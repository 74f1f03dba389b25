// sdm_solve_build.hip -- host-side planning of the triangular solves: the super-block width, the arena of the explicit inverses with the
// work lists of their inversion (sdm_solve_inv.hip), the transposed rows of L and the per-level table of the sweeps (sdm_solve.hip), computed
// once per symbolic factor.  solve_build (at the end) is the sequence of the steps below.  No kernel is defined or launched here.
#include "sdm_follow.h"
#include <algorithm>

namespace sdm {
namespace {

// leaves and combine tiles of the inversion in the order they are generated (arena_layout -> upload_longest_first)
struct InvItems {
  std::vector<int> i128;                                              // 128-column leaves: {s, h, 0, 0}
  std::vector<std::vector<int>> stage = std::vector<std::vector<int>>(2 * SINV_MAXLEV);     // combine tiles per stage st = 2 * level + (0: T, 1: X)
  std::vector<std::vector<int>> stage_w = std::vector<std::vector<int>>(2 * SINV_MAXLEV);   // and the number of K steps of each
};

bool front_active(const CholPlan &C, int s) { return C.sn_active.empty() || C.sn_active[s] != 0; }   // (supernodes of other ranks: a place in the arenas, no work)

// C.sbw: the width asked for, or the power of two that covers the widest front; the notes of the sweeps start afresh
void choose_width(sdm_plan *P) {
  CholPlan &C = P->chol;
  int W = C.sbw_req;
  if (W == 0) { W = SBW_MIN; while (W < C.maxns && W < SBW_MAX) W *= 2; }
  C.sbw = W;
  // a new solve: no ill-conditioned block met yet (sweeps of the previous symbolic factor still in flight would write their notes
  // after this reset: drained first -- set_chol happens once per solve)
  if (C.noted.host) SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
  C.noted.ensure(); C.noted.host[0] = C.noted.host[1] = 0; C.refine_on = false; C.sweep_seq = 0;
}

// The arena S of the inverse blocks: sn_soff, sn_sld, sn_sboff (and their device copies), ssize, nsbtot.  Returns the 128-column leaf
// items and, per stage, the combine tiles of every super-block with their K-step weights.
InvItems arena_layout(CholPlan &C) {
  const int nsuper = (int)C.nsuper, W = C.sbw;
  InvItems it;
  C.sn_soff.assign(nsuper, 0); C.sn_sld.assign(nsuper, 0); C.sn_sboff.assign(nsuper, 0);
  int64_t soff = 0; int sb = 0;
  for (int s = 0; s < nsuper; s++) {
    const int ns = C.sn_ns[s];
    // leading dimension of the front's inverse blocks: a multiple of 16 (whole 128-byte lines per 16-row slab), never a
    // multiple of 256 doubles (columns 2 KB-aligned to each other would land on the same memory channels)
    int sld = (std::min(ns, W) + 15) & ~15;
    if (sld % 256 == 0) sld += 16;
    C.sn_soff[s] = soff; C.sn_sld[s] = sld; C.sn_sboff[s] = sb;
    soff += (int64_t)sld * ns;
    const int nsb = (ns + W - 1) / W;
    const bool act = front_active(C, s);
    for (int h = 0; act && 128 * h < ns; h++) { it.i128.push_back(s); it.i128.push_back(h); it.i128.push_back(0); it.i128.push_back(0); }
    for (int Pb = 0; act && Pb < nsb; Pb++) {
      const int nb = std::min(W, ns - Pb * W);
      int prev = (nb + 127) / 128;                                    // what stage 0 waits for: the leaves of this super-block
      for (int lev = 0; lev < SINV_MAXLEV; lev++) {
        const int h = 128 << lev;
        if (h >= nb) break;
        int cnt = 0;
        for (int t = 0; t < 2; t++) {
          std::vector<int> &dst = it.stage[2 * lev + t];
          for (int pi = 0; pi * 2 * h + h < nb; pi++) {
            const int nc = std::min(h, nb - pi * 2 * h - h);
            for (int I = 0; 64 * I < nc; I++)
              for (int J = 0; 64 * J < h; J++) {
                const int item[8] = {s, Pb, lev, pi, I, J, t, prev};
                dst.insert(dst.end(), item, item + 8);
                it.stage_w[2 * lev + t].push_back(t == 0 ? h / 64 - J : std::min(I + 1, (nc + 63) / 64));   // its K steps (stile_body)
                if (t == 0) cnt++;
              }
          }
          prev = cnt;                                                  // T and X stages of a level have the same tiles
        }
      }
    }
    sb += nsb;
  }
  C.ssize = soff; C.nsbtot = sb;
  C.d_soff.upload(C.sn_soff); C.d_sld.upload(C.sn_sld); C.d_sboff.upload(C.sn_sboff);
  return it;
}

// The work lists of the inversion on the device: l_i128 / n_i128, and l_items / n_items / stage_ptr with every stage's tiles longest first
void upload_longest_first(CholPlan &C, const InvItems &it) {
  std::vector<int> items;
  C.stage_ptr.assign(2 * SINV_MAXLEV + 1, 0);
  for (int st = 0; st < 2 * SINV_MAXLEV; st++) {
    C.stage_ptr[st] = (int)items.size() / 8;
    // Longest items first.  The products are triangular (1 .. h/64 K steps per tile) and a launch of more tiles than fit the device
    // at once lasts as long as whatever is dispatched last: in the order the tiles are generated (long ones last in stage X) the two
    // 496-tile stages of MAXCUT-4000 took 107 and 103 us, sorted 90 and 89 (profiles/r07_inverse_tile_variants.txt).  Measured and
    // not kept: workgroups taking the tiles in pairs, longest with shortest (88 us, and the small stages slower: a workgroup alone on
    // its CU needs 4.6 us per K step, two on a CU 6.4 us each), and operand blocks two K steps ahead in registers (a few us, at the
    // price of the second workgroup per CU) -- a K step is 64 KB of operands at the ~16 GB/s a CU gets when all CUs stream.
    const std::vector<int> &w = it.stage_w[st];
    std::vector<int> ord(w.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = (int)i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return w[a] > w[b]; });
    for (int i : ord) items.insert(items.end(), it.stage[st].begin() + 8 * (size_t)i, it.stage[st].begin() + 8 * (size_t)i + 8);
  }
  C.stage_ptr[2 * SINV_MAXLEV] = (int)items.size() / 8;
  C.n_i128 = (int)it.i128.size() / 4; C.n_items = (int)items.size() / 8;
  C.l_i128.upload(it.i128); C.l_items.upload(items);
}

// fronts of several super-blocks: transposed copy of the rows of L below each super-block (forward step launches): sn_ltoff / d_ltoff,
// the 64x64 tiles of k_ltrans (l_lt, n_lt) and the arena LT itself
void lt_tiles(CholPlan &C) {
  const int nsuper = (int)C.nsuper, W = C.sbw;
  C.sn_ltoff.assign(nsuper, 0);
  std::vector<int> lt;
  int64_t ltoff = 0;
  for (int s = 0; s < nsuper; s++) {
    const int ns = C.sn_ns[s], nsb = (ns + W - 1) / W;
    C.sn_ltoff[s] = ltoff;
    if (!front_active(C, s)) continue;
    for (int Pb = 0; Pb + 1 < nsb; Pb++) {
      const int nr = ns - (Pb + 1) * W;
      for (int I = 0; 64 * I < nr; I++)
        for (int J = 0; 64 * J < W; J++) { lt.push_back(s); lt.push_back(Pb); lt.push_back(I); lt.push_back(J); }
      ltoff += (int64_t)nr * W;
    }
  }
  C.n_lt = (int)lt.size() / 4;
  C.l_lt.upload(lt); C.d_ltoff.upload(C.sn_ltoff);
  C.LT.alloc((size_t)std::max<int64_t>(ltoff, 1));
}

// S, ST (zeroed), Tarena; xfin, zdiv; sb_g and sweep_cnt (zeroed)
void alloc_buffers(CholPlan &C) {
  const size_t sz = (size_t)std::max<int64_t>(C.ssize, 1);
  C.S.alloc(sz); C.ST.alloc(sz); C.Tarena.alloc(C.n_items ? sz : 1);
  SDM_HIP_CHECK(hipMemset(C.S.p, 0, sz * sizeof(double)));            // upper triangles stay zero for good
  SDM_HIP_CHECK(hipMemset(C.ST.p, 0, sz * sizeof(double)));           // (here: the lower ones)
  C.xfin.alloc((size_t)std::max<sdm_int>(C.m, 1)); C.zdiv.alloc((size_t)std::max<sdm_int>(C.m, 1));
  // growth records (2 words per super-block), then the completion counters of k_sprep (SPREP_NCNT ints per super-block)
  const size_t gw = (size_t)std::max(C.nsbtot, 1) * (2 + SPREP_NCNT / 2);
  C.sb_g.alloc(gw);
  SDM_HIP_CHECK(hipMemset(C.sb_g.p, 0, gw * sizeof(unsigned long long)));
  C.sweep_cnt.alloc(2 * MC_SET);                                    // (the merged sweep launches' counters: merged_count)
  SDM_HIP_CHECK(hipMemset(C.sweep_cnt.p, 0, 2 * MC_SET * sizeof(int)));
}

// C.slev: what the sweeps need to size the launches of every etree level
void level_table(CholPlan &C) {
  const int W = C.sbw;
  C.slev.assign(C.nlevels, SolveLevel());
  for (int l = 0; l < C.nlevels; l++) {
    SolveLevel &L = C.slev[l];
    L.nfronts = C.levptr[l + 1] - C.levptr[l];
    for (int i = C.levptr[l]; i < C.levptr[l + 1]; i++) {
      const int s = C.levlist[i], ns = C.sn_ns[s], ms = C.sn_ms[s];
      L.maxns = std::max(L.maxns, ns); L.maxms = std::max(L.maxms, ms);
      if (C.childptr[s + 1] > C.childptr[s]) L.children = true;
      if (ms > ns) L.below = true;
    }
    L.nsb = (L.maxns + W - 1) / W;
    L.slabs_fw.assign(L.nsb, 0);
    for (int i = C.levptr[l]; i < C.levptr[l + 1]; i++) {
      const int s = C.levlist[i], ns = C.sn_ns[s], ms = C.sn_ms[s];
      for (int Pb = 0; Pb * W < ns; Pb++)                              // (slabs of the rows BELOW the supernode; its own later rows: k_sfw_rows)
        if (ms > ns) L.slabs_fw[Pb] = std::max(L.slabs_fw[Pb], (ms - (ns & ~1) + SROWS - 1) / SROWS);
    }
  }
}

// Can the inverses be built BEHIND the factorisation (k_sinv_follow)?  Every level must be a k_ldl_front level, every front
// one super-block, and the workgroups of both kernels of a level must fit the device together, one per compute unit
// (whichever of the two the hardware dispatches first, nobody may be kept out by workgroups that wait).
void follow_decide(sdm_plan *P) {
  CholPlan &C = P->chol;
  C.follow = false;
  C.lev_followT.assign(C.nlevels, 0);
  if (C.nlevels == 0 || C.maxns > C.sbw || C.front_disabled) return;
  int ncu = 1 << 20;
#ifndef SDM_EMU
  SDM_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, P->device));
#endif
  // (one workgroup of either kernel per compute unit is what the count below assumes: the follower must fit at least that)
  if (!solve_follow_fits()) return;
  for (int l = 0; l < C.nlevels; l++) {
    if (!C.lev_persist[l]) return;
    const int nfr = C.levptr[l + 1] - C.levptr[l];
    int Tn = 0;
    for (int i = C.levptr[l]; i < C.levptr[l + 1]; i++) Tn = std::max(Tn, (C.sn_ns[C.levlist[i]] + 63) / 64);
    C.lev_followT[l] = Tn * (Tn + 1) / 2;
    if ((int64_t)nfr * (C.lev_followT[l] + C.lev_maxT[l] + C.lev_ntw[l]) > ncu - ncu / 8) return;
  }
  C.follow = true;
}

}  // namespace

void solve_build(sdm_plan *P) {
  CholPlan &C = P->chol;
  choose_width(P);
  const InvItems it = arena_layout(C);
  upload_longest_first(C, it);
  lt_tiles(C);
  alloc_buffers(C);
  level_table(C);
  follow_decide(P);
}

}  // namespace sdm
