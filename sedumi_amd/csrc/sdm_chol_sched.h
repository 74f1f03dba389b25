// sdm_chol_sched.h -- which update tiles a launch of the launch-per-panel factor (k_ldl_panel) carries, and which tile columns a rank owns.
// Host and device: chol_build sizes the launches with it (sdm_chol_build.hip), the tile workgroups walk it (sdm_chol.hip), the tests read
// it through sdm_debug_tile_items.
#pragma once
#include "sdm_plan.h"

namespace sdm {

// ============================================================ schedule of the trailing updates of a big front (host + device)
// Panel p's rank-64 update of the trailing matrix, applied in the launch after it (the "eager" schedule), is a read-modify-write of every
// trailing tile per panel.  The panels are therefore taken UPD_G at a time (a GROUP g = panels G g .. G g + G - 1):
//   * tile columns up to G g + 2 G - 1 (those factored before the group's deferred update can have reached them) get every panel of the
//     group eagerly, as before: K = 64 in the launch after the panel;
//   * tile columns from G g + 2 G on get the whole group in ONE read-modify-write with K = 64 G once its last panel is final: columns
//     G g + 2 G .. G g + 3 G - 1 (the next group's eager window) in launch G g + G, the rest dealt over the launches G g + G .. G g + 2 G - 1.
// Every tile still receives the panels in ascending order, each as  c <- c - (product over the panel's 64 columns, accumulated from zero):
// the same operations in the same order as the eager schedule, i.e. the SAME BITS; only the trips of c through memory are saved.
// A group is deferred only if all its launches exist and have row-solve workgroups (NP >= G g + 2 G panels, T >= G g + 2 G + 4 tile rows).
// The unit of work is a MACRO TILE of 2 x 2 tiles (128 x 128; panel_role_tiles_stream says why): a region = the tiles (I, J) with
// J0 <= J < J0 + JW, J <= I < nt, cut into macro tiles from (J0, J0) on; tiles of a macro tile outside the region are masked.
constexpr int UPD_G = 2;
__host__ __device__ inline bool upd_group_deferred(int ns, int ms, int g) {
  return g >= 0 && (ns + NB - 1) / NB >= UPD_G * g + 2 * UPD_G && (ms + TILE - 1) / TILE >= UPD_G * g + 2 * UPD_G + 4;
}
// macro tiles of the region (nt, J0, JW): macro columns MJ < MC, macro rows MJ <= MI < MR
__host__ __device__ inline int macro_count(int nt, int J0, int JW) {
  const int R = nt - J0;
  if (R <= 0 || JW <= 0) return 0;
  const int C = JW < R ? JW : R, MC = (C + 1) / 2, MR = (R + 1) / 2;
  return MC * MR - MC * (MC - 1) / 2;
}
__host__ __device__ inline void macro_index(int t, int nt, int J0, int JW, int &MI, int &MJ) {   // column by column
  const int R = nt - J0, C = JW < R ? JW : R, MC = (C + 1) / 2, MR = (R + 1) / 2;
  MJ = 0;
  while (MJ + 1 < MC && t >= MR - MJ) { t -= MR - MJ; MJ++; }
  MI = MJ + t;
}
// of N items, those dealt to launch r of the group's UPD_G launches: t % 10 in [cut[r], cut[r+1])  (the first launch carries the
// group's first columns as well and gets less)
__host__ __device__ inline void share_range(int r, int &lo, int &hi) {
  lo = r == 0 ? 0 : 3 + (r - 1) * 7 / (UPD_G - 1 > 0 ? UPD_G - 1 : 1);
  hi = r == UPD_G - 1 ? 10 : 3 + r * 7 / (UPD_G - 1 > 0 ? UPD_G - 1 : 1);
  if (UPD_G == 1) { lo = 0; hi = 10; }
}
__host__ __device__ inline int share_count(int N, int r) {
  int lo, hi; share_range(r, lo, hi);
  const int rem = N % 10 - lo;
  return (N / 10) * (hi - lo) + (rem < 0 ? 0 : (rem > hi - lo ? hi - lo : rem));
}
__host__ __device__ inline int share_item(int k, int r) { int lo, hi; share_range(r, lo, hi); return 10 * (k / (hi - lo)) + lo + k % (hi - lo); }
// what the tile workgroups of launch q (the launch that factors panel q) of a front do, in macro tiles: NE of the eager region (panel q-1
// into the columns 1 .. JE relative to tile column q; column 0 is the row-solve workgroups'), NH + NR of the deferred group g2 (in its
// first launch the columns G .. 2G-1, and this launch's share of the triangle beyond them -- tile column G g2 + 3 G of the front = column
// 2 G - r relative to this launch; `all`: the whole triangle at once, when the next group is not deferred and its eager updates would
// otherwise meet these tiles in the launches to come)
struct TileSched { int nt, JE, NE, NH, NR, g2, r, all; };
__host__ __device__ inline TileSched tile_sched(int ns, int ms, int q) {
  TileSched S;
  S.nt = (ms - q * NB + TILE - 1) / TILE;
  const int g = (q - 1) / UPD_G;
  S.JE = upd_group_deferred(ns, ms, g) ? min(UPD_G * g + 2 * UPD_G - 1 - q, S.nt - 1) : S.nt - 1;
  S.NE = macro_count(S.nt, 1, S.JE);
  S.g2 = q >= UPD_G ? q / UPD_G - 1 : -1; S.r = q % UPD_G; S.NH = 0; S.NR = 0; S.all = 0;
  if (upd_group_deferred(ns, ms, S.g2)) {
    const int J0 = 2 * UPD_G - S.r, N = macro_count(S.nt, J0, S.nt);   // (the same triangle in all the group's launches: from tile column G g2 + 3 G)
    S.all = upd_group_deferred(ns, ms, S.g2 + 1) ? 0 : 1;
    if (S.r == 0) S.NH = macro_count(S.nt, UPD_G, UPD_G);
    S.NR = S.all ? (S.r == 0 ? N : 0) : share_count(N, S.r);
  } else S.g2 = -1;
  return S;
}
__host__ __device__ inline int tile_sched_items(const TileSched &S) { return S.NE + S.NH + S.NR; }
// item u of the launch's schedule: first tile (I, J) of its macro tile (relative to tile column q), which of its 2 x 2 tiles are the
// item's (bit 2a+b: tile (I+a, J+b)), first panel and number of panels it applies
__host__ __device__ inline void tile_sched_item(const TileSched &sc, int q, int u, int &I, int &J, int &act, int &p0, int &np) {
  int J0, JW, x = u;
  if (u < sc.NE) { J0 = 1; JW = sc.JE; np = 1; p0 = q - 1; }                                                  // eager: the panel before
  else {
    np = UPD_G; p0 = UPD_G * sc.g2;
    if (u < sc.NE + sc.NH) { x = u - sc.NE; J0 = UPD_G; JW = UPD_G; }                                        // the deferred group's first columns
    else { x = u - sc.NE - sc.NH; if (!sc.all) x = share_item(x, sc.r); J0 = 2 * UPD_G - sc.r; JW = sc.nt; }  // this launch's share of the triangle beyond them
  }
  int MI, MJ;
  macro_index(x, sc.nt, J0, JW, MI, MJ);
  I = J0 + 2 * MI; J = J0 + 2 * MJ;
  const int Jend = min(J0 + JW, sc.nt);
  act = 0;
  for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) if (I + a < sc.nt && J + b < Jend && I + a >= J + b) act |= 1 << (2 * a + b);
}

// ============================================================ block-column-cyclic ownership (several ranks factor ONE dense front: sedumi_amd.dist.BlockCyclicFactor)
// `own` = world | rank << 8 | blk << 16 (0: the plan owns everything).  Tile column c of the front belongs to rank (c / blk) % world.  The owner of
// tile column q factors panel q (diagonal block + row solves of launch q); EVERY update of a tile is applied by the owner of the tile's column, in
// the launch the single-plan schedule applies it in: per tile the same operations in the same order, i.e. the same bits (blkchol2.c:346-420 applied
// column by column; the relink rule of blkchol2.c:550-554 becomes "panel q goes to everybody once it is final": the caller broadcasts it).
__host__ __device__ inline bool owns_col(int own, int c) {
  const int world = own & 255;
  if (world <= 1) return true;
  const int blk = own >> 16;
  return (c / (blk > 0 ? blk : 1)) % world == ((own >> 8) & 255);
}

}  // namespace sdm
