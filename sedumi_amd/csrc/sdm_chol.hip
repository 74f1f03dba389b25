// sdm_chol.hip -- numeric supernodal LDL' (blkchol) and triangular solves
// (fwblkslv / bwblkslv) for gfx950.
//
// What the reference does (blkchol.c:157-231 spchol, blkchol2.c:464-563 blkLDL,
// :346-420 precorrect, :96-167 cholonBlk): a sequential left-looking supernodal
// LDL' built from level-1 BLAS calls, with a never-fail pivot rule.
//
// What this file does instead (MI355X-first): a level-scheduled MULTIFRONTAL
// LDL'.  Every supernode owns a dense column-major front in one HBM arena;
// independent fronts of an elimination-tree level are factored by the same
// launches; children pass their Schur complements to the parent by a
// deterministic, ownership-partitioned extend-add (no atomics).  Inside a
// front the elimination is blocked by 64 columns, ONE launch per panel
// (k_ldl_panel): workgroup 0 factors the diagonal block in registers / LDS (pivot
// rule applied column by column), further workgroups solve the rows below it as
// the block is published 16 columns at a time, and the trailing update
// C -= L21*D*L21' of the PREVIOUS panel (FP64 matrix cores, 64x64 tiles) rides
// along in the remaining workgroups; per-front counters in HBM order them.
// The result is the same L, d (unit diagonal stored explicitly, skipped
// columns returned as unit vectors, blkchol.c:409-414) up to rounding, and the
// pivot DECISIONS follow blkchol2.c:114-161 including the idamax quirk of
// maxabs (blkchol2.c:66-70).
//
// sdm_chol_build.hip plans the factor on the host (chol_build), sdm_chol_sched.h is the update schedule both sides read, and
// sdm_chol_dev.h holds the device functions the two factor kernels share.  Here: the small data-movement kernels, k_ldl_panel and
// its roles, k_ldl_front and its roles, k_ldl_update, the host code that launches them, the debug exports.
#include "sdm_chol_sched.h"
#include "sdm_chol_dev.h"
#include <cstring>
#include <algorithm>
#include <cmath>
#include <numeric>

namespace sdm {

struct FollowArgs { double *S, *STr; unsigned long long *sb_g; int nfront; };   // (k_ldl_front: the follower's workgroups behind the front's)

// ================================================================= kernels

// ---- permuteP: scatter tril(ADA(perm,perm)) into the (zeroed) fronts
// the same with the zero fill of the fronts folded in (arenas of up to ASM_FULL_MAX entries): one work-item per ENTRY of
// the arena through the inverse map (entry -> ADA value index, -1 = structural zero / padding), one launch less per
// factorisation than memset + scatter
__global__ void k_assemble_full(double *F, const double *ada, const int *fsrc, int64_t fsize, double *ub) {
  if (ub && blockIdx.x == 0 && threadIdx.x < 3) ub[threadIdx.x] = 0.0;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < fsize; t += stride) { const int s = fsrc[t]; F[t] = s < 0 ? 0.0 : ada[s]; }
}
__global__ void k_assemble(double *F, const double *ada, const int *src, const int64_t *dst, int64_t nnzL, double *ub) {
  // ub[0..2] (pivot thresholds of this factorisation, filled by k_prep_pivots -- the next launch on the stream) start at 0
  if (ub && blockIdx.x == 0 && threadIdx.x < 3) ub[threadIdx.x] = 0.0;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < nnzL; t += stride) { int s = src[t]; F[dst[t]] = s < 0 ? 0.0 : ada[s]; }
}
__global__ void k_extract(double *Lpr, const double *F, const int64_t *dst, int64_t nnzL) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < nnzL; t += stride) Lpr[t] = F[dst[t]];
}
__global__ void k_load_factor(double *F, double *FT, const double *Lpr, const int64_t *dst, const int64_t *dstT, int64_t nnzL) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < nnzL; t += stride) { const double v = Lpr[t]; F[dst[t]] = v; if (dstT[t] >= 0) FT[dstT[t]] = v; }
}

// ---- pivot thresholds (blkchol.c:168-184), grid-stride over the columns.
//   ub = max_j P(perm_j,perm_j) / maxu^2 ;  lb_j = max(abstol, canceltol * orgd_j)
// ub[2] collects max_j as the bit pattern of a non-negative double (ordered like the unsigned integer: atomicMax is
// exact and order independent); ub[1] = maxu; k_ldl_panel forms ub from them.  ub[2] is zeroed by the host before.
struct PrepArgs {
  int m; const double *ada; const int *asm_src; const int64_t *Ljc; const int *perm; const double *absd; int use_absd;
  double canceltol, maxu, abstol; double *lb, *ub; int *pivstat; double *pivval; int nsuper; int *upd_cnt, *diag_cnt;
  unsigned long long *sb_g; int nsbg; int *front_cnt; int nfc; unsigned long long *DTbits; int64_t ndt;
};
// the work of workgroup `bx` of `nb`: re-arms counters / tags, thresholds of its columns; returns the largest diagonal entry it saw
__device__ __forceinline__ double prep_pivots_part(const PrepArgs &A, int bx, int nb, double *red) {
  const int gid = bx * blockDim.x + threadIdx.x, gstride = nb * blockDim.x;
  for (int64_t i = gid; i < A.ndt; i += gstride) A.DTbits[i] = DT_SENTINEL;             // the data-tagged hand-over of the diagonal blocks (k_ldl_front)
  for (int i = gid; i < A.nsuper; i += gstride) { A.upd_cnt[i] = 0; A.diag_cnt[i] = 0; }   // counters of k_ldl_panel
  for (int i = gid; i < A.nfc; i += gstride) A.front_cnt[i] = 0;                        // counters of k_ldl_front
  for (int i = gid; i < A.nsbg; i += gstride) A.sb_g[i] = 0ull;                         // growth records of the solve inverses (sdm_solve.hip)
  double mx = 0.0;
  for (int j = gid; j < A.m; j += gstride) {
    int s = A.asm_src[A.Ljc[j]];
    double dj = s < 0 ? 0.0 : A.ada[s];
    if (dj > mx) mx = dj;
    double org = A.use_absd ? A.absd[A.perm[j]] : dj;
    double v = A.canceltol * org;
    A.lb[j] = v > A.abstol ? v : A.abstol;
    A.pivstat[j] = 0; A.pivval[j] = 0.0;
  }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s && red[threadIdx.x + s] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}
__global__ void k_prep_pivots(PrepArgs A) {
  __shared__ double red[256];
  const double mx = prep_pivots_part(A, blockIdx.x, gridDim.x, red);
  if (threadIdx.x == 0) {
    union { double d; unsigned long long u; } b; b.d = mx;
    atomicMax((unsigned long long *)&A.ub[2], b.u);
    A.ub[1] = A.maxu;
  }
}
// k_assemble_full and k_prep_pivots as ONE launch (fronts small enough for the inverse map: the bench workloads): workgroups
// [0, nprep) do the pivot bounds, the rest assemble.  The largest diagonal entry cannot be an atomicMax into a cell that this same
// launch would have to clear first: every bounds workgroup leaves its maximum in `part`, the last one to finish (a ticket that
// resets itself) takes the maximum of them -- order independent, like the atomicMax.
__global__ void k_begin_factor(PrepArgs A, int nprep, double *part, int *ticket, double *F, const int *fsrc, int64_t fsize) {
  if ((int)blockIdx.x >= nprep) {
    int64_t t = (int64_t)((int)blockIdx.x - nprep) * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)((int)gridDim.x - nprep) * blockDim.x;
    for (; t < fsize; t += stride) { const int s = fsrc[t]; F[t] = s < 0 ? 0.0 : A.ada[s]; }
    return;
  }
  __shared__ double red[256];
  __shared__ int last;
  const double mx = prep_pivots_part(A, blockIdx.x, nprep, red);
  // (write-through store, acknowledged, then the ticket; the last workgroup reads with L2-bypassing loads: the workgroups sit on
  // different XCDs -- with plain stores and a fence the soak of round 4 met a stale maximum twice in 3471 fronts)
  if (threadIdx.x == 0) sdm_store_wt(&part[blockIdx.x], mx);
  SDM_STORES_DONE();
  if (threadIdx.x == 0) last = sdm_ticket_take(ticket) == nprep - 1;
  __syncthreads();
  if (!last) return;
  double m2 = 0.0;
  for (int i = threadIdx.x; i < nprep; i += blockDim.x) { const double v = sdm_load_wt(&part[i]); if (v > m2) m2 = v; }
  __syncthreads();
  red[threadIdx.x] = m2;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s && red[threadIdx.x + s] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) { A.ub[0] = 0.0; A.ub[1] = A.maxu; A.ub[2] = red[0]; sdm_signal_add(ticket, -nprep); }   // (the ticket back to 0, where the tickets are counted)
}

// ---- extend-add: parent front += children's Schur complements.
// grid (T, fronts of the level).  Workgroup `slice` owns the parent columns
// J with J % T == slice, so every parent entry has exactly one writer and the
// children are applied in a fixed order: deterministic, no atomics.
__global__ void k_extend_add(double *F, FrontTab tab, const int *list) {
  const int p = list[blockIdx.y];
  const int slice = blockIdx.x, T = gridDim.x;
  const int msp = tab.ld[p];
  double *Fp = F + tab.foff[p];
  for (int ci = tab.childptr[p]; ci < tab.childptr[p + 1]; ci++) {
    const int c = tab.childlist[ci];
    const int nc = tab.ns[c], mu = tab.ms[c] - nc, mc = tab.ld[c];
    const int *rel = tab.relidx + tab.roff[c];
    const double *Fc = F + tab.foff[c];
    for (int j = 0; j < mu; j++) {
      const int J = rel[j];
      if (J % T != slice) continue;
      const double *src = Fc + (int64_t)(nc + j) * mc + nc;
      double *dst = Fp + (int64_t)J * msp;
      for (int i = j + threadIdx.x; i < mu; i += blockDim.x) dst[rel[i]] += src[i];
    }
    __syncthreads();
  }
}

// ================================================================== solves
// The triangular solves live in sdm_solve.hip (explicit inverses of the diagonal super-blocks, one GEMV launch per
// super-block column).  Only the small vector helpers they share with the factor remain here.
__global__ void k_gather_perm(double *dst, const double *src, const int *perm, int m, int forward) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < m) { if (forward) dst[k] = src[perm[k]]; else dst[perm[k]] = src[k]; }
}
// ./d of wrapPcg.m:57 with deninfac.m:89-94 folded in: skipped pivots (d = 0) act as 1
__global__ void k_divd(double *v, const double *d, int m) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < m) { const double dk = d[k]; v[k] /= dk > 0.0 ? dk : 1.0; }
}

// ---- the record of a finished panel that travels between block-cyclic ranks beside the panel's columns of the front: d, lb, pivval, pivstat
// (as doubles) of its 64 columns, the front's two progress counters, the transposed copy DT of its diagonal block  (3 NB + NB + 2 + NB NB doubles)
__global__ void k_panel_record(double *rec, double *d, double *lb, double *pivval, int *pivstat, int *upd_cnt, int *diag_cnt, double *DT, int first, int k0, int kb,
                               int s, int64_t toff, int unpack) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  for (int e = tid; e < 4 * NB + 2 + NB * NB; e += nth) {
    double *slot = nullptr; int *islot = nullptr;
    if (e < NB) { if (e < kb) slot = d + first + k0 + e; }
    else if (e < 2 * NB) { if (e - NB < kb) slot = lb + first + k0 + e - NB; }
    else if (e < 3 * NB) { if (e - 2 * NB < kb) slot = pivval + first + k0 + e - 2 * NB; }
    else if (e < 4 * NB) { if (e - 3 * NB < kb) islot = pivstat + first + k0 + e - 3 * NB; }
    else if (e == 4 * NB) islot = upd_cnt + s;
    else if (e == 4 * NB + 1) islot = diag_cnt + s;
    else slot = DT + toff + (int64_t)(k0 / NB) * NB * NB + (e - 4 * NB - 2);
    if (slot) { if (unpack) *slot = rec[e]; else rec[e] = *slot; }
    else if (islot) { if (unpack) *islot = (int)rec[e]; else rec[e] = (double)*islot; }
    else if (!unpack) rec[e] = 0.0;
  }
}

#ifdef SDM_EMU
#define SDM_NOINLINE
#else
// (a callable function does not inherit the kernel's launch bounds: the register allocator budgets it for the translation unit's
// default workgroup size -- 1024 work-items = 128 VGPRs unless the file is compiled with --gpu-max-threads-per-block=512, as
// sedumi_amd/build.py does for this file; with 128 the roles spill inside although their kernels may use 256)
// not_tail_called: a call the optimizer marks as a tail call (it does whenever no stack object of the caller is passed along) makes
// the callee ineligible for the "no callee-saved registers" treatment of internal functions, and it then saves and restores every
// callee-saved VGPR it touches through scratch on each call: 72 of them in the diagonal-block stage, 117 in panel_diag_rows.
#define SDM_NOINLINE __noinline__ __attribute__((not_tail_called))
#endif
#ifndef SDM_NI_ROWS
#define SDM_NI_ROWS __forceinline__       // (measured: +1 us per launch as a call -- while calls still saved callee-saved registers, see SDM_NOINLINE)
#endif
#ifndef SDM_NI_TILES
#define SDM_NI_TILES __forceinline__      // (the throughput role of big fronts: as a call it saved and reloaded 40 callee-saved VGPRs per workgroup, +4 us per launch on MAXCUT-4000 -- before not_tail_called; not measured again)
#endif
// The roles of a k_ldl_panel workgroup are REAL function calls (as in k_ldl_front below): inlined into one body they shared one
// register allocation and the kernel spilled 167 VGPRs (round 2); each role alone fits.
// ---- row-solve workgroup b of panel `panel` (see k_ldl_panel)
__device__ SDM_NI_ROWS SDM_NORETURN void panel_role_rows(char *smem, double *Fs, const double *Ds, double *d, int ns, int ms, int ld, int first, int panel, int b,
                                             int *upd_cnt_s, const int *diag_cnt_s, int phase, int *tmo) {
  SDM_FP_STRICT;
  double (*As)[UTP] = (double (*)[UTP])smem;
  double (*Bs)[UTP] = As + NB;
  __shared__ double dsh[NB];
  const int k0c = panel * NB, kbc = min(NB, ns - k0c);
  const int kp = (panel - 1) * NB;
  const bool mfma_rows = ms - min(NB, ns) >= MFMA_MIN_ROWS;
  if (phase != 2 && panel > 0) {
    if (mfma_rows)                                              // the result doubles as the row solve's wave tiles in LDS
      update_tile<LDL_THREADS / 64, false, true, true>(Fs, ld, ms, first, kp, NB, b + 1, 0, d, As, Bs, dsh, nullptr, nullptr, kbc,
                                                        threadIdx.x, true, (double *)smem + NB * (NB + 1));
    else
      update_tile<LDL_THREADS / 64, false, true>(Fs, ld, ms, first, kp, NB, b + 1, 0, d, As, Bs, dsh);
    SDM_STORES_DONE();
    __syncthreads();
    if (threadIdx.x == 0) sdm_signal_add(upd_cnt_s);
  }
  if (phase == 1) SDM_ENDPGM();
  double (*S)[NB + 1] = (double (*)[NB + 1])smem;
  double *RB = (double *)smem + NB * (NB + 1);
  __shared__ double dsr[NB];
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6, ny = LDL_THREADS >> 6;
  const int rbeg = k0c + NB * (b + 1), rend = min(ms, k0c + NB * (b + 2));      // = tile row b+1
  if (!mfma_rows) {
    // few rows: the faithful substitution needs the whole block
    spin_until(diag_cnt_s, 4 * (panel + 1), tmo);                  // (with the fence: panel_rows re-reads this workgroup's own updated rows)
    constexpr int NQ = NB / (LDL_THREADS / 64);
    double sv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) sv[q] = sdm_load_wt(&Ds[min(ty + ny * q, NB - 1) * NB + tx]);
#pragma unroll
    for (int q = 0; q < NQ; q++) { const int i = ty + ny * q; if (i < NB) S[i][tx] = (i < kbc && tx < i) ? sv[q] : 0.0; }
    if (tid < NB) dsr[tid] = tid < kbc ? sdm_load_wt(&d[first + k0c + tid]) : 0.0;
    __syncthreads();
    panel_rows(Fs, ld, ns, ms, k0c, kbc, rbeg, rend, ROWS_BATCH, S, dsr, RB);
    SDM_ENDPGM();
  }
  // blocked substitution, 16 rows per wavefront (4 of the 8 are busy), following the diagonal block as workgroup 0
  // publishes it 16 columns at a time
  const int R0 = rbeg + 16 * ty;
  const bool busy = R0 < rend;
  double *Tw = RB + ty * (NB * 17);
  if (!(phase == 0 && panel > 0) && busy) rows_stage(Fs, ld, rend, k0c, kbc, R0, Tw, tx);      // else staged by the update above
  for (int blk = 0; blk < NB / 16 && 16 * blk < kbc; blk++) {
    if (busy) rows_block_gemm(blk, S, Tw, tx);                   // needs earlier columns only: off the tail of the launch
    spin_until(diag_cnt_s, 4 * panel + blk + 1, tmo, false);       // columns 16 blk .. of L11 and their pivots are in DT / d (sc1 loads: no fence)
    for (int e = tid; e < NB * 16; e += LDL_THREADS) {
      const int i = e >> 4, j = 16 * blk + (e & 15);
      S[i][j] = (i < kbc && j < i) ? sdm_load_wt(&Ds[i * NB + j]) : 0.0;
    }
    if (tid < 16) dsr[16 * blk + tid] = 16 * blk + tid < kbc ? sdm_load_wt(&d[first + k0c + 16 * blk + tid]) : 0.0;
    __syncthreads();
    if (busy) rows_block_tri(blk, S, dsr, Tw, tx);
  }
  if (busy) rows_store(Fs, ld, rend, k0c, kbc, R0, dsr, Tw, tx);
  SDM_ENDPGM();                                                  // (the kernel has nothing left to do for this workgroup)
}
// ---- tile workgroup w: two tiles of the previous panel's update side by side, 4 wavefronts each
__device__ SDM_NI_TILES void panel_role_tiles(char *smem, double *Fs, const double *d, int ms, int ld, int first, int panel, int w, int nrw, int nt,
                                              int *upd_cnt_s, int own) {
  SDM_FP_STRICT;
  double (*As)[UTP] = (double (*)[UTP])smem;
  double (*Bs)[UTP] = As + NB;
  const int kp = (panel - 1) * NB;
  const int half = threadIdx.x >> 8, u = 2 * w + half;
  int I, J, ntl;
  bool active;
  if (nrw > 0) {                                               // block column 0 belongs to the row-solve workgroups
    ntl = (nt - 1) * nt / 2;
    if (2 * w >= ntl) SDM_ENDPGM();
    active = u < ntl;
    tile_index(active ? u : 0, I, J);
    I++; J++;
  } else {
    ntl = nt * (nt + 1) / 2 - 1;                               // all tiles but (0,0)
    if (2 * w >= ntl) SDM_ENDPGM();
    active = u < ntl;
    tile_index(active ? u + 1 : 1, I, J);
  }
  if (!owns_col(own, panel + J)) active = false;               // (another rank's tile column; the signal below is still given)
  __shared__ double dsh2[2][NB];
  update_tile<4, false, true>(Fs, ld, ms, first, kp, NB, I, J, d, As + half * 2 * NB, Bs + half * 2 * NB, dsh2[half],
                              nullptr, nullptr, 0, (int)threadIdx.x & 255, active);
  if (nrw == 0) {                                              // readers in this launch: workgroup 0's row solve / probe
    SDM_STORES_DONE();
    __syncthreads();
    if (threadIdx.x == 0) sdm_signal_add(upd_cnt_s);
  }
  SDM_ENDPGM();
}
// ---- the same for big fronts (those with row-solve workgroups: nobody in the launch reads these tiles): workgroup w of ntw works
// through the MACRO tiles w, w + ntw, ... of the launch's schedule (tile_sched: eager macro tiles of the panel before, K = 64; deferred
// ones of a whole group of panels, K = 64 UPD_G) as one pipeline over steps of half a chunk (32 columns).
// What shaped it, each step measured on MAXCUT-4000 (profiles/r05_factor_update_variants.txt, r05l / r05m / r05s_phase_tiles_*, r05r_ubench9_*):
//   * one pair of 64 x 64 tiles per workgroup and launch (round 4, panel_role_tiles): ~10 us per pair -- dispatch, a memory round trip,
//     staging, 3.4 us of MFMAs, acknowledged write-through stores, one after the other with nothing else on the compute unit;
//   * the same tiles streamed through persistent workgroups with prefetched operands, one or two LDS buffers, lock step or the wavefront
//     halves out of phase, 8- or 16-byte loads: 4.2 us per tile step whatever the arrangement -- a step fetches 64 KB of operands, and what
//     the workgroups get delivered together is ~3 TB/s (16 GB/s each), not what the matrix cores could take (2.0 us per step);
//   * hence 2 x 2 MACRO tiles: the operand blocks A(I), A(I+1), B(J), B(J+1) of a chunk are fetched once (all four in LDS: the launch's
//     whole LDS footprint) for FOUR tile products -- half the bytes per flop -- and the macro tile is ONE 128 x 128 product, 64 x 32 per
//     wavefront (8 accumulators, 6 operand reads from LDS per 8 MFMAs: the loop runs at the matrix rate, 3.97 us per half chunk against
//     3.95 for the loop alone, tools/ubench/ubench9; as four 64 x 64 products of 32 x 16 per wavefront it ran at 55 %);
//   * steps of HALF a chunk: the 32 prefetch registers more of a whole chunk spilled, and the reloads' s_waitcnt vmcnt(0) in front of
//     the MFMA loop waited for the prefetch itself (16 us per chunk instead of 8); with half chunks the LDS blocks double-buffer in place
//     (MFMAs on one half of their columns while the other half is written) and a step needs one barrier;
//   * a macro tile's own values first, operand loads behind them (the counter of outstanding loads retires in order), plain stores for the
//     finished tile (32 write-through stores took 8 us to issue; nobody reads these tiles before the launch ends);
//   * groups of UPD_G = 2 panels: a deferred macro tile of four panels is 32 us of MFMAs on one compute unit -- more than the 26 us of the
//     chain the tiles are meant to hide behind.
// What is left: a step is 4.0 us of MFMAs + 5.6 us of everything else (waiting for operands and tile values -- a macro tile moves 512 KB for
// its 15.8 us of MFMAs, the workgroups together ask for 3 TB/s --, LDS writes, stores, barrier) that the lock step of a barrier per step
// puts in front of the MFMAs instead of beside them.  The launches from the 15th on are bound by the chain of the diagonal blocks.
// A tile's own values make one trip through the registers per macro tile and group.  Per tile: the same operands, the same instructions on
// the same accumulators, the same order as the eager schedule -- the same bits.
struct TileItem { int I, J, nch, kp0, ds0, act; };               // first tile of the macro tile (relative to tile column q); act: bit 2a+b = tile (I+a, J+b) is the item's
__device__ SDM_NI_TILES void panel_role_tiles_stream(char *smem, double *Fs, const double *d, int ns, int ms, int ld, int first, int panel, int w, int ntw, int own) {
  SDM_FP_STRICT;
  const int tid = threadIdx.x;
  double (*Ab)[UTP] = (double (*)[UTP])smem;                   // A(I) = Ab, A(I+1) = Ab + NB, B(J) = Ab + 2 NB, B(J+1) = Ab + 3 NB   (4 NB UTP doubles = PANEL_LDS_RIDE)
  __shared__ double dshs[1 + UPD_G][NB];                       // pivots: row 0 the panel before, rows 1 .. G the panels of the deferred group
  const TileSched sc = tile_sched(ns, ms, panel);
  const int nitems = tile_sched_items(sc);
  if (w >= nitems) SDM_ENDPGM();
  const int r0 = panel * NB;
  for (int e = tid; e < (1 + UPD_G) * NB; e += LDL_THREADS) {
    const int row = e / NB, k = e % NB;
    dshs[row][k] = row == 0 ? d[first + (panel - 1) * NB + k] : (sc.g2 >= 0 ? d[first + (UPD_G * sc.g2 + row - 1) * NB + k] : 0.0);
  }
  // the macro tile as ONE 128 x 128 product: wavefront wv owns the block of 64 rows x 32 columns (4 x 2 MFMA accumulators: 6 operand reads
  // from LDS per 8 MFMAs; as four 64 x 64 products of 32 x 16 per wavefront it was 3 reads per 2 MFMAs and the LDS kept the matrix pipes at
  // 55 %: 3.6 us per product against 2.0) -- inside tile (qa, qb) of the macro tile
  const int wv = tid >> 6, l = tid & 63;
  const int qa = wv >> 2, qb = (wv & 3) >> 1, cj = (wv & 1) * 32, lk = l >> 4, ll = l & 15;
  const int i2 = (tid & 31) * 2, kq = tid >> 5;                // operand staging: a work-item takes the row pair i2, i2 + 1 of the columns kq + 16 q
  auto locate = [&](int u, TileItem &t) {
    int p0, np;
    tile_sched_item(sc, panel, u, t.I, t.J, t.act, p0, np);
    t.nch = np; t.kp0 = p0 * NB; t.ds0 = np == 1 ? 0 : 1;
    if (own) for (int b = 0; b < 2; b++) if (!owns_col(own, panel + t.J + b)) t.act &= ~((1 << b) | (1 << (2 + b)));   // (another rank's tile column)
  };
  // A step covers HALF a chunk: 32 columns of the four operand blocks (64 KB: 8 sixteen-byte loads per work-item, two rows each).  The LDS
  // blocks hold a whole chunk; while the MFMAs read one half of them, the next step's operands go from the registers into the other
  // half -- one barrier per step -- and the loads of the step after that are issued.  (With whole chunks per step the 32 prefetch registers
  // more spilled, and the reloads' s_waitcnt vmcnt(0) in front of the MFMA loop waited for the prefetch itself: 16 us per chunk, not 8.)
  sdm_double2 ov[4][2];
  const int rowcap = (ms - 1) & ~1;                            // (the row pair stays inside the column: ld is even)
  auto fetch_operands = [&](const TileItem &t, int kp, int h) {
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
      const int tr = (blk < 2 ? t.I : t.J) + (blk & 1);
      const double *pp = Fs + min(r0 + tr * TILE + i2, rowcap);
#pragma unroll
      for (int q = 0; q < 2; q++) ov[blk][q] = *(const sdm_double2 *)(pp + (int64_t)(kp + 32 * h + kq + 16 * q) * ld);
    }
  };
  auto stage = [&](const TileItem &t, int ch, int h) {         // registers -> LDS, B scaled by the pivots
    const double *dsh = dshs[t.ds0 + ch];
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
      const int row = r0 + ((blk < 2 ? t.I : t.J) + (blk & 1)) * TILE + i2;
      double (*Xs)[UTP] = Ab + blk * NB;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const int k = 32 * h + kq + 16 * q;
        const double dk = blk < 2 ? 1.0 : dsh[k];
        sdm_double2 x;
        x.x = row < ms ? ov[blk][q].x * dk : 0.0; x.y = row + 1 < ms ? ov[blk][q].y * dk : 0.0;
        *(sdm_double2 *)&Xs[k][i2] = x;
      }
    }
  };
  double c[4][2][4];                                           // this wavefront's 64 x 32 block: [16-row block][16-column block][register]
  auto tile_rw = [&](const TileItem &t, bool store) {
    if (t.act >> (2 * qa + qb) & 1) {                          // (uniform per wavefront)
#pragma unroll
      for (int ra = 0; ra < 4; ra++)
#pragma unroll
        for (int cb = 0; cb < 2; cb++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int gi = r0 + (t.I + qa) * TILE + ra * 16 + ll, gj = r0 + (t.J + qb) * TILE + cj + cb * 16 + lk + 4 * r;
            double *p = &Fs[(int64_t)min(gj, ms - 1) * ld + min(gi, ms - 1)];
            if (!store) c[ra][cb][r] = *p;
            else if (gi < ms && gj < ms && gi >= gj) *p = c[ra][cb][r];   // (plain stores: nobody reads these tiles before the launch ends; write-through ones took 8 us to issue)
          }
    }
  };
  // step = (macro tile, chunk of 64 columns, half of it); `it`/`ch`/`h` the step in LDS, `nx`/`nch`/`nh` the one in the registers
  int item = w, ch = 0, h = 0;
  TileItem it, nx;
  locate(item, it);
  fetch_operands(it, it.kp0, 0);
  __syncthreads();                                             // dshs
  stage(it, 0, 0);
  int nitem = item, nch = 0, nh = 1;
  bool more = true;
  nx = it;
  fetch_operands(nx, nx.kp0, 1);
  __syncthreads();
#ifdef SDM_PHASES
  long long tp_ = wall_clock64();
  // (free slots of this file's phase array: 9 product, 10 finished tile out, 11 barrier, 12 operands -> LDS (incl. the wait for them), 0 next tile + loads issued, 24 tile values; 13 = steps)
#define SDM_TP(n) do { const long long t_ = wall_clock64(); if (threadIdx.x == 0) atomicAdd(&sdm_phase_acc[(n)], (unsigned long long)(t_ - tp_)); tp_ = t_; } while (0)
#else
#define SDM_TP(n) do {} while (0)
#endif
  sdm_double4 acc[4][2];
  for (;;) {
    // (a new macro tile's own values first: the counter of outstanding loads retires in order, and  c -= acc  must not wait for operands behind them)
    if (ch == 0 && h == 0) tile_rw(it, false);
    SDM_TP(24);
    // ---- the next step: its operands (in flight since the step before) into the other half of the blocks, then the loads of the step after it
    TileItem n2 = nx;
    int n2item = nitem, n2ch = nch, n2h = nh ^ 1;
    bool more2 = more;
    if (more) {
      stage(nx, nch, nh);
      SDM_TP(12);
      if (n2h == 0) {                                          // (the step after the next starts a new chunk, or a new macro tile)
        n2ch = nch + 1;
        if (n2ch == nx.nch) { n2item = nitem + ntw; n2ch = 0; more2 = n2item < nitems; if (more2) locate(n2item, n2); }
      }
      if (more2) fetch_operands(n2, n2.kp0 + n2ch * NB, n2h);
      SDM_TP(0);
    }
    // ---- the product of this step: this wavefront's block of tile (qa, qb) = A(I+qa) B(J+qb)', columns 32 h .. 32 h + 31 of the chunk
    if (it.act >> (2 * qa + qb) & 1) {
      double (*As)[UTP] = Ab + qa * NB, (*Bs)[UTP] = Ab + (2 + qb) * NB;
      if (h == 0) for (int ra = 0; ra < 4; ra++) for (int cb = 0; cb < 2; cb++) for (int r = 0; r < 4; r++) acc[ra][cb][r] = 0.0;
      const int k0 = 32 * h;
      double ao[4], bo[2];
#pragma unroll
      for (int ra = 0; ra < 4; ra++) ao[ra] = As[k0 + lk][ra * 16 + ll];
#pragma unroll
      for (int cb = 0; cb < 2; cb++) bo[cb] = Bs[k0 + lk][cj + cb * 16 + ll];
#pragma unroll
      for (int kk = 0; kk < 32; kk += 4) {
        const int kn = k0 + min(kk + 4, 28);
        double an[4], bn[2];
#pragma unroll
        for (int ra = 0; ra < 4; ra++) an[ra] = As[kn + lk][ra * 16 + ll];
#pragma unroll
        for (int cb = 0; cb < 2; cb++) bn[cb] = Bs[kn + lk][cj + cb * 16 + ll];
#pragma unroll
        for (int ra = 0; ra < 4; ra++)
#pragma unroll
          for (int cb = 0; cb < 2; cb++) acc[ra][cb] = SDM_MFMA_F64_16x16x4(bo[cb], ao[ra], acc[ra][cb]);
#pragma unroll
        for (int ra = 0; ra < 4; ra++) ao[ra] = an[ra];
#pragma unroll
        for (int cb = 0; cb < 2; cb++) bo[cb] = bn[cb];
      }
      if (h == 1) {
#pragma unroll
        for (int ra = 0; ra < 4; ra++)
#pragma unroll
          for (int cb = 0; cb < 2; cb++)
#pragma unroll
            for (int r = 0; r < 4; r++) c[ra][cb][r] = c[ra][cb][r] - acc[ra][cb][r];
      }
    }
    SDM_TP(9);
    if (h == 1 && ch == it.nch - 1) tile_rw(it, true);         // the macro tile is finished
    SDM_TP(10);
    if (!more) break;
    __syncthreads();                                           // the other half of the blocks is complete, this one is free
    SDM_TP(11);
#ifdef SDM_PHASES
    if (threadIdx.x == 0) atomicAdd(&sdm_phase_acc[13], 1ull);
#endif
    it = nx; item = nitem; ch = nch; h = nh;
    nx = n2; nitem = n2item; nch = n2ch; nh = n2h; more = more2;
  }
  SDM_ENDPGM();
}
// ---- workgroup 0 = the dependency chain of the launch, as a CHAIN OF STAGES that never return: the role's prologue calls the update
// of its diagonal tile, which calls the LDL' of the block, which calls the rows left to this workgroup -- each call the last thing its
// caller does.  Each stage is a function for the sake of its own register allocation (inlined into one body they spilled 167 VGPRs,
// round 2); as calls that RETURN they made their caller park what it needed afterwards -- the work-item id, a dozen addresses --
// in scratch around every call, because a called stage uses the whole register file and saves nothing (SDM_NOINLINE).  A caller
// with nothing left to do has nothing to park: what the later stages need travels along as arguments, in registers.
// (The emulator's functions do return: every stage ends with SDM_ENDPGM = return there.)

// (its few-rows form: fronts whose rows below the first block are fewer than MFMA_MIN_ROWS -- the small fronts of arch0, nb)
__device__ SDM_NOINLINE SDM_NORETURN void panel_stage_rows_few(char *smem, SDM_GP(double) Fs_, int ld, int ns, int ms, int k0, int kb, int rbeg, int rend, const double *ds) {
  panel_rows<2>((double *)Fs_, ld, ns, ms, k0, kb, rbeg, rend, TRSM_ROWS, (const double (*)[NB + 1])smem, ds, (double *)smem + NB * (NB + 1));
  SDM_ENDPGM();
}
__device__ SDM_NOINLINE SDM_NORETURN void panel_stage_rows_blocked(char *smem, SDM_GP(double) Fs_, int ld, int ns, int ms, int k0, int kb, int rbeg, int rend, const double *ds) {
  panel_rows<1>((double *)Fs_, ld, ns, ms, k0, kb, rbeg, rend, TRSM_ROWS, (const double (*)[NB + 1])smem, ds, (double *)smem + NB * (NB + 1));
  SDM_ENDPGM();
}
// last stage: the rows of the block column that are this workgroup's own
__device__ SDM_NOINLINE SDM_NORETURN void panel_stage_rows(char *smem, const FrontDesc *fdp, int panel, SDM_GP(double) F_, SDM_GP(int) upd_cnt_, int q0,
                                                          SDM_GP(int) tmo_, const double *ds, bool ok) {
  double *F = (double *)F_;
  int *upd_cnt = (int *)upd_cnt_;
  int *tmo = (int *)tmo_;
  const FrontDesc &fd = *fdp;
  const int s = fd.s, ns = fd.ns, ms = fd.ms, ld = fd.ld;
  double *Fs = F + fd.foff;
  const int k0 = panel * NB, kb = min(NB, ns - k0);
  const int r0 = k0 + kb, nrows = ms - r0;
  SDM_PHASE_BEGIN();
  int rend = r0;                                                   // rows r0 .. rend-1 are solved here (one call site: panel_rows is big)
  if (nrows > TRSM_ROWS) {
    // a partial block (kb < 64, last panel of the supernode) leaves rows r0 .. k0+63 in this workgroup's own tile row:
    // they were updated by its tile (0,0) and are solved here (the row-solve workgroups own whole tile rows)
    if (kb < NB) {
      SDM_ACQUIRE_FENCE();                                         // its own tile-(0,0) stores, not a cached copy from before them
      rend = k0 + NB;
    }
  } else if (nrows > 0) {
    if (panel > 0 && ok) wait_prev_update(upd_cnt + s, ns, ms, panel, q0, tmo);
    rend = ms;
  }
  SDM_PHASE(22);
  if (rend > r0) {
    // (the two forms of the row solve as two stages: together in one function the few-rows form spilled inside its chunk loop)
    if (ms - min(NB, ns) >= MFMA_MIN_ROWS) panel_stage_rows_blocked(smem, (SDM_GP(double))Fs, ld, ns, ms, k0, kb, r0, rend, ds);
    else panel_stage_rows_few(smem, (SDM_GP(double))Fs, ld, ns, ms, k0, kb, r0, rend, ds);
  }
  SDM_PHASE(23);
  SDM_ENDPGM();
}
// middle stage: the LDL' of the block and its publication
__device__ SDM_NOINLINE SDM_NORETURN void panel_stage_block(char *smem, SDM_GP(double) F_, SDM_GP(double) DT_, const FrontDesc *fdp, int panel, SDM_GP(double) d_, SDM_GP(double) lb_,
                                                           SDM_GP(int) pivstat_, SDM_GP(double) pivval_, SDM_GP(const PanelCtx) ctx_, SDM_GP(int) upd_cnt_, SDM_GP(int) diag_cnt_,
                                                           int q0, SDM_GP(int) tmo_) {
  double *F = (double *)F_;
  double *DT = (double *)DT_;
  double *d = (double *)d_;
  double *lb = (double *)lb_;
  int *pivstat = (int *)pivstat_;
  double *pivval = (double *)pivval_;
  const PanelCtx *ctx = (const PanelCtx *)ctx_;
  int *upd_cnt = (int *)upd_cnt_;
  int *diag_cnt = (int *)diag_cnt_;
  int *tmo = (int *)tmo_;
  const FrontDesc &fd = *fdp;
  const int k0 = panel * NB, kb = min(NB, fd.ns - k0);
  const int nrows = fd.ms - (k0 + kb);
  __shared__ double ds[NB];
  __shared__ int npub;
  const bool ok = ldl_diag_block<false>(smem, F, DT, fd, panel, d, lb, pivstat, pivval, ctx, upd_cnt, diag_cnt, q0, tmo, panel == 0, nrows > TRSM_ROWS, ds, &npub);
  if (nrows > TRSM_ROWS) {                                         // the row-solve workgroups of this launch are waiting
    if (16 * npub < kb) SDM_STORES_DONE();                         // (uniform) something of the block is still unpublished
    __syncthreads();
    if (threadIdx.x == 0) sdm_signal_add(&diag_cnt[fd.s], 4 - npub);   // 4 counts per panel: one per 16 columns of the block
    if (kb == NB) SDM_ENDPGM();                                    // nothing of the block column is left to this workgroup
  } else {
    // nobody in this launch waits for this block; the launches to come find the count (= 4 x panels done) in place -- what they
    // read of THIS launch's rows is ordered by the launch boundary, so the count need not wait for the rows below
    SDM_STORES_DONE();
    __syncthreads();
    if (threadIdx.x == 0) sdm_signal_add(&diag_cnt[fd.s], 4);
    if (nrows <= 0) SDM_ENDPGM();
  }
  panel_stage_rows(smem, fdp, panel, (SDM_GP(double))F, (SDM_GP(int))upd_cnt, q0, (SDM_GP(int))tmo, ds, ok);
  SDM_ENDPGM();
}
// first stage (panels after the first): tile (0,0) of the previous update = this panel's diagonal block, straight into S
__device__ SDM_NOINLINE SDM_NORETURN void panel_stage_update(char *smem, SDM_GP(double) F_, SDM_GP(double) DT_, const FrontDesc *fdp, int panel, SDM_GP(double) d_, SDM_GP(double) lb_,
                                                            SDM_GP(int) pivstat_, SDM_GP(double) pivval_, SDM_GP(const PanelCtx) ctx_, SDM_GP(int) upd_cnt_, SDM_GP(int) diag_cnt_,
                                                            int q0, SDM_GP(int) tmo_) {
  SDM_FP_STRICT;
  {
    const FrontDesc &fd = *fdp;
    double *Fs = (double *)F_ + fd.foff;
    const double *d = (const double *)d_;
    double (*As)[UTP] = (double (*)[UTP])smem;
    double (*Bs)[UTP] = As + NB;
    __shared__ double dsh[NB];
    update_tile<LDL_THREADS / 64, true>(Fs, fd.ld, fd.ms, fd.first, (panel - 1) * NB, NB, 0, 0, d, As, Bs, dsh,
                                        (double (*)[NB + 1])smem, (double *)smem + NB * (NB + 1), min(NB, fd.ns - panel * NB));
  }
  panel_stage_block(smem, F_, DT_, fdp, panel, d_, lb_, pivstat_, pivval_, ctx_, upd_cnt_, diag_cnt_, q0, tmo_);
  SDM_ENDPGM();
}
// the role's prologue
__device__ SDM_NOINLINE SDM_NORETURN void panel_role_diag(char *smem, SDM_GP(double) F_, SDM_GP(double) DT_, FrontDesc *fdp, int panel, SDM_GP(double) d_,
                                                         SDM_GP(const PanelCtx) ctx_, SDM_GP(int) upd_cnt_, SDM_GP(int) diag_cnt_, int q0, SDM_GP(int) tmo_) {
  const PanelCtx *ctx = (const PanelCtx *)ctx_;
  // (uniform loads: one scalar round trip, issued before the tile of the previous update is fetched)
  double *lb = ctx->lb; int *pivstat = ctx->pivstat; double *pivval = ctx->pivval;
  {
    const double *ubp = ctx->ubp;
    const double maxu = ubp[1], ub = ubp[2] / (maxu * maxu);
    if (threadIdx.x == 0) { fdp->maxu = maxu; fdp->ub = ub; }      // (read behind the first barrier of the diagonal block)
  }
  if (panel > 0) panel_stage_update(smem, F_, DT_, fdp, panel, d_, (SDM_GP(double))lb, (SDM_GP(int))pivstat, (SDM_GP(double))pivval, ctx_, upd_cnt_, diag_cnt_, q0, tmo_);
  else panel_stage_block(smem, F_, DT_, fdp, panel, d_, (SDM_GP(double))lb, (SDM_GP(int))pivstat, (SDM_GP(double))pivval, ctx_, upd_cnt_, diag_cnt_, q0, tmo_);
  SDM_ENDPGM();
}

__global__ void __launch_bounds__(LDL_THREADS)
k_ldl_panel(double *F, double *DT, FrontTab tab, const int *list, int panel, double *d, const PanelCtx *ctx,
            int *upd_cnt, int *diag_cnt, int q0, int phase, int *tmo, int own) {
  SDM_FP_STRICT;   // no FMA contraction: the pivot decisions must see the reference's mul-then-subtract rounding
  SDM_DYN_SMEM(smem);
  // ONE launch per 64-column panel p.  grid = (workgroups, fronts); per front:
  //   workgroup 0        tile (0,0) of the trailing update of panel p-1 (its own diagonal block), then the LDL' of the
  //                      block, published (DT, d) for the row-solve workgroups;
  //   1 .. nrw           (fronts with more than TRSM_ROWS rows below the block) row solve of ROWS_BATCH rows each: first
  //                      the tile of the previous update that covers exactly those rows in this panel's columns, then
  //                      -- once workgroup 0 has published the factored block -- the substitution;
  //   the rest           the other tiles of the previous update, two side by side per workgroup (nobody in this launch
  //                      reads them, except in fronts without row-solve workgroups, where they signal).
  // All of this hides behind workgroup 0's dependency chain.  The emulator runs workgroups one after the other:
  // phase 1 (everything but the substitution, diagonal block last) and phase 2 (the substitution) are two launches
  // there; the GPU runs phase 0 = both.
  const int s = list[blockIdx.y];
  const int ns = tab.ns[s], ms = tab.ms[s], ld = tab.ld[s], first = tab.first[s];
  double *Fs = F + tab.foff[s];
  const int k0 = panel * NB, kb = min(NB, ns - k0);
  const int r0 = k0 + kb, nrows = ms - r0;
  const int nrw = nrows > TRSM_ROWS ? (ms - (k0 + NB) + ROWS_BATCH - 1) / ROWS_BATCH : 0;   // tile rows below the first
  const int nt = panel > 0 ? (ms - k0 + TILE - 1) / TILE : 0;    // tile rows of the previous panel's update
  // Roles by "logical" index bx: 0 = diagonal block, 1..nrw = row solves, beyond = update tiles.  The hardware hands
  // out workgroups in launch order, and a workgroup that waits must wait for one handed out BEFORE it (or for one
  // that does not wait before it signals), else a full device of waiting workgroups could keep the awaited one out:
  //   fronts with row-solve workgroups:  diagonal block < row solves (wait for it) < tiles (nobody waits for them);
  //   small fronts:                      tiles (never wait) < diagonal block (its in-workgroup row solve waits for them).
  // The emulator runs them one after the other in the order  tiles, row solves (phase 1: their update tile only),
  // diagonal block.
  int bx = blockIdx.x;
#ifdef SDM_EMU
  if (phase != 0) bx = (int)gridDim.x - 1 - (int)blockIdx.x;        // (phase 0 in the emulator: its workgroups run as concurrent processes, roles as on the device)
  else
#endif
  if (nrw == 0) {
    const int ntw = panel > 0 ? (nt * (nt + 1) / 2) / 2 : 0;
    if (bx > ntw) return;
    bx = bx < ntw ? 1 + bx : 0;
  }
  if (bx <= nrw && !owns_col(own, panel)) return;                  // (block-cyclic ranks: the panel is factored by the owner of its tile column alone)
  if (bx > 0 && bx <= nrw) {
    panel_role_rows(smem, Fs, DT + tab.toff[s] + (int64_t)panel * NB * NB, d, ns, ms, ld, first, panel, bx - 1, upd_cnt + s, diag_cnt + s, phase, tmo);
    return;
  }
  if (bx > nrw) {
    if (phase == 2 || panel == 0) return;
    if (nrw > 0) panel_role_tiles_stream(smem, Fs, d, ns, ms, ld, first, panel, bx - 1 - nrw, (int)gridDim.x - 1 - nrw, own);
    else panel_role_tiles(smem, Fs, d, ms, ld, first, panel, bx - 1 - nrw, nrw, nt, upd_cnt + s, own);
    return;
  }
  // ---- workgroup 0
  if (phase == 2) return;
  __shared__ FrontDesc fd;                                          // (every work-item writes the same values: no barrier needed before it reads them back)
  fd.ns = ns; fd.ms = ms; fd.ld = ld; fd.first = first; fd.foff = tab.foff[s]; fd.toff = tab.toff[s]; fd.woff = tab.woff[s]; fd.s = s;
  panel_role_diag(smem, (SDM_GP(double))F, (SDM_GP(double))DT, &fd, panel, (SDM_GP(double))d, (SDM_GP(const PanelCtx))ctx, (SDM_GP(int))upd_cnt, (SDM_GP(int))diag_cnt, q0,
                  (SDM_GP(int))tmo);
}

// k_ldl_front calls its three stages through real function calls: each gets a register allocation of its own.  Inlined
// into one body they share 256 VGPRs with the sweep code of the diagonal block and spill inside the store loops -- and a
// scratch reload between two write-through stores waits for the first one's acknowledgement (vmcnt counts in order):
// every stored tile then costs eight memory round trips instead of one.
__device__ SDM_NOINLINE bool front_diag(char *smem, SDM_GP(double) F_, SDM_GP(double) DT_, const FrontDesc *fd, int panel, SDM_GP(double) d_, SDM_GP(double) lb_,
                                        SDM_GP(int) pivstat_, SDM_GP(double) pivval_, SDM_GP(const PanelCtx) ctx_, SDM_GP(int) upd_done_, SDM_GP(int) diag_cnt_, SDM_GP(int) tmo_,
                                        bool load_block, bool publish, double *ds, int *npub, bool raw_in_lds, const double *lbs_pre) {
  double *F = (double *)F_;
  double *DT = (double *)DT_;
  double *d = (double *)d_;
  double *lb = (double *)lb_;
  int *pivstat = (int *)pivstat_;
  double *pivval = (double *)pivval_;
  const PanelCtx *ctx = (const PanelCtx *)ctx_;
  int *upd_done = (int *)upd_done_;
  int *diag_cnt = (int *)diag_cnt_;
  int *tmo = (int *)tmo_;
  return ldl_diag_block<true>(smem, F, DT, *fd, panel, d, lb, pivstat, pivval, ctx, upd_done, diag_cnt, 0, tmo, load_block, publish, ds, npub, raw_in_lds, 0, lbs_pre);
}
// kind 0: plain (result to the front only), 2: also the wave tiles of the next row solve (RB)
__device__ SDM_NOINLINE void front_update(int kind, SDM_GP(double) Fs_, int ld, int ms, int first, int k0, int I, int J, SDM_GP(const double) d_, char *smem,
                                          double *dsh, int kbn) {
  double *Fs = (double *)Fs_;
  const double *d = (const double *)d_;
  double (*As)[UTP] = (double (*)[UTP])smem;
  double (*Bs)[UTP] = As + NB;
  double *RB = (double *)smem + NB * (NB + 1);
  if (kind == 2) update_tile<LDL_THREADS / 64, false, true, true>(Fs, ld, ms, first, k0, NB, I, J, d, As, Bs, dsh, nullptr, nullptr, kbn, threadIdx.x, true, RB);
  else update_tile<LDL_THREADS / 64, false, true>(Fs, ld, ms, first, k0, NB, I, J, d, As, Bs, dsh);
}
// R: rows of tile row r against the diagonal block of panel q as it is published; have_tw: the tile is in the wave tiles already
__device__ SDM_NOINLINE void front_rows(SDM_GP(double) Fs_, SDM_GP(const double) Ds_, int ld, int ms, int q, int kb, int r, char *smem,
                                        double *dsr, SDM_GP(int) tmo_, bool have_tw, bool defer_ack) {
  double *Fs = (double *)Fs_;
  const double *Ds = (const double *)Ds_;
  int *tmo = (int *)tmo_;
  double (*S)[NB + 1] = (double (*)[NB + 1])smem;
  double *RB = (double *)smem + NB * (NB + 1);
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  const int k0 = q * NB, rbeg = r * TILE, rend = min(ms, rbeg + TILE);
  const int R0 = rbeg + 16 * ty;
  const bool busy = R0 < rend;
  double *Tw = RB + ty * (NB * 17);
  if (!have_tw && busy) rows_stage(Fs, ld, rend, k0, kb, R0, Tw, tx);
  for (int blk = 0; blk < NB / 16 && 16 * blk < kb; blk++) {
    if (busy) rows_block_gemm(blk, S, Tw, tx);
    diag_group_fetch(Ds, blk, kb, S, dsr, tmo);                      // polls the data itself (DT starts as a sentinel)
    if (busy) rows_block_tri(blk, S, dsr, Tw, tx);
  }
  if (busy) rows_store<true>(Fs, ld, rend, k0, kb, R0, dsr, Tw, tx);
  if (defer_ack) return;                                           // the caller counts the rows after its next piece of work
  SDM_STORES_DONE();
  __syncthreads();
}
// The two of them fused for the workgroup on the chain (r = q + 1): the rows are solved 16 columns at a time as before, but
// every finished 16-column block is scaled (l = x / d, as rows_store does) and kept in LDS (Lt, the wave tiles the four idle
// wavefronts do not use; it goes to the front write-through when the LAST block has arrived -- the column probe of the diagonal
// block's workgroup must find the rows unsolved until then), and the update of the workgroup's own diagonal tile reads its operands
// from there -- A operand l, B operand l * d, the products in the same k order as update_tile, so the same bits.  The
// K = 48 part of the update runs while the last 16 columns of the diagonal block are still being factored; after they
// arrive only their triangle, 4 of the 16 k-steps and the epilogue are left.  The raw updated block stays in LDS (cvl:
// the general path of the LDL' reloads it from there); it reaches the front as the factored block.
__device__ SDM_NOINLINE void front_rows_diag(SDM_GP(double) Fs_, SDM_GP(const double) Ds_, int ld, int ms, int q, int r, char *smem,
                                             double *dsr, SDM_GP(int) tmo_, bool have_tw, int kbn) {
  double *Fs = (double *)Fs_;
  const double *Ds = (const double *)Ds_;
  int *tmo = (int *)tmo_;
  double (*S)[NB + 1] = (double (*)[NB + 1])smem;
  double *RB = (double *)smem + NB * (NB + 1);
  double *cvl = (double *)smem + FRONT_CV_OFF;
  constexpr int NW = LDL_THREADS / 64;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  const int k0 = q * NB, rbeg = r * TILE, rend = min(ms, rbeg + TILE);
  const int R0 = rbeg + 16 * ty;
  const bool busy = R0 < rend && ty < 4;
  double *Tw = RB + ty * (NB * 17);
  double *Lt = RB + 4 * (NB * 17);                                    // Lt[w * NB*17 + c*17 + li] = l(row 16w + li, column c)
  const int li = tx & 15, lk = tx >> 4;
  const int wi = ty >> 2, wj = ty & 3;                                // update_tile's NW = 8 mapping: rows 32 wi + 16 a + li, columns 16 wj + ..
  sdm_double4 acc[2];
  for (int a = 0; a < 2; a++) for (int x = 0; x < 4; x++) acc[a][x] = 0.0;
  if (!have_tw && busy) rows_stage(Fs, ld, rend, k0, NB, R0, Tw, tx);
  for (int blk = 0; blk < NB / 16; blk++) {
    if (busy) rows_block_gemm(blk, S, Tw, tx);
    diag_group_fetch(Ds, blk, NB, S, dsr, tmo);                      // polls the data itself (DT starts as a sentinel)
    SDM_TRACE(16 * q + 2 + blk);                                     // R of the chain workgroup: group blk has arrived
    if (busy) {
      rows_block_tri(blk, S, dsr, Tw, tx);
      // l = x / d of the block's 16 columns: to the front (write-through) and to Lt (rows beyond the front: 0)
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++) {
        const int c = 16 * blk + 4 * c4 + lk, row = R0 + li;
        const double dc = dsr[c], xv = Tw[c * 17 + li];
        const double l = (row < rend && dc > 0.0) ? xv / dc : 0.0;
        if (blk == 3 && row < rend) sdm_store_wt(&Fs[(int64_t)(k0 + c) * ld + row], l);
        Lt[ty * (NB * 17) + c * 17 + li] = l;
      }
    } else if (blk == 3 && ty >= 4) {
      // the rows of the first three groups go to the front only NOW, when the last group has arrived.  Until then workgroup q may
      // still take the general path for a later column of its block, and the column probe reads these rows' unsolved values
      // from the front (a store per finished group -- the first form of this function -- replaced them with multipliers under
      // the probe's eyes: wrong pivot decisions on rank-deficient fronts, profiles/r03ap_soak_def.txt).  The four wavefronts
      // without rows of their own write them from Lt, beside the last group's substitution.  (Keeping the store per group and
      // giving the probe a shadow copy of the unsolved rows is no faster: profiles/r03at.  The loop must NOT be unrolled: with
      // 12 loads and addresses in flight the function needs callee-saved VGPRs and saves 76 of them through scratch on every
      // call, 1.4 us per panel -- tests/test_abi.py checks.)
      const int w = ty - 4, rowb = rbeg + 16 * w + li;
#pragma unroll 1
      for (int c4 = 0; c4 < 12; c4++) {
        const int c = 4 * c4 + lk;
        if (rowb < rend) sdm_store_wt(&Fs[(int64_t)(k0 + c) * ld + rowb], Lt[w * (NB * 17) + c * 17 + li]);
      }
    }
    if (blk < 2) continue;
    __syncthreads();                                                  // Lt of the columns up to 16 blk + 15 is complete
    if (blk == 3) {
      // S and the wave tiles are dead (the substitution is over), Lt is not: S / Lc of the LDL' (Lc overlays the wave tiles, not
      // Lt) are prepared beside the update's last k-steps instead of behind them
      static_assert(NB * NB <= 4 * (NB * 17), "Lc of the LDL' must end before Lt");
      double *Lc = RB;
      for (int j = ty; j < NB; j += NW) { S[tx][j] = (tx == j && tx >= kbn) ? 1.0 : 0.0; Lc[j * NB + tx] = 0.0; }
    }
    // k-steps of the update whose columns are final: 0 .. 11 after block 2, 12 .. 15 after block 3
    for (int kk = (blk == 2 ? 0 : 48); kk < (blk == 2 ? 48 : 64); kk += 4) {
      const int k = kk + lk;
      const double bv = Lt[wj * (NB * 17) + k * 17 + li] * dsr[k];
#pragma unroll
      for (int a = 0; a < 2; a++) acc[a] = SDM_MFMA_F64_16x16x4(bv, Lt[(2 * wi + a) * (NB * 17) + k * 17 + li], acc[a]);
    }
  }
  __syncthreads();                                                    // S / Lc of the LDL' are cleared
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const int ti = wi * 32 + a * 16 + li, tj = 16 * wj + lk + 4 * x;
      if (rbeg + ti < ms && rbeg + tj < ms && ti >= tj) {
        const double v = cvl[tj * TILE + ti] - acc[a][x];
        cvl[tj * TILE + ti] = v;                                      // the raw updated block (general path of the LDL')
        if (ti < kbn) S[ti][tj] = v;
      }
    }
  SDM_TRACE(16 * q + 7);                                               // chain workgroup: its diagonal tile is in the LDS arrays of the LDL'
}

// ---- the whole LDL' of a front in ONE launch (fronts of FRONT_MINMS <= m_s <= 64 FRONT_MAXT rows; chol_build decides per
// level).  All workgroups resident.  One ROW workgroup per 64-row tile row r of the front; for the panels q = 0, 1, ... it does
//   q <  r   R: rows of tile (r, q) against the factored diagonal block of panel q (published by workgroup q, 16 columns
//               at a time, exactly as in k_ldl_panel), result stored write-through and counted in row_cnt[r];
//            U: the LAST update of the tile in the next panel's column, (r, q+1) -= L(r, q) D_q L(q+1, q)': it stays in LDS
//               as the next R's input, or -- r = q+1 -- goes straight into the LDS arrays of the LDL';
//   q == r   D: LDL' of the diagonal block (ldl_diag_block), then the workgroup is done.
// The TILE workgroups apply the other updates q = 0 .. c-2 of the tiles (r, c), 2 <= c <= r, as soon as row_cnt says L(r, q)
// and L(c, q) are there, and count them in tile_cnt (the row workgroup waits for it before the tile's last update): a row
// workgroup never has more than one tile update between two row solves.  One workgroup per tile by default (chol_build's
// FRONT_POOL rule); with fewer, workgroup w owns the tiles w, w + ntw, ... and goes through them panel by panel.
// The chain per panel is D -> (hand-over) -> last block of R in workgroup q+1 -> its diagonal tile -> D: no launch
// boundary, no wait for the slowest row workgroup.  Arithmetic and its order per entry are those of the launch-per-panel
// path (same device functions), so both produce the same bits.  upd_done[r] counts the U steps finished (the rare column
// probe of a later diagonal block waits for them).  The emulator runs workgroups one after the other: there the host
// loops over (step, phase 1 = D, 2 = R, 3 = U) and nothing is carried in LDS.
// (scalar arguments: they travel in the 32 argument registers of the convention; a FrontTab by reference made the kernel keep its copy in scratch)
static_assert(FOLLOW_DT_SENTINEL == DT_SENTINEL, "the follower polls the words of DT for the sentinel the factor arms them with");
__device__ SDM_NOINLINE void front_follow_stage(char *smem, int bx, int fs, int ns, int ld, int sld, int slot, int sboff, int64_t foff, int64_t soff, int64_t toff,
                                                 SDM_GP(const double) F_, SDM_GP(const double) DT_, SDM_GP(double) S_, SDM_GP(double) STr_, SDM_GP(int) front_cnt_,
                                                 SDM_GP(const int) diag_cnt_, SDM_GP(unsigned long long) sb_g_, SDM_GP(int) tmo_) {
  FollowDesc fd;
  fd.s = fs; fd.ns = ns; fd.ld = ld; fd.sld = sld; fd.slot = slot; fd.sboff = sboff; fd.foff = foff; fd.soff = soff; fd.toff = toff;
  sinv_follow_body(smem, bx, fd, (const double *)F_, (const double *)DT_, (double *)S_, (double *)STr_, (int *)front_cnt_, (const int *)diag_cnt_,
                   (unsigned long long *)sb_g_, (int *)tmo_);
}
__global__ void __launch_bounds__(LDL_THREADS)
k_ldl_front(double *F, double *DT, FrontTab tab, const int *list, double *d, double *lb, const double *ubp, int *pivstat,
            double *pivval, const PanelCtx *ctx, int *front_cnt, int *diag_cnt, int phase, int step, int tile_wg0, int *tmo, FollowArgs fa) {
  SDM_FP_STRICT;
  SDM_DYN_SMEM(smem);
  if (fa.S && (int)blockIdx.x >= fa.nfront) {
    // ---- the workgroups that build the front's inverse for the solves BEHIND its factorisation (sdm_follow.h; they poll the counters
    // the workgroups below count).  They used to be a launch of their own on a second stream: forking to it and joining it again cost
    // 6.8 + 11.5 us of every factorisation (event record, cross-queue wait: profiles/r04p_*, r04q_*); as the last workgroups of this
    // launch -- dispatched after every workgroup they wait for -- they cost nothing.  256 of the 512 work-items do the work: a
    // wavefront that has ended is not waited for by the barriers of the others.
    if (threadIdx.x >= ST) return;
    const FollowDesc fd = follow_desc(tab, list, (int)blockIdx.y);
    front_follow_stage(smem, (int)blockIdx.x - fa.nfront, fd.s, fd.ns, fd.ld, fd.sld, fd.slot, fd.sboff, fd.foff, fd.soff, fd.toff, (SDM_GP(const double))F,
                       (SDM_GP(const double))DT, (SDM_GP(double))fa.S, (SDM_GP(double))fa.STr, (SDM_GP(int))front_cnt, (SDM_GP(const int))diag_cnt,
                       (SDM_GP(unsigned long long))fa.sb_g, (SDM_GP(int))tmo);
    return;
  }
  const int s = list[blockIdx.y];
  const int ns = tab.ns[s], ms = tab.ms[s], ld = tab.ld[s], first = tab.first[s];
  const int T = (ms + TILE - 1) / TILE, NP = (ns + NB - 1) / NB;
  double *Fs = F + tab.foff[s];
  int *row_cnt = front_cnt + (int64_t)tab.fslot[s] * FRONT_CNT, *upd_done = row_cnt + FRONT_MAXT, *tile_cnt = upd_done + FRONT_MAXT;
  __shared__ double dsh[NB], ds[NB], dsr[NB];
  __shared__ int npub;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= tile_wg0) {
    // ---- tile workgroup: owner of the tiles t = w, w + ntw, ... (tiles (rt, ct), 2 <= ct <= rt, counted column by column)
    // for the updates of the panels q <= ct - 2 (the last update of a tile, q = ct - 1, belongs to the row workgroup: its
    // result is the next R's / D's input).  Panel by panel, and within a panel its tiles left to right: the tiles the
    // chain needs next (column q + 2) come first.  Everything it waits for (the rows of panel q) depends on tile updates
    // of EARLIER panels only, which this loop has finished by then.
    if (phase != 0 && phase != 3) return;
    const int w = (int)blockIdx.x - tile_wg0, ntw = fa.nfront - tile_wg0;   // (the grid carries the follower workgroups behind the fa.nfront of the factorisation)
    if (w >= (T - 1) * (T - 2) / 2) return;
    for (int q = (phase == 0 ? 0 : step); q < (phase == 0 ? NP : step + 1) && q <= T - 3; q++) {
      int ct = 2, c0 = 0;                                              // c0 = index of tile (ct, ct)
      for (int t = w; t < (T - 1) * (T - 2) / 2; t += ntw) {
        while (t >= c0 + (T - ct)) { c0 += T - ct; ct++; }
        const int rt = ct + (t - c0);
        if (q > ct - 2) continue;
        spin_until(row_cnt + rt, q + 1, tmo);
        if (ct < rt) spin_until(row_cnt + ct, q + 1, tmo);
        front_update(0, (SDM_GP(double))Fs, ld, ms, first, q * NB, rt - (q + 1), ct - (q + 1), (SDM_GP(const double))d, smem, dsh, 0);
        SDM_STORES_DONE();
        __syncthreads();
        if (tid == 0) sdm_signal_add(&tile_cnt[rt * FRONT_MAXT + ct]);
      }
    }
    return;
  }
  const int r = blockIdx.x;
  if (r >= T) return;
  const bool carry = phase == 0;
  __shared__ FrontDesc fd;                                          // (every work-item writes the same values: no barrier needed before it reads them back)
  fd.ns = ns; fd.ms = ms; fd.ld = ld; fd.first = first; fd.foff = tab.foff[s]; fd.toff = tab.toff[s]; fd.woff = tab.woff[s]; fd.s = s;
  { const double maxu = ubp[1]; fd.maxu = maxu; fd.ub = ubp[2] / (maxu * maxu); }
  __shared__ double lbs_pre[NB];
  if (carry && r < NP && tid < NB) lbs_pre[tid] = r * NB + tid < ns ? lb[first + r * NB + tid] : 0.0;      // thresholds of the block this workgroup will factor
  bool have_S = false, have_tw = false, raw_in_lds = false;
  for (int q = carry ? 0 : step; q < (carry ? NP : step + 1) && q <= r; q++) {
    const int k0 = q * NB, kb = min(NB, ns - k0);
    if (q == r) {
      if (phase == 0 || phase == 1) {
        const int nrows = ms - (k0 + kb);
        front_diag(smem, (SDM_GP(double))F, (SDM_GP(double))DT, &fd, q, (SDM_GP(double))d, (SDM_GP(double))lb, (SDM_GP(int))pivstat, (SDM_GP(double))pivval, (SDM_GP(const PanelCtx))ctx,
                   (SDM_GP(int))upd_done, (SDM_GP(int))diag_cnt, (SDM_GP(int))tmo, !have_S, nrows > 0, ds, &npub, raw_in_lds, carry ? lbs_pre : nullptr);
        if (nrows > 0) {
          if (16 * npub < kb) SDM_STORES_DONE();
          __syncthreads();
          if (tid == 0) sdm_signal_add(&diag_cnt[s], 4 - npub);
        } else {                                                      // nobody in this launch waits for the last block; k_sinv_follow does
          SDM_STORES_DONE();
          __syncthreads();
          if (tid == 0) sdm_signal_add(&diag_cnt[s], 4);
        }
      }
      break;
    }
    const int rbeg = r * TILE;
#if defined(SDM_PHASES) && !defined(SDM_EMU)
    const bool crit = r == q + 1;
    long long fph_ = wall_clock64();
#define SDM_FPHASE(n) do { const long long t_ = wall_clock64(); if (crit && threadIdx.x == 0) atomicAdd(&sdm_phase_acc[n], (unsigned long long)(t_ - fph_)); fph_ = t_; } while (0)
#else
#define SDM_FPHASE(n) do {} while (0)
#endif
    const bool crit_lds = carry && r == q + 1 && q + 1 < NP;         // the next diagonal block's workgroup: its tile update runs from LDS
    if (crit_lds) {
      // the tile's current values into LDS while the diagonal block of panel q is still being factored
      if (r >= 2) spin_until(tile_cnt + r * FRONT_MAXT + r, q, tmo);
      else SDM_ACQUIRE_FENCE();
      double *cvl = (double *)smem + FRONT_CV_OFF;
      double t8[NB * TILE / LDL_THREADS];
#pragma unroll
      for (int j = 0; j < NB * TILE / LDL_THREADS; j++) {
        const int e = tid + LDL_THREADS * j, ti = e & 63, tj = e >> 6;
        t8[j] = Fs[(int64_t)min(rbeg + tj, ms - 1) * ld + min(rbeg + ti, ms - 1)];
      }
#pragma unroll
      for (int j = 0; j < NB * TILE / LDL_THREADS; j++) cvl[tid + LDL_THREADS * j] = t8[j];
    }
    if (phase == 0 || phase == 2) {
      // ---- R: 16 rows per wavefront (4 of the 8 busy), following the diagonal block as workgroup q publishes it
      if (crit_lds) front_rows_diag((SDM_GP(double))Fs, (SDM_GP(const double))(DT + tab.toff[s] + (int64_t)q * NB * NB), ld, ms, q, r, smem, dsr, (SDM_GP(int))tmo, have_tw,
                                    min(NB, ns - (q + 1) * NB));
      else front_rows((SDM_GP(double))Fs, (SDM_GP(const double))(DT + tab.toff[s] + (int64_t)q * NB * NB), ld, ms, q, kb, r, smem, dsr, (SDM_GP(int))tmo, have_tw, false);
      SDM_FPHASE(1);
      have_tw = false;
      if (crit_lds) {
        have_S = true; raw_in_lds = true;
        SDM_FPHASE(4);
        // (counting these from inside the next LDL', behind its first sweep, takes the acknowledgement wait off this workgroup's
        // path -- and puts 2 us on the path of tile row r + 1, whose last update before ITS turn waits for exactly this count:
        // measured slower, profiles/r03l)
        SDM_STORES_DONE();
        __syncthreads();
        if (tid == 0) { sdm_signal_add(&row_cnt[r]); sdm_signal_add(&upd_done[r]); }
        SDM_FPHASE(5);
        SDM_TRACE(16 * q + 8);                                         // its rows acknowledged and counted
        continue;
      }
      if (tid == 0) sdm_signal_add(&row_cnt[r]);
      SDM_FPHASE(2);                                                  // rows stored, acknowledged, counted
    }
    if (phase == 0 || phase == 3) {
      // ---- U: the LAST update of the tile in the next panel's column, (r, q+1); its earlier ones came from the tile's
      // own workgroup (tile_cnt), the others of this row are theirs altogether
      const int c1 = q + 1;
      if (c1 <= r) {
        SDM_ACQUIRE_FENCE();                                          // this workgroup's own L(r, q), not a cached copy from before
        if (c1 >= 2) spin_until(tile_cnt + r * FRONT_MAXT + c1, q, tmo);
        if (c1 < r) spin_until(row_cnt + c1, q + 1, tmo);
        SDM_FPHASE(3);                                                // fence + counters
        const int I = r - c1, J = 0;
        const int kbn = min(NB, ns - c1 * NB);                        // columns of the next panel (<= 0: none)
        if (c1 < r && carry && c1 < NP) { front_update(2, (SDM_GP(double))Fs, ld, ms, first, k0, I, J, (SDM_GP(const double))d, smem, dsh, kbn); have_tw = true; }
        else front_update(0, (SDM_GP(double))Fs, ld, ms, first, k0, I, J, (SDM_GP(const double))d, smem, dsh, kbn);
      }
      SDM_FPHASE(4);                                                  // the tile update
      SDM_STORES_DONE();
      __syncthreads();
      if (tid == 0) sdm_signal_add(&upd_done[r]);
      SDM_FPHASE(5);
    }
  }
}

// stand-alone update.  Supernodes that END with this panel: all tiles (the update of the rows beyond, passed up to the
// parent).  Supernodes with a next panel: nothing when `riding` (their tiles ride along with the diagonal-block launch
// of the next panel, k_ldl_panel), else every tile but tile 0 (which k_ldl_panel's workgroup 0 always applies itself).
__global__ void __launch_bounds__(256)
k_ldl_update(double *F, FrontTab tab, const int *list, int panel, const double *d, int riding) {
  __shared__ double As[NB][UTP];
  __shared__ double Bs[NB][UTP];
  __shared__ double dsh[NB];
  const int s = list[blockIdx.y];
  const int ns = tab.ns[s], ms = tab.ms[s], ld = tab.ld[s], first = tab.first[s];
  const int k0 = panel * NB, kb = min(NB, ns - k0);
  const bool has_next = ns > k0 + NB;
  if (has_next && riding) return;
  const int nrem = ms - (k0 + kb);
  const int nt = (nrem + TILE - 1) / TILE;
  const int t = blockIdx.x + (has_next ? 1 : 0);
  if (t >= nt * (nt + 1) / 2) return;
  int I, J;
  tile_index(t, I, J);
  update_tile<4, false>(F + tab.foff[s], ld, ms, first, k0, kb, I, J, d, As, Bs, dsh);
}

// ============================================================ host drivers
void chol_forget_plan(sdm_plan *P) { PersistTurn::forget(P); }
FrontTab front_tab(CholPlan &C) {
  FrontTab t;
  t.soff = C.d_soff.p; t.sld = C.d_sld.p; t.sboff = C.d_sboff.p; t.ltoff = C.d_ltoff.p;
  t.first = C.d_first.p; t.ns = C.d_ns.p; t.ms = C.d_ms.p; t.ld = C.d_ld.p;
  t.foff = C.d_foff.p; t.xl = C.d_xl.p; t.woff = C.d_woff.p; t.roff = C.d_roff.p; t.toff = C.d_toff.p; t.fslot = C.d_fslot.p;
  t.childptr = C.d_childptr.p; t.childlist = C.d_childlist.p; t.lindx = C.d_lindx.p; t.relidx = C.d_relidx.p;
  return t;
}
#ifndef SDM_EMU
// the launch is sized from what the runtime says fits: workgroups of k_ldl_front per compute unit at its LDS and register
// footprint (1 on gfx950: 135 KB of LDS) -- 0 means the kernel cannot be resident on this device at all (a partition with
// less LDS, a debugger's reservation): no level takes the one-launch path then
int chol_front_wgs_per_cu() {
  int per_cu = 0;
  SDM_HIP_CHECK(hipFuncSetAttribute((const void *)k_ldl_front, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FRONT_LDS));
  SDM_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_ldl_front, LDL_THREADS, FRONT_LDS));
  return per_cu;
}
#endif
static inline int grid1d(int64_t n, int bs, int cap = 4096) {
  int64_t g = (n + bs - 1) / bs;
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}

void chol_begin(sdm_plan *P, const double canceltol, const double maxu, const double abstol, int use_absd) {
  CholPlan &C = P->chol;
  hipStream_t st = P->stream;
  const int m = (int)C.m;
  P->factored = false;               // until the launches below have all been issued: a factorisation that throws leaves no factor behind
#ifndef SDM_EMU
  SDM_HIP_CHECK(hipFuncSetAttribute((const void *)k_ldl_panel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PANEL_LDS_RIDE));
  SDM_HIP_CHECK(hipFuncSetAttribute((const void *)k_ldl_front, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FRONT_LDS));
#endif
  // (DT needs its sentinel only where k_ldl_front runs; the launch-per-panel levels wait on counters)
  bool any_persist = false;
  for (int l = 0; l < C.nlevels; l++) any_persist = any_persist || C.lev_persist[l];
  const int64_t ndt = any_persist ? C.tsize : 0;
  PrepArgs pa = {m, P->ada_val.p, C.d_asm_src.p, C.d_Ljc.p, C.d_perm.p, P->absd.p, use_absd, canceltol, maxu, abstol, C.lb.p, C.ub.p, C.pivstat.p, C.pivval.p,
                 (int)C.nsuper, C.upd_cnt.p, C.diag_cnt.p, C.sb_g.p, (int)C.sb_g.n, C.front_cnt.p, (int)C.front_cnt.n, (unsigned long long *)C.frontsT.p, ndt};
  const int nprep = grid1d(std::max<int64_t>(m, ndt / 4), 256, 256);
  if (C.d_asm_fsrc.n) {
    if (!C.prep_part.p) { C.prep_part.alloc(256); C.prep_ticket.alloc(1); SDM_HIP_CHECK(hipMemsetAsync(C.prep_ticket.p, 0, sizeof(int), st)); }
    SDM_KLAUNCH(P, k_begin_factor, dim3(nprep + grid1d(C.fsize, 256)), dim3(256), 0, pa, nprep, C.prep_part.p, C.prep_ticket.p, C.fronts.p, C.d_asm_fsrc.p, (int64_t)C.fsize);
  } else {
    SDM_HIP_CHECK(hipMemsetAsync(C.fronts.p, 0, (size_t)C.fsize * sizeof(double), st));
    SDM_KLAUNCH(P, k_assemble, dim3(grid1d(C.nnzL, 256)), dim3(256), 0, C.fronts.p, P->ada_val.p, C.d_asm_src.p,
               C.d_asm_dst.p, (int64_t)C.nnzL, C.ub.p);
    SDM_KLAUNCH(P, k_prep_pivots, dim3(nprep), dim3(256), 0, pa);
  }
  C.pars_canceltol = canceltol; C.pars_maxu = maxu; C.pars_abstol = abstol; C.pars_use_absd = use_absd;
  {
    PanelCtx c = {};
    c.lb = C.lb.p; c.ubp = C.ub.p; c.pivstat = C.pivstat.p; c.pivval = C.pivval.p; c.colbuf = C.colbuf.p; c.ada = P->ada_val.p;
    c.asm_src = C.d_asm_src.p; c.Ljc = C.d_Ljc.p; c.mtot = m;
    if (!C.panel_ctx.p || memcmp(&c, &C.panel_ctx_host, sizeof(c)) != 0) {
      if (!C.panel_ctx.p) C.panel_ctx.alloc(1);
      C.panel_ctx_host = c;
      SDM_HIP_CHECK(hipMemcpyAsync(C.panel_ctx.p, &C.panel_ctx_host, sizeof(c), hipMemcpyHostToDevice, st));
    }
  }
  SDM_HIP_CHECK(hipGetLastError());
  C.begun = true;
}
// The one place that writes each factor kernel's argument list, for chol_levels (which has P, C, tab, own and, per level, l, list, nfr).
// Macros, because the launch macros name the kernel themselves; `how`: SDM_KLAUNCH, or -- the emulator's launch whose workgroups wait
// for each other, one process per workgroup -- SDM_KLAUNCH_CONCURRENT.  The callers say only the grid's width, phase, step and follower.
#define SDM_LAUNCH_FRONT(how, nwg, phase, step, fa)                                                                                      \
  how(P, k_ldl_front, dim3((nwg), nfr), dim3(LDL_THREADS), FRONT_LDS, C.fronts.p, C.frontsT.p, tab, list, C.d.p, C.lb.p, C.ub.p, C.pivstat.p, \
      C.pivval.p, C.panel_ctx.p, C.front_cnt.p, C.diag_cnt.p, (phase), (step), C.lev_maxT[l], C.tmo.dev(), (fa))
#define SDM_LAUNCH_PANEL(how, L, phase)                                                                                                  \
  how(P, k_ldl_panel, dim3(1 + (L).ride_wgs, (L).nactive), dim3(LDL_THREADS), PANEL_LDS_RIDE, C.fronts.p, C.frontsT.p, tab, list, (L).panel, \
      C.d.p, C.panel_ctx.p, C.upd_cnt.p, C.diag_cnt.p, 1, (phase), C.tmo.dev(), own)
// levels l0 .. l1-1: children's update matrices into the fronts of the level (extend-add), then -- unless extend_only -- its LDL'
void chol_levels(sdm_plan *P, int l0, int l1, bool extend_only, int own, int pan0, int pan1) {
  // pan0 .. pan1-1: of every level's panel launches only these (sdm_plan_blkchol_panels: ranks that factor one front block-cyclically
  // exchange the finished panel between two launches, own says which tile columns are theirs); the extend-add of a level runs with its first launch
  CholPlan &C = P->chol;
  hipStream_t st = P->stream; (void)st;                              // (used by the emulator's launches of the follower only)
  FrontTab tab = front_tab(C);
  const bool follow = C.follow;
  for (int l = std::max(l0, 0); l < std::min(l1, C.nlevels); l++) {
    const int *list = C.d_levlist.p + C.levptr[l];
    const int nfr = C.levptr[l + 1] - C.levptr[l];
    if (nfr == 0) continue;
    if (l > 0 && pan0 <= 0) SDM_KLAUNCH(P, k_extend_add, dim3(C.lev_T[l], nfr), dim3(256), 0, C.fronts.p, tab, list);
    if (extend_only) continue;
    if (C.lev_persist[l] && !C.front_disabled) {                     // the whole level in one launch (k_ldl_front)
      PersistTurn turn(P);
      const int nwg = C.lev_maxT[l] + C.lev_ntw[l];                   // row + tile workgroups per front
      FollowArgs fa = {nullptr, nullptr, nullptr, nwg};
#ifdef SDM_EMU
      int maxnp = 0;
      for (int i = C.levptr[l]; i < C.levptr[l + 1]; i++) maxnp = std::max(maxnp, (C.sn_ns[C.levlist[i]] + NB - 1) / NB);
      if (emu_concurrent()) {
        emu_group_begin();
        // the kernel exactly as the GPU runs it (phase 0: everything carried in LDS, the fused row solve of the chain workgroup,
        // the data-tagged hand-over): one process per workgroup, all at once (tests/hipemu: emu_launch_concurrent)
        SDM_LAUNCH_FRONT(SDM_KLAUNCH_CONCURRENT, nwg, 0, 0, fa);
        if (follow) solve_follow(P, l, st);                          // beside it, polling its counters -- as the last workgroups of the launch do on the device
        emu_group_end();
        continue;
      }
      for (int step = 0; step < maxnp; step++)
        for (int phase = 1; phase <= 3; phase++) SDM_LAUNCH_FRONT(SDM_KLAUNCH, nwg, phase, step, fa);
      if (follow) solve_follow(P, l, st);                            // (workgroups run one after the other here: behind = after)
      if (emu_take_injected_timeout()) *(volatile int *)C.tmo.host = 1;   // (tests: as if a workgroup of this launch had given up waiting)
#else
      // the inverse of the level's fronts is built BEHIND their factorisation by the last workgroups of the same launch (k_ldl_front,
      // sdm_follow.h: they poll the progress counters; both kinds of workgroup fit the device together: solve_build)
      if (follow) { fa.S = C.S.p; fa.STr = C.ST.p; fa.sb_g = C.sb_g.p; C.growth_used = C.growth_max; }
      SDM_LAUNCH_FRONT(SDM_KLAUNCH, nwg + (follow ? C.lev_followT[l] : 0), 0, 0, fa);
#endif
      continue;
    }
    for (int li = C.lev_first_launch[l]; li < C.lev_first_launch[l + 1]; li++) {
      const LevelLaunch &L = C.launches[li];
      if (L.panel < pan0 || L.panel >= pan1) continue;
      // ONE launch per panel: diagonal block (+ tile 0 of the previous panel's update), the row solves and the rest of
      // the previous update (see k_ldl_panel).  The emulator runs it in two phases (workgroups are sequential there).
#ifdef SDM_EMU
      if (emu_concurrent() && (1 + L.ride_wgs) * L.nactive <= 200)   // as on the device: one launch, the roles wait for each other (one process per workgroup)
        SDM_LAUNCH_PANEL(SDM_KLAUNCH_CONCURRENT, L, 0);
      else
        for (int phase = 1; phase <= 2; phase++) SDM_LAUNCH_PANEL(SDM_KLAUNCH, L, phase);
#else
      SDM_LAUNCH_PANEL(SDM_KLAUNCH, L, 0);
#endif
      if (L.lasttiles > 0)                                           // supernodes that end with this panel and have rows beyond
        SDM_KLAUNCH(P, k_ldl_update, dim3(L.lasttiles, L.nactive), dim3(256), 0, C.fronts.p, tab, list, L.panel, C.d.p, 1);
    }
  }
  SDM_HIP_CHECK(hipGetLastError());
}
#undef SDM_LAUNCH_FRONT
#undef SDM_LAUNCH_PANEL
void chol_panel_record(sdm_plan *P, int panel, int unpack) {
  CholPlan &C = P->chol;
  if (C.nsuper != 1) throw std::runtime_error("panel records: block-cyclic factorisation is for ONE dense front");
  if (C.panelrec.n < (size_t)(4 * NB + 2 + NB * NB)) C.panelrec.alloc((size_t)(4 * NB + 2 + NB * NB));
  const int ns = C.sn_ns[0], k0 = panel * NB, kb = std::min(NB, ns - k0);
  if (panel < 0 || k0 >= ns) throw std::runtime_error("panel record: no such panel");
  SDM_KLAUNCH(P, k_panel_record, dim3(8), dim3(256), 0, C.panelrec.p, C.d.p, C.lb.p, C.pivval.p, C.pivstat.p, C.upd_cnt.p, C.diag_cnt.p, C.frontsT.p, C.sn_first[0], k0, kb, 0,
              C.sn_toff[0], unpack);
}
void chol_end(sdm_plan *P) {
  if (!P->chol.follow) solve_prepare(P, /*sb_g_is_zero=*/true);      // inverses of the diagonal super-blocks for the solves (else: built behind the levels)
  SDM_HIP_CHECK(hipGetLastError());
  P->chol.begun = false;
  P->factored = true;
}
void chol_factor(sdm_plan *P, const double canceltol, const double maxu, const double abstol, int use_absd) {
  chol_begin(P, canceltol, maxu, abstol, use_absd);
  chol_levels(P, 0, P->chol.nlevels, false, /*own=*/0);
  chol_end(P);
}

// Non-zero when a workgroup gave up waiting for another one inside a launch (never expected).  Reads and clears the plan's own
// flags (pinned host memory the kernels of THIS plan write to); call after a stream synchronise.
//   TMO_FACTOR: the results of that factorisation are unusable: the plan is marked "not factored", so the solves refuse to run on it.
//   TMO_SWEEP: the output of that solve is unusable, the factor is not touched: the plan's later sweeps run unmerged.
int chol_wait_timeouts(sdm_plan *P) {
  CholPlan &C = P->chol;
  if (!C.tmo.host) return 0;
  volatile int *flag = C.tmo.host;
  const int r = (flag[0] ? TMO_FACTOR : 0) | (flag[1] ? TMO_SWEEP : 0);
  if (r & TMO_FACTOR) {
    flag[0] = 0; P->factored = false;
    // k_ldl_front needs ALL its workgroups resident and they wait for each other: another process on the same device (or a partition
    // smaller than the one the plan was built on) can keep some of them out until the bounded waits give up.  The launch-per-panel
    // path only ever waits for workgroups dispatched earlier, so this plan's later factorisations take that one.
    C.front_disabled = true; C.follow = false;
  }
  if (r & TMO_SWEEP) {
    // the same for the merged launches (sdm_solve.hip: merged_wait): the separate ones only wait for launches that came before them
    flag[1] = 0; C.merge_disabled = true;
  }
  return r;
}

void chol_extract(sdm_plan *P, double *d_Lpr_out) {
  CholPlan &C = P->chol;
  SDM_KLAUNCH(P, k_extract, dim3(grid1d(C.nnzL, 256)), dim3(256), 0, d_Lpr_out, C.fronts.p, C.d_asm_dst.p,
             (int64_t)C.nnzL);
}

void chol_load_factor(sdm_plan *P, const double *h_Lpr, const double *h_d) {
  CholPlan &C = P->chol;
  if (h_d) {                                                         // an externally computed factor with its d: no pivot report
    const int m = (int)C.m;
    SDM_HIP_CHECK(hipMemcpyAsync(C.d.p, h_d, (size_t)m * sizeof(double), hipMemcpyHostToDevice, P->stream));
    SDM_HIP_CHECK(hipMemsetAsync(C.pivstat.p, 0, (size_t)m * sizeof(int), P->stream));
    SDM_HIP_CHECK(hipMemsetAsync(C.lb.p, 0, (size_t)m * sizeof(double), P->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(P->stream));                  // h_d may be pageable
  }
  DevBuf<double> tmp;
  tmp.upload(h_Lpr, (size_t)C.nnzL);
  SDM_HIP_CHECK(hipMemsetAsync(C.fronts.p, 0, (size_t)C.fsize * sizeof(double), P->stream));    // padding rows / Schur parts: defined
  SDM_HIP_CHECK(hipMemsetAsync(C.frontsT.p, 0, (size_t)C.tsize * sizeof(double), P->stream));
  SDM_KLAUNCH(P, k_load_factor, dim3(grid1d(C.nnzL, 256)), dim3(256), 0, C.fronts.p, C.frontsT.p, tmp.p, C.d_asm_dst.p,
              C.d_asm_dstT.p, (int64_t)C.nnzL);
  solve_prepare(P, false);
  SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
  P->factored = true;
}

void vec_gather(sdm_plan *P, double *dst, const double *src, bool forward) {
  const int m = (int)P->chol.m;
  SDM_KLAUNCH(P, k_gather_perm, dim3((m + 255) / 256), dim3(256), 0, dst, src, P->chol.d_perm.p, m, forward ? 1 : 0);
}
void vec_divd(sdm_plan *P, double *v) {
  const int m = (int)P->chol.m;
  SDM_KLAUNCH(P, k_divd, dim3((m + 255) / 256), dim3(256), 0, v, solve_d(P), m);
}

}  // namespace sdm

#if defined(SDM_PHASES) && !defined(SDM_EMU)
// tools-only build (python -m sedumi_amd.build --phases): read / reset the in-kernel phase clocks of this file
extern "C" int sdm_debug_trace_chol(long long *out2048) {
  return hipMemcpyFromSymbol(out2048, HIP_SYMBOL(sdm_trace_buf), 2048 * sizeof(long long)) != hipSuccess;
}
#endif
// (tests) the update work of panel launch q of a front with ns columns and ms rows that has row-solve workgroups: per item five ints
// {I, J, act, first panel, panels} (tile_sched_item; tile coordinates relative to tile column q); returns the number of items, -1 if the
// launch has no row-solve workgroups (its tiles are the eager ones of panel_role_tiles: every tile of the trailing matrix but those of column 0)
extern "C" int sdm_debug_tile_items(int ns, int ms, int q, int *out, int cap) {
  using namespace sdm;
  const int kb = std::min(NB, ns - q * NB), nrows = ms - (q * NB + kb);
  if (nrows <= TRSM_ROWS) return -1;
  const TileSched sc = tile_sched(ns, ms, q);
  const int n = tile_sched_items(sc);
  for (int u = 0; u < n && u < cap; u++) tile_sched_item(sc, q, u, out[5 * u], out[5 * u + 1], out[5 * u + 2], out[5 * u + 3], out[5 * u + 4]);
  return n;
}
#if defined(SDM_PHASES) && !defined(SDM_EMU)
extern "C" int sdm_debug_phases_chol(unsigned long long *out32, int reset) {
  if (out32 && hipMemcpyFromSymbol(out32, HIP_SYMBOL(sdm_phase_acc), 32 * sizeof(unsigned long long)) != hipSuccess) return 1;
  if (reset) { unsigned long long z[32] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(sdm_phase_acc), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif
