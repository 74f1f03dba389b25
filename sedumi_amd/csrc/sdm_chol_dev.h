// sdm_chol_dev.h -- the device functions that the two factor kernels of sdm_chol.hip (k_ldl_panel: one launch per panel; k_ldl_front:
// one launch per level) share: the pivot rule's column probe, the trailing-update tile, the row solves, the waits on progress
// counters, the LDL' of a diagonal block and the data-tagged hand-over of a finished block.  Included by sdm_chol.hip only.
#pragma once
#include "sdm_follow.h"

namespace sdm {

// ---- rare path of the pivot rule: value that the reference's maxabs() reads
// for column k of the current panel, i.e. x[idamax+1-based] (blkchol2.c:66-70,
// 121-131).  Column storage order = front rows below the diagonal.  All
// threads of the workgroup call this (uniform).  S = diagonal block in LDS
// (unscaled, updated by the columns < k), Lc[j*NB+i] = l_ij of the finished
// columns, ds = their pivots, rows below the block are
// obtained by forward substitution against those columns.  cb = scratch of >= ms+1
// doubles.
__device__ __noinline__ double pivot_probe(const double (*S)[NB + 1], const double *Lc, int k, int kb, int k0, int ns,
                                           int ms, int ld, SDM_GP(const double) Fs_, const double *ds, SDM_GP(double) cb_,
                                           double next_raw_diag, double *red_v, int *red_i) {
  SDM_FP_STRICT;   // no FMA contraction: the pivot decisions must see the reference's mul-then-subtract rounding
  const double *Fs = (const double *)Fs_;
  double *cb = (double *)cb_;
  const int tid = threadIdx.x, bs = LDL_THREADS;              // (blockDim.x inside a called function is two dependent loads from the dispatch packet)
  const int len = ms - (k0 + k) - 1;          // entries below the diagonal of this column
  const int nin = kb - k - 1;                 // of which inside the LDS block
  // gather the column into cb[0..len-1]; cb[len] = what lies after the column in L's storage
  for (int i = tid; i < nin; i += bs) cb[i] = S[k + 1 + i][k];
  for (int r = k0 + kb + tid; r < ms; r += bs) {
    double x[NB];
    double diagacc = 0.0;
    for (int c = 0; c <= k; c++) {
      double v = Fs[(int64_t)(k0 + c) * ld + r];
      for (int j = 0; j < c; j++) v -= x[j] * Lc[j * NB + c];   // l_cj, scaled
      double dc = (c < k) ? ds[c] : 1.0;
      x[c] = (dc > 0.0) ? v : 0.0;
      if (c < k && dc > 0.0) diagacc += x[c] * (x[c] / dc);
    }
    cb[nin + (r - (k0 + kb))] = x[k];
    if (r == k0 + kb && nin == 0 && k0 + k + 1 < ns)   // next column = first row below the block
      cb[len] = Fs[(int64_t)r * ld + r] - diagacc;
  }
  if (tid == 0) {
    if (k0 + k + 1 >= ns) cb[len] = next_raw_diag;      // next column lives in the next supernode: untouched so far
    else if (nin > 0) cb[len] = S[k + 1][k + 1];
  }
  __syncthreads();
  // first index of maximum |.| (Fortran IDAMAX semantics)
  double bv = -1.0; int bi = 0x7fffffff;
  for (int i = tid; i < len; i += bs) { double a = fabs(cb[i]); if (a > bv) { bv = a; bi = i; } }
  red_v[tid] = bv; red_i[tid] = bi;
  __syncthreads();
  for (int s = bs / 2; s > 0; s >>= 1) {
    if (tid < s) {
      double ov = red_v[tid + s]; int oi = red_i[tid + s];
      if (ov > red_v[tid] || (ov == red_v[tid] && oi < red_i[tid])) { red_v[tid] = ov; red_i[tid] = oi; }
    }
    __syncthreads();
  }
  const int imax = red_i[0];
  const double val = fabs(cb[imax + 1]);      // 1-based index used as 0-based: the element AFTER the max
  __syncthreads();
  return val;
}

// ---- K3: trailing update C -= L21 * D * L21' on the FP64 matrix cores, one 64x64 lower tile per workgroup.
// NW wavefronts share the tile: 4 (32x32 quadrants of 2x2 v_mfma_f64_16x16x4_f64 tiles) in the stand-alone kernel,
// 8 (32x16 blocks) when the update rides along with the next diagonal-block launch.  The product is formed
// transposed (D^T = B * A^T) so that the 16 consecutive lanes of a result register map to 16 consecutive rows of
// the column-major front: coalesced read-modify-write.  As[k][i] = L21[I-tile row i][k], Bs[k][j] = L21[J-tile
// row j][k] * d_k, dsh = NB doubles (all LDS).
// DIAG (tile (0,0) in the workgroup that factors the next diagonal block right away): the result also goes to LDS
// as that kernel's S / Lc arrays (which overlay As / Bs), kbn = columns of the next panel.
template <int NW, bool DIAG, bool WT = false, bool TW = false>
__device__ __forceinline__ void update_tile(double *Fs, int ld, int ms, int first, int k0, int kb, int I, int J, const double *d,
                                            double (*As)[UTP], double (*Bs)[UTP], double *dsh,
                                            double (*S)[NB + 1] = nullptr, double *Lc = nullptr, int kbn = 0,
                                            int tid = threadIdx.x, bool active = true, double *tw = nullptr) {
  // TW: the result also goes to LDS as the row solve's wave tiles (tw[(row/16)*NB*17 + col*17 + row%16], columns
  // beyond kbn zeroed) -- the workgroup that solves these rows next needs no second trip to HBM
  // tid: position inside the group of NW wavefronts that shares the tile (two groups of one workgroup may run two
  // tiles side by side: same barriers); active = false: go through the motions (barriers) without storing
  constexpr int BJ = 8 / NW;                                  // 16-column MFMA tiles per wavefront along J
  const int r0 = k0 + kb;
  SDM_PHASE_BEGIN();
  if (tid < NB) dsh[tid] = tid < kb ? d[first + k0 + tid] : 0.0;
  const int w = tid >> 6, l = tid & 63;
  const int wi = NW == 4 ? w >> 1 : w >> 2, wj = NW == 4 ? w & 1 : w & 3;
  const int cj = wj * 16 * BJ;                                // first tile column of this wavefront
  const int lk = l >> 4, ll = l & 15;
  // read-modify-write of the tile: its loads go out together with the operands' (one memory round trip for both)
  double cv[2][BJ][4];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < BJ; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int jj = lk + 4 * r;                 // result row  -> J dimension (front column)
        const int gi = r0 + I * TILE + wi * 32 + a * 16 + ll;
        const int gj = r0 + J * TILE + cj + b * 16 + jj;
        cv[a][b][r] = Fs[(int64_t)min(gj, ms - 1) * ld + min(gi, ms - 1)];
      }
  {
    // all loads of a work-item are issued before the first use (addresses clamped, masked afterwards): one
    // memory round trip per tile instead of one per element
    const int i = tid & 63, kq = tid >> 6;
    const int ri = r0 + I * TILE + i, rj = r0 + J * TILE + i;
    const double *pa = Fs + min(ri, ms - 1), *pb = Fs + min(rj, ms - 1);
    double av[NB / NW], bv[NB / NW];
#pragma unroll
    for (int q = 0; q < NB / NW; q++) {
      const int64_t off = (int64_t)(k0 + min(kq + NW * q, kb - 1)) * ld;
      av[q] = pa[off]; bv[q] = pb[off];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NB / NW; q++) {
      const int k = kq + NW * q;
      As[k][i] = (k < kb && ri < ms) ? av[q] : 0.0;
      Bs[k][i] = (k < kb && rj < ms) ? bv[q] * dsh[k] : 0.0;
    }
  }
  __syncthreads();
  SDM_PHASE(DIAG ? 14 : 28);
  sdm_double4 acc[2][BJ];
  for (int a = 0; a < 2; a++) for (int b = 0; b < BJ; b++) for (int r = 0; r < 4; r++) acc[a][b][r] = 0.0;
  // operands of step kk+4 are fetched from LDS while the MFMAs of step kk issue (As/Bs rows beyond kb are zero)
  double bv[BJ], av[2];
#pragma unroll
  for (int b = 0; b < BJ; b++) bv[b] = Bs[lk][cj + b * 16 + ll];
#pragma unroll
  for (int a = 0; a < 2; a++) av[a] = As[lk][wi * 32 + a * 16 + ll];
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    double bn[BJ], an[2];
    const int kn = min(kk + 4, NB - 4);
#pragma unroll
    for (int b = 0; b < BJ; b++) bn[b] = Bs[kn + lk][cj + b * 16 + ll];
#pragma unroll
    for (int a = 0; a < 2; a++) an[a] = As[kn + lk][wi * 32 + a * 16 + ll];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < BJ; b++) acc[a][b] = SDM_MFMA_F64_16x16x4(bv[b], av[a], acc[a][b]);
#pragma unroll
    for (int b = 0; b < BJ; b++) bv[b] = bn[b];
#pragma unroll
    for (int a = 0; a < 2; a++) av[a] = an[a];
  }
  SDM_PHASE(DIAG ? 15 : 29);
  if (TW) __syncthreads();                         // As / Bs are dead: the wave tiles overlay them
  if (DIAG) {
    __syncthreads();                               // As / Bs are dead: S and Lc overlay them
    const int tx = tid & 63, ty = tid >> 6;
    for (int j = ty; j < NB; j += NW) { S[tx][j] = (tx == j && tx >= kbn) ? 1.0 : 0.0; Lc[j * NB + tx] = 0.0; }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < BJ; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int jj = lk + 4 * r;
        const int ti = wi * 32 + a * 16 + ll, tj = cj + b * 16 + jj;
        const int gi = r0 + I * TILE + ti, gj = r0 + J * TILE + tj;
        if (active && gi < ms && gj < ms && gi >= gj) {
          const double v = cv[a][b][r] - acc[a][b][r];
          if (WT) sdm_store_wt(&Fs[(int64_t)gj * ld + gi], v); else Fs[(int64_t)gj * ld + gi] = v;
          if (DIAG && ti < kbn) S[ti][tj] = v;
          if (TW) tw[(ti >> 4) * (NB * 17) + tj * 17 + (ti & 15)] = tj < kbn ? v : 0.0;
        }
      }
  SDM_PHASE(DIAG ? 31 : 30);
}
// lower tile t -> (I, J), I >= J
__device__ __forceinline__ void tile_index(int t, int &I, int &J) {
  I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) I++;
  while (I * (I + 1) / 2 > t) I--;
  J = t - I * (I + 1) / 2;
}

// ---- K1 (k_ldl_panel): one workgroup per front of a level, 64-column panel p: LDL' of the kb x kb diagonal
// block; when the rows below the block fit one workgroup (<= TRSM_ROWS) they are solved here as well and the
// block is written back in place.  Otherwise the factored block goes to the transposed copy DT only and
// the row-solve workgroups of the same launch solve the rows and copy the block in place -- nobody may
// overwrite the panel while the never-fail rule's column probe of K1 can still read its raw values.
//
// Diagonal block (bit-faithful to cholonBlk, blkchol2.c:114-161: column i -= (x_ik / x_kk) * x(:,k), one multiply
// and one subtract per entry, columns in order): the 64 columns are swept SW at a time.  Wavefront 0 holds the SW
// current columns of all 64 rows in registers (lane = row) and runs the sweep -- pivots and multipliers travel by
// v_readlane, there is no LDS traffic and no barrier inside a sweep.  The sweep is a chain of dependent FP64
// divisions (~120 clocks per column measured, tools/ubench/ubench6) and it is issue bound when several wavefronts
// repeat it, so it is pipelined against the rest: while wavefront 0 first brings the NEXT SW columns up to date
// (look-ahead) and sweeps them, the other wavefronts apply the sweep before to the remaining trailing columns
// (x_rj -= l_jk * x_rk, k ascending: the same operations in the same order as the column-by-column reference).
// One barrier per sweep.
// A pivot that needs the never-fail rule's column probe (x_kk < ub) abandons this path; the block is reloaded
// and factored by the general all-work-items loop, which can call pivot_probe.
//
// Rows below the block: fronts with few rows use the faithful substitution (one row per work-item,
// x_rc = a_rc - sum_{j<c} x_rj * l_cj in ascending j, l_rc = x_rc / d_c).  Fronts with >= MFMA_MIN_ROWS rows below
// the block solve 16 rows per wavefront by blocked substitution: per 16-column block the GEMM part
// T_b = A_b - sum_{b'<b} X_b' L_bb'^T runs on the FP64 matrix cores, the 16x16 triangle is solved by substitution
// (no inverse is formed: the never-fail pivot rule allows multipliers up to maxu = 5e5); results agree with the
// plain substitution to rounding.
// 16 rows x 64 columns of the panel -> LDS wave tile Tw[col*17 + row]
template <bool WT = false>
__device__ __forceinline__ void rows_stage(const double *Fs, int ld, int ms, int k0, int kb, int R0, double *Tw, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  double tv[NB / 4];
  const double *pr = Fs + min(R0 + li, ms - 1);
#pragma unroll
  for (int c4 = 0; c4 < NB / 4; c4++) {                                                                // 16 loads in flight
    const double *a = &pr[(int64_t)(k0 + min(4 * c4 + lk, kb - 1)) * ld];
    tv[c4] = WT ? sdm_load_wt(a) : *a;
  }
#pragma unroll
  for (int c4 = 0; c4 < NB / 4; c4++) { const int c = 4 * c4 + lk; Tw[c * 17 + li] = c < kb ? tv[c4] : 0.0; }
}
// 16-column block b of the blocked substitution on the wave tile, in two halves: the product part needs the columns
// 0 .. 16b-1 of L11 only (rows 16b .. 16b+15 of them), the triangle its columns 16b .. 16b+15 and their pivots -- the
// row-solve workgroups run the first half BEFORE they wait for the publication of the block's own 16 columns
__device__ __forceinline__ void rows_block_gemm(int b, const double (*S)[NB + 1], double *Tw, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  const int cb = 16 * b;
  if (b > 0) {
    // T = A_b - sum_{b'<b} X_b' L_bb'^T on the matrix cores (D layout: lane holds rows lk+4r of column li)
    sdm_double4 acc;
    for (int r = 0; r < 4; r++) acc[r] = Tw[(cb + li) * 17 + lk + 4 * r];
    for (int bp = 0; bp < b; bp++)
      for (int q = 0; q < 4; q++) {
        const double a = Tw[(16 * bp + 4 * q + lk) * 17 + li];          // X_bp[row li][k]
        const double bv = S[cb + li][16 * bp + 4 * q + lk];             // L11[cb + j][k]
        acc = SDM_MFMA_F64_16x16x4(-a, bv, acc);
      }
    for (int r = 0; r < 4; r++) Tw[(cb + li) * 17 + lk + 4 * r] = acc[r];
    SDM_WAVE_SYNC();
  }
}
__device__ __forceinline__ void rows_block_tri(int b, const double (*S)[NB + 1], const double *ds, double *Tw, int lane) {
  const int li = lane & 15;
  const int cb = 16 * b;
  // the 16x16 triangle by substitution, lane li = row (the 4 lane groups lk compute the same row redundantly),
  // column-oriented: once x_j is final, x_c -= x_j l_cj for all c > j (independent updates, one LDS round trip
  // per column of the triangle) -- no inverse of the block is formed (multipliers may be as large as maxu)
  double x[16];
#pragma unroll
  for (int c = 0; c < 16; c++) x[c] = Tw[(cb + c) * 17 + li];
  double lcol[16], dsv[16];
#pragma unroll
  for (int c = 0; c < 16; c++) { lcol[c] = c > 0 ? S[cb + c][cb] : 0.0; dsv[c] = ds[cb + c]; }
#pragma unroll
  for (int j = 0; j < 16; j++) {
    double lnext[16];                                                   // column j+1 is fetched while column j is applied
#pragma unroll
    for (int c = 0; c < 16; c++) lnext[c] = (j + 1 < 16 && c > j + 1) ? S[cb + c][cb + j + 1] : 0.0;
    if (dsv[j] <= 0.0) x[j] = 0.0;                                      // skipped pivot: column not used (blkchol2.c:157-161)
#pragma unroll
    for (int c = 0; c < 16; c++)
      if (c > j) x[c] -= x[j] * lcol[c];
#pragma unroll
    for (int c = 0; c < 16; c++) lcol[c] = lnext[c];
  }
  SDM_WAVE_SYNC();
#pragma unroll
  for (int c = 0; c < 16; c++) Tw[(cb + c) * 17 + li] = x[c];
  SDM_WAVE_SYNC();
}
__device__ __forceinline__ void rows_block(int b, const double (*S)[NB + 1], const double *ds, double *Tw, int lane) {
  rows_block_gemm(b, S, Tw, lane);
  rows_block_tri(b, S, ds, Tw, lane);
}
// l = x / d out of the wave tile into the front
template <bool WT = false>
__device__ __forceinline__ void rows_store(double *Fs, int ld, int ms, int k0, int kb, int R0, const double *ds, const double *Tw, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  for (int c4 = 0; c4 < NB / 4; c4++) {
    const int c = 4 * c4 + lk, row = R0 + li;
    if (c < kb && row < ms) {
      const double dc = ds[c], xv = Tw[c * 17 + li];
      const double v = dc > 0.0 ? xv / dc : 0.0;
      if (WT) sdm_store_wt(&Fs[(int64_t)(k0 + c) * ld + row], v); else Fs[(int64_t)(k0 + c) * ld + row] = v;
    }
  }
}
__device__ __forceinline__ void panel_rows_mfma(double *Fs, int ld, int ms, int k0, int kb, int R0, const double (*S)[NB + 1],
                                                const double *ds, double *Tw, int lane, bool staged = false) {
  if (!staged) rows_stage(Fs, ld, ms, k0, kb, R0, Tw, lane);
  SDM_WAVE_SYNC();
  SDM_PHASE_BEGIN();
  for (int b = 0; b < NB / 16 && 16 * b < kb; b++) rows_block(b, S, ds, Tw, lane);
  SDM_PHASE(26);
  rows_store(Fs, ld, ms, k0, kb, R0, ds, Tw, lane);
}

// rows [rbeg, rend) below the diagonal block of panel k0 (at most brows = TRSM_ROWS of them per call)
// ONLY: 0 both paths compiled in, 1 the blocked (MFMA) path alone, 2 the few-rows path alone (callers that have chosen already)
template <int ONLY = 0>
__device__ __forceinline__ void panel_rows(double *Fs, int ld, int ns, int ms, int k0, int kb, int rbeg, int rend, int brows,
                                           const double (*S)[NB + 1], const double *ds, double *RB, bool staged = false) {
  SDM_FP_STRICT;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6, ny = LDL_THREADS >> 6;
  rend = min(rend, ms);
  if (ONLY != 2 && (ONLY == 1 || ms - min(NB, ns) >= MFMA_MIN_ROWS)) {   // per front, the same path for all its panels
    // 16 rows per wavefront at a time, blocked substitution with the GEMM part on the matrix cores
    for (int R0 = rbeg + 16 * ty; R0 < rend; R0 += 16 * ny)
      panel_rows_mfma(Fs, ld, rend, k0, kb, R0, S, ds, RB + ty * (NB * 17), tx, staged);
    return;
  }
  // few rows: faithful substitution, one row per work-item, 16-column chunks; x of earlier chunks parked in LDS
  double *Xs = RB;
  const int r = rbeg + tid;
  if (tid >= brows || r >= rend) return;
  for (int c0 = 0; c0 < kb; c0 += CHK) {
    double acc[CHK], x[CHK];
#pragma unroll
    for (int cc = 0; cc < CHK; cc++) acc[cc] = (c0 + cc < kb) ? Fs[(int64_t)(k0 + c0 + cc) * ld + r] : 0.0;
    for (int j = 0; j < c0; j++) {
      const double xj = Xs[j * brows + tid];
#pragma unroll
      for (int cc = 0; cc < CHK; cc++) acc[cc] -= xj * S[c0 + cc][j];
    }
#pragma unroll
    for (int cc = 0; cc < CHK; cc++) {
      double v = acc[cc];
#pragma unroll
      for (int jj = 0; jj < CHK; jj++)
        if (jj < cc) v -= x[jj] * S[c0 + cc][c0 + jj];
      const double dc = ds[c0 + cc];
      x[cc] = dc > 0.0 ? v : 0.0;
      if (c0 + cc < kb) Fs[(int64_t)(k0 + c0 + cc) * ld + r] = dc > 0.0 ? v / dc : 0.0;
      if (c0 + CHK < NB) Xs[(c0 + cc) * brows + tid] = x[cc];
    }
  }
}

// Workgroup 0 of k_ldl_panel before it reads rows below its diagonal block: the tiles of the previous panel's update
// that cover them (block column 0) are applied by other workgroups of the same launch -- by the row-solve workgroups
// when the panel has them (more than TRSM_ROWS rows below the block: one signal each), else by the tile workgroups
// (one signal per pair of tiles).  upd_cnt[s] counts those signals since the factorisation began (reset by
// k_prep_pivots); all work-items call this.  The spin gives up after a few seconds rather than hang the device.
__device__ __forceinline__ int panel_row_wgs(int ns, int ms, int q) {
  const int kbq = min(NB, ns - q * NB), nrows = ms - (q * NB + kbq);
  return nrows > TRSM_ROWS ? (ms - (q * NB + NB) + ROWS_BATCH - 1) / ROWS_BATCH : 0;
}
// tmo: the plan's own time-out flag (pinned host memory, CholPlan::tmo): a spin that gives up raises it; the host turns
// it into an error at the next read-back of that plan (chol_wait_timeouts)
// fence = false: the caller reads what it waited for with sdm_load_wt only (no acquire fence needed, 1.7 us less)
__device__ __forceinline__ void spin_until(const int *cnt, int target, int *tmo, bool fence = true) {
  if (threadIdx.x == 0) {
    for (long it = 0; sdm_signal_load(cnt) < target; it++) { if (sdm_spin_giveup(it, tmo)) break; SDM_SPIN_PAUSE(); }
  }
  __syncthreads();
  if (fence) SDM_ACQUIRE_FENCE();
}
__device__ __forceinline__ void wait_prev_update(const int *cnt, int ns, int ms, int panel, int q0, int *tmo) {
  int target = 0;                                              // launches q0 .. panel carried update tiles
  for (int q = max(q0, 1); q <= panel; q++) {
    const int nt = (ms - q * NB + TILE - 1) / TILE, nrw = panel_row_wgs(ns, ms, q);
    target += nrw > 0 ? nrw : (nt * (nt + 1) / 2) / 2;
  }
  spin_until(cnt, target, tmo);
}

// ---- LDL' of the 64-column diagonal block of panel `panel` of front s by ALL work-items of the calling workgroup (the
// header of k_ldl_panel describes the method).  S (= smem) holds the block on entry unless load_block (then it is read
// from the front), Lc = zero.  publish: other workgroups wait for the factored block -- it goes to DT / d 16 columns at
// a time as it becomes final, diag_cnt[s] counts those publications (*npub of the 4 are out on return; the caller
// signals the rest once the write-back below has been acknowledged).  On return: S = unit lower factor (scaled columns),
// ds = pivots (LDS), the block written in place and to DT, d / pivstat / pivval stored.  Returns false when the block
// went through the general path (a pivot asked for the never-fail rule's column probe).
// PERSIST (k_ldl_front): upd_cnt = the front's per-tile-row counters of finished update steps.
// (k_ldl_front) every tile row below `panel` has applied the updates of the panels before it
__device__ __forceinline__ void front_wait_updates(const int *upd_done, int panel, int T, int *tmo) {
  for (int r = panel + 1; r < T; r++) spin_until(upd_done + r, panel, tmo);
  // the probe of the block's last column also looks at the first diagonal entry of the next block (what lies behind the column in
  // L's storage): that tile's updates q <= panel - 1 are its tile workgroup's, counted in tile_cnt (behind upd_done)
  if (panel + 1 < T && panel + 1 >= 2) spin_until(upd_done + FRONT_MAXT + (panel + 1) * FRONT_MAXT + panel + 1, panel, tmo);
}
// ---- the two inner pieces of the diagonal block's LDL' (ldl_diag_block describes the method; k_ldl_front's chain
// workgroup runs the same pieces with a different cast of wavefronts).
// Wavefront 0, one sweep: sweep s (columns c0 = s*SW ..) is final and sits in xs (unscaled); the next SW columns cn .. are
// brought up to date with it (look-ahead), swept in registers (lane = row; pivots and multipliers by v_readlane), written
// back to S / Lc, and the bookkeeping of their pivots is done in the pivots' own lanes.
__device__ __forceinline__ void diag_sweep_w0(double (*S)[NB + 1], double *Lc, int s, double (&xs)[SW], double mylb, int tx, int kb, int k0, int ms,
                                              double ub, double *ds, int *stt, double *pv, int *badflag_p) {
  SDM_FP_STRICT;
  int &badflag = *badflag_p;
      const int c0 = s * SW, cn = c0 + SW;                             // sweep s is final; sweep columns cn .. cn+SW-1 now
      double x[SW], lsc[SW];
      SDM_PHASE_BEGIN();
#pragma unroll
      for (int cc = 0; cc < SW; cc++) x[cc] = S[tx][cn + cc];
      if (s >= 0) {
        // look-ahead: the columns of the next sweep receive sweep s here (x_rj -= l_jk * x_rk, k ascending)
        // (multipliers fetched in two batches of SW/2 columns, all loads of a batch in flight before the first use)
#pragma unroll
        for (int kh = 0; kh < SW; kh += SW / 2) {
          double lj[SW / 2][SW];
#pragma unroll
          for (int k = 0; k < SW / 2; k++)
#pragma unroll
            for (int cc = 0; cc < SW; cc++) lj[k][cc] = Lc[(c0 + kh + k) * NB + cn + cc];
#pragma unroll
          for (int k = 0; k < SW / 2; k++)
#pragma unroll
            for (int cc = 0; cc < SW; cc++) SDM_PIN(lj[k][cc]);
#pragma unroll
          for (int k = 0; k < SW / 2; k++)
#pragma unroll
            for (int cc = 0; cc < SW; cc++) x[cc] -= lj[k][cc] * xs[kh + k];
        }
      }
      SDM_PHASE(6);
#pragma unroll
      for (int k = 0; k < SW; k++) {
        const int gc = cn + k;
        const double xkk = sdm_bcast_lane(x[k], gc);
        const bool accept = sdm_lane_pred(x[k] > mylb, gc);           // uniform: the pivot's own lane decides (x_kk > lb_k)
        const double l = accept ? x[k] / xkk : 0.0;                    // skipped pivot: unit column
#pragma unroll
        for (int j = k + 1; j < SW; j++) x[j] -= sdm_bcast_lane(l, cn + j) * x[k];
        lsc[k] = l;
      }
      SDM_PHASE(7);
      // rows above the diagonal carry don't-care values from here on (nobody reads them: every consumer of S and Lc
      // is restricted to the lower triangle), which saves the masks
#pragma unroll
      for (int k = 0; k < SW; k++) {
        Lc[(cn + k) * NB + tx] = lsc[k];
        S[tx][cn + k] = x[k];
        xs[k] = x[k];
      }
      if (tx >= cn && tx < cn + SW && tx < kb) {                       // bookkeeping of pivot tx in lane tx (its own register copy of x_tt)
        double pval = x[0];
#pragma unroll
        for (int k = 1; k < SW; k++) pval = (tx == cn + k) ? x[k] : pval;
        const bool acc = pval > mylb;
        ds[tx] = acc ? pval : 0.0;
        if (!acc) { stt[tx] = 1; pv[tx] = pval; }
        if (acc && ms - (k0 + tx) > 1 && pval < ub) badflag = 1;       // needs the column probe: general path below
      }
      SDM_PHASE(8);
}
// One of nw helper wavefronts (widx = 0 .. nw-1), one sweep: sweep s goes into the trailing columns from c0 + 2 SW on
// (x_rj -= l_jk * x_rk, k ascending), 4 columns per wavefront at a time.
__device__ __forceinline__ void diag_trail(double (*S)[NB + 1], const double *Lc, int s, int kb, int tx, int widx, int nw) {
  SDM_FP_STRICT;
      const int c0 = s * SW;
      double xk[SW];
#pragma unroll
      for (int k = 0; k < SW; k++) xk[k] = S[tx][c0 + k];
      for (int j0 = c0 + 2 * SW + 4 * widx; j0 < kb; j0 += 4 * nw) {   // 4 columns per wavefront at a time
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = S[tx][min(j0 + u, NB - 1)];
#pragma unroll
        for (int k = 0; k < SW; k++) {
          double lj[4];
#pragma unroll
          for (int u = 0; u < 4; u++) lj[u] = Lc[(c0 + k) * NB + min(j0 + u, NB - 1)];
#pragma unroll
          for (int u = 0; u < 4; u++) v[u] -= lj[u] * xk[k];
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
          if (j0 + u < kb && tx >= j0 + u) S[tx][j0 + u] = v[u];
      }
}

// columns 16 g .. 16 g + 15 of the factored block into its transposed copy DT, one wavefront, lane = row: a row's 16 entries are
// contiguous there (128 bytes), so they go out as eight 16-byte write-through stores -- full fabric writes -- instead of one
// 8-byte write per lane and column (the publication lagged the sweeps by 4-5 us per group that way: profiles/r03k).  The pivot
// travels in the diagonal slot; what lies above the diagonal is not read by anybody (zeros).
__device__ __forceinline__ void publish_group(double *Dsp, const double *Lc, const double *ds, int g, int tx) {
  if (tx < 16 * g) return;
  double v[16];
#pragma unroll
  for (int c = 0; c < 16; c++) {
    const int j = 16 * g + c;
    v[c] = tx > j ? Lc[j * NB + tx] : (tx == j ? ds[j] : 0.0);
  }
#if defined(SDM_PUB8)
#pragma unroll
  for (int c = 0; c < 16; c++) sdm_store_wt(&Dsp[tx * NB + 16 * g + c], v[c]);
#else
#pragma unroll
  for (int p2 = 0; p2 < 8; p2++) sdm_store_wt2(&Dsp[tx * NB + 16 * g + 2 * p2], v[2 * p2], v[2 * p2 + 1]);
#endif
}
// what ldl_diag_block needs of a front's descriptor, fetched ONCE per workgroup (every read of the tables in HBM is a dependent
// load of a microsecond, and the noinline stages would each repeat them on the chain).  It lives in LDS and is handed on BY
// ADDRESS: a struct passed by value to a called function travels through the stack (scratch memory) behind a pointer -- two
// dependent memory round trips at the top of every diagonal block.  For the same reason the function's other arguments are
// kept to the 32 registers the calling convention has: what only the rare general path needs comes through PanelCtx.
struct FrontDesc { int ns, ms, ld, first; int64_t foff, toff, woff; double maxu, ub; int s, pad; };
template <bool PERSIST>
__device__ __forceinline__ bool ldl_diag_block(char *smem, double *F, double *DT, const FrontDesc &fd, int panel, double *d, double *lb,
                                               int *pivstat, double *pivval, const PanelCtx *ctx, int *upd_cnt, int *diag_cnt, int q0, int *tmo,
                                               bool load_block, bool publish, double *ds, int *npub, bool raw_in_lds = false, int pub_skip = 0,
                                               const double *lbs_pre = nullptr) {
  // ctx: what only the general path reads (probe scratch, the next supernode's raw diagonal); fd.maxu / fd.ub are read behind the first barrier
  // lbs_pre (k_ldl_front): the block's pivot thresholds, fetched into LDS when the workgroup started (one global round trip off the chain)
  // pub_skip (k_ldl_front's chain workgroup redoing a block on the general path): 16-column groups of this block already counted in diag_cnt
  // raw_in_lds (k_ldl_front): the raw block is not in the front but in LDS behind the wave tiles (front_rows_diag)
  SDM_FP_STRICT;   // no FMA contraction: the pivot decisions must see the reference's mul-then-subtract rounding
  double (*S)[NB + 1] = (double (*)[NB + 1])smem;                 // diagonal block, S[row][col]
  double *RB = (double *)smem + NB * (NB + 1);                    // Lc during the LDL', then Xs / the wave tiles of the row solve
  double *Lc = RB;                                                // Lc[k*NB+i] = l_ik
  __shared__ double lbs[NB], pv[NB];
  __shared__ int stt[NB];
  __shared__ int badflag;
  __shared__ double red_v[LDL_THREADS];
  __shared__ int red_i[LDL_THREADS];
  const int ns = fd.ns, ms = fd.ms, ld = fd.ld, first = fd.first;
  const int64_t toff_s = fd.toff;
  const int k0 = panel * NB, kb = min(NB, ns - k0);
  double *Fs = F + fd.foff;
  const int s = fd.s;
  const int tid = threadIdx.x, bs = LDL_THREADS;                    // (both kernels launch LDL_THREADS work-items; blockDim.x inside a called function is two dependent loads)
  const int tx = tid & 63, ty = tid >> 6, ny = bs >> 6;
  if (load_block) {
    double sv[NB / (LDL_THREADS / 64)];
    const double *pc = Fs + (int64_t)k0 * ld + k0 + min(tx, kb - 1);
#pragma unroll
    for (int q = 0; q < NB / (LDL_THREADS / 64); q++) sv[q] = pc[(int64_t)min(ty + ny * q, kb - 1) * ld];     // all loads in flight
#pragma unroll
    for (int q = 0; q < NB / (LDL_THREADS / 64); q++) {
      const int j = ty + ny * q;
      // (columns beyond a partial block: unit diagonal, so that the straight-line sweep stays finite there)
      if (j < NB) { S[tx][j] = (tx < kb && j <= tx) ? sv[q] : ((tx == j && tx >= kb) ? 1.0 : 0.0); Lc[j * NB + tx] = 0.0; }
    }
  }
  if (tid < NB) { lbs[tid] = lbs_pre ? lbs_pre[tid] : (tid < kb ? lb[first + k0 + tid] : 0.0); ds[tid] = 0.0; stt[tid] = 0; pv[tid] = 0.0; }
  if (tid == 0) { badflag = 0; *npub = 0; }
  SDM_PHASE_BEGIN();
  __syncthreads();
  const double ub = fd.ub;                                           // max diagonal (k_prep_pivots) / maxu^2; (k_ldl_panel: written just before this block)
  SDM_PHASE(16);
  if (PERSIST) SDM_TRACE(16 * panel + 0);                              // D: sweeps start
  // ---- LDL' of the block (see the header): wavefront 0 sweeps SW columns in registers while the other wavefronts
  // apply the previous sweep to the trailing columns.  The sweep is straight-line code: a skipped pivot gives the
  // multiplier 0, a pivot that needs the probe only raises `bad` (everything computed after it is discarded: the
  // block is redone by the general path), the bookkeeping of pivot gc lives in lane gc.
  const int nsw = (kb + SW - 1) / SW;
  if (ty == 0) {
    SDM_SETPRIO(3);
    const double mylb = lbs[tx];
    double xs[SW];                                                     // columns of the sweep just finished (unscaled)
    for (int s = -1; s < nsw - 1; s++) {
      diag_sweep_w0(S, Lc, s, xs, mylb, tx, kb, k0, ms, ub, ds, stt, pv, &badflag);
      SDM_PHASE(17);
      __syncthreads();
      SDM_PHASE(19);
    }
    SDM_SETPRIO(0);
    if (PERSIST) SDM_TRACE(16 * panel + 1);                            // D: sweeps end
  } else if (ty < ny - 1) {
    __syncthreads();                                                   // sweep 0
    for (int s = 0; s < nsw - 1; s++) {
      diag_trail(S, Lc, s, kb, tx, ty - 1, ny - 2);
      SDM_PHASE(18);
      __syncthreads();
    }
  } else {
    // ---- the last wavefront publishes the factor as it grows: after every second sweep 16 more columns of L11 (and
    // their pivots) are final; they go to DT / d write-through and, one sweep later (the stores have been acknowledged
    // by then), the count the row-solve workgroups of this launch poll goes up by one.  Nothing is published from a
    // sweep on in which a pivot asked for the probe (the block is redone by the general path; what was published
    // before is what the general path computes again).
    double *Dsp = DT + toff_s + (int64_t)panel * NB * NB;
    int issued = pub_skip, signalled = pub_skip;
    __syncthreads();                                                   // sweep 0
    for (int sw = 0; sw < nsw - 1; sw++) {
      if (publish) {
        // (k_ldl_front: the row workgroups read the data-tagged DT itself; the count is for consumers off the chain -- the follower,
        // the column probe -- and goes up behind the last sweep: no acknowledgement wait inside the sweeps, whose barrier it would hold)
        if (!PERSIST && issued > signalled) {                          // columns stored during the previous sweep
          SDM_STORES_DONE();
          if (tx == 0) sdm_signal_add(&diag_cnt[s]);
          signalled = issued;
        }
        const int g = issued;                                          // sweeps 0 .. sw are final: columns < 8 (sw+1)
        if (SW * (sw + 1) >= 16 * (g + 1) && badflag == 0) {
          publish_group(Dsp, Lc, ds, g, tx);
          if (tx < 16 && 16 * g + tx < kb) sdm_store_wt(&d[first + k0 + 16 * g + tx], ds[16 * g + tx]);
          issued = g + 1;
        }
      }
      __syncthreads();
    }
    // after the last sweep: what is left of the block, right away (the epilogue below would be 2-3 us later)
    if (publish && badflag == 0) {
      for (int g = issued; 16 * g < kb; g++) {
        publish_group(Dsp, Lc, ds, g, tx);
        if (tx < 16 && 16 * g + tx < kb) sdm_store_wt(&d[first + k0 + 16 * g + tx], ds[16 * g + tx]);
        issued = g + 1;
      }
    }
    if (issued > signalled) { SDM_STORES_DONE(); if (tx == 0) sdm_signal_add(&diag_cnt[s], issued - signalled); }
    if (tx == 0) *npub = issued;
  }
  const bool bad = badflag != 0;
  const bool ok = !bad;
  if (!ok) {
    // ---- general path: one column per step by all work-items, pivot_probe available
    if (panel > 0) {                                                 // the probe reads the rows below the block
      if (PERSIST) front_wait_updates(upd_cnt, panel, (ms + TILE - 1) / TILE, tmo);
      else wait_prev_update(upd_cnt + s, ns, ms, panel, q0, tmo);
    }
    for (int j = ty; j < NB; j += ny) {
      const double raw = raw_in_lds ? ((const double *)smem)[FRONT_CV_OFF + j * TILE + tx] : Fs[(int64_t)(k0 + min(j, kb - 1)) * ld + k0 + min(tx, kb - 1)];
      S[tx][j] = (tx < kb && j <= tx) ? raw : 0.0; Lc[j * NB + tx] = 0.0;
    }
    if (tid < NB) { ds[tid] = 0.0; stt[tid] = 0; pv[tid] = 0.0; }
    __syncthreads();
    for (int k = 0; k < kb; k++) {
      double xkk = S[k][k];
      if (xkk > lbs[k]) {
        if (ms - (k0 + k) > 1 && xkk < ub) {                         // rare: stability probe of the never-fail rule
          double nraw = 0.0;
          const double maxu = fd.maxu;
          double *cb = ctx->colbuf + fd.woff + s;                    // probe scratch: ms + 1 doubles per front
          if (k0 + k + 1 >= ns && first + ns < ctx->mtot) { int sidx = ctx->asm_src[ctx->Ljc[first + ns]]; nraw = sidx < 0 ? 0.0 : ctx->ada[sidx]; }
          const double ubk = pivot_probe(S, Lc, k, kb, k0, ns, ms, ld, (SDM_GP(const double))Fs, ds, (SDM_GP(double))cb, nraw, red_v, red_i) / maxu;
          if (xkk < ubk) {
            if (tid == 0) { stt[k] = 2; pv[k] = ubk - xkk; lbs[k] = ubk - xkk; }
            xkk = ubk;
          }
        }
        // every work-item forms the multipliers it needs itself (same division, same rounding): one barrier per column
        const double sik = S[tx][k];
        if (tid > k && tid < kb) Lc[k * NB + tid] = sik / xkk;
        if (tid == 0) ds[k] = xkk;
        for (int i = k + 1 + ty; i < kb; i += ny)
          if (tx >= i) S[tx][i] -= (S[i][k] / xkk) * sik;
      } else {
        // skipped pivot: d = 0, the column becomes the unit vector (blkchol2.c:157-161, blkchol.c:409-414)
        if (tid == 0) { stt[k] = 1; pv[k] = xkk; ds[k] = 0.0; }
      }
      __syncthreads();
    }
  }
  SDM_PHASE(20);
  for (int j = ty; j < NB; j += ny) if (tx > j) S[tx][j] = Lc[j * NB + tx];     // scaled columns for the row solve
  __syncthreads();
  SDM_PHASE(21);
  {
    double *Ds = DT + toff_s + (int64_t)panel * NB * NB;
    // the factored block goes in place from THIS workgroup in every case: it also stored the raw updated block (tile
    // (0,0) of the previous update), and two workgroups writing the same lines in one launch may sit behind different
    // L2s whose write-back order is not defined
    const bool inplace = true;
    for (int j = ty; j < kb; j += ny)
      if (tx < kb && tx >= j) {
        const double v = (tx == j) ? 1.0 : S[tx][j];                // unit diagonal stored explicitly (blkchol2.c:136)
        if (inplace) Fs[(int64_t)(k0 + j) * ld + k0 + tx] = v;
        sdm_store_wt(&Ds[tx * NB + j], tx == j ? ds[j] : v);        // transposed copy of the block for the row solves; its diagonal slots carry the pivots
      }
    if (tid < kb) {
      const int gk = first + k0 + tid;
      sdm_store_wt(&d[gk], ds[tid]);
      if (stt[tid]) { pivstat[gk] = stt[tid]; pivval[gk] = pv[tid]; }   // pivval = amount added (what blkchol2.c:127 keeps in lb[k])
    }
  }
  return ok;
}

constexpr unsigned long long DT_SENTINEL = 0x7ff8dead5ed00001ull;     // what DT holds until a diagonal block is published (diag_group_fetch): a quiet NaN no computation produces
// ---- hand-over of a factored diagonal block to the workgroups of k_ldl_front that solve rows against it: DATA-TAGGED.  The
// transposed copy DT of every block starts a factorisation filled with a sentinel (k_prep_pivots); the block's workgroup
// stores each 16-column group write-through as it becomes final -- the pivots in the diagonal slots of DT, which nobody else
// reads -- and the consumers poll the 8-byte words they need until none of them is the sentinel.  No counter, no
// acknowledgement wait, no second round trip between "it is there" and "here it is": the flag-then-load form (store,
// s_waitcnt, counter, poll, sc1 read) was 5.5 us of the 22.8 us per panel of control07's chain.  diag_cnt
// is still counted for the consumers that are not on the chain (k_ldl_panel's row solves, k_sinv_follow, the column probe).
__device__ __forceinline__ bool is_dt_sentinel(double v) { union { double d; unsigned long long u; } b; b.d = v; return b.u == DT_SENTINEL; }
__device__ __forceinline__ double dt_tagged_load(const double *a, int *tmo) {
  double v = sdm_load_wt(a);
  for (long it = 0; is_dt_sentinel(v); it++) { if (sdm_spin_giveup(it, tmo)) break; SDM_SPIN_PAUSE(); v = sdm_load_wt(a); }
  return v;
}
// columns 16 blk .. 16 blk + 15 of the block (strictly lower part, rows < kb) into S, their pivots into dsr; all work-items.
// Every load of a work-item (two entries, for 16 of them a pivot) is in flight before the first one is looked at: ONE memory
// round trip per group when the data is there, not one per word.
__device__ __forceinline__ void diag_group_fetch(const double *Ds, int blk, int kb, double (*S)[NB + 1], double *dsr, int *tmo) {
  const int tid = threadIdx.x;
  constexpr int NE = NB * 16 / LDL_THREADS;
  const double *a[NE + 1];
  double v[NE + 1];
  bool need[NE + 1];
#pragma unroll
  for (int t = 0; t < NE; t++) {
    const int e = tid + LDL_THREADS * t, i = e >> 4, j = 16 * blk + (e & 15);
    need[t] = i < kb && j < i;
    a[t] = &Ds[i * NB + j];
  }
  need[NE] = tid < 16 && 16 * blk + tid < kb;
  a[NE] = &Ds[(16 * blk + (tid & 15)) * NB + 16 * blk + (tid & 15)];
#pragma unroll
  for (int t = 0; t <= NE; t++) v[t] = need[t] ? sdm_load_wt(a[t]) : 0.0;
#pragma unroll
  for (int t = 0; t <= NE; t++)
    if (need[t])
      for (long it = 0; is_dt_sentinel(v[t]); it++) { if (sdm_spin_giveup(it, tmo)) break; SDM_SPIN_PAUSE(); v[t] = sdm_load_wt(a[t]); }
#pragma unroll
  for (int t = 0; t < NE; t++) {
    const int e = tid + LDL_THREADS * t, i = e >> 4, j = 16 * blk + (e & 15);
    S[i][j] = v[t];
  }
  if (tid < 16) dsr[16 * blk + tid] = v[NE];
  __syncthreads();
}

}  // namespace sdm
