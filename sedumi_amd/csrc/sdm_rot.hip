// sdm_rot.hip -- the re-pivoting chain of updtransfo.m:99-107 on the device:
//   [u, perm, gjc, g] = urotorder(u, K, maxu, permIN)   rotorder / prpirotorder   (urotorder.c:79-180, :197-304)
//   y = givensrot(gjc, g, x, K)                         matgivens / prpimatgivens (givensrot.c:60-84, auxgivens.c:43-99)
//   y = sqrtinv(q, vlab, K)                             qdivv / prpiqdivv         (sqrtinv.c:58-86)
// in the reference's conventions and in its compact rotation form: gjc = n entries per block (0-based, gjc[n-1] = the block's rotation
// count), g = 2 doubles {x, y} per rotation of a real block, 3 {x, xim, y} of a Hermitian one, the blocks behind each other.
//
// k_urotorder  one workgroup per PSD block, all blocks in one launch, longest first.  The algorithm is a chain of n - 1 steps and the
//   decision of a step needs row k of every column after the previous step's rotations: the parallelism is across the columns inside
//   the workgroup and across the blocks in the grid.  No hand-over between workgroups, no counters, no atomics; a block's bits depend on
//   nothing but the block.  Columns never move: perm (position -> column) and its inverse pos are kept and the physical column is
//   addressed; a work-item owns the columns tid, tid + UR_T, ... for the whole kernel.  The working copy is TRANSPOSED (entry (i, c) at
//   W[i * ld + c]: lanes that own adjacent columns read adjacent addresses for a given row), in LDS when the block fits the budget and
//   in global memory otherwise -- the same operations in the same order, the same bits.  perm, pos and d live in LDS up to order
//   UR_AUX_NMAX, in global memory beyond.  Per step: d is recomputed when d[perm[k]] <= h (every column summed by its owner in the
//   reference's order), one reduction gives ukmax and the pivot (the largest d, the LOWEST position among equal ones: urotorder.c:123-128),
//   and an unstable step generates its m = pivk - k rotations from the pivot column bottom-up in chunks of UR_GC: the running sum y by
//   one lane in the reference's order, the square roots and divisions over the lanes, the chunk through LDS to every column's owner,
//   which carries z2 in a register down its column (between two chunks through the row both touch).  The column order uperm and the
//   mirroring triu2sym / triu2herm are the epilogue.  A stable step costs the reduction and the compare.
// k_urot_pack  the blocks' rotations, written at the reference's CAPACITY offsets, moved behind each other.
// k_givensrot  Y = G X: grid over (block, strip of GR_W columns), one column per work-item, the strip transposed in LDS (budget) or in
//   global memory; the rotations are uniform over the wavefront and come from read-only global memory.
// k_sqrtinv    y(i, j) = conj(q(j, i)) / sqrt(v_i): a 64 x 64 tiled transpose through LDS.
// The arithmetic is compiled without fused contraction (below): what feeds decisions and rotations rounds as the reference's does.
#include "sdm_plan.h"
#include <algorithm>
#include <climits>
#include <cstring>

#ifndef SDM_EMU
#pragma clang fp contract(off)
#endif

namespace sdm {

constexpr int UR_T = 256, UR_WV = UR_T / 64, UR_GC = 256;   // work-items, wavefronts, rotations per chunk
constexpr int UR_RB = 8;                                     // rotations whose operands are fetched ahead of the dependent chain
constexpr int UR_AUX_NMAX = 1024;                            // perm, pos and d in LDS up to this order (16 bytes per column)
constexpr sdm_int UR_LDS_DEFAULT = 96 * 1024;                // working copy of urotorder / strip of givensrot (+ 16 KB aux + 8.3 KB static: below 160 KB)
constexpr int GR_W = 64, GR_LD = GR_W + 1;                   // columns of a givensrot strip (a wavefront), its padded leading dimension
static sdm_int g_rot_lds = UR_LDS_DEFAULT;

struct RotBlk { const int *n, *herm, *loff; const int64_t *off, *goff, *woff; };   // per block: order, Hermitian?, offset in perm / gjc, in u, in g (capacity), in the scratch

// ---------------------------------------------------------------- urotorder
template <bool HERM>
__device__ __forceinline__ void urot_block(double *W, int64_t ld, int64_t pim, int *perm, int *pos, double *d, const double *U, double *Uo,
                                           const double *pin, double *pout, double *gjc, double *g, int n, double maxusqr, double *cs, double *gb,
                                           double *red, int *redi) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t nn = (int64_t)n * n;
  double *Wi = W + pim;
  // the upper triangle in the incoming column order, transposed; the strict lower triangle (and Im diag) is not read (urotorder.c reads none of it)
  for (int64_t e = tid; e < nn; e += UR_T) {
    const int i = (int)(e % n), c = (int)(e / n);
    W[(int64_t)i * ld + c] = i <= c ? U[e] : 0.0;
    if (HERM) Wi[(int64_t)i * ld + c] = i < c ? U[nn + e] : 0.0;
  }
  for (int c = tid; c < n; c += UR_T) { perm[c] = c; pos[c] = c; d[c] = 0.0; }
  __syncthreads();
  double h = 1.0, ycar = 0.0;
  int inz = 0;
  for (int k = 0; k < n - 1; k++) {
    if (tid == 0) gjc[k] = (double)inz;
    const int pk = perm[k];
    double dk = d[pk];
    if (dk <= h) {                                                      // urotorder.c:102-108 / :221-227
      __syncthreads();                                                  // (everybody has read d[pk])
      for (int c = tid; c < n; c += UR_T) {
        const int j = pos[c];
        if (j >= k) {
          double s = 0.0;
          for (int r = k; r <= j; r++) { const double a = W[(int64_t)r * ld + c]; s += a * a; }
          if (HERM) {
            double s2 = 0.0;
            for (int r = k; r < j; r++) { const double b = Wi[(int64_t)r * ld + c]; s2 += b * b; }
            s = s + s2;
          }
          d[c] = s;
        }
      }
      __syncthreads();
      dk = d[pk];
      h = dk * 1E-10;
    }
    // ---- ukmax = max |u(k, later)|^2 and the pivot candidate: the largest d > 0 among the later columns, the lowest position among equal ones
    double um = 0.0, bd = 0.0;
    int bp = INT_MAX, bc = -1;
    for (int c = tid; c < n; c += UR_T) {
      const int j = pos[c];
      if (j > k) {
        const double a = W[(int64_t)k * ld + c];
        double v = a * a;
        if (HERM) { const double b = Wi[(int64_t)k * ld + c]; v = v + b * b; }
        um = v > um ? v : um;
        const double dc = d[c];
        if (dc > bd || (dc == bd && j < bp && dc > 0.0)) { bd = dc; bp = j; bc = c; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ou = __shfl_xor(um, o), od = __shfl_xor(bd, o);
      const int op = __shfl_xor(bp, o), oc = __shfl_xor(bc, o);
      um = ou > um ? ou : um;
      if (od > bd || (od == bd && op < bp)) { bd = od; bp = op; bc = oc; }
    }
    double *rd = red + (k & 1) * 2 * UR_WV;                             // (two sets of slots: the next step's writes pass no barrier after this step's reads)
    int *ri = redi + (k & 1) * 2 * UR_WV;
    if (lane == 0) { rd[wave] = um; rd[UR_WV + wave] = bd; ri[wave] = bp; ri[UR_WV + wave] = bc; }
    __syncthreads();
    um = rd[0]; bd = rd[UR_WV]; bp = ri[0]; bc = ri[UR_WV];
#pragma unroll
    for (int w = 1; w < UR_WV; w++) {
      const double ou = rd[w], od = rd[UR_WV + w];
      const int op = ri[w], oc = ri[UR_WV + w];
      um = ou > um ? ou : um;
      if (od > bd || (od == bd && op < bp)) { bd = od; bp = op; bc = oc; }
    }
    // (bc < 0: no later column has d > 0 -- the reference would pivot on a stale position; nothing is rotated here)
    if (um > maxusqr * dk && bc >= 0) {                                 // urotorder.c:122: pivot k is unstable
      const int pivk = bp, m = pivk - k, cp = bc;
      for (int c = tid; c < n; c += UR_T) {                             // urotorder.c:153-154: the pivot to position k, k .. pivk-1 one up
        const int j = pos[c];
        if (j >= k && j < pivk) { pos[c] = j + 1; perm[j + 1] = c; }
        else if (j == pivk) { pos[c] = k; perm[k] = c; }
      }
      for (int hi = m; hi > 0; hi -= UR_GC) {                           // rotations lo .. hi-1 (rotation r turns rows k+r, k+r+1), bottom-up
        const int lo = max(hi - UR_GC, 0), cnt = hi - lo;
        if (tid < cnt) {
          const double x = W[(int64_t)(k + lo + tid) * ld + cp];
          double v = x * x;
          gb[tid] = x;
          if (HERM) { const double xi = Wi[(int64_t)(k + lo + tid) * ld + cp]; v = v + xi * xi; gb[2 * UR_GC + tid] = xi; }
          cs[tid] = v;
        }
        if (tid == 0 && hi == m) { const double t = W[(int64_t)(k + m) * ld + cp]; cs[UR_GC + 1] = t; ycar = t * t; }   // urotorder.c:138-139
        __syncthreads();
        if (tid == 0) {                                                 // y in the reference's order (:143): cs[t] = sum of squares of rows k+lo+t .. k+m
          double y = ycar;
          cs[cnt] = y;
          for (int tb = cnt - 1; tb >= 0; tb -= UR_RB) {                 // (UR_RB squares fetched ahead of the chain of additions)
            double v[UR_RB];
#pragma unroll
            for (int j = 0; j < UR_RB; j++) v[j] = tb - j >= 0 ? cs[tb - j] : 0.0;
#pragma unroll
            for (int j = 0; j < UR_RB; j++)
              if (tb - j >= 0) { y += v[j]; cs[tb - j] = y; }
          }
          ycar = y;
        }
        __syncthreads();
        if (tid < cnt) {                                                // :144-147
          const int r = lo + tid;
          const double ny = sqrt(cs[tid]), prev = r + 1 == m ? cs[UR_GC + 1] : sqrt(cs[tid + 1]);
          const double gx = gb[tid] / ny, gy = prev / ny;
          gb[tid] = gx; gb[UR_GC + tid] = gy;
          if (!HERM) { g[2 * (int64_t)(inz + r)] = gx; g[2 * (int64_t)(inz + r) + 1] = gy; }
          else {
            const double gxi = gb[2 * UR_GC + tid] / ny;
            gb[2 * UR_GC + tid] = gxi;
            g[3 * (int64_t)(inz + r)] = gx; g[3 * (int64_t)(inz + r) + 1] = gxi; g[3 * (int64_t)(inz + r) + 2] = gy;
          }
          if (r == 0) W[(int64_t)k * ld + cp] = ny;                     // :149 the new pivotal diagonal entry
        }
        __syncthreads();
        // ---- :160-163: 1, 2, ..., m rotations on the columns now at positions k+1 .. pivk (givensrotuj: the entry at row k+i counts as 0), m on the later ones
        for (int c = tid; c < n; c += UR_T) {
          const int p = pos[c];
          if (p <= k) continue;
          const bool full = p - k > m;
          const int cc = full ? m : p - k;                              // this column takes the rotations cc-1 .. 0
          if (cc <= lo) continue;
          double *z = W + (int64_t)k * ld + c, *zi = Wi + (int64_t)k * ld + c;
          double z2 = 0.0, z2i = 0.0;
          if (full || cc > hi) { z2 = z[(int64_t)hi * ld]; if (HERM) z2i = zi[(int64_t)hi * ld]; }
          // (r uniform over the wavefront: the rotation is an LDS broadcast; the column's entries of UR_RB rotations are fetched ahead of the chain:
          //  rotation r reads row r as it was and writes row r+1, so every row is read before it is written)
          for (int rb = hi - 1; rb >= lo; rb -= UR_RB) {
            double a[UR_RB], ai[UR_RB];
#pragma unroll
            for (int j = 0; j < UR_RB; j++) {
              const int r = rb - j;
              const bool on = r >= lo && r < cc;
              a[j] = on ? z[(int64_t)r * ld] : 0.0;
              ai[j] = HERM && on ? zi[(int64_t)r * ld] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < UR_RB; j++) {
              const int r = rb - j;
              if (r >= lo && r < cc) {
                const double gx = gb[r - lo], gy = gb[UR_GC + r - lo], z1 = a[j];
                if (!HERM) {
                  if (!full && r == cc - 1) { z2 = z1; z[(int64_t)(r + 1) * ld] = z2 * gy; z2 *= gx; }   // auxgivens.c:126-128
                  else {
                    z[(int64_t)(r + 1) * ld] = gy * z1 - gx * z2;       // :57-58
                    z2 = gx * z1 + gy * z2;
                  }
                } else {
                  const double gxi = gb[2 * UR_GC + r - lo], z1i = ai[j];
                  if (!full && r == cc - 1) {                           // auxgivens.c:170-173
                    z2 = z1; z[(int64_t)(r + 1) * ld] = z2 * gy;
                    z2i = -z2 * gxi; z2 *= gx;
                  } else {
                    z[(int64_t)(r + 1) * ld] = gy * z1 - gx * z2 + gxi * z2i;   // :91-95
                    zi[(int64_t)(r + 1) * ld] = gy * z1i - gx * z2i - gxi * z2;
                    const double t2 = gx * z1 + gxi * z1i + gy * z2;
                    z2i = gx * z1i - gxi * z1 + gy * z2i;
                    z2 = t2;
                  }
                }
              }
            }
          }
          z[(int64_t)lo * ld] = z2;
          if (HERM) zi[(int64_t)lo * ld] = z2i;
        }
        if (lo > 0) __syncthreads();                                    // (the next chunk overwrites cs and gb)
      }
      for (int c = tid; c < n; c += UR_T)                               // :169-172
        if (pos[c] > k) {
          const double a = W[(int64_t)k * ld + c];
          if (!HERM) d[c] -= a * a;
          else { const double b = Wi[(int64_t)k * ld + c]; d[c] -= a * a + b * b; }
        }
      inz += m;
      __syncthreads();
    }
  }
  if (tid == 0) gjc[n - 1] = (double)inz;
  __syncthreads();
  // ---- uperm, triu2sym / triu2herm (:400-401, :434-436) and perm_out (:405-412)
  for (int64_t e = tid; e < nn; e += UR_T) {
    const int i = (int)(e % n), j = (int)(e / n);
    if (i <= j) {
      Uo[e] = W[(int64_t)i * ld + perm[j]];
      if (HERM) Uo[nn + e] = i == j ? 0.0 : Wi[(int64_t)i * ld + perm[j]];
    } else {
      Uo[e] = W[(int64_t)j * ld + perm[i]];
      if (HERM) Uo[nn + e] = -Wi[(int64_t)j * ld + perm[i]];
    }
  }
  for (int j = tid; j < n; j += UR_T) pout[j] = pin ? pin[perm[j]] : 1.0 + (double)perm[j];
}

// items: (block, working copy in LDS?, perm / pos / d in LDS?, -) per workgroup
__global__ void __launch_bounds__(UR_T)
k_urotorder(const double *u, double *uout, const double *pin, double *pout, double *gjc, double *g, double *scratch, RotBlk B, const int *items,
            double maxusqr) {
  SDM_DYN_SMEM(smem);
  __shared__ double cs[UR_GC + 2], gb[3 * UR_GC], red[4 * UR_WV];
  __shared__ int redi[4 * UR_WV];
  const int b = items[4 * blockIdx.x], w_lds = items[4 * blockIdx.x + 1], a_lds = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t ld = n | 1, wsz = (int64_t)(herm ? 2 : 1) * n * ld;
  // the scratch of a block: [d (n) | perm, pos (n int32 each) | the working copy, when it is not in LDS]; LDS: [working copy | d | perm | pos]
  double *sg = scratch + B.woff[b], *sl = (double *)smem;
  double *Wg = sg + 2 * (int64_t)n, *dl = sl + (w_lds ? wsz : 0);
  int *pl = (int *)(dl + n), *pg = (int *)(sg + n);
  const double *U = u + B.off[b], *pi = pin ? pin + B.loff[b] : nullptr;
  double *Uo = uout + B.off[b], *po = pout + B.loff[b], *gj = gjc + B.loff[b], *gg = g + B.goff[b];
  const int64_t pim = (int64_t)n * ld;
#define UROT_GO(H, WP, DP, PP) urot_block<H>(WP, ld, pim, PP, PP + n, DP, U, Uo, pi, po, gj, gg, n, maxusqr, cs, gb, red, redi)
  if (herm) {
    if (w_lds) UROT_GO(true, sl, dl, pl);
    else if (a_lds) UROT_GO(true, Wg, dl, pl);
    else UROT_GO(true, Wg, sg, pg);
  } else {
    if (w_lds) UROT_GO(false, sl, dl, pl);
    else if (a_lds) UROT_GO(false, Wg, dl, pl);
    else UROT_GO(false, Wg, sg, pg);
  }
#undef UROT_GO
}

// the rotations of block b from their capacity offset to behind those of the blocks before it
__global__ void __launch_bounds__(UR_T)
k_urot_pack(const double *gjc, const double *g, double *gout, RotBlk B, int nb) {
  __shared__ int64_t dst;
  const int b = blockIdx.x, n = B.n[b];
  if (n == 0) return;
  if (threadIdx.x == 0) {
    int64_t o = 0;
    for (int a = 0; a < b; a++)
      if (B.n[a] > 0) o += (B.herm[a] ? 3 : 2) * (int64_t)gjc[B.loff[a] + B.n[a] - 1];
    dst = o;
  }
  __syncthreads();
  const int64_t len = (B.herm[b] ? 3 : 2) * (int64_t)gjc[B.loff[b] + n - 1];
  const double *src = g + B.goff[b];
  double *out = gout + dst;
  for (int64_t e = threadIdx.x; e < len; e += UR_T) out[e] = src[e];
}

// ---------------------------------------------------------------- givensrot
// S: the strip transposed, entry (r, t) of column j0 + t at S[r * GR_LD + t], the imaginary plane pim doubles further
template <bool HERM>
__device__ __forceinline__ void givens_strip(double *S, int64_t pim, double *Y, const int *__restrict__ gjc, const double *__restrict__ g, int n, int j0) {
  const int t = threadIdx.x, w = min(GR_W, n - j0);
  const int64_t nn = (int64_t)n * n;
  double *Si = S + pim;
  for (int c = 0; c < w; c++)
    for (int r = t; r < n; r += GR_W) {
      S[(int64_t)r * GR_LD + c] = Y[(int64_t)(j0 + c) * n + r];
      if (HERM) Si[(int64_t)r * GR_LD + c] = Y[nn + (int64_t)(j0 + c) * n + r];
    }
  __syncthreads();
  if (t < w) {
    double *z = S + t, *zi = Si + t;
    for (int k = 0; k < n - 1; k++) {                                   // givensrot.c:68-69: step k turns rows k .. k+m
      const int g0 = gjc[k], m = gjc[k + 1] - g0;
      if (m == 0) continue;
      double z2 = z[(int64_t)(k + m) * GR_LD], z2i = HERM ? zi[(int64_t)(k + m) * GR_LD] : 0.0;
      for (int ib = m; ib > 0; ib -= UR_RB) {                           // rotations ib-1 .. ib-UR_RB: their rows and values fetched ahead of the chain
        double a[UR_RB], ai[UR_RB], gx[UR_RB], gy[UR_RB], gxi[UR_RB];
#pragma unroll
        for (int j = 0; j < UR_RB; j++) {
          const int i = ib - j;
          const bool on = i > 0;
          const int64_t r = (int64_t)(k + i - 1) * GR_LD, q = g0 + i - 1;
          a[j] = on ? z[r] : 0.0;
          ai[j] = HERM && on ? zi[r] : 0.0;
          gx[j] = on ? g[(HERM ? 3 : 2) * q] : 0.0;
          gxi[j] = HERM && on ? g[3 * q + 1] : 0.0;
          gy[j] = on ? g[(HERM ? 3 : 2) * q + (HERM ? 2 : 1)] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < UR_RB; j++) {
          const int i = ib - j;
          if (i > 0) {
            const int64_t r = (int64_t)(k + i - 1) * GR_LD;
            const double z1 = a[j];
            if (!HERM) {
              z[r + GR_LD] = gy[j] * z1 - gx[j] * z2;                   // auxgivens.c:57-58
              z2 = gx[j] * z1 + gy[j] * z2;
            } else {
              const double z1i = ai[j];
              z[r + GR_LD] = gy[j] * z1 - gx[j] * z2 + gxi[j] * z2i;    // :91-95
              zi[r + GR_LD] = gy[j] * z1i - gx[j] * z2i - gxi[j] * z2;
              const double t2 = gx[j] * z1 + gxi[j] * z1i + gy[j] * z2;
              z2i = gx[j] * z1i - gxi[j] * z1 + gy[j] * z2i;
              z2 = t2;
            }
          }
        }
      }
      z[(int64_t)k * GR_LD] = z2;
      if (HERM) zi[(int64_t)k * GR_LD] = z2i;
    }
  }
  __syncthreads();
  for (int c = 0; c < w; c++)
    for (int r = t; r < n; r += GR_W) {
      Y[(int64_t)(j0 + c) * n + r] = S[(int64_t)r * GR_LD + c];
      if (HERM) Y[nn + (int64_t)(j0 + c) * n + r] = Si[(int64_t)r * GR_LD + c];
    }
}

// items: (block, first column of the strip, strip in LDS?, number of the strip among those in global memory) per workgroup; gjc: int32, sum n entries;
// B.goff: the block's offset in the compact g; scratch: 2 n GR_LD doubles at most per strip in global memory
__global__ void __launch_bounds__(GR_W)
k_givensrot(double *y, const int *gjc, const double *g, double *scratch, RotBlk B, const int *items, int64_t slot) {
  SDM_DYN_SMEM(smem);
  const int b = items[4 * blockIdx.x], j0 = items[4 * blockIdx.x + 1], lds = items[4 * blockIdx.x + 2];
  const int n = B.n[b];
  double *S = scratch + (int64_t)items[4 * blockIdx.x + 3] * slot;      // (the strip in global memory: a global pointer on that path, not a choice of two)
  const int64_t pim = (int64_t)n * GR_LD;
  if (B.herm[b]) {
    if (lds) givens_strip<true>((double *)smem, pim, y + B.off[b], gjc + B.loff[b], g + B.goff[b], n, j0);
    else givens_strip<true>(S, pim, y + B.off[b], gjc + B.loff[b], g + B.goff[b], n, j0);
  } else {
    if (lds) givens_strip<false>((double *)smem, pim, y + B.off[b], gjc + B.loff[b], g + B.goff[b], n, j0);
    else givens_strip<false>(S, pim, y + B.off[b], gjc + B.loff[b], g + B.goff[b], n, j0);
  }
}

// ---------------------------------------------------------------- sqrtinv
// item (b, I, J) = the 64 x 64 tile of y with rows 64 I .., columns 64 J ..:  y(i, j) = conj(q(j, i)) / sqrt(v_i)   (sqrtinv.c:63-67, :77-84)
__global__ void __launch_bounds__(256)
k_sqrtinv(const double *q, const double *v, double *y, RotBlk B, const int *items) {
  __shared__ double Ts[64][65], sv[64];
  const int b = items[4 * blockIdx.x], i0 = 64 * items[4 * blockIdx.x + 1], j0 = 64 * items[4 * blockIdx.x + 2];
  const int n = B.n[b], nplanes = B.herm[b] ? 2 : 1, tid = threadIdx.x, f = tid & 63;
  const int64_t nn = (int64_t)n * n;
  if (tid < 64 && i0 + tid < n) sv[tid] = sqrt(v[B.loff[b] + i0 + tid]);
  for (int pl = 0; pl < nplanes; pl++) {
    const double *Q = q + B.off[b] + pl * nn;
    double *Y = y + B.off[b] + pl * nn;
    __syncthreads();
    for (int s = tid >> 6; s < 64; s += 4)                              // column i0 + s of q, rows j0 + f
      if (i0 + s < n && j0 + f < n) Ts[s][f] = Q[(int64_t)(i0 + s) * n + j0 + f];
    __syncthreads();
    for (int s = tid >> 6; s < 64; s += 4)                              // column j0 + s of y, rows i0 + f
      if (j0 + s < n && i0 + f < n) Y[(int64_t)(j0 + s) * n + i0 + f] = pl ? -Ts[f][s] / sv[f] : Ts[f][s] / sv[f];
  }
}

// =========================================================================== host
void rot_set_lds_budget(sdm_int bytes) {
  if (bytes < 0 || bytes > UR_LDS_DEFAULT) throw std::runtime_error("rotation LDS budget: 0 (default) .. 98304 bytes");
  g_rot_lds = bytes ? bytes : UR_LDS_DEFAULT;
}

static void rot_offsets(RotPlan &S, const std::vector<int> &ns, int rsdpN, std::vector<int64_t> &goff) {
  goff.assign(std::max<size_t>(ns.size(), 1), 0);
  S.gcap = 0;
  for (size_t b = 0; b < ns.size(); b++) {
    if (ns[b] < 0) throw std::runtime_error("K.s: negative order");
    goff[b] = S.gcap;
    S.gcap += ((int)b < rsdpN ? 2 : 3) * ((int64_t)ns[b] * (ns[b] - 1) / 2);
  }
}
static void rot_image(RotPlan &S, const std::vector<int64_t> &goff, const std::vector<int64_t> &woff, std::vector<int> &items) {
  S.nitems = (int)items.size() / 4;
  if (items.empty()) items.assign(4, 0);
  if (items.size() & 1) items.push_back(0);
  S.img.assign(goff.begin(), goff.end());
  S.img.insert(S.img.end(), woff.begin(), woff.end());
  S.w_items = S.img.size();
  S.img.resize(S.w_items + items.size() / 2);
  memcpy(S.img.data() + S.w_items, items.data(), items.size() * sizeof(int));
}
static RotBlk rot_blk(const ConeTabs &T, const RotPlan &S, const int64_t *tab) {
  RotBlk B; B.n = T.n; B.herm = T.herm; B.loff = T.loff; B.off = T.off; B.goff = tab; B.woff = tab + S.w_items / 2;
  return B;
}
template <class Kern>
static void rot_allow_lds(Kern kern, size_t lds) {
#ifndef SDM_EMU
  if (lds > 48 * 1024) SDM_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
#endif
}

void urot_plan(RotPlan &S, const std::vector<int> &ns, int rsdpN) {
  const int nb = (int)ns.size();
  std::vector<int64_t> goff, woff(std::max(nb, 1), 0);
  rot_offsets(S, ns, rsdpN, goff);
  std::vector<int> order, items;
  S.ws = 0; S.lds = 0;
  for (int b = 0; b < nb; b++) if (ns[b] > 0) order.push_back(b);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ns[a] > ns[b]; });   // longest first
  for (int b : order) {
    const int64_t n = ns[b], wsz = (b < rsdpN ? 1 : 2) * n * (n | 1);
    const int w_lds = wsz * (int64_t)sizeof(double) <= g_rot_lds ? 1 : 0, a_lds = n <= UR_AUX_NMAX ? 1 : 0;
    woff[b] = S.ws;
    S.ws += 2 * n + (w_lds ? 0 : wsz);
    S.lds = std::max(S.lds, (size_t)((w_lds ? wsz : 0) + (a_lds ? 2 * n : 0)) * sizeof(double));
    items.insert(items.end(), {b, w_lds, a_lds, 0});
  }
  rot_image(S, goff, woff, items);
}

// u, uout: lenud doubles; pin: sum n doubles or null; pout, gjc: sum n doubles; gslot, gout: S.gcap doubles each; area: S.words() doubles (all device)
void urot_run(sdm_plan *P, const ConeTabs &T, const RotPlan &S, double *area, const double *u, double *uout, const double *pin, double *pout, double *gjc,
              double *gslot, double *gout, double maxu) {
  if (S.nitems == 0) return;
  int64_t *tab = (int64_t *)(area + S.ws);
  SDM_HIP_CHECK(hipMemcpy(tab, S.img.data(), S.img.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  const int *items = (const int *)(tab + S.w_items);
  const RotBlk B = rot_blk(T, S, tab);
  rot_allow_lds(k_urotorder, S.lds);
  SDM_KLAUNCH(P, k_urotorder, dim3(S.nitems), dim3(UR_T), S.lds, u, uout, pin, pout, gjc, gslot, area, B, items, maxu * maxu);
  const int nb = (int)(S.w_items / 2);
  SDM_KLAUNCH(P, k_urot_pack, dim3(nb), dim3(UR_T), 0, (const double *)gjc, (const double *)gslot, gout, B, nb);
  SDM_HIP_CHECK(hipGetLastError());
}

// goff_compact: the offset of every block in the compact g (the caller has read them off gjc)
void givens_plan(RotPlan &S, const std::vector<int> &ns, int rsdpN, const std::vector<int64_t> &goff_compact) {
  const int nb = (int)ns.size();
  std::vector<int64_t> goff(std::max(nb, 1), 0), woff(std::max(nb, 1), 0);
  std::copy(goff_compact.begin(), goff_compact.end(), goff.begin());
  struct Strip { int b, j0, lds; int64_t cost; };
  std::vector<Strip> st;
  S.ws = 0; S.lds = 0; S.gcap = 0; S.slot = 0;
  for (int b = 0; b < nb; b++) {
    const int64_t n = ns[b], bytes = (b < rsdpN ? 1 : 2) * n * GR_LD * (int64_t)sizeof(double);
    const int lds = bytes <= g_rot_lds ? 1 : 0;
    for (int j0 = 0; j0 < n; j0 += GR_W) {
      st.push_back({b, j0, lds, n});
      if (lds) S.lds = std::max(S.lds, (size_t)bytes);
      else S.slot = std::max(S.slot, bytes / (int64_t)sizeof(double));
    }
  }
  std::stable_sort(st.begin(), st.end(), [](const Strip &a, const Strip &b) { return a.cost > b.cost; });   // longest first
  std::vector<int> items;
  int nglob = 0;
  for (const Strip &s : st) items.insert(items.end(), {s.b, s.j0, s.lds, s.lds ? 0 : nglob++});
  S.ws = (int64_t)nglob * S.slot;
  rot_image(S, goff, woff, items);
}

// y: lenud doubles holding x; gjc: sum n int32; g: the compact rotations; area: S.words() doubles (all device)
void givens_run(sdm_plan *P, const ConeTabs &T, const RotPlan &S, double *area, double *y, const int *gjc, const double *g) {
  if (S.nitems == 0) return;
  int64_t *tab = (int64_t *)(area + S.ws);
  SDM_HIP_CHECK(hipMemcpy(tab, S.img.data(), S.img.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  const int *items = (const int *)(tab + S.w_items);
  rot_allow_lds(k_givensrot, S.lds);
  SDM_KLAUNCH(P, k_givensrot, dim3(S.nitems), dim3(GR_W), S.lds, y, gjc, g, area, rot_blk(T, S, tab), items, S.slot);
  SDM_HIP_CHECK(hipGetLastError());
}

// q, y: lenud doubles; v: sum n doubles (all device)
void sqrtinv_run(sdm_plan *P, const ConeTabs &T, const double *q, const double *v, double *y) {
  if (T.nfull == 0) return;
  RotBlk B; B.n = T.n; B.herm = T.herm; B.loff = T.loff; B.off = T.off; B.goff = nullptr; B.woff = nullptr;
  SDM_KLAUNCH(P, k_sqrtinv, dim3(T.nfull), dim3(256), 0, q, v, y, B, T.items_full);
  SDM_HIP_CHECK(hipGetLastError());
}

}  // namespace sdm
