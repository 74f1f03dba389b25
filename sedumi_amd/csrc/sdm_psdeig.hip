// sdm_psdeig.hip -- psdeig.m:44-93 and minpsdeig.m:40-75 on the device: the eigenvalues, and on request the eigenvectors, of
// X + X^H for every PSD block at once, lab = half the eigenvalue, ascending per block.  Blocks are column major, Hermitian blocks [Re; Im] planes;
// the block tables are cone_tables', the matrix-core blocking is cone_mma's (sdm_cone_dev.h).
//
// One-sided (Hestenes) BLOCK JACOBI on 32-wide column blocks, a pair of them being the 64 columns of one cone_mma tile:
//   k_eig_sym      B = X + X^H (the full block is read; Im diag = 0.0 without being read), V = I when eigenvectors are wanted
//   k_eig_sq       the absolute row sums of A^H A = A^2, tile by tile on the matrix cores: ||A||_2 <= sqrt(||A^2||_inf), which is far closer than
//                  ||A||_inf when A's entries have mixed signs (exact for A^2 = I) -- every rounding error below scales with ||B||, so with sigma
//   k_eig_shift    one workgroup per block: sigma = 1.5 min(largest absolute row sum, Frobenius norm, sqrt of the largest row sum of |A^2|)
//                  >= 1.5 ||A||_2, B += sigma I; a row sum that
//                  is not finite marks the block (status 1): it never enters a sweep.  B is then positive definite with eigenvalues in
//                  [sigma / 3, 5 sigma / 3]: the eigenvalues of A are the column norms of the converged B V minus sigma, whatever their signs
//                  (plain Hestenes returns Rayleigh quotients of 0 for [[0,1],[1,0]]), and no column of B V is ever small beside another one, so
//                  the relative measure below can always be met.
//   sweeps         a round-robin pairing of the nb = ceil(n / 32) column blocks (circle method on nb rounded up to even: nb - 1 steps for even
//                  nb, nb for odd nb with one bye per step; nb = 1 pairs the block with an empty one).  Per step three launches, ordered by the
//                  stream, over all pairs of all blocks still iterating:
//     k_eig_gram     G = P^H P of the pair's n x 64 panel on the FP64 matrix cores, row chunks in ascending order, and the pair's measure
//                    max_{i>j} |g_ij| / sqrt(g_ii g_jj) (a norm of zero counts as orthogonal)
//     k_eig_inner    the eigenvectors W of G by a cyclic two-sided Jacobi in LDS, up to 32 disjoint (complex) rotations per step in a fixed parallel
//                    order; Z = W - I overwrites G (a W close to I keeps the digits of what it differs by).  A pair whose measure is at rounding level (4 u) returns at entry, here and in k_eig_apply
//     k_eig_apply    P <- P W for B, and for V, on the matrix cores, one workgroup per (pair, 64-row chunk, matrix)
//   k_eig_conv     the largest measure of the sweep per block: the one word per block the host reads after every sweep.  A block whose sweep
//                  met no measure above 4 max(n, 64) u is done; it drops out of the next sweep's lists.
//   k_eig_norms    lab_j = (||b_j|| - sigma) / 2;  k_eig_sort: rank by counting (strictly smaller entries, plus equal ones before it), lab in
//                  that order;  k_eig_q: the columns of V in that order, each divided by its norm;  k_eig_min: the minimum over all of lab.
// No spin waits, no flags another workgroup polls, no atomics: a block's bits depend on nothing but the block, and the eigenvalue-only mode does
// the same rotations on B, so its lab is the same bit for bit.  A block that is not done after SDM_EIG_MAX_SWEEPS sweeps, or whose measure is NaN
// (overflow), gets status 2; blocks with a status get lab = q = NaN and are reported through info.
#include "sdm_plan.h"
#include "sdm_cone_dev.h"
#include <algorithm>
#include <cstring>

namespace sdm {

constexpr int EG_W = 32;                            // columns of a column block
constexpr int EG_INNER_SWEEPS = 15;                 // cap of the inner solver
constexpr double EG_U = 1.1102230246251565e-16;     // 2^-53
constexpr double EG_TOL_IN = 32 * EG_U;             // inner solver: a sweep whose largest relative off-diagonal entry is within this was the last
constexpr double EG_ROT_EPS = EG_U;                 // a rotation for a relative entry within this is the identity

// The two outer thresholds on a pair's measure |g_ij| / sqrt(g_ii g_jj).  SKIP: at rounding level; a pair within it is left alone (W is never
// formed), every other pair is rotated, so that what a sweep leaves behind is as orthogonal as rounding allows and not merely within a threshold.
// CONV: a block whose sweep MET no measure above it is done: the Gram sums carry a relative error of up to n u themselves, and the columns a
// rotation leaves behind measure some tens of u.  (A looser CONV that counts on the quadratic convergence of the sweep's own rotations is wrong
// for clustered eigenvalues: with 2^-27 the log-spaced spectrum of order 129 came out with 18 times the residual.)
constexpr double EG_TOL_SKIP = 4 * EG_U;
__host__ __device__ inline double eig_tol(int n) { (void)n; return EG_TOL_SKIP; }
inline double eig_tol_conv(int n) { return 4.0 * (n > 64 ? n : 64) * EG_U; }
// column j of a pair's panel in the block; >= n: an empty column
__device__ __forceinline__ int eig_col(int p, int q, int j) { return j < EG_W ? EG_W * p + j : EG_W * q + j - EG_W; }
// max that keeps a NaN
__device__ __forceinline__ double eig_maxnan(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
__device__ __forceinline__ double eig_nan() { return __builtin_nan(""); }

// ---------------------------------------------------------------- B = X + X^H, V = I.  items: cone_tables' full tile list (block, I, J, -)
__global__ void __launch_bounds__(CN_T)
k_eig_sym(const double *x, double *bw, double *v, ConeBlk B, const int *items) {
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *X = x + B.off[b];
  for (int e = threadIdx.x; e < 64 * 64; e += CN_T) {
    const int r = 64 * I + (e & 63), c = 64 * J + (e >> 6);
    if (r >= n || c >= n) continue;
    const int64_t rc = (int64_t)c * n + r, cr = (int64_t)r * n + c;
    bw[B.off[b] + rc] = X[rc] + X[cr];
    if (herm) bw[B.off[b] + nn + rc] = r == c ? 0.0 : X[nn + rc] - X[nn + cr];   // (Im of the diagonal is not read: X + X^H cancels it)
    if (v) { v[B.off[b] + rc] = r == c ? 1.0 : 0.0; if (herm) v[B.off[b] + nn + rc] = 0.0; }
  }
}

// ---------------------------------------------------------------- row sums of |A^H A| per tile.  items: cone_tables' full tile list (block, I, J, -)
// rsq[J lenlab + loff + i] = sum over the columns j of tile J of |Re T_ij| + |Im T_ij|, T = A(:, I)^H A(:, J), i a row of tile I
__global__ void __launch_bounds__(CN_T)
k_eig_sq(const double *bw, ConeBlk B, const int *items, double *rsq, int64_t lenlab) {
  __shared__ double sa[64 * CN_P], sb[64 * CN_P];
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *A = bw + B.off[b];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nplanes = herm ? 2 : 1;
  ConeAcc acc[2];
  // Re = ArI^T ArJ + AiI^T AiJ ;  Im = ArI^T AiJ - AiI^T ArJ
#pragma unroll
  for (int opl = 0; opl < 2; opl++) {
    if (opl >= nplanes) continue;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[opl].t[i][j][r] = 0.0;
    for (int term = 0; term < nplanes; term++) {
      const int apl = term, bpl = opl ^ term;
      const bool neg = opl == 1 && term == 1;
      for (int kb = 0; kb < n; kb += 64) {
        __syncthreads();
        for (int e = tid; e < 64 * 64; e += CN_T) {
          const int f = e & 63, j = e >> 6, r = kb + f, ca = 64 * I + j, cb = 64 * J + j;
          const double va = (r < n && ca < n) ? A[(int64_t)apl * nn + (int64_t)ca * n + r] : 0.0;
          sa[f * CN_P + j] = neg ? -va : va;
          sb[f * CN_P + j] = (r < n && cb < n) ? A[(int64_t)bpl * nn + (int64_t)cb * n + r] : 0.0;
        }
        __syncthreads();
        cone_mma(acc[opl], sa, sb, wave, lane);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r, col = 32 * (wave >> 1) + 16 * j + (lane & 15);
        sa[row * CN_P + col] = fabs(acc[0].t[i][j][r]) + (herm ? fabs(acc[1].t[i][j][r]) : 0.0);
      }
  __syncthreads();
  if (tid < 64 && 64 * I + tid < n) {
    double s = 0.0;
    for (int j = 0; j < 64; j++) s += sa[tid * CN_P + j];
    rsq[(int64_t)J * lenlab + B.loff[b] + 64 * I + tid] = s;
  }
}

// ---------------------------------------------------------------- the shift, one workgroup per block
__global__ void __launch_bounds__(CN_T)
k_eig_shift(double *bw, ConeBlk B, const double *rsq, int64_t lenlab, double *sig, int *status) {
  __shared__ double rs[CN_T], fs[CN_T], qs[CN_T];
  const int b = blockIdx.x, n = B.n[b], herm = B.herm[b], tid = threadIdx.x;
  const int64_t nn = (int64_t)n * n;
  double *A = bw + B.off[b];
  double rmax = 0.0, fro = 0.0, qmax = 0.0;
  const int nt = (n + 63) / 64;
  for (int r = tid; r < n; r += CN_T) {
    double s = 0.0, s2 = 0.0;
    for (int J = 0; J < nt; J++) s2 += rsq[(int64_t)J * lenlab + B.loff[b] + r];
    qmax = eig_maxnan(qmax, s2);
    for (int c = 0; c < n; c++) {
      const double vr = A[(int64_t)c * n + r], vi = herm ? A[nn + (int64_t)c * n + r] : 0.0;
      s += fabs(vr) + fabs(vi); fro += vr * vr + vi * vi;
    }
    rmax = eig_maxnan(rmax, s);
  }
  rs[tid] = rmax; fs[tid] = fro; qs[tid] = qmax;
  __syncthreads();
  rmax = 0.0; fro = 0.0; qmax = 0.0;
  for (int t = 0; t < CN_T; t++) { rmax = eig_maxnan(rmax, rs[t]); fro += fs[t]; qmax = eig_maxnan(qmax, qs[t]); }   // (everybody, in one order: the decision below is uniform)
  const bool finite = fabs(rmax) <= 1.7976931348623157e308;                          // (an entry that is Inf or NaN makes its row sum so)
  fro = sqrt(fro); qmax = sqrt(qmax);
  double bound = rmax;                                                               // (fro, qmax = Inf or NaN by overflow of the squares: not taken)
  if (fro < bound) bound = fro;
  if (qmax < bound) bound = qmax;
  const double s = finite ? 1.5 * bound : eig_nan();
  if (tid == 0) { sig[b] = s; status[b] = finite ? 0 : 1; }
  if (!finite) return;
  for (int r = tid; r < n; r += CN_T) A[(int64_t)r * n + r] += s;
}

// ---------------------------------------------------------------- G = P^H P and the pair's measure.  items: (block, p, q, -); slot = blockIdx.x
__global__ void __launch_bounds__(CN_T)
k_eig_gram(const double *bw, ConeBlk B, const int *items, double *gw, double *meas) {
  __shared__ double sr[64 * CN_P], si[64 * CN_P], sn[64 * CN_P], red[CN_T];
  const int b = items[4 * blockIdx.x], p = items[4 * blockIdx.x + 1], q = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *A = bw + B.off[b];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  ConeAcc gr, gi;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) { gr.t[i][j][r] = 0.0; gi.t[i][j][r] = 0.0; }
  // Re G = Pr^T Pr + Pi^T Pi ;  Im G = Pr^T Pi - Pi^T Pr ;  the panel's rows kb .. kb+63 staged as S[row][column]
  for (int kb = 0; kb < n; kb += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += CN_T) {
      const int f = e & 63, j = e >> 6, c = eig_col(p, q, j), r = kb + f;
      const bool ok = c < n && r < n;
      sr[f * CN_P + j] = ok ? A[(int64_t)c * n + r] : 0.0;
      if (herm) { const double vi = ok ? A[nn + (int64_t)c * n + r] : 0.0; si[f * CN_P + j] = vi; sn[f * CN_P + j] = -vi; }
    }
    __syncthreads();
    cone_mma(gr, sr, sr, wave, lane);
    if (herm) { cone_mma(gr, si, si, wave, lane); cone_mma(gi, sr, si, wave, lane); cone_mma(gi, sn, sr, wave, lane); }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r, col = 32 * (wave >> 1) + 16 * j + (lane & 15);
        sr[row * CN_P + col] = gr.t[i][j][r];
        if (herm) si[row * CN_P + col] = gi.t[i][j][r];
      }
  __syncthreads();
  double *G = gw + (int64_t)blockIdx.x * 8192;
  double mx = 0.0;
  for (int e = tid; e < 64 * 64; e += CN_T) {
    const int i = e >> 6, j = e & 63;
    const double vr = sr[i * CN_P + j], vi = herm ? si[i * CN_P + j] : 0.0;
    G[e] = vr;
    if (herm) G[4096 + e] = vi;
    if (i > j) {
      const double a = sr[i * CN_P + i], c = sr[j * CN_P + j];
      if (a != a || c != c) mx = eig_nan();
      else if (a > 0.0 && c > 0.0) {
        const double d = sqrt(a) * sqrt(c), xr = vr / d, xi = vi / d;
        mx = eig_maxnan(mx, herm ? sqrt(xr * xr + xi * xi) : fabs(xr));
      }
    }
  }
  red[tid] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < CN_T; t++) mx = eig_maxnan(mx, red[t]);
    meas[blockIdx.x] = mx;
  }
}

// ---------------------------------------------------------------- W: the eigenvectors of G, in its place
// The rotation of (p, q) for the Hermitian [[a, g], [conj g, b]], g = |g| e:  J = [[c, s e], [-s conj e, c]], t = s / c the smaller root of
// t^2 + 2 tau t - 1 = 0, tau = (b - a) / (2 |g|).  G <- J^H G J, W <- W J.
__global__ void __launch_bounds__(CN_T)
k_eig_inner(ConeBlk B, const int *items, double *gw, const double *meas) {
  __shared__ double Gr[64 * CN_P], Gi[64 * CN_P], Wr[64 * CN_P], Wi[64 * CN_P];
  __shared__ double rc[32], rc1[32], rsr[32], rsi[32], rmx[32];
  __shared__ int rp[32], rq[32], ron[32], act[65];
  const int b = items[4 * blockIdx.x], bp = items[4 * blockIdx.x + 1], bq = items[4 * blockIdx.x + 2], n = B.n[b], herm = B.herm[b], tid = threadIdx.x;
  if (!(meas[blockIdx.x] > eig_tol(n))) return;                      // (the whole workgroup alike)
  double *G = gw + (int64_t)blockIdx.x * 8192;
  for (int e = tid; e < 64 * 64; e += CN_T) {                         // the lower triangle, mirrored; Im diag = 0
    const int i = e >> 6, j = e & 63;
    if (i >= j) {
      const double vr = G[e], vi = (herm && i > j) ? G[4096 + e] : 0.0;
      Gr[i * CN_P + j] = vr; Gr[j * CN_P + i] = vr; Gi[i * CN_P + j] = vi; Gi[j * CN_P + i] = -vi;
      if (i == j) Gi[i * CN_P + i] = 0.0;
    }
    Wr[i * CN_P + j] = 0.0; Wi[i * CN_P + j] = 0.0;                   // Z = W - I
  }
  // the panel's columns that exist, ascending: the rotations run over these alone (the others are zero rows and columns of G)
  if (tid == 0) {
    int m = 0;
    for (int j = 0; j < 64; j++)
      if (eig_col(bp, bq, j) < n) act[m++] = j;
    act[64] = m;
  }
  __syncthreads();
  const int mact = act[64], meven = mact + (mact & 1), mhalf = meven / 2;   // circle method on meven players: meven - 1 steps of mhalf pairs
  for (int sw = 0; sw < EG_INNER_SWEEPS; sw++) {
    double mx = 0.0;
    for (int s = 0; s < meven - 1; s++) {
      if (tid < mhalf) {
        const int u = tid == 0 ? s : (s + tid) % (meven - 1), w = tid == 0 ? meven - 1 : (s - tid + meven - 1) % (meven - 1);
        const bool bye = (u > w ? u : w) >= mact;                        // (odd mact: the last player does not exist)
        const int p = bye ? 0 : act[u < w ? u : w], q = bye ? 0 : act[u < w ? w : u];
        const double a = Gr[p * CN_P + p], c = Gr[q * CN_P + q], g_r = Gr[p * CN_P + q], g_i = herm ? Gi[p * CN_P + q] : 0.0;
        const double ag = herm ? sqrt(g_r * g_r + g_i * g_i) : fabs(g_r);
        double m = 0.0; bool on;
        if (a > 0.0 && c > 0.0) { m = ag / (sqrt(a) * sqrt(c)); on = m > EG_ROT_EPS; }
        else on = ag > 0.0 && a == a && c == c;
        if (a != a || c != c || ag != ag) m = eig_nan();
        if (bye) { on = false; m = 0.0; }
        mx = eig_maxnan(mx, m);
        double cs = 1.0, cm1 = 0.0, s_r = 0.0, s_i = 0.0;
        if (on) {
          const double tau = (c - a) / (2.0 * ag), t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          cs = 1.0 / sqrt(1.0 + t * t);
          const double sn = t * cs;
          cm1 = -(sn * sn) / (1.0 + cs);                              // c - 1 without cancellation
          s_r = sn * (g_r / ag); s_i = sn * (g_i / ag);
        }
        rp[tid] = p; rq[tid] = q; ron[tid] = on ? 1 : 0; rc[tid] = cs; rc1[tid] = cm1; rsr[tid] = s_r; rsi[tid] = s_i;
      }
      __syncthreads();
      {                                                                // columns p, q of G and of W, a lane owning a row
        const int r = tid & 63;
        for (int t = tid >> 6; t < mhalf; t += 4) {
          if (!ron[t]) continue;
          const int p = rp[t], q = rq[t];
          const double c = rc[t], s_r = rsr[t], s_i = rsi[t];
#pragma unroll
          for (int m = 0; m < 2; m++) {
            double *Xr = m ? Wr : Gr, *Xi = m ? Wi : Gi;
            const double pr = Xr[r * CN_P + p], qr = Xr[r * CN_P + q];
            double npr, nqr, npi = 0.0, nqi = 0.0;
            if (!herm) { npr = c * pr - s_r * qr; nqr = s_r * pr + c * qr; }
            else {
              const double pi = Xi[r * CN_P + p], qi = Xi[r * CN_P + q];
              npr = c * pr - (s_r * qr + s_i * qi); npi = c * pi - (s_r * qi - s_i * qr);                              // c x_p - conj(s e) x_q
              nqr = (s_r * pr - s_i * pi) + c * qr; nqi = (s_r * pi + s_i * pr) + c * qi;                              // s e x_p + c x_q
            }
            // W is held as Z = W - I, so that a W close to I keeps the digits of what it differs by: (I + Z) J - I = Z J + (J - I)
            if (m && r == p) { npr += rc1[t]; nqr += s_r; nqi += s_i; }
            if (m && r == q) { npr -= s_r; npi += s_i; nqr += rc1[t]; }
            Xr[r * CN_P + p] = npr; Xr[r * CN_P + q] = nqr;
            if (herm) { Xi[r * CN_P + p] = npi; Xi[r * CN_P + q] = nqi; }
          }
        }
      }
      __syncthreads();
      {                                                                // rows p, q of G, a lane owning a column; (p, q), (q, p) and Im diag are 0
        const int j = tid & 63;
        for (int t = tid >> 6; t < mhalf; t += 4) {
          if (!ron[t]) continue;
          const int p = rp[t], q = rq[t];
          const double c = rc[t], s_r = rsr[t], s_i = rsi[t];
          const double pr = Gr[p * CN_P + j], qr = Gr[q * CN_P + j];
          double npr, nqr, npi = 0.0, nqi = 0.0;
          if (!herm) { npr = c * pr - s_r * qr; nqr = s_r * pr + c * qr; }
          else {
            const double pi = Gi[p * CN_P + j], qi = Gi[q * CN_P + j];
            npr = c * pr - (s_r * qr - s_i * qi); npi = c * pi - (s_r * qi + s_i * qr);                                // c g_p - s e g_q
            nqr = (s_r * pr + s_i * pi) + c * qr; nqi = (s_r * pi - s_i * pr) + c * qi;                                // conj(s e) g_p + c g_q
          }
          if (j == q) { npr = 0.0; npi = 0.0; }
          if (j == p) { nqr = 0.0; nqi = 0.0; npi = 0.0; }
          if (j == q) nqi = 0.0;
          Gr[p * CN_P + j] = npr; Gr[q * CN_P + j] = nqr;
          if (herm) { Gi[p * CN_P + j] = npi; Gi[q * CN_P + j] = nqi; }
        }
      }
      __syncthreads();
    }
    if (tid < 32) rmx[tid] = tid < mhalf ? mx : 0.0;
    __syncthreads();
    double m = 0.0;
    for (int t = 0; t < 32; t++) m = eig_maxnan(m, rmx[t]);           // (everybody, in one order: the decision is uniform)
    __syncthreads();
    if (!(m > EG_TOL_IN)) break;
  }
  for (int e = tid; e < 64 * 64; e += CN_T) {
    const int i = e >> 6, j = e & 63;
    G[e] = Wr[i * CN_P + j];
    if (herm) G[4096 + e] = Wi[i * CN_P + j];
  }
}

// ---------------------------------------------------------------- P <- P W = P + P Z for B (m0) and V (m1): workgroup = (pair, 64-row chunk, matrix)
__global__ void __launch_bounds__(CN_T)
k_eig_apply(double *m0, double *m1, ConeBlk B, const int *items, const double *gw, const double *meas, int npairs, int nchunks) {
  __shared__ double sa[64 * CN_P], sb[64 * CN_P];
  const int e0 = blockIdx.x % npairs, rest = blockIdx.x / npairs, r0 = 64 * (rest % nchunks), which = rest / nchunks;
  const int b = items[4 * e0], p = items[4 * e0 + 1], q = items[4 * e0 + 2];
  const int n = B.n[b], herm = B.herm[b];
  if (r0 >= n || !(meas[e0] > eig_tol(n))) return;                    // (the whole workgroup alike)
  const int64_t nn = (int64_t)n * n;
  double *M = (which ? m1 : m0) + B.off[b];
  const double *W = gw + (int64_t)e0 * 8192;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nplanes = herm ? 2 : 1;
  ConeAcc acc[2];
  // Re = Pr Wr - Pi Wi ;  Im = Pi Wr + Pr Wi
#pragma unroll
  for (int opl = 0; opl < 2; opl++) {
    if (opl >= nplanes) continue;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[opl].t[i][j][r] = 0.0;
    for (int term = 0; term < nplanes; term++) {
      const int apl = opl ^ term, wpl = term;
      const bool neg = opl == 0 && term == 1;
      __syncthreads();
      for (int e = tid; e < 64 * 64; e += CN_T) {
        const int f = e & 63, i = e >> 6, c = eig_col(p, q, i), r = r0 + f;
        const double v = (c < n && r < n) ? M[(int64_t)apl * nn + (int64_t)c * n + r] : 0.0;
        sa[i * CN_P + f] = neg ? -v : v;                               // As[k = panel column][row]
        sb[i * CN_P + f] = W[wpl * 4096 + e];                          // Bs[k][output column]: W(i, f)
      }
      __syncthreads();
      cone_mma(acc[opl], sa, sb, wave, lane);
    }
  }
  // every fetch of the panel is behind the barrier in front of the last cone_mma: the rows are written in place, through LDS, row fastest
#pragma unroll
  for (int opl = 0; opl < 2; opl++) {                                  // (unrolled: acc[opl] stays in registers)
    if (opl >= nplanes) continue;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r, col = 32 * (wave >> 1) + 16 * j + (lane & 15);
          sa[col * CN_P + row] = acc[opl].t[i][j][r];
        }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += CN_T) {
      const int f = e & 63, j = e >> 6, c = eig_col(p, q, j), r = r0 + f;
      if (c < n && r < n) M[(int64_t)opl * nn + (int64_t)c * n + r] += sa[j * CN_P + f];      // P + P Z
    }
  }
}

// ---------------------------------------------------------------- the largest measure of the sweep per block.  act: the blocks of this sweep
__global__ void __launch_bounds__(CN_T)
k_eig_conv(const int *act, const int *items, int nitems, const double *meas, double *bmeas) {
  __shared__ double red[CN_T];
  const int b = act[blockIdx.x], tid = threadIdx.x;
  double mx = 0.0;
  for (int e = tid; e < nitems; e += CN_T)
    if (items[4 * e] == b) mx = eig_maxnan(mx, meas[e]);
  red[tid] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < CN_T; t++) mx = eig_maxnan(mx, red[t]);
    bmeas[b] = mx;
  }
}

// ---------------------------------------------------------------- the finish
// raw_j = (||b_j|| - sigma) / 2; workgroup = (block, 64 columns), a lane owning a column
__global__ void __launch_bounds__(64)
k_eig_norms(const double *bw, ConeBlk B, const double *sig, const int *status, double *raw, int nchunks) {
  const int b = blockIdx.x / nchunks, c = 64 * (blockIdx.x % nchunks) + threadIdx.x, n = B.n[b], herm = B.herm[b];
  if (c >= n) return;
  if (status[b]) { raw[B.loff[b] + c] = eig_nan(); return; }
  const int64_t nn = (int64_t)n * n;
  const double *A = bw + B.off[b] + (int64_t)c * n;
  double ss = 0.0;
  for (int r = 0; r < n; r++) { const double vr = A[r], vi = herm ? A[nn + r] : 0.0; ss += vr * vr; ss += vi * vi; }
  raw[B.loff[b] + c] = (sqrt(ss) - sig[b]) / 2.0;
}
// rank by counting: the entries strictly smaller, plus the equal ones before it.  One workgroup per block
__global__ void __launch_bounds__(CN_T)
k_eig_sort(ConeBlk B, const int *status, const double *raw, double *lab, int *perm) {
  const int b = blockIdx.x, n = B.n[b], lo = B.loff[b];
  for (int j = threadIdx.x; j < n; j += CN_T) {
    const double v = raw[lo + j];
    int rank = j;
    if (!status[b]) {
      rank = 0;
      for (int k = 0; k < n; k++) { const double w = raw[lo + k]; rank += (w < v || (w == v && k < j)) ? 1 : 0; }
    }
    lab[lo + rank] = v; perm[lo + rank] = j;
  }
}
// q(:, r) = v_j / ||v_j||, j = perm[r]; workgroup = (block, 64 columns), a lane owning a column
__global__ void __launch_bounds__(64)
k_eig_q(const double *v, ConeBlk B, const int *status, const int *perm, double *q, int nchunks) {
  const int b = blockIdx.x / nchunks, c = 64 * (blockIdx.x % nchunks) + threadIdx.x, n = B.n[b], herm = B.herm[b];
  if (c >= n) return;
  const int64_t nn = (int64_t)n * n;
  double *Q = q + B.off[b] + (int64_t)c * n;
  if (status[b]) {
    for (int r = 0; r < n; r++) { Q[r] = eig_nan(); if (herm) Q[nn + r] = eig_nan(); }
    return;
  }
  const double *V = v + B.off[b] + (int64_t)perm[B.loff[b] + c] * n;
  double ss = 0.0;
  for (int r = 0; r < n; r++) { const double vr = V[r], vi = herm ? V[nn + r] : 0.0; ss += vr * vr; ss += vi * vi; }
  const double nrm = sqrt(ss);
  for (int r = 0; r < n; r++) { Q[r] = V[r] / nrm; if (herm) Q[nn + r] = V[nn + r] / nrm; }
}
// the minimum of lab (a NaN stays); one workgroup
__global__ void __launch_bounds__(CN_T)
k_eig_min(const double *lab, int len, double *out) {
  __shared__ double red[CN_T];
  const int tid = threadIdx.x;
  double m = __builtin_inf();
  for (int e = tid; e < len; e += CN_T) m = -eig_maxnan(-m, -lab[e]);
  red[tid] = m;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < CN_T; t++) m = -eig_maxnan(-m, -red[t]);
    out[0] = m;
  }
}

// =========================================================================== host
// the column blocks' pairs of block `ncb` column blocks at step s of a sweep (circle method); a pair with an empty partner is a bye, but for ncb = 1
static void eig_pairs(int ncb, int s, std::vector<std::pair<int, int>> &out) {
  out.clear();
  const int m = ncb + (ncb & 1);
  if (ncb <= 0 || s >= m - 1) return;
  for (int i = 0; i < m / 2; i++) {
    const int u = i == 0 ? s : (s + i) % (m - 1), w = i == 0 ? m - 1 : (s - i + m - 1) % (m - 1);
    const int p = std::min(u, w), q = std::max(u, w);
    if (q >= ncb && ncb > 1) continue;
    out.push_back({p, q});
  }
}

void psdeig_plan(PsdEigPlan &S, const std::vector<int> &ns, int rsdpN) {
  (void)rsdpN;
  S.ns = ns; S.nb = (int)ns.size(); S.ncb.assign(ns.size(), 0);
  S.lenlab = 0; S.maxitems = 0; S.maxpairs = 0;
  std::vector<int> active;
  for (int b = 0; b < S.nb; b++) {
    if (ns[b] < 0) throw std::runtime_error("K.s: negative order");
    S.ncb[b] = (ns[b] + EG_W - 1) / EG_W;
    S.lenlab += ns[b];
    if (ns[b] > 0) active.push_back(b);
  }
  std::vector<int> items; std::vector<PsdEigPlan::Step> steps;
  psdeig_sweep(S, active, items, steps);
  S.maxitems = (int64_t)items.size() / 4;
  for (const PsdEigPlan::Step &st : steps) S.maxpairs = std::max<int64_t>(S.maxpairs, st.n);
  const int64_t nbk = std::max(S.nb, 1);
  int64_t o = 0;
  S.o_sig = o; o += nbk;
  S.o_bmeas = o; o += nbk;
  S.o_min = o; o += 1;
  S.o_status = o; o += (nbk + 1) / 2;
  S.o_raw = o; o += S.lenlab;
  S.o_perm = o; o += (S.lenlab + 1) / 2;
  S.o_meas = o; o += S.maxitems;
  S.o_items = o; o += 2 * S.maxitems + (nbk + 1) / 2;                   // 4 int32 per item, then the sweep's blocks
  S.o_gw = o; o += 8192 * S.maxpairs;
  int ntmax = 0;
  for (int n : ns) ntmax = std::max(ntmax, (n + 63) / 64);
  S.o_rsq = o; o += (int64_t)ntmax * S.lenlab;
  S.ws = o;
}

// the item lists of one sweep over the blocks `active` (ascending): per step the pairs (block, p, q, 0) of every block that has that step
void psdeig_sweep(const PsdEigPlan &S, const std::vector<int> &active, std::vector<int> &items, std::vector<PsdEigPlan::Step> &steps) {
  items.clear(); steps.clear();
  int maxsteps = 0;
  for (int b : active) maxsteps = std::max(maxsteps, S.ncb[b] + (S.ncb[b] & 1) - 1);
  std::vector<std::pair<int, int>> pr;
  for (int s = 0; s < maxsteps; s++) {
    PsdEigPlan::Step st{};
    st.first0 = (int)items.size() / 4;
    for (int b : active) {
      eig_pairs(S.ncb[b], s, pr);
      for (const auto &pq : pr) items.insert(items.end(), {b, pq.first, pq.second, 0});
      if (!pr.empty()) st.nchunks = std::max(st.nchunks, (S.ns[b] + 63) / 64);
    }
    st.n = (int)items.size() / 4 - st.first0;
    steps.push_back(st);
  }
}

// x (lenud doubles, device): the blocks; bw, and v unless null: lenud doubles of work; lab: lenlab doubles; q (unless v is null; may be x): the
// eigenvectors; area: S.words() doubles.  Returns the first block that is not done (its lab and q are NaN) or -1; with dmin the device address of
// the minimum of lab.  Synchronises once per sweep; the results are complete on return.
int psdeig_run(sdm_plan *P, const ConeTabs &T, const PsdEigPlan &S, double *area, const double *x, double *bw, double *v, double *lab, double *q,
               bool want_min, int *sweeps_out) {
  const ConeBlk B = cone_blk(T);
  double *sig = area + S.o_sig, *bmeas = area + S.o_bmeas, *raw = area + S.o_raw, *meas = area + S.o_meas, *gw = area + S.o_gw;
  int *status = (int *)(area + S.o_status), *perm = (int *)(area + S.o_perm), *items = (int *)(area + S.o_items);
  int *act = items + 4 * S.maxitems;
  const int nb = S.nb;
  int ntmax = 0;
  for (int n : S.ns) ntmax = std::max(ntmax, (n + 63) / 64);
  SDM_KLAUNCH(P, k_eig_sym, dim3(T.nfull), dim3(CN_T), 0, x, bw, v, B, T.items_full);
  SDM_KLAUNCH(P, k_eig_sq, dim3(T.nfull), dim3(CN_T), 0, (const double *)bw, B, T.items_full, area + S.o_rsq, S.lenlab);
  SDM_KLAUNCH(P, k_eig_shift, dim3(nb), dim3(CN_T), 0, bw, B, (const double *)(area + S.o_rsq), S.lenlab, sig, status);
  std::vector<int> st((size_t)nb, 0), active, prev, hitems;
  std::vector<double> bm((size_t)nb, 0.0);
  std::vector<PsdEigPlan::Step> steps;
  SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
  SDM_HIP_CHECK(hipMemcpy(st.data(), status, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost));
  for (int b = 0; b < nb; b++)
    if (S.ns[b] > 0 && !st[b]) active.push_back(b);
  int sweeps = 0;
  bool late = false;
  for (; !active.empty() && sweeps < SDM_EIG_MAX_SWEEPS; sweeps++) {
    if (active != prev) {
      psdeig_sweep(S, active, hitems, steps);
      const size_t ni = hitems.size();
      hitems.insert(hitems.end(), active.begin(), active.end());
      SDM_HIP_CHECK(hipMemcpy(items, hitems.data(), ni * sizeof(int), hipMemcpyHostToDevice));
      SDM_HIP_CHECK(hipMemcpy(act, hitems.data() + ni, active.size() * sizeof(int), hipMemcpyHostToDevice));
      hitems.resize(ni);
      prev = active;
    }
    for (const PsdEigPlan::Step &s : steps) {
      if (!s.n) continue;
      const int *it = items + 4 * s.first0;
      SDM_KLAUNCH(P, k_eig_gram, dim3(s.n), dim3(CN_T), 0, (const double *)bw, B, it, gw, meas + s.first0);
      SDM_KLAUNCH(P, k_eig_inner, dim3(s.n), dim3(CN_T), 0, B, it, gw, (const double *)(meas + s.first0));
      SDM_KLAUNCH(P, k_eig_apply, dim3(s.n * s.nchunks * (v ? 2 : 1)), dim3(CN_T), 0, bw, v, B, it, (const double *)gw,
                  (const double *)(meas + s.first0), s.n, s.nchunks);
    }
    SDM_KLAUNCH(P, k_eig_conv, dim3((int)active.size()), dim3(CN_T), 0, (const int *)act, (const int *)items, (int)hitems.size() / 4,
                (const double *)meas, bmeas);
    SDM_HIP_CHECK(hipGetLastError());
    SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
    SDM_HIP_CHECK(hipMemcpy(bm.data(), bmeas, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> next;
    for (int b : active) {
      if (bm[b] != bm[b]) { st[b] = 2; late = true; }                  // overflow inside the block: it will not get better
      else if (bm[b] > eig_tol_conv(S.ns[b])) next.push_back(b);
    }
    active.swap(next);
  }
  for (int b : active) { st[b] = 2; late = true; }                     // not done at the cap
  if (late) SDM_HIP_CHECK(hipMemcpy(status, st.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice));
  SDM_KLAUNCH(P, k_eig_norms, dim3(nb * std::max(ntmax, 1)), dim3(64), 0, (const double *)bw, B, (const double *)sig, (const int *)status, raw,
              std::max(ntmax, 1));
  SDM_KLAUNCH(P, k_eig_sort, dim3(nb), dim3(CN_T), 0, B, (const int *)status, (const double *)raw, lab, perm);
  if (v) SDM_KLAUNCH(P, k_eig_q, dim3(nb * std::max(ntmax, 1)), dim3(64), 0, (const double *)v, B, (const int *)status, (const int *)perm, q,
                     std::max(ntmax, 1));
  if (want_min) SDM_KLAUNCH(P, k_eig_min, dim3(1), dim3(CN_T), 0, (const double *)lab, (int)S.lenlab, area + S.o_min);
  SDM_HIP_CHECK(hipGetLastError());
  SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
  if (sweeps_out) *sweeps_out = sweeps;
  for (int b = 0; b < nb; b++)
    if (st[b]) return b;
  return -1;
}

}  // namespace sdm
