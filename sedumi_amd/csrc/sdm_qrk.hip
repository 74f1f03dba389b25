// sdm_qrk.hip -- [q, r] = qrK(x, K) on the device: the producer of the PSD frames sdm_cone.hip consumes.  Per PSD
// block of order n:  x = Q_0 Q_1 ... Q_{n-2} (diag(q)) R,  Q_k = I - c_k c_k^H / beta_k on rows / columns k .. n-1, in the reference's
// conventions (qrK.c:86-227; include/sedumi_hip.h at sdm_qrk) and in its output layout (the frame described on top of sdm_cone.hip).
// The reference applies every reflector to every trailing column with a dot and an axpy (4 n^3 / 3 flops at memory speed); here it is a
// blocked right-looking Householder QR: panels of QR_NB columns, and per panel [j0, j1) of all blocks that still have one, three launches
//   k_qrk_panel   one workgroup per block: the panel's reflectors one after the other, each applied to the panel's remaining columns;
//                 writes c_k, beta_k (Hermitian: the sign q_k and R_kk = |u_kk| too), the finished rows of R inside the panel and the
//                 QR_NB x QR_NB upper triangular T with Q_j0 ... Q_{j1-1} = I - V T V^H:  T_kk = 1/beta_k,
//                 T(0:k,k) = -T(0:k,0:k) V(:,0:k)^H v_k / beta_k
//   k_qrk_w       W = T^H (V^H A) for the trailing columns A = x(j0:n-1, j1:n-1), QR_NB x 64 per workgroup, K over the rows
//   k_qrk_update  A -= V W, 64 x 64 tiles, K = QR_NB
// the two products on v_mfma_f64_16x16x4_f64 in cone_mma's blocking, Hermitian blocks as products of planes with the conjugates in the
// operand fetch (k_cone_gemm's way); after the last panel k_qrk_sign turns the rows of a Hermitian R by conj(q_i) and makes the last sign.
// Dependencies are launch boundaries on one stream: no counters, no atomics, no hand-over between workgroups inside a launch.
//
// Panel step: a work-item owns the rows j0 + tid (mod QR_T) of the panel for the whole step -- everything it reads or writes in the panel
// is its own rows, so the panel may live in LDS (when it fits the budget) or in place in r in global memory: the same operations in the
// same order, the same bits (the model of frame_strip<IN_LDS>).  The only exchange inside the workgroup is two reductions per reflector,
// each summed over the lanes by shuffles and over the wavefronts in a fixed order: the norm of the column (with x_kk), and one batch of at
// most QR_NB - 1 dots: c_k^H a_j for the panel's columns j > k (the reflection) and c_j^H c_k for j < k (the column of T).
#include "sdm_plan.h"
#include <algorithm>
#include <cstring>

namespace sdm {

constexpr int QR_NB = 32, QR_T = 256, QR_WV = QR_T / 64;
constexpr sdm_int QR_LDS_DEFAULT = 40 * 1024;          // (+ 18.3 KB of reduction slots and T: below the 64 KB a workgroup gets unasked)
static sdm_int g_qr_lds = QR_LDS_DEFAULT;

struct QrkBlk { const int *n; const int64_t *off, *foff; const int *herm; const int64_t *woff; };   // per block: order, offset in r, in q, Hermitian?, in the workspace
// workspace of a block: T (QR_NB x QR_NB per plane, T(t, l) at t * QR_NB + l), then W (QR_NB x n per plane, W(k, c) at k * n + c)

// ---------------------------------------------------------------- panel step
// P: the panel, entry (j0 + li, j0 + c) at P[c * ld + li], its imaginary part pim doubles further
template <bool IN_LDS, bool HERM>
__device__ __forceinline__ void qr_panel(double *P, int64_t ld, int64_t pim, double *Q, double *beta, double *R, double *Tg, int n, int j0,
                                         double *redA, double *redB, double *Ts) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t nn = (int64_t)n * n;
  const int m = n - j0, w = min(QR_NB, m), nref = min(w, m - 1);
  constexpr int TP = QR_NB * QR_NB, RP = QR_WV * QR_NB;
  for (int e = tid; e < (HERM ? 2 : 1) * TP; e += QR_T) Ts[e] = 0.0;
  if (IN_LDS)
    for (int c = 0; c < w; c++)
      for (int li = tid; li < m; li += QR_T) {
        P[c * ld + li] = R[(int64_t)(j0 + c) * n + j0 + li];
        if (HERM) P[pim + c * ld + li] = R[nn + (int64_t)(j0 + c) * n + j0 + li];
      }
  __syncthreads();
  for (int kk = 0; kk < nref; kk++) {
    const int k = j0 + kk;
    double *pk = P + kk * ld;
    // ---- the norm of x(k+1 : n-1, k), and x_kk to everybody
    double ss = 0.0;
    for (int li = tid; li < m; li += QR_T)
      if (li > kk) {
        const double a = pk[li]; ss += a * a;
        if (HERM) { const double b = pk[pim + li]; ss += b * b; }
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if (lane == 0) redA[wave] = ss;
    if (tid == kk) { redA[QR_WV] = pk[kk]; redA[QR_WV + 1] = HERM ? pk[pim + kk] : 0.0; }
    __syncthreads();
    const double xr = redA[QR_WV], xi = redA[QR_WV + 1], tot = ((redA[0] + redA[1]) + redA[2]) + redA[3];
    double ckr, cki = 0.0, bk, ukr, uki = 0.0;
    if (!HERM) {                                                        // qrK.c:99-108
      const double dk = (xr >= 0.0 ? 1.0 : -1.0) * sqrt(xr * xr + tot);
      ckr = xr + dk; bk = dk * ckr; ukr = -dk;
      if (bk == 0.0) bk = 1.0;
    } else {                                                            // qrK.c:158-182
      double ax = xr * xr + xi * xi;
      const double nx = sqrt(ax + tot);
      ax = sqrt(ax);
      if (ax > 0.0) { ukr = -(xr / ax) * nx; uki = -(xi / ax) * nx; } else { ukr = -nx; uki = xi; }
      ckr = xr - ukr; cki = xi - uki;
      bk = nx == 0.0 ? 1.0 : nx * (nx + ax);
    }
    const double rb = 1.0 / bk;
    if (tid == kk) {
      Q[(int64_t)k * n + k] = ckr; beta[k] = bk;
      if (!HERM) pk[kk] = ukr;
      else {                                                            // qrK.c:213-219 for i = k: the sign and |u_kk|
        const double au = sqrt(ukr * ukr + uki * uki);
        Q[nn + (int64_t)k * n + k] = cki;
        Q[(int64_t)(n - 1) * n + k] = ukr / au; Q[nn + (int64_t)(n - 1) * n + k] = uki / au;
        pk[kk] = au; pk[pim + kk] = 0.0;
      }
    }
    // ---- one batch of dots over this work-item's rows: slot jj > kk  c_k^H a_jj,  slot jj < kk  c_jj^H c_k
    double pr[QR_NB], pi[QR_NB];
#pragma unroll
    for (int jj = 0; jj < QR_NB; jj++) { pr[jj] = 0.0; pi[jj] = 0.0; }
    for (int li = tid; li < m; li += QR_T)
      if (li >= kk) {
        const double cr = li == kk ? ckr : pk[li], ci = HERM ? (li == kk ? cki : pk[pim + li]) : 0.0;
        if (li > kk) { Q[(int64_t)k * n + j0 + li] = cr; if (HERM) Q[nn + (int64_t)k * n + j0 + li] = ci; }
#pragma unroll
        for (int jj = 0; jj < QR_NB; jj++)
          if (jj != kk && jj < w) {
            const double ar = P[jj * ld + li];
            if (!HERM) pr[jj] += cr * ar;
            else {
              const double ai = P[pim + jj * ld + li];
              pr[jj] += cr * ar + ci * ai;
              pi[jj] += jj > kk ? cr * ai - ci * ar : ar * ci - ai * cr;
            }
          }
      }
#pragma unroll
    for (int jj = 0; jj < QR_NB; jj++)
      if (jj != kk && jj < w) {                                         // (uniform over the workgroup)
        double a = pr[jj], b = pi[jj];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); if (HERM) b += __shfl_xor(b, o); }
        if (lane == 0) { redB[wave * QR_NB + jj] = a; if (HERM) redB[RP + wave * QR_NB + jj] = b; }
      }
    __syncthreads();
    // ---- a_jj -= c_k (c_k^H a_jj / beta_k) on this work-item's rows
#pragma unroll
    for (int jj = 0; jj < QR_NB; jj++)
      if (jj > kk && jj < w) {
        pr[jj] = (((redB[jj] + redB[QR_NB + jj]) + redB[2 * QR_NB + jj]) + redB[3 * QR_NB + jj]) * rb;
        if (HERM) pi[jj] = (((redB[RP + jj] + redB[RP + QR_NB + jj]) + redB[RP + 2 * QR_NB + jj]) + redB[RP + 3 * QR_NB + jj]) * rb;
      }
    for (int li = tid; li < m; li += QR_T)
      if (li >= kk) {
        const double cr = li == kk ? ckr : pk[li], ci = HERM ? (li == kk ? cki : pk[pim + li]) : 0.0;
#pragma unroll
        for (int jj = 0; jj < QR_NB; jj++)
          if (jj > kk && jj < w) {
            if (!HERM) P[jj * ld + li] -= cr * pr[jj];
            else {
              P[jj * ld + li] -= cr * pr[jj] - ci * pi[jj];
              P[pim + jj * ld + li] -= cr * pi[jj] + ci * pr[jj];
            }
          }
      }
    // ---- column kk of T: work-item t < kk its own row t
    if (tid < kk) {
      double tr = 0.0, ti = 0.0;
      for (int l = tid; l < kk; l++) {
        const double zr = ((redB[l] + redB[QR_NB + l]) + redB[2 * QR_NB + l]) + redB[3 * QR_NB + l];
        const double a = Ts[tid * QR_NB + l];
        if (!HERM) tr += a * zr;
        else {
          const double zi = ((redB[RP + l] + redB[RP + QR_NB + l]) + redB[RP + 2 * QR_NB + l]) + redB[RP + 3 * QR_NB + l];
          const double b = Ts[TP + tid * QR_NB + l];
          tr += a * zr - b * zi; ti += a * zi + b * zr;
        }
      }
      Ts[tid * QR_NB + kk] = -tr * rb;
      if (HERM) Ts[TP + tid * QR_NB + kk] = -ti * rb;
    } else if (tid == kk) Ts[kk * QR_NB + kk] = rb;
  }
  __syncthreads();
  for (int e = tid; e < (HERM ? 2 : 1) * TP; e += QR_T) Tg[e] = Ts[e];
  // the panel's part of r: R on and above the diagonal, 0 below it
  for (int c = 0; c < w; c++)
    for (int li = tid; li < m; li += QR_T) {
      if (IN_LDS) {
        R[(int64_t)(j0 + c) * n + j0 + li] = li <= c ? P[c * ld + li] : 0.0;
        if (HERM) R[nn + (int64_t)(j0 + c) * n + j0 + li] = li <= c ? P[pim + c * ld + li] : 0.0;
      } else if (li > c) {
        P[c * ld + li] = 0.0;
        if (HERM) P[pim + c * ld + li] = 0.0;
      }
    }
}

__global__ void __launch_bounds__(QR_T)
k_qrk_panel(double *q, double *r, double *ws, QrkBlk B, const int *items, int j0) {
  SDM_DYN_SMEM(smem);
  __shared__ double redA[QR_WV + 2], redB[2 * QR_WV * QR_NB], Ts[2 * QR_NB * QR_NB];
  const int b = items[4 * blockIdx.x], use_lds = items[4 * blockIdx.x + 1];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const int m = n - j0, w = min(QR_NB, m);
  double *Q = q + B.foff[b], *R = r + B.off[b], *Tg = ws + B.woff[b];
  double *beta = herm ? Q + 2 * nn : Q + nn - n;
  double *G = R + (int64_t)j0 * n + j0, *S = (double *)smem;
  if (herm) {
    if (use_lds) qr_panel<true, true>(S, m, (int64_t)m * w, Q, beta, R, Tg, n, j0, redA, redB, Ts);
    else qr_panel<false, true>(G, n, nn, Q, beta, R, Tg, n, j0, redA, redB, Ts);
  } else {
    if (use_lds) qr_panel<true, false>(S, m, 0, Q, beta, R, Tg, n, j0, redA, redB, Ts);
    else qr_panel<false, false>(G, n, 0, Q, beta, R, Tg, n, j0, redA, redB, Ts);
  }
}

// ---------------------------------------------------------------- trailing update
constexpr int QW_KC = 32, QW_AP = QR_NB + 1, QW_BP = 65;

// W = T^H (V^H A): item (b, J) = columns j1 + 64 J .. of block b, j1 = j0 + QR_NB
__global__ void __launch_bounds__(QR_T)
k_qrk_w(const double *q, const double *r, double *ws, QrkBlk B, const int *items, int j0) {
  __shared__ double As[QW_KC * QW_AP], Bs[QW_KC * QW_BP], Ys[2 * QR_NB * QW_BP];
  const int b = items[4 * blockIdx.x], J = items[4 * blockIdx.x + 1];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *Q = q + B.foff[b], *R = r + B.off[b];
  const int nplanes = herm ? 2 : 1;
  const double *Tg = ws + B.woff[b];
  double *Wg = ws + B.woff[b] + nplanes * QR_NB * QR_NB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
  const int c0 = j0 + QR_NB + 64 * J;
  // V^H(kk, i) = conj(c_{j0+kk}(i)), rows i >= j0 + kk
  auto Aval = [&](int kk, int i, int pl) -> double {
    if (i >= n || i < j0 + kk) return 0.0;
    const double v = Q[(int64_t)pl * nn + (int64_t)(j0 + kk) * n + i];
    return pl ? -v : v;
  };
  auto Bval = [&](int i, int c, int pl) -> double { return (i < n && c < n) ? R[(int64_t)pl * nn + (int64_t)c * n + i] : 0.0; };
  for (int opl = 0; opl < nplanes; opl++) {
    sdm_double4 acc[2];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int g = 0; g < 4; g++) acc[t][g] = 0.0;
    for (int term = 0; term < nplanes; term++) {
      const int apl = term, bpl = opl ^ term;
      const double sgn = (opl == 0 && term == 1) ? -1.0 : 1.0;
      for (int kb = j0; kb < n; kb += QW_KC) {
        __syncthreads();
        for (int e = tid; e < QW_KC * 64; e += QR_T) {
          const int kx = e & (QW_KC - 1), s = e >> 5;                  // the row index i fastest: as both operands are stored
          if (s < QR_NB) As[kx * QW_AP + s] = sgn * Aval(s, kb + kx, apl);
          Bs[kx * QW_BP + s] = Bval(kb + kx, c0 + s, bpl);
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < QW_KC; kk += 4) {
          const double a0 = As[(kk + kq) * QW_AP + l15], a1 = As[(kk + kq) * QW_AP + 16 + l15];
          const double bv = Bs[(kk + kq) * QW_BP + 16 * wave + l15];
          acc[0] = SDM_MFMA_F64_16x16x4(a0, bv, acc[0]);
          acc[1] = SDM_MFMA_F64_16x16x4(a1, bv, acc[1]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int g = 0; g < 4; g++) Ys[opl * QR_NB * QW_BP + (16 * t + kq + 4 * g) * QW_BP + 16 * wave + l15] = acc[t][g];
  }
  __syncthreads();
  // W(kk, c) = sum_{l <= kk} conj(T(l, kk)) Y(l, c)
  const int c = tid & 63;
  if (c0 + c < n)
    for (int kk = tid >> 6; kk < QR_NB; kk += QR_WV) {
      double wr = 0.0, wi = 0.0;
      for (int l = 0; l <= kk; l++) {
        const double tr = Tg[l * QR_NB + kk], yr = Ys[l * QW_BP + c];
        if (!herm) wr += tr * yr;
        else {
          const double ti = Tg[QR_NB * QR_NB + l * QR_NB + kk], yi = Ys[QR_NB * QW_BP + l * QW_BP + c];
          wr += tr * yr + ti * yi; wi += tr * yi - ti * yr;
        }
      }
      Wg[(int64_t)kk * n + c0 + c] = wr;
      if (herm) Wg[(int64_t)QR_NB * n + (int64_t)kk * n + c0 + c] = wi;
    }
}

// A -= V W: item (b, I, J) = rows j0 + 64 I .., columns j1 + 64 J .. of block b
__global__ void __launch_bounds__(QR_T)
k_qrk_update(const double *q, double *r, const double *ws, QrkBlk B, const int *items, int j0) {
  __shared__ double As[QR_NB * QW_BP], Bs[QR_NB * QW_BP];
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *Q = q + B.foff[b];
  double *R = r + B.off[b];
  const int nplanes = herm ? 2 : 1;
  const double *Wg = ws + B.woff[b] + nplanes * QR_NB * QR_NB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = j0 + 64 * I, c0 = j0 + QR_NB + 64 * J;
  const int rb = 32 * (wave & 1) + (lane & 15), cb = 32 * (wave >> 1) + (lane & 15), kq = lane >> 4;
  for (int opl = 0; opl < nplanes; opl++) {
    sdm_double4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int g = 0; g < 4; g++) acc[i][j][g] = 0.0;
    for (int term = 0; term < nplanes; term++) {
      const int apl = term, bpl = opl ^ term;
      const double sgn = (opl == 0 && term == 1) ? -1.0 : 1.0;
      __syncthreads();
      for (int e = tid; e < QR_NB * 64; e += QR_T) {
        const int f = e & 63, kk = e >> 6, i = r0 + f, cc = c0 + f;
        As[kk * QW_BP + f] = (i < n && i >= j0 + kk) ? sgn * Q[(int64_t)apl * nn + (int64_t)(j0 + kk) * n + i] : 0.0;
        Bs[kk * QW_BP + f] = cc < n ? Wg[(int64_t)bpl * QR_NB * n + (int64_t)kk * n + cc] : 0.0;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < QR_NB; kk += 4) {
        const double a0 = As[(kk + kq) * QW_BP + rb], a1 = As[(kk + kq) * QW_BP + rb + 16];
        const double b0 = Bs[(kk + kq) * QW_BP + cb], b1 = Bs[(kk + kq) * QW_BP + cb + 16];
        acc[0][0] = SDM_MFMA_F64_16x16x4(a0, b0, acc[0][0]);
        acc[0][1] = SDM_MFMA_F64_16x16x4(a0, b1, acc[0][1]);
        acc[1][0] = SDM_MFMA_F64_16x16x4(a1, b0, acc[1][0]);
        acc[1][1] = SDM_MFMA_F64_16x16x4(a1, b1, acc[1][1]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int row = r0 + 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * g, col = c0 + 32 * (wave >> 1) + 16 * j + (lane & 15);
          if (row < n && col < n) R[(int64_t)opl * nn + (int64_t)col * n + row] -= acc[i][j][g];
        }
  }
}

// Hermitian blocks, after the last panel (qrK.c:207-226): row i of R right of the diagonal times conj(q_i); the last sign q_{n-1} and
// R_{n-1,n-1} = |u_{n-1,n-1}| (those of i < n-1 are the panel step's).  item (b, k0) = columns k0 .. k0 + 3, a wavefront each
__global__ void __launch_bounds__(QR_T)
k_qrk_sign(double *q, double *r, QrkBlk B, const int *items) {
  const int b = items[4 * blockIdx.x], k = items[4 * blockIdx.x + 1] + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = B.n[b];
  const int64_t nn = (int64_t)n * n;
  if (k >= n) return;
  double *Sr = q + B.foff[b] + (int64_t)(n - 1) * n, *Si = Sr + nn, *Ur = r + B.off[b] + (int64_t)k * n, *Ui = Ur + nn;
  for (int i = lane; i < k; i += 64) {
    const double sr = Sr[i], si = Si[i], ur = Ur[i], ui = Ui[i];
    Ur[i] = sr * ur + si * ui;                                          // isconjhadamul, qrK.c:61-71
    Ui[i] = sr * ui - si * ur;
  }
  if (k == n - 1 && lane == 0) {
    const double ur = Ur[k], ui = Ui[k], au = sqrt(ur * ur + ui * ui);
    Sr[k] = ur / au; Si[k] = ui / au;
    Ur[k] = au; Ui[k] = 0.0;
  }
}

// =========================================================================== host
void qrk_set_panel_lds_budget(sdm_int bytes) {
  if (bytes < 0 || bytes > QR_LDS_DEFAULT) throw std::runtime_error("QR panel LDS budget: 0 (default) .. 40960 bytes");
  g_qr_lds = bytes ? bytes : QR_LDS_DEFAULT;
}

// the launches of every panel step of the PSD blocks `ns` (the first rsdpN real, the others Hermitian) and their item tables
void qrk_plan(QrkSteps &S, const std::vector<int> &ns, int rsdpN) {
  const int nb = (int)ns.size();
  std::vector<int64_t> woff(std::max(nb, 1), 0);
  std::vector<int> items;
  int nmax = 0;
  S.ws = 0;
  for (int b = 0; b < nb; b++) {
    if (ns[b] < 0) throw std::runtime_error("K.s: negative order");
    woff[b] = S.ws;
    S.ws += (int64_t)(b < rsdpN ? 1 : 2) * QR_NB * (QR_NB + ns[b]);
    nmax = std::max(nmax, ns[b]);
  }
  S.steps.clear();
  for (int j0 = 0; j0 < nmax - 1; j0 += QR_NB) {
    QrkSteps::Step st{};
    st.j0 = j0; st.panel0 = (int)items.size() / 4;
    for (int b = 0; b < nb; b++)
      if (ns[b] - 1 > j0) {                                             // (a last column alone has no reflector)
        const int64_t m = ns[b] - j0, bytes = (b < rsdpN ? 1 : 2) * m * std::min<int64_t>(QR_NB, m) * (int64_t)sizeof(double);
        const int lds = bytes <= g_qr_lds ? 1 : 0;                      // else in place in r
        if (lds) st.lds = std::max(st.lds, (size_t)bytes);
        items.insert(items.end(), {b, lds, 0, 0});
      }
    st.npanel = (int)items.size() / 4 - st.panel0; st.strip0 = (int)items.size() / 4;
    for (int b = 0; b < nb; b++)
      for (int J = 0; j0 + QR_NB + 64 * J < ns[b]; J++) items.insert(items.end(), {b, J, 0, 0});
    st.nstrip = (int)items.size() / 4 - st.strip0; st.tile0 = (int)items.size() / 4;
    for (int b = 0; b < nb; b++)
      for (int J = 0; j0 + QR_NB + 64 * J < ns[b]; J++)
        for (int I = 0; j0 + 64 * I < ns[b]; I++) items.insert(items.end(), {b, I, J, 0});
    st.ntile = (int)items.size() / 4 - st.tile0;
    S.steps.push_back(st);
  }
  S.sign0 = (int)items.size() / 4;
  for (int b = rsdpN; b < nb; b++)
    for (int k0 = 0; k0 < ns[b]; k0 += QR_WV) items.insert(items.end(), {b, k0, 0, 0});
  S.nsign = (int)items.size() / 4 - S.sign0;
  if (items.size() & 1) items.push_back(0);
  S.img.assign(woff.begin(), woff.end());
  S.w_items = S.img.size();
  S.img.resize(S.w_items + items.size() / 2);
  if (!items.empty()) memcpy(S.img.data() + S.w_items, items.data(), items.size() * sizeof(int));
}

void qrk_run(sdm_plan *P, const ConeTabs &T, const QrkSteps &S, double *area, double *q, double *r) {
  int64_t *tab = (int64_t *)(area + S.ws);
  SDM_HIP_CHECK(hipMemcpy(tab, S.img.data(), S.img.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  const int *items = (const int *)(tab + S.w_items);
  QrkBlk B; B.n = T.n; B.off = T.off; B.foff = T.foff; B.herm = T.herm; B.woff = tab;
  SDM_HIP_CHECK(hipMemsetAsync(q, 0, (size_t)T.lenfr * sizeof(double), P->stream));   // what the reference's zero-initialised q keeps
  double *ws = area;
  for (const QrkSteps::Step &st : S.steps) {
    if (st.npanel) SDM_KLAUNCH(P, k_qrk_panel, dim3(st.npanel), dim3(QR_T), st.lds, q, r, ws, B, items + 4 * st.panel0, st.j0);
    if (st.nstrip) {
      SDM_KLAUNCH(P, k_qrk_w, dim3(st.nstrip), dim3(QR_T), 0, (const double *)q, (const double *)r, ws, B, items + 4 * st.strip0, st.j0);
      SDM_KLAUNCH(P, k_qrk_update, dim3(st.ntile), dim3(QR_T), 0, (const double *)q, r, (const double *)ws, B, items + 4 * st.tile0, st.j0);
    }
  }
  if (S.nsign) SDM_KLAUNCH(P, k_qrk_sign, dim3(S.nsign), dim3(QR_T), 0, q, r, B, items + 4 * S.sign0);
  SDM_HIP_CHECK(hipGetLastError());
}

}  // namespace sdm
