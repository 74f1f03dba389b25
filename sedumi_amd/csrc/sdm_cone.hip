// sdm_cone.hip -- the PSD part of frameit.m / wregion.m on the device: the two congruences sedumi.m applies
// with the unitary frame of qrK, per PSD block of order n:
//   psdframeit   X = Qb^H diag(lab) Qb                                       psdframeit.c:65-99
//   psdinvjmul   Z = Qb^H ((Qb Ysym Qb^H) o 2/(x_i + x_j)) Qb                psdinvjmul.c:101-157 (diagjdiv :69-84)
// The reference applies the n - 1 Householder reflections of the frame one after the other from both sides (reflect.c:52-96,
// :203-215, :286-302); here the frame is expanded once into the explicit Qb and the congruences are FP64 GEMMs on the matrix cores.
//
// Frame (qrK.c:86-227):  real block      frms = n x n, column k (k < n-1) rows k.. = c_k, column n-1 = beta[0 .. n-2]
//                        Hermitian block frms = [Re c (n x n), Im c (n x n), beta (n)], column n-1 of the planes = the sign vector q
//   Q_k = I - c_k c_k^H / beta_k on rows / columns k .. n-1,   Qb = Q_0 Q_1 ... Q_{n-2} (diag(q) for Hermitian blocks)
//
// k_frame_expand: column j of Qb is Q_0 ... Q_{n-2} e_j and Q_k e_j = e_j for k > j, so the columns are independent.  A workgroup owns a
// strip of columns of one block (in LDS; in the output array itself when even four columns do not fit the LDS budget) and walks the
// reflectors from the strip's last column (n-2 at most) down to 0.  Inside the workgroup every wavefront owns whole columns and every lane
// the rows i = lane (mod 64) of them, for the dot c_k^H v (reduced over the lanes by shuffles) and for the update v -= c_k (c_k^H v / beta_k):
// a work-item only ever uses what it wrote itself -- no barrier, no hand-over between workgroups.  Strips are dealt longest first.
// The result does not depend on the strip width or on where the strip lives: per column the same operations in the same order.
//
// k_cone_gemm<MODE>: 64 x 64 output tiles, 4 wavefronts of 2 x 2 v_mfma_f64_16x16x4_f64 tiles each (the blocking of k_psdscale), over a
// tile list of all blocks; the operand accessors carry the transposes, conjugates, diag(lab) and the mirrored lower triangle of y.
// Products that are Hermitian by construction form only tiles I >= J and write every entry twice, mirrored (Im diag = 0).
//
// k_triumtriu (row N8): Z = triu(X) triu(Y) + the conjugate mirror of its strict upper triangle (triumtriu.m:63-64), the two ends of the
// re-pivoting chain of updtransfo.m:99-108; the same blocking on the tiles I <= J, k-tiles I .. J only (see at the kernel).
//
// k_psdjmul (row N11): Z = (X Y + (X Y)^H) / 2 (psdjmul.m:40-73), wregion.m's corrector; the same blocking on the tiles I <= J over all k-tiles,
// both terms into one accumulator (see at the kernel).
#include "sdm_plan.h"
#include "sdm_cone_dev.h"
#include <algorithm>
#include <cstring>

namespace sdm {

// ---------------------------------------------------------------- frame expansion
constexpr int FX_T = 256, FX_CW = 8;                   // work-items of a strip's workgroup; columns per wavefront at most
constexpr int FX_WMIN = FX_T / 64, FX_WMAX = FX_WMIN * FX_CW;   // strip widths: one column per wavefront ... FX_CW per wavefront
constexpr sdm_int FX_LDS_DEFAULT = 64 * 1024;
static sdm_int g_frame_lds = FX_LDS_DEFAULT;

// one strip: Vr / Vi = its w columns of pitch n (LDS, or the strip's place in the output Q itself).  A template so that each of the two callers
// gets a copy whose accesses to the strip are LDS or global instructions (behind one generic pointer they would all be flat ones)
template <bool IN_LDS, int FX_R>
__device__ __forceinline__ void frame_strip(double *Vr, double *Vi, double *Q, const double *Cr, const double *Ci, const double *beta,
                                            int n, int herm, int j0, int w) {
  const int64_t nn = (int64_t)n * n;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < FX_CW; t++) {
    const int jj = wave + FX_WMIN * t;
    if (jj < w)
      for (int i = lane; i < n; i += 64) { Vr[(int64_t)jj * n + i] = (i == j0 + jj) ? 1.0 : 0.0; if (herm) Vi[(int64_t)jj * n + i] = 0.0; }
  }
  for (int k = min(j0 + w - 1, n - 2); k >= 0; k--) {
    const double rbk = 1.0 / beta[k];
    const double *cr = Cr + (int64_t)k * n, *ci = Ci + (int64_t)k * n;
    // This lane's rows at or below k, FX_R at a time (FX_R = 2, 4, 8: up to 128, 256, more rows in the block).  Straight-line code inside a round: the coefficients of its rows are fetched together,
    // then per column its FX_R entries together (rows outside k .. n-1 read a clamped address against a zero coefficient, and are not written).
    const int first = k & ~63;
    double ar[FX_CW], ai[FX_CW];
#pragma unroll
    for (int t = 0; t < FX_CW; t++) { ar[t] = 0.0; ai[t] = 0.0; }
    for (int base = first + lane; base < n; base += 64 * FX_R) {
      double c_r[FX_R], c_i[FX_R]; int ix[FX_R];
#pragma unroll
      for (int r = 0; r < FX_R; r++) {
        const int i = base + 64 * r;
        const bool ok = i >= k && i < n;
        ix[r] = min(i, n - 1);
        c_r[r] = ok ? cr[ix[r]] : 0.0; c_i[r] = (ok && herm) ? ci[ix[r]] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < FX_CW; t++) {
        const int jj = wave + FX_WMIN * t;
        if (jj < w && j0 + jj >= k) {                                // (uniform over the wavefront; Q_k e_j = e_j for k > j)
          const double *vcr = Vr + (int64_t)jj * n, *vci = Vi + (int64_t)jj * n;
          double vr[FX_R], vi[FX_R];
#pragma unroll
          for (int r = 0; r < FX_R; r++) { vr[r] = vcr[ix[r]]; vi[r] = herm ? vci[ix[r]] : 0.0; }
#pragma unroll
          for (int r = 0; r < FX_R; r++) {
            ar[t] += c_r[r] * vr[r];
            if (herm) { ar[t] += c_i[r] * vi[r]; ai[t] += c_r[r] * vi[r] - c_i[r] * vr[r]; }
          }
        }
      }
    }
    // (all FX_CW sums in one piece of straight-line code, columns the strip does not have included: independent chains the scheduler interleaves)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int t = 0; t < FX_CW; t++) ar[t] += __shfl_xor(ar[t], o);
      if (herm) {
#pragma unroll
        for (int t = 0; t < FX_CW; t++) ai[t] += __shfl_xor(ai[t], o);
      }
    }
#pragma unroll
    for (int t = 0; t < FX_CW; t++) { ar[t] *= rbk; ai[t] *= rbk; }
    for (int base = first + lane; base < n; base += 64 * FX_R) {
      double c_r[FX_R], c_i[FX_R]; int ix[FX_R]; bool ok[FX_R];
#pragma unroll
      for (int r = 0; r < FX_R; r++) {
        const int i = base + 64 * r;
        ok[r] = i >= k && i < n;
        ix[r] = min(i, n - 1);
        c_r[r] = ok[r] ? cr[ix[r]] : 0.0; c_i[r] = (ok[r] && herm) ? ci[ix[r]] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < FX_CW; t++) {
        const int jj = wave + FX_WMIN * t;
        if (jj < w && j0 + jj >= k) {
          double *vcr = Vr + (int64_t)jj * n, *vci = Vi + (int64_t)jj * n;
          double vr[FX_R], vi[FX_R];
#pragma unroll
          for (int r = 0; r < FX_R; r++) { vr[r] = vcr[ix[r]]; vi[r] = herm ? vci[ix[r]] : 0.0; }
#pragma unroll
          for (int r = 0; r < FX_R; r++)
            if (ok[r]) {
              vcr[ix[r]] = vr[r] - (c_r[r] * ar[t] - c_i[r] * ai[t]);
              if (herm) vci[ix[r]] = vi[r] - (c_r[r] * ai[t] + c_i[r] * ar[t]);
            }
        }
      }
    }
  }
  if (!IN_LDS && !herm) return;                                      // already where it belongs
#pragma unroll
  for (int t = 0; t < FX_CW; t++) {
    const int jj = wave + FX_WMIN * t, j = j0 + jj;
    if (jj < w) {
      const double qr = herm ? Cr[(int64_t)(n - 1) * n + j] : 1.0, qi = herm ? Ci[(int64_t)(n - 1) * n + j] : 0.0;   // Qb = ... diag(q)
      for (int i = lane; i < n; i += 64) {
        const double vr = Vr[(int64_t)jj * n + i];
        if (herm) {
          const double vi = Vi[(int64_t)jj * n + i];
          Q[(int64_t)j * n + i] = vr * qr - vi * qi;
          Q[nn + (int64_t)j * n + i] = vr * qi + vi * qr;
        } else Q[(int64_t)j * n + i] = vr;
      }
    }
  }
}

__global__ void __launch_bounds__(FX_T)
k_frame_expand(double *qb, const double *frms, ConeBlk B, const int *strips) {
  SDM_DYN_SMEM(smem);
  const int b = strips[4 * blockIdx.x], j0 = strips[4 * blockIdx.x + 1], w = strips[4 * blockIdx.x + 2], use_lds = strips[4 * blockIdx.x + 3];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *Cr = frms + B.foff[b], *Ci = Cr + nn;
  const double *beta = herm ? Cr + 2 * nn : Cr + nn - n;
  double *Q = qb + B.off[b];
  // the strip: w columns of pitch n, [Re; Im] -- in LDS, or in place in the output
  double *Sr = (double *)smem, *Si = Sr + (int64_t)w * n, *Gr = Q + (int64_t)j0 * n, *Gi = Gr + nn;
  if (use_lds) {
    if (n <= 128) frame_strip<true, 2>(Sr, Si, Q, Cr, Ci, beta, n, herm, j0, w);
    else if (n <= 256) frame_strip<true, 4>(Sr, Si, Q, Cr, Ci, beta, n, herm, j0, w);
    else frame_strip<true, 8>(Sr, Si, Q, Cr, Ci, beta, n, herm, j0, w);
  } else {
    if (n <= 128) frame_strip<false, 2>(Gr, Gi, Q, Cr, Ci, beta, n, herm, j0, w);
    else if (n <= 256) frame_strip<false, 4>(Gr, Gi, Q, Cr, Ci, beta, n, herm, j0, w);
    else frame_strip<false, 8>(Gr, Gi, Q, Cr, Ci, beta, n, herm, j0, w);
  }
}

// ---------------------------------------------------------------- congruence passes
//   MODE 0  X  = Qb^H (diag(lab) Qb)        tiles I >= J, mirrored        psdframeit
//   MODE 1  T1 = Qb Ysym                    Ysym = tril(y) mirrored (conjugated) in the fetch
//   MODE 2  T  = (T1 Qb^H) o jdiv           tiles I >= J, mirrored; diagjdiv folded into the write
//   MODE 3  Z1 = Qb^H T
//   MODE 4  Z  = Z1 Qb                      tiles I >= J, mirrored
template <int MODE>
__global__ void __launch_bounds__(CN_T)
k_cone_gemm(double *out, const double *in, const double *qb, const double *lab, ConeBlk B, const int *items) {
  __shared__ double As[64 * CN_P], Bs[64 * CN_P];
  constexpr bool LOWER = MODE == 0 || MODE == 2 || MODE == 4;       // Hermitian product: tiles I >= J, written twice
  constexpr bool A_KFAST = MODE == 0 || MODE == 3;                   // operand stored with k along its columns: fetch k fastest
  constexpr bool B_KFAST = MODE != 2;
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *Q = qb + B.off[b], *In = in ? in + B.off[b] : nullptr, *x = lab + B.loff[b];
  double *O = out + B.off[b];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = 64 * I, c0 = 64 * J;
  auto Mv = [&](const double *M, int r, int c, int pl) -> double { return (r < n && c < n) ? M[(int64_t)pl * nn + (int64_t)c * n + r] : 0.0; };
  auto Aval = [&](int r, int k, int pl) -> double {
    if (MODE == 0 || MODE == 3) { const double v = Mv(Q, k, r, pl); return pl ? -v : v; }     // Qb^H(r, k) = conj(Qb(k, r))
    if (MODE == 1) return Mv(Q, r, k, pl);
    return Mv(In, r, k, pl);
  };
  auto Bval = [&](int k, int c, int pl) -> double {
    if (MODE == 0) return k < n ? x[k] * Mv(Q, k, c, pl) : 0.0;
    if (MODE == 1) { if (k >= c) return Mv(In, k, c, pl); const double v = Mv(In, c, k, pl); return pl ? -v : v; }   // only tril(y) is read
    if (MODE == 2) { const double v = Mv(Q, c, k, pl); return pl ? -v : v; }                   // Qb^H(k, c)
    if (MODE == 3) return Mv(In, k, c, pl);
    return Mv(Q, k, c, pl);
  };
  const int nplanes = herm ? 2 : 1;
  for (int opl = 0; opl < nplanes; opl++) {
    ConeAcc acc;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc.t[i][j][r] = 0.0;
    // C = A B on planes: Cre = Are Bre - Aim Bim ; Cim = Are Bim + Aim Bre (the conjugates are in the accessors)
    for (int term = 0; term < nplanes; term++) {
      const int apl = term, bpl = opl ^ term;
      const double sgn = (opl == 0 && term == 1) ? -1.0 : 1.0;
      for (int kb = 0; kb < n; kb += 64) {
        __syncthreads();
        for (int e = tid; e < 64 * 64; e += CN_T) {
          const int f = e & 63, s = e >> 6;                           // As[k][row], Bs[k][col]
          { const int k = A_KFAST ? f : s, rr = A_KFAST ? s : f; As[k * CN_P + rr] = sgn * Aval(r0 + rr, kb + k, apl); }
          { const int k = B_KFAST ? f : s, cc = B_KFAST ? s : f; Bs[k * CN_P + cc] = Bval(kb + k, c0 + cc, bpl); }
        }
        __syncthreads();
        cone_mma(acc, As, Bs, wave, lane);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = r0 + 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r, col = c0 + 32 * (wave >> 1) + 16 * j + (lane & 15);
          if (row < n && col < n && (!LOWER || row >= col)) {
            double v = acc.t[i][j][r];
            if (MODE == 2) v = (row == col) ? v / x[row] : v * (2.0 / (x[row] + x[col]));      // diagjdiv, psdinvjmul.c:78-83
            if (LOWER && opl == 1 && row == col) v = 0.0;             // tril2herm: Im diag = 0
            O[(int64_t)opl * nn + (int64_t)col * n + row] = v;
            if (LOWER && row != col) O[(int64_t)opl * nn + (int64_t)row * n + col] = opl ? -v : v;
          }
        }
  }
}

// ---------------------------------------------------------------- triumtriu (updtransfo.m:99, :108)
//   ZZ = triu(X) triu(Y);  Z = ZZ + triu(ZZ, 1)^H                               triumtriu.m:63-64
// The blocking of k_cone_gemm on the tiles I <= J only, and of the k-tiles only K = I .. J: X(r, k) = 0 for k < r and Y(k, c) = 0 for k > c, so
// every other k-tile is zero by structure.  On the diagonal tiles (K = I for X, K = J for Y) the fetch SELECTS 0.0 below the diagonal: the
// strict lower triangle of neither operand is read (urotorder and psdfactor leave a mirrored copy there; whatever is there stays out of the
// arithmetic).  Every entry with row <= col is written to (row, col) and, conjugated, to (col, row); the diagonal as computed on both planes --
// triumtriu.m does not zero its imaginary part.  A tile is formed by one workgroup on its own: no hand-over between workgroups, no counters, no
// atomics, and a block's bits depend on nothing but the block.  Tiles are dealt longest k loop first (cone_tables).
__global__ void __launch_bounds__(CN_T)
k_triumtriu(double *out, const double *xin, const double *yin, ConeBlk B, const int *items) {
  __shared__ double As[64 * CN_P], Bs[64 * CN_P];
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *X = xin + B.off[b], *Y = yin + B.off[b];
  double *O = out + B.off[b];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = 64 * I, c0 = 64 * J;
  // triu(M)(r, c): the entry for r <= c inside the block, 0.0 (not fetched) elsewhere
  auto Uv = [&](const double *M, int r, int c, int pl) -> double { return (r <= c && c < n) ? M[(int64_t)pl * nn + (int64_t)c * n + r] : 0.0; };
  const int nplanes = herm ? 2 : 1;
  for (int opl = 0; opl < nplanes; opl++) {
    ConeAcc acc;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc.t[i][j][r] = 0.0;
    // Z = X Y on planes: Zre = Xre Yre - Xim Yim ; Zim = Xre Yim + Xim Yre
    for (int term = 0; term < nplanes; term++) {
      const int apl = term, bpl = opl ^ term;
      const bool neg = opl == 0 && term == 1;
      for (int kb = r0; kb <= c0; kb += 64) {
        __syncthreads();
        for (int e = tid; e < 64 * 64; e += CN_T) {
          const int f = e & 63, s = e >> 6;                           // As[k][row]: row fastest; Bs[k][col]: k fastest (as stored)
          { const double v = Uv(X, r0 + f, kb + s, apl); As[s * CN_P + f] = neg ? -v : v; }
          Bs[f * CN_P + s] = Uv(Y, kb + f, c0 + s, bpl);
        }
        __syncthreads();
        cone_mma(acc, As, Bs, wave, lane);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = r0 + 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r, col = c0 + 32 * (wave >> 1) + 16 * j + (lane & 15);
          if (row <= col && col < n) {
            const double v = acc.t[i][j][r];
            O[(int64_t)opl * nn + (int64_t)col * n + row] = v;
            if (row != col) O[(int64_t)opl * nn + (int64_t)row * n + col] = opl ? -v : v;
          }
        }
  }
}

// ---------------------------------------------------------------- psdjmul (wregion.m's corrector)
//   ZZ = X Y;  Z = (ZZ + ZZ^H) / 2                                              psdjmul.m:40-73
// The blocking of k_triumtriu on the tiles I <= J, without the triangle structure: the full blocks of x and y are read (no symmetry assumed, Im of
// a Hermitian block's diagonal included) over all nt k-tiles.  (X Y)^H = Y^H X^H, so tile (I, J) of 2 Z is
//   sum_k  X(I, k) Y(k, J)  +  Y(k, I)^H X(J, k)^H
// ONE accumulator per output plane over 2 nt k-tiles and no transposition through LDS: the second term stages As[k][row] = conj Y(k, r0 + row),
// Bs[k][col] = conj X(c0 + col, k).  On planes (the signs go in with the staging of As)
//   Re = Xr Yr - Xi Yi + Yr^T Xr^T - Yi^T Xi^T          Im = Xr Yi + Xi Yr - Yr^T Xi^T - Yi^T Xr^T
// Every operand is fetched along its stored column: row fastest for X(I, k) and X(J, k)^H's columns, k fastest for Y(k, J) and Y(k, I).  Rows and
// columns beyond n are staged as 0.0 and not fetched.  Entries with row <= col are halved (exact) and written to (row, col) and, conjugated, to
// (col, row) -- on a diagonal tile (r, c) and (c, r) are summed in different orders, hence the mirror there too; Im of a Hermitian diagonal, which
// the .m file gets as a + (-a), is written as 0.0.  A tile is formed by one workgroup on its own: no hand-over between workgroups, no counters, no
// atomics, and a block's bits depend on nothing but the block.  Every tile has the same k loop: the order of T.items_up does not matter here.
__global__ void __launch_bounds__(CN_T)
k_psdjmul(double *out, const double *xin, const double *yin, ConeBlk B, const int *items) {
  __shared__ double As[64 * CN_P], Bs[64 * CN_P];
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  const double *X = xin + B.off[b], *Y = yin + B.off[b];
  double *O = out + B.off[b];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = 64 * I, c0 = 64 * J;
  const int nplanes = herm ? 2 : 1;
  for (int opl = 0; opl < nplanes; opl++) {
    ConeAcc acc;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc.t[i][j][r] = 0.0;
    for (int term = 0; term < nplanes; term++) {
      const int apl = term, bpl = opl ^ term;
      // half 0: X Y on planes, Re = Xr Yr - Xi Yi ; Im = Xr Yi + Xi Yr.  half 1: Y^H X^H with A = conj Y^T (planes Yr^T, -Yi^T) and B = conj X^T
      // (Xr^T, -Xi^T): Re = Yr^T Xr^T - Yi^T Xi^T ; Im = -Yr^T Xi^T - Yi^T Xr^T
      for (int half = 0; half < 2; half++) {
        const bool neg = half ? !(opl == 0 && term == 0) : (opl == 0 && term == 1);
        const double *Am = (half ? Y : X) + (int64_t)apl * nn, *Bm = (half ? X : Y) + (int64_t)bpl * nn;
        const int ar = half ? 0 : r0, ac = half ? r0 : 0, br = half ? c0 : 0, bc = half ? 0 : c0;    // where the tile begins; kb goes on the other index
        const int ap = half ? CN_P : 1, aq = half ? 1 : CN_P, bp = half ? 1 : CN_P, bq = half ? CN_P : 1;
        for (int kb = 0; kb < n; kb += 64) {
          // f runs along the stored column of both operands; all 32 fetches of a work-item are issued before the first is stored
          // half 0: As[k = s][row = f] = X(r0 + f, kb + s), Bs[k = f][col = s] = Y(kb + f, c0 + s)
          // half 1: As[k = f][row = s] = Y(kb + f, r0 + s), Bs[k = s][col = f] = X(c0 + f, kb + s)
          const int f = tid & 63;
          const int arow = ar + (half ? kb : 0) + f, brow = br + (half ? 0 : kb) + f;
          double va[16], vb[16];
#pragma unroll
          for (int t = 0; t < 16; t++) {
            const int s = (tid >> 6) + 4 * t;
            const int acol = ac + (half ? 0 : kb) + s, bcol = bc + (half ? kb : 0) + s;
            va[t] = (arow < n && acol < n) ? Am[(int64_t)acol * n + arow] : 0.0;
            vb[t] = (brow < n && bcol < n) ? Bm[(int64_t)bcol * n + brow] : 0.0;
          }
          __syncthreads();
#pragma unroll
          for (int t = 0; t < 16; t++) {
            const int s = (tid >> 6) + 4 * t;
            As[f * ap + s * aq] = neg ? -va[t] : va[t];
            Bs[f * bp + s * bq] = vb[t];
          }
          __syncthreads();
          cone_mma(acc, As, Bs, wave, lane);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = r0 + 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r, col = c0 + 32 * (wave >> 1) + 16 * j + (lane & 15);
          if (row <= col && col < n) {
            const double v = (opl == 1 && row == col) ? 0.0 : 0.5 * acc.t[i][j][r];
            O[(int64_t)opl * nn + (int64_t)col * n + row] = v;
            O[(int64_t)opl * nn + (int64_t)row * n + col] = (opl == 1 && row != col) ? -v : v;       // (the diagonal: the same value to the same place again)
          }
        }
  }
}

// =========================================================================== host
void cone_set_frame_lds_budget(sdm_int bytes) {
  if (bytes < 0 || bytes > FX_LDS_DEFAULT) throw std::runtime_error("frame LDS budget: 0 (default) .. 65536 bytes");
  g_frame_lds = bytes ? bytes : FX_LDS_DEFAULT;
}

// block tables, tile lists and the strips of the expansion for the PSD blocks `ns` (the first rsdpN real, the others Hermitian)
void cone_tables(ConeTabs &T, const std::vector<int> &ns, int rsdpN, int n_ud, int n_fr, int n_lab, int64_t extra) {
  const int nb = (int)ns.size();
  std::vector<int> bn(std::max(nb, 1), 0), bh(std::max(nb, 1), 0), bl(std::max(nb, 1), 0), full, low;
  std::vector<int64_t> bo(std::max(nb, 1), 0), bf(std::max(nb, 1), 0);
  struct Strip { int b, j0, w, lds; double cost; };
  std::vector<Strip> st;
  struct Tile { int b, I, J, cost; };
  std::vector<Tile> ut;
  int64_t o = 0, fo = 0; int lo = 0;
  T.lds = 0;
  for (int k = 0; k < nb; k++) {
    const int n = ns[k], planes = k < rsdpN ? 1 : 2;
    if (n < 0) throw std::runtime_error("K.s: negative order");
    bn[k] = n; bh[k] = planes - 1; bo[k] = o; bf[k] = fo; bl[k] = lo;
    o += (int64_t)planes * n * n; fo += (int64_t)planes * n * n + (planes == 2 ? n : 0); lo += n;
    const int nt = (n + 63) / 64;
    for (int I = 0; I < nt; I++)
      for (int J = 0; J < nt; J++) {
        full.insert(full.end(), {k, I, J, 0});
        if (I >= J) low.insert(low.end(), {k, I, J, 0});
        if (I <= J) ut.push_back({k, I, J, (J - I + 1) * planes * planes});   // k-tiles I .. J, on every pair of planes
      }
    // strip width from the LDS budget: as many columns as fit, a multiple of the wavefronts, FX_WMAX at most; fewer than FX_WMIN: in global memory
    const int64_t colbytes = (int64_t)planes * std::max(n, 1) * (int64_t)sizeof(double);
    const int fit = (int)std::min<int64_t>(g_frame_lds / colbytes, FX_WMAX) / FX_WMIN * FX_WMIN;
    const int w = fit >= FX_WMIN ? fit : FX_WMIN, lds = fit >= FX_WMIN ? 1 : 0;
    for (int j0 = 0; j0 < n; j0 += w) {
      Strip s{k, j0, std::min(w, n - j0), lds, 0.0};
      for (int j = j0; j < j0 + s.w; j++) { const double K = std::min(j, n - 2) + 1; s.cost += K * n - K * (K - 1) / 2; }
      if (lds) T.lds = std::max(T.lds, (size_t)(s.w * colbytes));
      st.push_back(s);
    }
  }
  std::stable_sort(st.begin(), st.end(), [](const Strip &a, const Strip &b) { return a.cost > b.cost; });   // longest first
  std::vector<int> strips;
  for (const Strip &s : st) strips.insert(strips.end(), {s.b, s.j0, s.w, s.lds});
  std::stable_sort(ut.begin(), ut.end(), [](const Tile &a, const Tile &b) { return a.cost > b.cost; });     // longest first
  std::vector<int> up;
  for (const Tile &t : ut) up.insert(up.end(), {t.b, t.I, t.J, 0});
  T.nfull = (int)full.size() / 4; T.nlow = (int)low.size() / 4; T.nstrips = (int)strips.size() / 4; T.nup = (int)up.size() / 4;
  if (full.empty()) full.assign(4, 0);
  if (low.empty()) low.assign(4, 0);
  if (strips.empty()) strips.assign(4, 0);
  if (up.empty()) up.assign(4, 0);
  // one allocation, one copy: [off, foff | n, herm, loff, tiles, tiles I >= J, strips, tiles I <= J (int32, padded to 8 bytes) | the caller's doubles]
  std::vector<int> ints;
  const size_t o_n = 0, o_h = o_n + bn.size(), o_l = o_h + bh.size(), o_f = o_l + bl.size(), o_w = o_f + full.size(), o_s = o_w + low.size(),
               o_u = o_s + strips.size();
  for (const std::vector<int> *v : {&bn, &bh, &bl, &full, &low, &strips, &up}) ints.insert(ints.end(), v->begin(), v->end());
  if (ints.size() & 1) ints.push_back(0);
  std::vector<int64_t> img(bo);
  img.insert(img.end(), bf.begin(), bf.end());
  const size_t w_int = img.size(), w_dat = w_int + ints.size() / 2;
  img.resize(w_dat);
  memcpy(img.data() + w_int, ints.data(), ints.size() * sizeof(int));
  T.arena.alloc(w_dat + (size_t)(n_ud * o + n_fr * fo + n_lab * lo + extra));
  SDM_HIP_CHECK(hipMemcpy(T.arena.p, img.data(), w_dat * sizeof(int64_t), hipMemcpyHostToDevice));
  T.off = T.arena.p; T.foff = T.arena.p + bo.size();
  const int *ip = (const int *)(T.arena.p + w_int);
  T.n = ip + o_n; T.herm = ip + o_h; T.loff = ip + o_l; T.items_full = ip + o_f; T.items_low = ip + o_w; T.strips = ip + o_s; T.items_up = ip + o_u;
  T.data = (double *)(T.arena.p + w_dat);
  T.lenud = o; T.lenfr = fo; T.lenlab = lo;
}

// qb (lenud doubles, device) = the explicit Qb of the Householder frames frms (lenud + hLen doubles, device)
void cone_expand(sdm_plan *P, const ConeTabs &T, const double *frms, double *qb) {
  if (T.nstrips == 0) return;
  SDM_KLAUNCH(P, k_frame_expand, dim3(T.nstrips), dim3(FX_T), T.lds, qb, frms, cone_blk(T), T.strips);
  SDM_HIP_CHECK(hipGetLastError());
}
// x = Qb^H diag(lab) Qb per block; everything on the device
void cone_frameit(sdm_plan *P, const ConeTabs &T, const double *qb, const double *lab, double *x) {
  if (T.nlow == 0) return;
  SDM_KLAUNCH(P, k_cone_gemm<0>, dim3(T.nlow), dim3(CN_T), 0, x, (const double *)nullptr, qb, lab, cone_blk(T), T.items_low);
  SDM_HIP_CHECK(hipGetLastError());
}
// z = Qb^H ((Qb Ysym Qb^H) o 2/(x_i + x_j)) Qb per block; t1, t2: scratch of lenud doubles each
void cone_invjmul(sdm_plan *P, const ConeTabs &T, const double *qb, const double *xlab, const double *y, double *t1, double *t2, double *z) {
  if (T.nlow == 0) return;
  const ConeBlk B = cone_blk(T);
  SDM_KLAUNCH(P, k_cone_gemm<1>, dim3(T.nfull), dim3(CN_T), 0, t1, y, qb, xlab, B, T.items_full);
  SDM_KLAUNCH(P, k_cone_gemm<2>, dim3(T.nlow), dim3(CN_T), 0, t2, (const double *)t1, qb, xlab, B, T.items_low);
  SDM_KLAUNCH(P, k_cone_gemm<3>, dim3(T.nfull), dim3(CN_T), 0, t1, (const double *)t2, qb, xlab, B, T.items_full);
  SDM_KLAUNCH(P, k_cone_gemm<4>, dim3(T.nlow), dim3(CN_T), 0, z, (const double *)t1, qb, xlab, B, T.items_low);
  SDM_HIP_CHECK(hipGetLastError());
}
// z = triu(x) triu(y) + the conjugate mirror of its strict upper triangle, per block; everything on the device, z distinct from x and y
void cone_triumtriu(sdm_plan *P, const ConeTabs &T, const double *x, const double *y, double *z) {
  if (T.nup == 0) return;
  SDM_KLAUNCH(P, k_triumtriu, dim3(T.nup), dim3(CN_T), 0, z, x, y, cone_blk(T), T.items_up);
  SDM_HIP_CHECK(hipGetLastError());
}
// z = (x y + (x y)^H) / 2 per block; everything on the device, z distinct from x and y
void cone_psdjmul(sdm_plan *P, const ConeTabs &T, const double *x, const double *y, double *z) {
  if (T.nup == 0) return;
  SDM_KLAUNCH(P, k_psdjmul, dim3(T.nup), dim3(CN_T), 0, z, x, y, cone_blk(T), T.items_up);
  SDM_HIP_CHECK(hipGetLastError());
}

}  // namespace sdm
