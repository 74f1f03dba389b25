// sdm_psdfact.hip -- psdfactor.m:44-80 and psdinvscale.m:40-83 on the device: the Cholesky factor of every PSD block and the
// two-sided triangular solve with it, what the line search runs once per trial step (trydif.m:62-63, widelen.m:101-103, maxstep.m:63).
//   psdfactor     X = L L^H per block, computed lower; the result is L + tril(L,-1)^H (Hermitian blocks: Im diag = 0.0).  Only the lower triangle
//                 of x and the real part of its diagonal are read, as chol(XX,'lower') does.
//   psdinvscale   Y = T^{-1} X T^{-H}, T = triu(ud): only the upper triangle of ud is read (its diagonal on both planes, as stored); no symmetry
//                 of X is assumed; Im diag(Y) = 0.0 on Hermitian blocks (psdinvscale.m:79).
// Blocks are column major, Hermitian blocks [Re; Im] planes, tiles 64 x 64, work lists of 4-int items built on the host (psdfact_plan); the block
// tables are cone_tables', the matrix-core blocking is cone_mma's (sdm_cone_dev.h).
//
// Both are tile algorithms over ALL blocks at once, one launch per step and kind of tile; blocks that have no tile column / row of that index drop
// out of the step's list.  Every dependency is stream order between launches: no spin waits, no flags another workgroup polls, no counters, no
// atomics; a workgroup forms its tile on its own, and a block's bits depend on nothing but the block.
//
// psdfactor, left-looking by tile column J, in place on a copy of x -- two launches per tile column (the update merged into both):
//   k_chol_diag    one workgroup per block: A(J,J) -= sum_{K<J} L(J,K) L(J,K)^H on the matrix cores, then the unblocked Cholesky of the tile in LDS
//   k_chol_panel   one workgroup per tile I > J: A(I,J) -= sum_{K<J} L(I,K) L(J,K)^H on the matrix cores, then L(I,J) = A(I,J) L(J,J)^{-H} by
//                  substitution against L(J,J) in LDS, a lane owning a row
// Every L entry is stored at (r, c) and, conjugated, at (c, r): the strict upper triangle is only ever written, so what x holds there (and in the
// imaginary part of its diagonal) never enters the arithmetic.  A pivot that is not > 0 (<= 0 or NaN: LAPACK's rule) makes the workgroup that owns
// the diagonal tile store the block's flag (a plain store) and leave; every later launch reads the flag of its block at entry and returns, the
// whole workgroup alike.  The host reads the flags once, after the last launch.
//
// psdinvscale, two passes in place on a copy of x, one launch per tile column / row (2 nt in all):
//   k_invscale<1>  W T^H = X by tile columns J = nt-1 .. 0:  W(I,J) = (X(I,J) - sum_{K>J} W(I,K) T(J,K)^H) T(J,J)^{-H}, a lane owning a row
//   k_invscale<2>  T Y = W   by tile rows    I = nt-1 .. 0:  Y(I,J) = T(I,I)^{-1} (W(I,J) - sum_{K>I} T(I,K) Y(K,J)),   a lane owning a column
//                  (Im diag(Y) = 0.0 is made in the last step, I = 0: the steps before it read the diagonal tiles as computed)
// the tile sums on the matrix cores, then substitution against the diagonal tile in LDS.  A zero on diag(T) gives what the division gives.
//
// Entries of a tile are always obtained by SUBSTITUTION against the diagonal tile, never by a product with an inverted one: the componentwise
// backward error bounds of a triangular solve (Higham, Accuracy and Stability, Lemma 8.4, Thm 10.3) then hold for any order of the sums.
#include "sdm_plan.h"
#include "sdm_cone_dev.h"
#include <algorithm>
#include <cstring>

namespace sdm {

// LDS of a workgroup: the staging tiles of cone_mma, which later hold the diagonal tile D (Re, Im), and the tile being formed C (Re, Im)
struct FactLds { double *a, *b, *cr, *ci; };

// acc[pl] = plane pl of sum_k A(r, k) conj(B(c, k)) over k = k0 .. k1-1 (k0 a multiple of 64), r and c inside the 64 x 64 tile.
// Aval(r, k, pl), Bval(c, k, pl): the operands' planes, 0.0 outside the block.  B_KFAST: B is stored with k along its columns.
//   Re = Are Bre^T + Aim Bim^T ;  Im = Aim Bre^T - Are Bim^T
template <bool B_KFAST, class FA, class FB>
__device__ __forceinline__ void fact_tile_sum(ConeAcc *acc, const FactLds &S, int herm, int k0, int k1, FA Aval, FB Bval) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nplanes = herm ? 2 : 1;
#pragma unroll
  for (int opl = 0; opl < 2; opl++) {                                  // (unrolled: acc[opl] stays in registers)
    if (opl >= nplanes) continue;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[opl].t[i][j][r] = 0.0;
    for (int term = 0; term < nplanes; term++) {
      const int apl = opl ^ term, bpl = term;
      const bool neg = opl == 1 && term == 1;                          // - Are Bim^T
      for (int kb = k0; kb < k1; kb += 64) {
        __syncthreads();
        for (int e = tid; e < 64 * 64; e += CN_T) {
          const int f = e & 63, s = e >> 6;                             // As[k][row]: row fastest, as stored
          { const double v = Aval(f, kb + s, apl); S.a[s * CN_P + f] = neg ? -v : v; }
          { const int k = B_KFAST ? f : s, c = B_KFAST ? s : f; S.b[k * CN_P + c] = Bval(c, kb + k, bpl); }
        }
        __syncthreads();
        cone_mma(acc[opl], S.a, S.b, wave, lane);
      }
    }
  }
}

// C = M - acc into LDS, C(r, c) at [r * CN_P + c], or -- OWN_COL -- at [c * CN_P + r]: the lane that owns a row (column) walks its own LDS row.
// Mval(r, c, pl): the tile of the matrix in global memory, 0.0 outside the block
template <bool OWN_COL, class FM>
__device__ __forceinline__ void fact_tile_rest(const ConeAcc *acc, const FactLds &S, int herm, FM Mval) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  __syncthreads();
#pragma unroll
  for (int opl = 0; opl < 2; opl++) {
    if (opl && !herm) continue;
    double *C = opl ? S.ci : S.cr;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 32 * (wave & 1) + 16 * i + (lane >> 4) + 4 * r, col = 32 * (wave >> 1) + 16 * j + (lane & 15);
          C[OWN_COL ? col * CN_P + row : row * CN_P + col] = Mval(row, col, opl) - acc[opl].t[i][j][r];
        }
  }
}

// The m unknowns x_0 .. x_{m-1} of the calling lane, in place in its LDS row C[own * CN_P + .]:   sum_k x_k d(c, k) = rhs_c,
//   d(c, k) = D[c * CN_P + k], conjugated with CONJ; the triangle k <= c (FWD: c = 0 .. m-1) or k >= c (c = m-1 .. 0).
// REAL_DIAG: the diagonal of D is real (a Cholesky factor): one real division per plane; else the complex quotient, formed as it is written.
template <bool FWD, bool CONJ, bool REAL_DIAG>
__device__ __forceinline__ void fact_subst(const FactLds &S, int own, int m, int herm) {
  double *xr = S.cr + own * CN_P, *xi = S.ci + own * CN_P;
  const double *Dr = S.a, *Di = S.b;
  for (int t = 0; t < m; t++) {
    const int c = FWD ? t : m - 1 - t;
    const int ka = FWD ? 0 : c + 1, kb = FWD ? c : m;
    const double *dr = Dr + c * CN_P, *di = Di + c * CN_P;
    double sr = xr[c], si = herm ? xi[c] : 0.0;
    if (!herm) {
      for (int k = ka; k < kb; k++) sr -= xr[k] * dr[k];
      xr[c] = sr / dr[c];
    } else {
      for (int k = ka; k < kb; k++) {
        const double tr = dr[k], ti = CONJ ? -di[k] : di[k];
        sr -= xr[k] * tr; sr += xi[k] * ti;                           // x t: Re = xr tr - xi ti
        si -= xr[k] * ti; si -= xi[k] * tr;                           //      Im = xr ti + xi tr
      }
      if (REAL_DIAG) { xr[c] = sr / dr[c]; xi[c] = si / dr[c]; }
      else {
        const double pr = dr[c], pi = CONJ ? -di[c] : di[c], den = pr * pr + pi * pi;
        xr[c] = (sr * pr + si * pi) / den;
        xi[c] = (si * pr - sr * pi) / den;
      }
    }
  }
}

#define SDM_FACT_LDS(S)                                                                              \
  __shared__ double fact_a_[64 * CN_P], fact_b_[64 * CN_P], fact_cr_[64 * CN_P], fact_ci_[64 * CN_P]; \
  FactLds S; S.a = fact_a_; S.b = fact_b_; S.cr = fact_cr_; S.ci = fact_ci_

// ---------------------------------------------------------------- psdfactor
// items: (block, J, -, -).  a: the working copy of x, L where it is final
__global__ void __launch_bounds__(CN_T)
k_chol_diag(double *a, ConeBlk B, const int *items, int *flags) {
  SDM_FACT_LDS(S);
  const int b = items[4 * blockIdx.x], J = items[4 * blockIdx.x + 1];
  if (flags[b]) return;                                                // (the whole workgroup alike: nothing diverges around a barrier)
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  double *A = a + B.off[b];
  const int tid = threadIdx.x, c0 = 64 * J, m = min(64, n - c0);
  auto Lv = [&](int r, int k, int pl) -> double { return c0 + r < n ? A[(int64_t)pl * nn + (int64_t)k * n + c0 + r] : 0.0; };   // L(J, K): k < c0 <= row
  ConeAcc acc[2];
  fact_tile_sum<false>(acc, S, herm, 0, c0, Lv, Lv);
  // only the lower triangle of the tile and the real part of its diagonal are fetched
  fact_tile_rest<false>(acc, S, herm, [&](int r, int c, int pl) -> double {
    return (r < m && c <= r && !(pl && r == c)) ? A[(int64_t)pl * nn + (int64_t)(c0 + c) * n + c0 + r] : 0.0; });
  __syncthreads();
  // unblocked right-looking Cholesky of the m x m tile: per column the pivot, the column scaled by a division, the rank-1 update of what is right of it
  bool bad = false;
  for (int k = 0; k < m; k++) {
    const double d = S.cr[k * CN_P + k];                               // (everybody reads the same value: the decision is uniform)
    if (!(d > 0.0)) { bad = true; break; }
    const double l = sqrt(d);
    if (tid > k && tid < m) { S.cr[tid * CN_P + k] /= l; if (herm) S.ci[tid * CN_P + k] /= l; }
    __syncthreads();
    if (tid == k) S.cr[k * CN_P + k] = l;                              // (nothing below reads (k, k), and d is in everybody's register)
    for (int e = tid; e < 64 * 64; e += CN_T) {
      const int r = e & 63, c = e >> 6;
      if (c > k && r >= c && r < m) {
        const double ar = S.cr[r * CN_P + k], br = S.cr[c * CN_P + k];
        if (!herm) S.cr[r * CN_P + c] -= ar * br;
        else {
          const double ai = S.ci[r * CN_P + k], bi = S.ci[c * CN_P + k];
          double vr = S.cr[r * CN_P + c], vi = S.ci[r * CN_P + c];
          vr -= ar * br; vr -= ai * bi;                                // a conj(b): Re = ar br + ai bi
          vi -= ai * br; vi += ar * bi;                                //            Im = ai br - ar bi
          S.cr[r * CN_P + c] = vr; S.ci[r * CN_P + c] = vi;
        }
      }
    }
    __syncthreads();
  }
  if (bad) { if (tid == 0) flags[b] = 1; return; }
  for (int e = tid; e < 64 * 64; e += CN_T) {
    const int r = e & 63, c = e >> 6;
    if (r < m && c <= r)
      for (int pl = 0; pl <= herm; pl++) {
        const double v = (pl && r == c) ? 0.0 : (pl ? S.ci : S.cr)[r * CN_P + c];
        A[(int64_t)pl * nn + (int64_t)(c0 + c) * n + c0 + r] = v;
        if (r != c) A[(int64_t)pl * nn + (int64_t)(c0 + r) * n + c0 + c] = pl ? -v : v;
      }
  }
}

// items: (block, I, J, -), I > J
__global__ void __launch_bounds__(CN_T)
k_chol_panel(double *a, ConeBlk B, const int *items, const int *flags) {
  SDM_FACT_LDS(S);
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  if (flags[b]) return;
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  double *A = a + B.off[b];
  const int tid = threadIdx.x, r0 = 64 * I, c0 = 64 * J, mr = min(64, n - r0);      // (tile column J < I is whole)
  auto Av = [&](int r, int k, int pl) -> double { return r0 + r < n ? A[(int64_t)pl * nn + (int64_t)k * n + r0 + r] : 0.0; };
  auto Bv = [&](int c, int k, int pl) -> double { return A[(int64_t)pl * nn + (int64_t)k * n + c0 + c]; };
  ConeAcc acc[2];
  fact_tile_sum<false>(acc, S, herm, 0, c0, Av, Bv);
  fact_tile_rest<false>(acc, S, herm, [&](int r, int c, int pl) -> double { return r < mr ? A[(int64_t)pl * nn + (int64_t)(c0 + c) * n + r0 + r] : 0.0; });
  // L(J, J), lower triangle (its diagonal is real), over the staging tiles: the last cone_mma is behind the barrier of fact_tile_rest
  for (int e = tid; e < 64 * 64; e += CN_T) {
    const int r = e & 63, c = e >> 6;
    if (c <= r) {
      S.a[r * CN_P + c] = A[(int64_t)(c0 + c) * n + c0 + r];
      if (herm) S.b[r * CN_P + c] = A[nn + (int64_t)(c0 + c) * n + c0 + r];
    }
  }
  __syncthreads();
  if (tid < mr) fact_subst<true, true, true>(S, tid, 64, herm);
  __syncthreads();
  for (int pl = 0; pl <= herm; pl++) {
    const double *C = pl ? S.ci : S.cr;
    for (int e = tid; e < 64 * 64; e += CN_T) {                        // (r, c): row fastest
      const int r = e & 63, c = e >> 6;
      if (r < mr) A[(int64_t)pl * nn + (int64_t)(c0 + c) * n + r0 + r] = C[r * CN_P + c];
    }
    for (int e = tid; e < 64 * 64; e += CN_T) {                        // the mirror (c, r): c fastest
      const int c = e & 63, r = e >> 6;
      if (r < mr) { const double v = C[r * CN_P + c]; A[(int64_t)pl * nn + (int64_t)(r0 + r) * n + c0 + c] = pl ? -v : v; }
    }
  }
}

// ---------------------------------------------------------------- psdinvscale
// items: (block, I, J, -); y: X on entry, W behind pass 1, Y behind pass 2
template <int PASS>
__global__ void __launch_bounds__(CN_T)
k_invscale(double *y, const double *ud, ConeBlk B, const int *items) {
  SDM_FACT_LDS(S);
  const int b = items[4 * blockIdx.x], I = items[4 * blockIdx.x + 1], J = items[4 * blockIdx.x + 2];
  const int n = B.n[b], herm = B.herm[b];
  const int64_t nn = (int64_t)n * n;
  double *Y = y + B.off[b];
  const double *T = ud + B.off[b];
  const int tid = threadIdx.x, r0 = 64 * I, c0 = 64 * J, mr = min(64, n - r0), mc = min(64, n - c0);
  const int d0 = PASS == 1 ? c0 : r0, md = PASS == 1 ? mc : mr;        // the diagonal tile of T the substitution runs against
  auto Yv = [&](int r, int c, int pl) -> double { return (r < n && c < n) ? Y[(int64_t)pl * nn + (int64_t)c * n + r] : 0.0; };
  // T(r, k) for the k-tiles right of the diagonal tile: r < k there, the upper triangle
  auto Tv = [&](int r, int k, int pl) -> double { return (r < n && k < n) ? T[(int64_t)pl * nn + (int64_t)k * n + r] : 0.0; };
  ConeAcc acc[2];
  if (PASS == 1)                                                       // sum_{k} W(r, k) conj(T(c, k))
    fact_tile_sum<false>(acc, S, herm, c0 + 64, n, [&](int r, int k, int pl) -> double { return Yv(r0 + r, k, pl); },
                         [&](int c, int k, int pl) -> double { return Tv(c0 + c, k, pl); });
  else                                                                 // sum_{k} T(r, k) Y(k, c): B(c, k) = conj(Y(k, c))
    fact_tile_sum<true>(acc, S, herm, r0 + 64, n, [&](int r, int k, int pl) -> double { return Tv(r0 + r, k, pl); },
                        [&](int c, int k, int pl) -> double { const double v = Yv(k, c0 + c, pl); return pl ? -v : v; });
  // psdinvscale.m:79 sets Im diag(Y) = 0 once Y is complete: the steps I < J of pass 2 still read Y(J, J) as computed.  Its last reader is this
  // tile (0, J) of the last step, and the only one in this launch: with its tile sum formed (every fetch is behind the barriers of the sum) it
  // zeroes that diagonal; tile (0, 0) zeroes its own when it writes
  if (PASS == 2 && herm && I == 0 && J > 0 && tid < mc) Y[nn + (int64_t)(c0 + tid) * n + c0 + tid] = 0.0;
  fact_tile_rest<PASS == 2>(acc, S, herm, [&](int r, int c, int pl) -> double { return Yv(r0 + r, c0 + c, pl); });
  // the diagonal tile of T, upper triangle with its diagonal on both planes as stored; what lies below it is not fetched
  for (int e = tid; e < 64 * 64; e += CN_T) {
    const int r = e & 63, c = e >> 6;
    if (r <= c && c < md) {
      S.a[r * CN_P + c] = T[(int64_t)(d0 + c) * n + d0 + r];
      if (herm) S.b[r * CN_P + c] = T[nn + (int64_t)(d0 + c) * n + d0 + r];
    }
  }
  __syncthreads();
  if (PASS == 1) { if (tid < mr) fact_subst<false, true, false>(S, tid, md, herm); }
  else if (tid < mc) fact_subst<false, false, false>(S, tid, md, herm);
  __syncthreads();
  for (int pl = 0; pl <= herm; pl++) {
    const double *C = pl ? S.ci : S.cr;
    for (int e = tid; e < 64 * 64; e += CN_T) {
      const int r = e & 63, c = e >> 6;
      if (r < mr && c < mc) {
        double v = C[PASS == 2 ? c * CN_P + r : r * CN_P + c];
        if (PASS == 2 && pl && I == 0 && r == c0 + c) v = 0.0;          // psdinvscale.m:79: Im diag = 0, behind the last step (see above)
        Y[(int64_t)pl * nn + (int64_t)(c0 + c) * n + r0 + r] = v;
      }
    }
  }
}

// =========================================================================== host
// the launches of both functions for the PSD blocks `ns` and the image of their item lists
void psdfact_plan(PsdFactPlan &S, const std::vector<int> &ns, int rsdpN) {
  (void)rsdpN;
  const int nb = (int)ns.size();
  std::vector<int> items;
  int ntmax = 0;
  for (int b = 0; b < nb; b++) {
    if (ns[b] < 0) throw std::runtime_error("K.s: negative order");
    ntmax = std::max(ntmax, (ns[b] + 63) / 64);
  }
  S.nb = nb; S.ws = (std::max(nb, 1) + 1) / 2;                          // the blocks' flags (int32) in front of the lists
  S.chol.clear(); S.pass1.clear(); S.pass2.clear();
  for (int J = 0; J < ntmax; J++) {
    PsdFactPlan::Step st{};
    st.first0 = (int)items.size() / 4;
    for (int b = 0; b < nb; b++)
      if (64 * J < ns[b]) items.insert(items.end(), {b, J, 0, 0});
    st.nfirst = (int)items.size() / 4 - st.first0; st.second0 = (int)items.size() / 4;
    for (int b = 0; b < nb; b++)
      for (int I = J + 1; 64 * I < ns[b]; I++) items.insert(items.end(), {b, I, J, 0});
    st.nsecond = (int)items.size() / 4 - st.second0;
    S.chol.push_back(st);
  }
  for (int pass = 1; pass <= 2; pass++)
    for (int t = ntmax - 1; t >= 0; t--) {                              // tile column J = t (pass 1), tile row I = t (pass 2), last first
      PsdFactPlan::Step st{};
      st.first0 = (int)items.size() / 4;
      for (int b = 0; b < nb; b++)
        if (64 * t < ns[b])
          for (int o = 0; 64 * o < ns[b]; o++) items.insert(items.end(), {b, pass == 1 ? o : t, pass == 1 ? t : o, 0});
      st.nfirst = (int)items.size() / 4 - st.first0;
      (pass == 1 ? S.pass1 : S.pass2).push_back(st);
    }
  if (items.size() & 1) items.push_back(0);
  S.img.assign(items.size() / 2, 0);
  if (!items.empty()) memcpy(S.img.data(), items.data(), items.size() * sizeof(int));
}

static const int *psdfact_upload(const PsdFactPlan &S, double *area) {
  int64_t *tab = (int64_t *)(area + S.ws);
  if (!S.img.empty()) SDM_HIP_CHECK(hipMemcpy(tab, S.img.data(), S.img.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  return (const int *)tab;
}

// a (lenud doubles, device, holding x on entry) = L + tril(L,-1)^H of every block whose flag stays 0; area: S.words() doubles on the device
void psdfactor_run(sdm_plan *P, const ConeTabs &T, const PsdFactPlan &S, double *area, double *a) {
  const int *items = psdfact_upload(S, area);
  int *flags = (int *)area;
  SDM_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)S.ws * sizeof(double), P->stream));
  const ConeBlk B = cone_blk(T);
  for (const PsdFactPlan::Step &st : S.chol) {
    if (st.nfirst) SDM_KLAUNCH(P, k_chol_diag, dim3(st.nfirst), dim3(CN_T), 0, a, B, items + 4 * st.first0, flags);
    if (st.nsecond) SDM_KLAUNCH(P, k_chol_panel, dim3(st.nsecond), dim3(CN_T), 0, a, B, items + 4 * st.second0, (const int *)flags);
  }
  SDM_HIP_CHECK(hipGetLastError());
}
// the one transfer behind the factorisation: drains the stream and returns the first block that met a pivot that is not > 0, or -1
int psdfactor_first_bad(sdm_plan *P, const PsdFactPlan &S, const double *area) {
  std::vector<int> fl((size_t)std::max(S.nb, 1), 0);
  SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
  SDM_HIP_CHECK(hipMemcpy(fl.data(), area, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int b = 0; b < S.nb; b++)
    if (fl[b]) return b;
  return -1;
}
// y (lenud doubles, device, holding x on entry) = triu(ud)^{-1} X triu(ud)^{-H} of every block
void psdinvscale_run(sdm_plan *P, const ConeTabs &T, const PsdFactPlan &S, double *area, const double *ud, double *y) {
  const int *items = psdfact_upload(S, area);
  const ConeBlk B = cone_blk(T);
  for (const PsdFactPlan::Step &st : S.pass1)
    if (st.nfirst) SDM_KLAUNCH(P, k_invscale<1>, dim3(st.nfirst), dim3(CN_T), 0, y, ud, B, items + 4 * st.first0);
  for (const PsdFactPlan::Step &st : S.pass2)
    if (st.nfirst) SDM_KLAUNCH(P, k_invscale<2>, dim3(st.nfirst), dim3(CN_T), 0, y, ud, B, items + 4 * st.first0);
  SDM_HIP_CHECK(hipGetLastError());
}

}  // namespace sdm
