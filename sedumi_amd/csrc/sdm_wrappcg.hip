// sdm_wrappcg.hip -- one whole normal-equations solve on the resident plan: wrapPcg.m:43-130 with loopPcg.m:52-170 inside it
// (sdm_plan_wrappcg), composed of the operators of sdm_pcg.hip (Amul, vecsym, psdscale), the triangular solves of sdm_solve.hip
// and the vector work below: the Lorentz scaling (asmDxq.m, PopK.m), the reductions and the fused updates of a CG step.
// Only the scalars that pick the next branch come back to the host: once per CG step, one copy of SC_N doubles into pinned
// memory and a stream synchronise.
//   Reductions: every workgroup writes one partial in a fixed order, one workgroup adds the partials in a fixed order
//   (k_wp_finish) and derives the step's scalars from them on the device -- no float atomics, repeated calls give the same bits.
//   The inner products are accumulated in double-double (exact products by Dekker's splitting, error-free sums) and rounded once:
//   the correctly rounded inner product up to O(n u^2), which is what the host loop's BLAS dots give on most calls -- a step
//   length alpha that the host computes to the last bit is then reproduced to the last bit, not only to the reordering error.
//   quadadd (quadadd.c:57-83) is applied to the rounded fl(alpha*p): nothing in this file may be contracted into an FMA.
#include "sdm_plan.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace sdm {

constexpr int WP_T = 256;     // work-items of the vector kernels and of k_wp_finish
constexpr int WP_G = 64;      // most workgroups of a partial reduction
// the loop's scalars on the device (AdaPlan::wp_sc) and in the pinned copy the host reads
enum { SC_SSQRNEW, SC_SSQROLD, SC_BETA, SC_SSQRDAP, SC_ALPHA, SC_FINEW, SC_FIPREV, SC_NORMR, SC_NORMRMIN, SC_BETTER, SC_SSQRDX, SC_N = 12 };
// what k_wp_finish derives from its sums
enum { OP_SSQR_FIRST, OP_SSQR_NEXT, OP_SSQRDX, OP_POPK, OP_RES, OP_NORMRMIN, OP_NORMR };
// segment kinds of k_wp_finish: sum of the values, sum of their squares, largest value
enum { SEG_SUM, SEG_SQR, SEG_MAX };

static int wp_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(WP_G, (n + WP_T - 1) / WP_T)); }

__device__ __forceinline__ double wp_wg_sum(double v, double *red) {     // fixed-order tree over a WP_T workgroup
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = WP_T / 2; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
  const double r = red[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double wp_wg_max(double v, double *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = WP_T / 2; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]); __syncthreads(); }
  const double r = red[0];
  __syncthreads();
  return r;
}
// double-double accumulator (hi + lo, |lo| <= ulp(hi)/2)
struct WpDD { double hi, lo; };
__device__ __forceinline__ WpDD wp_dd_add(WpDD a, WpDD b) {
  const double s = a.hi + b.hi, bb = s - a.hi, e = (a.hi - (s - bb)) + (b.hi - bb);   // two-sum: s + e = a.hi + b.hi exactly
  const double lo = e + (a.lo + b.lo), hi = s + lo;
  return {hi, lo - (hi - s)};
}
// a + x*y with the product kept exactly: x*y = p + e (Dekker / Veltkamp splitting; no FMA in this file)
__device__ __forceinline__ WpDD wp_dd_dot(WpDD a, double x, double y) {
  const double p = x * y, c = 134217729.0;
  double t = c * x;
  const double xh = t - (t - x), xl = x - xh;
  t = c * y;
  const double yh = t - (t - y), yl = y - yh;
  const double e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl;
  return wp_dd_add(a, WpDD{p, e});
}
__device__ __forceinline__ WpDD wp_wg_dd(WpDD v, double *rh, double *rl) {   // fixed-order tree over a WP_T workgroup
  rh[threadIdx.x] = v.hi; rl[threadIdx.x] = v.lo;
  __syncthreads();
  for (int s = WP_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const WpDD r = wp_dd_add(WpDD{rh[threadIdx.x], rl[threadIdx.x]}, WpDD{rh[threadIdx.x + s], rl[threadIdx.x + s]});
      rh[threadIdx.x] = r.hi; rl[threadIdx.x] = r.lo;
    }
    __syncthreads();
  }
  const WpDD r{rh[0], rl[0]};
  __syncthreads();
  return r;
}
__device__ __forceinline__ WpDD wp_wave_dd(WpDD v) {                        // (lane 0's result is the one used)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = wp_dd_add(v, WpDD{__shfl_xor(v.hi, o), __shfl_xor(v.lo, o)});
  return v;
}
// butterfly over one wavefront: every lane ends with the same bits (each level adds the same two values in either order)
__device__ __forceinline__ double wp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---------------------------------------------------------------- reductions
// part[wg] + part[G + wg] (G = the grid) = sum a[i] * b[i] (b null: a[i]^2) over the work-items' strided share, in double-double;
// rounded_sq: the ROUNDED squares fl(a[i]^2) are summed (PopK.m's sum(Dxp.^2), where the host squares first), else exact products (x'*x)
__global__ void __launch_bounds__(WP_T) k_wp_dot(const double *a, const double *b, int64_t n, double *part, int rounded_sq) {
  __shared__ double rh[WP_T], rl[WP_T];
  WpDD s{0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * WP_T)
    s = rounded_sq ? wp_dd_add(s, WpDD{a[i] * a[i], 0.0}) : wp_dd_dot(s, a[i], b ? b[i] : a[i]);
  s = wp_wg_dd(s, rh, rl);
  if (threadIdx.x == 0) { part[blockIdx.x] = s.hi; part[gridDim.x + blockIdx.x] = s.lo; }
}
__global__ void __launch_bounds__(WP_T) k_wp_amax(const double *a, int64_t n, double *part) {
  __shared__ double red[WP_T];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * WP_T) s = fmax(s, fabs(a[i]));
  s = wp_wg_max(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// tmp = Lr ./ L.d with skipped pivots (d = 0) acting as 1 (the k_divd rule, deninfac.m:89-94); part[wg] = its share of Lr' tmp
__global__ void __launch_bounds__(WP_T) k_wp_divd_dot(const double *Lr, const double *d, double *tmp, int64_t m, double *part) {
  __shared__ double rh[WP_T], rl[WP_T];
  WpDD s{0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x; i < m; i += (int64_t)gridDim.x * WP_T) {
    const double dk = d[i], t = Lr[i] / (dk > 0.0 ? dk : 1.0);
    tmp[i] = t;
    s = wp_dd_dot(s, Lr[i], t);
  }
  s = wp_wg_dd(s, rh, rl);
  if (threadIdx.x == 0) { part[blockIdx.x] = s.hi; part[gridDim.x + blockIdx.x] = s.lo; }
}
// one workgroup: up to three segments summed (or maximised) in a fixed order, then the scalars of the step (loopPcg.m / wrapPcg.m).
// SEG_SUM: n double-double partials, hi at s[i] and lo at s[n + i]; SEG_SQR: n values whose rounded squares are summed (np.sum(v.^2));
// SEG_MAX: n values.  Sums stay double-double to the end and are rounded once.
__global__ void __launch_bounds__(WP_T) k_wp_finish(const double *s0, int n0, int k0, const double *s1, int n1, int k1, const double *s2, int n2,
                                                     int k2, double *sc, int op) {
  __shared__ double rh[WP_T], rl[WP_T];
  const double *seg[3] = {s0, s1, s2};
  const int len[3] = {n0, n1, n2}, kind[3] = {k0, k1, k2};
  double v[3] = {0.0, 0.0, 0.0};
  for (int q = 0; q < 3; q++) {
    if (len[q] <= 0) continue;
    if (kind[q] == SEG_MAX) {
      double a = 0.0;
      for (int i = threadIdx.x; i < len[q]; i += WP_T) a = fmax(a, seg[q][i]);
      v[q] = wp_wg_max(a, rh);
      continue;
    }
    WpDD a{0.0, 0.0};
    for (int i = threadIdx.x; i < len[q]; i += WP_T) {
      const double x = seg[q][i];
      a = wp_dd_add(a, kind[q] == SEG_SQR ? WpDD{x * x, 0.0} : WpDD{x, seg[q][len[q] + i]});
    }
    a = wp_wg_dd(a, rh, rl);
    v[q] = a.hi + a.lo;
  }
  if (threadIdx.x != 0) return;
  switch (op) {
    case OP_SSQR_FIRST: sc[SC_SSQRNEW] = v[0]; break;                                      // ssqrNew = Lr'*tmp
    case OP_SSQR_NEXT:                                                                      // loopPcg.m:88-91
      sc[SC_SSQROLD] = sc[SC_SSQRNEW]; sc[SC_SSQRNEW] = v[0]; sc[SC_BETA] = sc[SC_SSQRNEW] / sc[SC_SSQROLD]; break;
    case OP_SSQRDX:                                                                         // wrapPcg.m:66-77
      sc[SC_SSQRDX] = v[0];
      if (v[0] > 0.0) sc[SC_ALPHA] = sc[SC_SSQRNEW] / v[0];
      break;
    case OP_POPK: {                                                                         // PopK.m: xTy; loopPcg.m:99-104
      const double t = (v[0] + v[1]) + v[2];
      sc[SC_SSQRDAP] = t; sc[SC_BETTER] = 0.0;
      if (t > 0.0) sc[SC_ALPHA] = sc[SC_SSQRNEW] / t;
      break;
    }
    case OP_RES:                                                                            // loopPcg.m:127-140
      if (!(sc[SC_SSQRDAP] > 0.0)) break;
      sc[SC_FIPREV] = sc[SC_FINEW];
      sc[SC_FINEW] = n1 > 0 ? v[0] + v[1] : v[0];
      sc[SC_NORMR] = v[2];
      if (v[2] < sc[SC_NORMRMIN]) { sc[SC_BETTER] = 1.0; sc[SC_NORMRMIN] = v[2]; }
      break;
    case OP_NORMRMIN: sc[SC_NORMRMIN] = v[0]; sc[SC_FINEW] = 0.0; sc[SC_BETTER] = 0.0; break;   // loopPcg.m:57-62
    case OP_NORMR: sc[SC_NORMR] = v[0]; break;
  }
}

// ---------------------------------------------------------------- Lorentz scaling (64 work-items per workgroup)
// workgroups [0, nlpb): 64 LP entries each; then one per Lorentz cone k (trace x(l + k), norm-bound rows qblk[k] .. qblk[k+1])
// out[0:lq] = [sqrt(d.l).*x(1:l); asmDxq(d, x, K, ddin)]  (asmDxq.m; ddin null: ddotx = d.q1.*x_trace + ddot(d.q2, x)),
// each entry times *alpha when alpha is given (loopPcg.m:156: alpha*[...])
__global__ void __launch_bounds__(64) k_wp_dx_lq(double *out, const double *x, const double *dl, const double *det, const double *q1, const double *q2,
                                                 const double *auxdet, const double *auxtr, const int64_t *qblk, int l, int nlpb,
                                                 const double *ddin, const double *alpha) {
  const int lane = threadIdx.x;
  const double al = alpha ? *alpha : 1.0;
  if ((int)blockIdx.x < nlpb) {
    const int i = blockIdx.x * 64 + lane;
    if (i < l) { const double v = sqrt(dl[i]) * x[i]; out[i] = alpha ? al * v : v; }
    return;
  }
  const int k = blockIdx.x - nlpb;
  const int64_t b0 = qblk[k], b1 = qblk[k + 1], q0 = qblk[0];
  const double t = x[l + k];
  double dd;
  if (ddin) dd = ddin[k];
  else {
    double s = 0.0;
    for (int64_t i = b0 + lane; i < b1; i += 64) s += q2[i - q0] * x[i];
    dd = q1[k] * t + wp_wave_sum(s);
  }
  const double tt = (dd + t * auxdet[k]) / auxtr[k];
  const double sd = sqrt(det[k]);
  if (lane == 0) { const double v = (tt * auxdet[k] - sd * t) + tt * q1[k]; out[l + k] = alpha ? al * v : v; }
  for (int64_t i = b0 + lane; i < b1; i += 64) { const double v = sd * x[i] + tt * q2[i - q0]; out[i] = alpha ? al * v : v; }
}
// PopK.m on the LP and Lorentz part: y(1:lq) = [d.l.*x(1:l); -d.det.*x_trace; qblkmul(d.det, x)], ddotx = d.q1.*x_trace + ddot(d.q2, x);
// part[wg] + part[G + wg] (G = the grid) = its share of x(1:lq)' y(1:lq) in double-double
__global__ void __launch_bounds__(64) k_wp_popk_lq(double *y, double *ddotx, const double *x, const double *dl, const double *det, const double *q1,
                                                   const double *q2, const int64_t *qblk, int l, int nlpb, double *part) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x < nlpb) {
    const int i = blockIdx.x * 64 + lane;
    WpDD s{0.0, 0.0};
    if (i < l) { const double v = dl[i] * x[i]; y[i] = v; s = wp_dd_dot(s, x[i], v); }
    s = wp_wave_dd(s);
    if (lane == 0) { part[blockIdx.x] = s.hi; part[gridDim.x + blockIdx.x] = s.lo; }
    return;
  }
  const int k = blockIdx.x - nlpb;
  const int64_t b0 = qblk[k], b1 = qblk[k + 1], q0 = qblk[0];
  const double t = x[l + k], dk = det[k];
  WpDD sxy{0.0, 0.0};
  double sq = 0.0;
  for (int64_t i = b0 + lane; i < b1; i += 64) {
    const double v = dk * x[i];
    y[i] = v;
    sxy = wp_dd_dot(sxy, x[i], v);
    sq += q2[i - q0] * x[i];
  }
  sq = wp_wave_sum(sq);
  const double yt = -dk * t;
  if (lane == 0) sxy = wp_dd_dot(sxy, t, yt);
  sxy = wp_wave_dd(sxy);
  if (lane == 0) {
    y[l + k] = yt;
    ddotx[k] = q1[k] * t + sq;
    part[blockIdx.x] = sxy.hi; part[gridDim.x + blockIdx.x] = sxy.lo;
  }
}

// ---------------------------------------------------------------- fused vector updates
// loopPcg.m:87-93: p = pb (first step of a loopPcg without p) or p = (ssqrNew/ssqrOld)*p + pb
__global__ void __launch_bounds__(WP_T) k_wp_pupdate(double *p, const double *pb, int64_t m, const double *sc, int first) {
  const int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x;
  if (i >= m) return;
  p[i] = first ? pb[i] : sc[SC_BETA] * p[i] + pb[i];
}
// (zhi, zlo) = (xhi + xlo) + y in doubled precision: quadadd.c:57-83
__device__ __forceinline__ void wp_quadadd(double xhi, double xlo, double y, double &zhi, double &zlo) {
  if (fabs(y) > fabs(xhi)) {
    zhi = y + xhi;
    zlo = xlo + (xhi - (zhi - y));
  } else {
    const double zlo1 = xlo + y;
    const double xlo2 = xlo - (zlo1 - y);
    zhi = xhi + zlo1;
    zlo = xlo2 + (zlo1 - (zhi - xhi));
  }
}
// one CG step after PopK, when ssqrDAp > 0 (loopPcg.m:103-126): y += alpha*p (quadadd with qprec), r -= alpha*(amr + DAt.q' ddotx)
// with amr = At' DDAp; double-double partials of (b + r)' y.hi at part[wg], part[G + wg] and of (b + r)' y.lo at part[2G + wg],
// part[3G + wg]; norm(r, inf) at part[4G + wg]
__global__ void __launch_bounds__(WP_T) k_wp_step_quadadd(int64_t m, const double *p, double *yhi, double *ylo, double *r, const double *b, const double *amr,
                                                          const int64_t *Qjc, const int *Qir, const double *qpr, const double *ddotx, int nq,
                                                          const double *sc, int first, int qprec, double *part) {
  __shared__ double rh[WP_T], rl[WP_T];
  if (!(sc[SC_SSQRDAP] > 0.0)) return;                                 // (the same for every work-item: STOP = 1 without a step)
  const double al = sc[SC_ALPHA];
  WpDD shi{0.0, 0.0}, slo{0.0, 0.0};
  double mx = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * WP_T + threadIdx.x; j < m; j += (int64_t)gridDim.x * WP_T) {
    const double ap = al * p[j];
    double hi, lo = 0.0;
    if (first) hi = ap;
    else if (qprec) wp_quadadd(yhi[j], ylo[j], ap, hi, lo);
    else hi = yhi[j] + ap;
    yhi[j] = hi;
    if (qprec) ylo[j] = lo;
    double tv = amr[j];
    if (nq > 0) {
      double qv = 0.0;
      for (int64_t t = Qjc[j]; t < Qjc[j + 1]; t++) qv += qpr[t] * ddotx[Qir[t]];
      tv = tv + qv;
    }
    const double rj = r[j] - al * tv;
    r[j] = rj;
    const double br = b[j] + rj;
    shi = wp_dd_dot(shi, br, hi);
    if (qprec) slo = wp_dd_dot(slo, br, lo);
    mx = fmax(mx, fabs(rj));
  }
  shi = wp_wg_dd(shi, rh, rl); slo = wp_wg_dd(slo, rh, rl); mx = wp_wg_max(mx, rh);
  const int G = gridDim.x;
  if (threadIdx.x == 0) {
    part[blockIdx.x] = shi.hi; part[G + blockIdx.x] = shi.lo; part[2 * G + blockIdx.x] = slo.hi; part[3 * G + blockIdx.x] = slo.lo;
    part[4 * G + blockIdx.x] = mx;
  }
}
// ymin = y when the step improved norm(r, inf) (loopPcg.m:130-133)
__global__ void __launch_bounds__(WP_T) k_wp_copy_if(double *dst, const double *src, int64_t n, const double *sc) {
  const int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x;
  if (i < n && sc[SC_BETTER] != 0.0) dst[i] = src[i];
}
// wrapPcg.m:78-80: y = alpha*p ; dx = rv - alpha*dx
__global__ void __launch_bounds__(WP_T) k_wp_first(double *Y, const double *p, int64_t m, double *DX, const double *rv, const double *X, int64_t N, const double *sc) {
  const int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x;
  const double al = sc[SC_ALPHA];
  if (i < m) Y[i] = al * p[i];
  if (i < N) DX[i] = rv[i] - al * X[i];
}
// out = a + b (sub = 0) or a - b (sub = 1); out may be a
__global__ void __launch_bounds__(WP_T) k_wp_add(double *out, const double *a, const double *b, int64_t n, int sub) {
  const int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x;
  if (i < n) out[i] = sub ? a[i] - b[i] : a[i] + b[i];
}
// out = alpha*x
__global__ void __launch_bounds__(WP_T) k_wp_scale(double *out, const double *x, int64_t n, const double *sc) {
  const int64_t i = (int64_t)blockIdx.x * WP_T + threadIdx.x;
  if (i < n) out[i] = sc[SC_ALPHA] * x[i];
}

// =========================================================================== host
namespace {
struct Wrap {
  sdm_plan *P;
  AdaPlan &A;
  int64_t m, N, lq, lenud;
  int l, nq, nlpb;
  bool perm, qprec;
  // m-vectors of the loop, cone-space vectors, the Lorentz and PSD parts of PopK
  double *lr, *Lr, *tmp, *pb, *p, *yhi, *ylo, *ymhi, *ymlo, *amr, *X, *Ap, *DDAp, *DAy, *ddotx, *Dxp;
  double *part, *sc, *host;
  Wrap(sdm_plan *P_, bool use_perm, bool qp) : P(P_), A(P_->ada), perm(use_perm), qprec(qp) {
    m = A.m; N = A.N; lenud = A.lenud; lq = N - lenud; l = (int)A.lpN; nq = (int)A.lorN; nlpb = (l + 63) / 64;
    const int64_t mm = std::max<int64_t>(m, 1), nn = std::max<int64_t>(N, 1);
    const size_t need = (size_t)(10 * mm + 4 * nn + std::max(nq, 1) + std::max<int64_t>(lenud, 1));
    if (A.wp_work.n < need) A.wp_work.alloc(need);                       // (all at the first call: never inside the loop)
    const size_t npart = (size_t)(6 * WP_G + 2 * (nlpb + nq) + 8);
    if (A.wp_part.n < npart) A.wp_part.alloc(npart);
    if (A.wp_sc.n < SC_N) { A.wp_sc.alloc(SC_N); SDM_HIP_CHECK(hipMemsetAsync(A.wp_sc.p, 0, SC_N * sizeof(double), P->stream)); }
    if (A.wp_y.n < (size_t)mm) A.wp_y.alloc(mm);
    if (A.wp_r.n < (size_t)mm) A.wp_r.alloc(mm);
    if (A.wp_dx.n < (size_t)nn) A.wp_dx.alloc(nn);
    A.wp_host.ensure(2 * SC_N);
    double *w = A.wp_work.p;
    double **mv[] = {&lr, &Lr, &tmp, &pb, &p, &yhi, &ylo, &ymhi, &ymlo, &amr};
    for (double **v : mv) { *v = w; w += mm; }
    double **nv[] = {&X, &Ap, &DDAp, &DAy};
    for (double **v : nv) { *v = w; w += nn; }
    ddotx = w; w += std::max(nq, 1);
    Dxp = w;
    part = A.wp_part.p; sc = A.wp_sc.p; host = (double *)A.wp_host.p;
  }
  dim3 g1(int64_t n) const { return dim3((unsigned)std::max<int64_t>(1, (n + WP_T - 1) / WP_T)); }
  // scalars back to the host: the one read-back of a CG step
  const double *read() {
    SDM_HIP_CHECK(hipMemcpyAsync(host, sc, SC_N * sizeof(double), hipMemcpyDeviceToHost, P->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
    return host;
  }
  void finish(int op, int n0, int k0, const double *s1 = nullptr, int n1 = 0, int k1 = SEG_SUM, const double *s2 = nullptr, int n2 = 0, int k2 = SEG_SUM,
              const double *s0 = nullptr) {
    SDM_KLAUNCH(P, k_wp_finish, dim3(1), dim3(WP_T), 0, s0 ? s0 : part, n0, k0, s1, n1, k1, s2, n2, k2, sc, op);
  }
  void amax(const double *v, int64_t n, int op) {
    const int G = wp_grid(n);
    SDM_KLAUNCH(P, k_wp_amax, dim3(G), dim3(WP_T), 0, v, n, part);
    finish(op, G, SEG_MAX);
  }
  void add(double *out, const double *a, const double *b, int64_t n, int sub) { SDM_KLAUNCH(P, k_wp_add, g1(n), dim3(WP_T), 0, out, a, b, n, sub); }
  // out = [sqrt(d.l).*x(1:l); asmDxq(d, x, K); psdscale(d, x, K[, transp])]   (wrapPcg.m:46,65,82; loopPcg.m:159-165)
  void Dx(const double *x, double *out, int transp) {
    if (nlpb + nq > 0)
      SDM_KLAUNCH(P, k_wp_dx_lq, dim3(nlpb + nq), dim3(64), 0, out, x, A.dl.p, A.ddet.p, A.q1.p, A.q2.p, A.qauxdet.p, A.qauxtr.p, A.d_qblk.p, l, nlpb,
                  (const double *)nullptr, (const double *)nullptr);
    if (lenud) pcg_psdscale_on(P, transp, perm, x + lq, out + lq);
  }
  // r = At' x (+ rb)
  void residual(const double *x, double *r, bool use_rb) {
    pcg_amul_on(P, 0, x, r);
    if (use_rb) add(r, r, A.wp_rb.p, m, 0);
  }
  // The sweeps decide on iterative refinement from what the sweeps before them reported (CholPlan::noted, read without a
  // synchronise when a sweep is enqueued: sdm_solve.hip).  The host loop synchronises after every solve, so each of its sweeps is
  // decided with the news of all earlier ones.  The same holds here when a backward sweep waits for the forward one before it:
  // before the first backward sweep of a call, and later only while the factor has blocks that refinement may take (a sweep has
  // reported one) -- the solves then take the host loop's decisions, and most factors cost no second synchronise per CG step.
  bool bw_waited = false;
  void wait_before_bw() {
    CholPlan &C = P->chol;
    if (C.refine_mode != 1) return;
    if (bw_waited && !(C.noted.host && ((volatile int *)C.noted.host)[0] > 0)) return;
    bw_waited = true;
    SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
  }
  // tmp = Lr ./ L.d, Lr = L \ r; the ssqr scalars of op
  void precond(const double *r, int op) {
    solve_run(P, r, Lr, 1);
    const int G = wp_grid(m);
    SDM_KLAUNCH(P, k_wp_divd_dot, dim3(G), dim3(WP_T), 0, Lr, solve_d(P), tmp, m, part);
    finish(op, G, SEG_SUM);
  }
  // loopPcg.m with b = the wrapPcg residual (A.wp_r), p = this->p when have_p; returns dk, or -1 when y stays empty; DAy in this->DAy,
  // the step in this->yhi
  int loop(const sdm_cgpars *cg, double restol, bool have_p, int &stop) {
    const double *b = A.wp_r.p;
    SDM_HIP_CHECK(hipMemcpyAsync(lr, b, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, P->stream));
    amax(lr, m, OP_NORMRMIN);
    int k = 0;
    stop = 0;
    bool have_y = false, have_ymin = false;
    const int Gm = wp_grid(m), Gd = wp_grid(lenud);
    while (stop == 0) {
      precond(lr, have_p ? OP_SSQR_NEXT : OP_SSQR_FIRST);
      wait_before_bw();
      solve_run(P, tmp, pb, 4);
      SDM_KLAUNCH(P, k_wp_pupdate, g1(m), dim3(WP_T), 0, p, pb, m, sc, have_p ? 0 : 1);
      have_p = true;
      // Ap = vecsym(At p) ; [DDAp, DApq, DAps, ssqrDAp] = PopK(d, Ap)
      pcg_amul_on(P, 1, p, Ap);
      pcg_vecsym_on(P, Ap);
      if (nlpb + nq > 0)
        SDM_KLAUNCH(P, k_wp_popk_lq, dim3(nlpb + nq), dim3(64), 0, DDAp, ddotx, Ap, A.dl.p, A.ddet.p, A.q1.p, A.q2.p, A.d_qblk.p, l, nlpb, part + 2 * WP_G);
      if (lenud) {
        pcg_psdscale_on(P, 0, perm, Ap + lq, Dxp);
        pcg_psdscale_on(P, 1, perm, Dxp, DDAp + lq);
        SDM_KLAUNCH(P, k_wp_dot, dim3(Gd), dim3(WP_T), 0, Dxp, (const double *)nullptr, lenud, part, 1);
      }
      finish(OP_POPK, nlpb + nq, SEG_SUM, ddotx, nq, SEG_SQR, part, lenud ? Gd : 0, SEG_SUM, part + 2 * WP_G);
      // the step, guarded on the device by ssqrDAp > 0
      pcg_amul_on(P, 0, DDAp, amr);
      SDM_KLAUNCH(P, k_wp_step_quadadd, dim3(Gm), dim3(WP_T), 0, m, p, yhi, ylo, lr, b, amr, A.d_Qjc.p, A.d_Qir.p, A.qpr.p, ddotx, nq, sc,
                  have_y ? 0 : 1, qprec ? 1 : 0, part);
      finish(OP_RES, Gm, SEG_SUM, part + 2 * Gm, qprec ? Gm : 0, SEG_SUM, part + 4 * Gm, Gm, SEG_MAX);
      SDM_KLAUNCH(P, k_wp_copy_if, g1(m), dim3(WP_T), 0, ymhi, yhi, m, sc);
      if (qprec) SDM_KLAUNCH(P, k_wp_copy_if, g1(m), dim3(WP_T), 0, ymlo, ylo, m, sc);
      const double *h = read();
      if (h[SC_SSQRDAP] > 0.0) {
        k++;
        have_y = true;
        if (h[SC_BETTER] != 0.0) have_ymin = true;
        const double finew = h[SC_FINEW], fiprev = h[SC_FIPREV];
        if (h[SC_NORMR] < restol) stop = 1;
        else if (finew - fiprev < cg->stagtol * fiprev) stop = 2;
        else if (k >= cg->maxiter) stop = 2;
      } else {
        stop = 1;
      }
    }
    double *ry = yhi, *rl = ylo;
    if (stop == 2) { ry = ymhi; rl = ymlo; have_y = have_ymin; }
    if (!have_y) return -1;
    if (k == 1) {                                      // DAy = alpha*[sqrt(d.l).*Ap(1:l); asmDxq(d, Ap, K, DApq); DAps]
      if (nlpb + nq > 0)
        SDM_KLAUNCH(P, k_wp_dx_lq, dim3(nlpb + nq), dim3(64), 0, DAy, Ap, A.dl.p, A.ddet.p, A.q1.p, A.q2.p, A.qauxdet.p, A.qauxtr.p, A.d_qblk.p, l, nlpb,
                    (const double *)ddotx, (const double *)(sc + SC_ALPHA));
      if (lenud) SDM_KLAUNCH(P, k_wp_scale, g1(lenud), dim3(WP_T), 0, DAy + lq, Dxp, lenud, sc);
    } else {                                           // DAy = Dx(vecsym(At y.hi)) + Dx(vecsym(At y.lo))
      pcg_amul_on(P, 1, ry, Ap); pcg_vecsym_on(P, Ap);
      Dx(Ap, DAy, 0);
      if (qprec) {
        pcg_amul_on(P, 1, rl, Ap); pcg_vecsym_on(P, Ap);
        Dx(Ap, X, 0);
        add(DAy, DAy, X, N, 0);
      }
    }
    if (ry != yhi) SDM_HIP_CHECK(hipMemcpyAsync(yhi, ry, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, P->stream));
    return k;
  }
};
}  // namespace

void pcg_wrap(sdm_plan *P, const sdm_cgpars *cg, double y0, bool use_rb, bool use_perm, sdm_int *kout, sdm_int *info) {
  pcg_prepare(P);
  Wrap W(P, use_perm, cg->qprec > 0);
  AdaPlan &A = P->ada;
  double *Y = A.wp_y.p, *DX = A.wp_dx.p, *R = A.wp_r.p;
  const double *rv = A.wp_rv.p;
  const double restol = y0 * cg->restol;
  sdm_int inf[SDM_WRAPPCG_INFO] = {0, 0, 0, 0};
  auto done = [&](sdm_int k, int exitcode) {
    inf[3] = exitcode;
    if (kout) *kout = k;
    if (info) for (int i = 0; i < SDM_WRAPPCG_INFO; i++) info[i] = inf[i];
  };
  // wrapPcg.m:46-60: dx = D' rv ; r = A dx (+ rb) ; p = L' \ ((L \ r) ./ L.d)
  W.Dx(rv, DX, 1);
  W.residual(DX, R, use_rb);
  W.precond(R, OP_SSQR_FIRST);
  W.wait_before_bw();
  solve_run(P, W.tmp, W.p, 4);
  // wrapPcg.m:65-67: x = vecsym(At p) ; dx = D x ; ssqrdx = norm(dx)^2
  pcg_amul_on(P, 1, W.p, W.Ap);
  pcg_vecsym_on(P, W.Ap);
  W.Dx(W.Ap, W.X, 0);
  const int GN = wp_grid(W.N);
  SDM_KLAUNCH(P, k_wp_dot, dim3(GN), dim3(WP_T), 0, W.X, (const double *)nullptr, W.N, W.part, 0);
  W.finish(OP_SSQRDX, GN, SEG_SUM);
  if (!(W.read()[SC_SSQRDX] > 0.0)) {                                 // wrapPcg.m:68-73
    SDM_HIP_CHECK(hipMemsetAsync(Y, 0, (size_t)W.m * sizeof(double), P->stream));
    SDM_HIP_CHECK(hipMemcpyAsync(DX, rv, (size_t)W.N * sizeof(double), hipMemcpyDeviceToDevice, P->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
    return done(0, 0);
  }
  // wrapPcg.m:78-91: the first step, its residual
  sdm_int k = 1;
  SDM_KLAUNCH(P, k_wp_first, W.g1(std::max(W.m, W.N)), dim3(WP_T), 0, Y, W.p, W.m, DX, rv, W.X, W.N, W.sc);
  W.Dx(DX, W.X, 1);
  W.residual(W.X, R, use_rb);
  W.amax(R, W.m, OP_NORMR);
  if (W.read()[SC_NORMR] < restol) return done(k, 1);
  // wrapPcg.m:100-130: loopPcg, refinement trials with p = []
  for (int trial = 0;; trial++) {
    int stop = 0;
    const int dk = W.loop(cg, restol, trial == 0, stop);
    inf[0] = trial; inf[1] = stop; inf[2]++;
    if (dk < 0) return done(k, 2);
    k += dk;
    W.add(Y, Y, W.yhi, W.m, 0);
    W.add(DX, DX, W.DAy, W.N, 1);
    W.Dx(DX, W.X, 1);
    W.residual(W.X, R, use_rb);
    W.amax(R, W.m, OP_NORMR);
    if (W.read()[SC_NORMR] < restol) return done(k, 3);
    if (trial >= cg->refine) return done(k, 4);
  }
}

}  // namespace sdm
