// sdm_gateways.hip -- extern "C" entry points of libsedumi_hip.so (include/sedumi_hip.h), tier (1): the stateless MEX equivalents.  Each
// builds a plan (sdm_capi.hip) for the one call; the gw_* plan builders are shared with the cache behind the mexFunction shims
// (sdm_mexcache.hip).
#include "../../include/sedumi_hip.h"
#include "sdm_plan.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace sdm;

struct PlanGuard {                                     // the plan of one stateless call
  sdm_plan *p;
  explicit PlanGuard(void *stream = nullptr) : p(sdm_plan_create(0, stream)) { if (!p) plan_ok(1); }
  ~PlanGuard() { sdm_plan_destroy(p); }
};

namespace sdm {
void gw_upload_invperm(DevBuf<int> &buf, const sdm_int *perm, sdm_int m) {
  std::vector<int> ip(m);
  for (sdm_int k = 0; k < m; k++) {
    if (perm[k] < 0 || perm[k] >= m) throw std::runtime_error("permutation entry out of range");
    ip[perm[k]] = (int)k;
  }
  buf.upload(ip);
}
// a trivial symbolic factor (diagonal) so that an ADA-only plan can be built
static void set_trivial_chol(sdm_plan *p, sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir) {
  std::vector<sdm_int> Ljc(m + 1), Lir(m), perm(m), xs(m + 1);
  for (sdm_int j = 0; j <= m; j++) { Ljc[j] = j; xs[j] = j; }
  for (sdm_int j = 0; j < m; j++) { Lir[j] = j; perm[j] = j; }
  plan_ok(sdm_plan_set_chol(p, m, Ljc.data(), Lir.data(), perm.data(), m, xs.data(), ADAjc, ADAir));
}
// ---- gateway-shaped plans: a plan that holds exactly what ONE of the getada gateways needs (its slice of At / DAt.q, the ADA
// pattern).  The stateless tier-1 entry points below build one per call; the MEX cache (sdm_mexcache.hip) keeps them.
// ADA' values live in p->ada_val, absd in p->absd.
void gw_build_getada1(sdm_plan *p, sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, const sdm_int *Ajc, const sdm_int *Air,
                      const double *Apr, const sdm_int *Ajc2, sdm_int lpN, sdm_int lorN, const sdm_int *qblkstart) {
  set_trivial_chol(p, m, ADAjc, ADAir);
  // only the LP/Lorentz rows matter here: present At as if it had no PSD part (rows >= qblkstart[lorN] are never touched:
  // Ajc2 is the end of the LP/Lorentz nonzeros)
  std::vector<sdm_int> Qjc(m + 1, 0);
  const sdm_int nlq = lorN > 0 ? qblkstart[lorN] : lpN;
  ada_build(p, nlq, m, Ajc, Air, Apr, Ajc2, lpN, lorN, 0, 0, nullptr, qblkstart, nullptr, Qjc.data(), nullptr, ADAjc, ADAir);
}
void gw_run_getada1(sdm_plan *p, const int *d_invperm, const double *dl, const double *ddet) {
  AdaPlan &A = p->ada;
  if (A.lpN) SDM_HIP_CHECK(hipMemcpyAsync(A.dl.p, dl, A.lpN * sizeof(double), hipMemcpyHostToDevice, p->stream));
  if (A.lorN) SDM_HIP_CHECK(hipMemcpyAsync(A.ddet.p, ddet, A.lorN * sizeof(double), hipMemcpyHostToDevice, p->stream));
  SDM_HIP_CHECK(hipMemsetAsync(p->ada_val.p, 0, p->ada_val.n * sizeof(double), p->stream));   // getada1.c:222-225
  if (A.nnz_lq == 0) return;     // no LP / Lorentz nonzeros at all (MAXCUT): ADA' stays zero -- nnz(ADA') empty sparse dots took 0.6 ms at n = 4000
  ada_lq(p, p->ada_val.p, d_invperm, false);
}
bool gw_getada1_is_zero(sdm_plan *p) { return p->ada.nnz_lq == 0; }
void gw_build_getada2(sdm_plan *p, sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, sdm_int lorN, const sdm_int *Qjc, const sdm_int *Qir) {
  set_trivial_chol(p, m, ADAjc, ADAir);
  std::vector<sdm_int> Ajc(m + 1, 0), qb(lorN + 1, 0);
  ada_build(p, lorN, m, Ajc.data(), nullptr, nullptr, Ajc.data(), 0, lorN, 0, 0, nullptr, qb.data(), nullptr, Qjc, Qir, ADAjc, ADAir);
}
void gw_run_getada2(sdm_plan *p, const int *d_invperm, const double *Qpr) {   // p->ada_val in/out
  if (p->ada.nnzQ) SDM_HIP_CHECK(hipMemcpyAsync(p->ada.qpr.p, Qpr, p->ada.nnzQ * sizeof(double), hipMemcpyHostToDevice, p->stream));
  ada_q(p, p->ada_val.p, d_invperm, true);
}
void gw_build_getada3(sdm_plan *p, sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, sdm_int N, const sdm_int *Ajc, const sdm_int *Air,
                      const double *Apr, const sdm_int *Ajc1, const sdm_cone *K, const sdm_int *psd_blkstart) {
  set_trivial_chol(p, m, ADAjc, ADAir);
  std::vector<sdm_int> Qjc(m + 1, 0), qb(K->lorN + 1, 0);
  // the LP/Lorentz rows are not read by getada3: describe them as plain LP rows up to the first PSD row
  const sdm_int nlq = K->sdpN > 0 ? psd_blkstart[0] : N;
  ada_build(p, N, m, Ajc, Air, Apr, Ajc1, nlq, 0, K->sdpN, K->rsdpN, K->sdpNL, qb.data(), psd_blkstart, Qjc.data(), nullptr, ADAjc, ADAir);
}
void gw_run_getada3(sdm_plan *p, const double *udsqr, bool input_is_zero) {   // p->ada_val in/out, p->absd out
  // input_is_zero: the ADA' handed in is known to be the zero matrix (getada1 / getada2 had nothing to add): nothing to symmetrise
  // (k_symmetrize + the copy back: 0.28 ms and 1.8 GB of traffic at n = 4000)
  if (p->ada.lenud) SDM_HIP_CHECK(hipMemcpyAsync(p->ada.udsqr.p, udsqr, p->ada.lenud * sizeof(double), hipMemcpyHostToDevice, p->stream));
  ada_psd(p, p->ada_val.p, nullptr, !input_is_zero);
}
// the whole ADA' of a problem WITHOUT PSD blocks (getada.m:13-40)
void gw_build_getada(sdm_plan *p, sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, const sdm_int *Ajc, const sdm_int *Air, const double *Apr,
                     sdm_int lpN, sdm_int lorN, const sdm_int *qblkstart, const sdm_int *Qjc, const sdm_int *Qir) {
  set_trivial_chol(p, m, ADAjc, ADAir);
  const sdm_int nlq = lorN > 0 ? qblkstart[lorN] : lpN;             // = K.mainblks(3)-1: rows of Alq (getada.m:25)
  std::vector<sdm_int> ajc2(m), zq(m + 1, 0);
  for (sdm_int j = 0; j < m; j++) ajc2[j] = std::lower_bound(Air + Ajc[j], Air + Ajc[j + 1], nlq) - Air;
  ada_build(p, nlq, m, Ajc, Air, Apr, ajc2.data(), lpN, lorN, 0, 0, nullptr, qblkstart, nullptr,
            lorN > 0 ? Qjc : zq.data(), lorN > 0 ? Qir : nullptr, ADAjc, ADAir);
}
void gw_run_getada(sdm_plan *p, const double *dl, const double *ddet, const double *Qpr) {
  AdaPlan &A = p->ada;
  if (A.lpN) SDM_HIP_CHECK(hipMemcpyAsync(A.dl.p, dl, A.lpN * sizeof(double), hipMemcpyHostToDevice, p->stream));
  if (A.lorN) SDM_HIP_CHECK(hipMemcpyAsync(A.ddet.p, ddet, A.lorN * sizeof(double), hipMemcpyHostToDevice, p->stream));
  if (A.lorN && A.nnzQ) SDM_HIP_CHECK(hipMemcpyAsync(A.qpr.p, Qpr, A.nnzQ * sizeof(double), hipMemcpyHostToDevice, p->stream));
  plan_ok(sdm_plan_getada(p));
}
// values of ADA' (and absd) back to the host once the plan's stream has drained
void gw_download(sdm_plan *p, double *ADApr, double *absd) {
  if (ADApr) SDM_HIP_CHECK(hipMemcpyAsync(ADApr, p->ada_val.p, p->ada_val.n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  if (absd) SDM_HIP_CHECK(hipMemcpyAsync(absd, p->absd.p, (size_t)p->chol.m * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
}
// the PSD blocks of K and a permutation of each (invcholfac, here and on a plan; the frame calls)
void cone_blocks(const sdm_cone *K, std::vector<int> &ns, sdm_int &lenud, sdm_int &plen) {
  ns.resize((size_t)K->sdpN); lenud = 0; plen = 0;
  for (sdm_int k = 0; k < K->sdpN; k++) {
    ns[k] = (int)K->sdpNL[k];
    lenud += (k < K->rsdpN ? 1 : 2) * K->sdpNL[k] * K->sdpNL[k];
    plen += K->sdpNL[k];
  }
}
void perm32(const sdm_int *perm, const std::vector<int> &ns, std::vector<int> &out) {
  out.clear();
  size_t o = 0;
  for (int n : ns) {
    std::vector<char> seen((size_t)n, 0);
    for (int i = 0; i < n; i++) {
      const sdm_int v = perm[o + i];
      if (v < 0 || v >= n || seen[(size_t)v]) throw std::runtime_error("perm is not a permutation of the block");
      seen[(size_t)v] = 1; out.push_back((int)v);
    }
    o += (size_t)n;
  }
}
}  // namespace sdm

extern "C" {

int sdm_getada1(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, sdm_int N, const sdm_int *Ajc,
                const sdm_int *Air, const double *Apr, const sdm_int *Ajc2, const sdm_int *perm, sdm_int lpN,
                const double *dl, sdm_int lorN, const double *ddet, const sdm_int *qblkstart, double *ADApr) {
  SDM_TRY
  (void)N;
  PlanGuard G; sdm_plan *p = G.p;
  gw_build_getada1(p, m, ADAjc, ADAir, Ajc, Air, Apr, Ajc2, lpN, lorN, qblkstart);
  DevBuf<int> ip; gw_upload_invperm(ip, perm, m);
  gw_run_getada1(p, ip.p, dl, ddet);
  gw_download(p, ADApr, nullptr);
  SDM_CATCH
}

int sdm_getada2(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, double *ADApr, sdm_int lorN,
                const sdm_int *Qjc, const sdm_int *Qir, const double *Qpr, const sdm_int *qperm) {
  SDM_TRY
  if (lorN <= 0) return 0;                          // getada2.c:154-155: nothing to do without Lorentz cones
  PlanGuard G; sdm_plan *p = G.p;
  gw_build_getada2(p, m, ADAjc, ADAir, lorN, Qjc, Qir);
  SDM_HIP_CHECK(hipMemcpy(p->ada_val.p, ADApr, (size_t)ADAjc[m] * sizeof(double), hipMemcpyHostToDevice));
  DevBuf<int> ip; gw_upload_invperm(ip, qperm, m);
  gw_run_getada2(p, ip.p, Qpr);
  gw_download(p, ADApr, nullptr);
  SDM_CATCH
}

int sdm_getada3(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, double *ADApr, sdm_int N, const sdm_int *Ajc,
                const sdm_int *Air, const double *Apr, const sdm_int *Ajc1, const sdm_int *sperm, const double *udsqr,
                const sdm_cone *K, const sdm_int *psd_blkstart, double *absd) {
  SDM_TRY
  (void)sperm;   // the sum is independent of the fill order (see sdm_ada.hip header)
  PlanGuard G; sdm_plan *p = G.p;
  gw_build_getada3(p, m, ADAjc, ADAir, N, Ajc, Air, Apr, Ajc1, K, psd_blkstart);
  SDM_HIP_CHECK(hipMemcpy(p->ada_val.p, ADApr, (size_t)ADAjc[m] * sizeof(double), hipMemcpyHostToDevice));
  gw_run_getada3(p, udsqr, false);
  gw_download(p, ADApr, absd);
  SDM_CATCH
}

// absd = getada(A, K, d, DAt) with the global ADA_sedumi_ : the whole ADA' of a problem WITHOUT PSD blocks
// (sedumi.m:446-448 -> getada.m:13-40):  ADA = DAt.q' DAt.q + Alq' diag([d.l; -d.det; d.det per norm-bound row]) Alq
// on the pattern of the global (both triangles), absd = diag(ADA) (getada.m:40).
int sdm_getada(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, sdm_int N, const sdm_int *Ajc, const sdm_int *Air,
               const double *Apr, sdm_int lpN, const double *dl, sdm_int lorN, const double *ddet, const sdm_int *qblkstart,
               const sdm_int *Qjc, const sdm_int *Qir, const double *Qpr, double *ADApr, double *absd) {
  SDM_TRY
  (void)N;
  PlanGuard G; sdm_plan *p = G.p;
  gw_build_getada(p, m, ADAjc, ADAir, Ajc, Air, Apr, lpN, lorN, qblkstart, Qjc, Qir);
  gw_run_getada(p, dl, ddet, Qpr);
  gw_download(p, ADApr, absd);
  SDM_CATCH
}

int sdm_blkchol(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const sdm_int *perm, sdm_int nsuper,
                const sdm_int *xsuper, const sdm_int *Xjc, const sdm_int *Xir, const double *Xpr,
                const sdm_cholpars *pars, const double *absd, double *Lpr, double *d, sdm_int *nskip,
                sdm_int *skip_idx, double *skip_val, sdm_int *nadd, sdm_int *add_idx, double *add_val) {
  SDM_TRY
  PlanGuard G; sdm_plan *p = G.p;
  plan_ok(sdm_plan_set_chol(p, m, Ljc, Lir, perm, nsuper, xsuper, Xjc, Xir));
  SDM_HIP_CHECK(hipMemcpy(p->ada_val.p, Xpr, (size_t)Xjc[m] * sizeof(double), hipMemcpyHostToDevice));
  if (absd) SDM_HIP_CHECK(hipMemcpy(p->absd.p, absd, m * sizeof(double), hipMemcpyHostToDevice));
  plan_ok(sdm_plan_blkchol_wait(p, pars, absd ? 1 : 0));
  plan_ok(sdm_plan_download(p, "lpr", Lpr, Ljc[m]));
  plan_ok(sdm_plan_download(p, "d", d, m));
  plan_ok(sdm_plan_pivots(p, nskip, skip_idx, skip_val, nadd, add_idx, add_val));
  SDM_CATCH
}

static int solve_common(bool fw, sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr,
                         const sdm_int *perm, sdm_int nsuper, const sdm_int *xsuper, sdm_int nrhs, const double *b,
                         double *y) {
  SDM_TRY
  PlanGuard G; sdm_plan *p = G.p;
  // the ADA pattern is irrelevant for a solve: use an empty one
  std::vector<sdm_int> zj(m + 1, 0), idperm;
  if (!perm) { idperm.resize(m); for (sdm_int i = 0; i < m; i++) idperm[i] = i; perm = idperm.data(); }
  plan_ok(sdm_plan_set_chol(p, m, Ljc, Lir, perm, nsuper, xsuper, zj.data(), nullptr));
  chol_load_factor(p, Lpr);
  for (sdm_int c = 0; c < nrhs; c++) {
    SDM_HIP_CHECK(hipMemcpyAsync(p->rhs.p, b + c * m, m * sizeof(double), hipMemcpyHostToDevice, p->stream));
    plan_ok(fw ? sdm_plan_fwsolve(p) : sdm_plan_bwsolve(p));
    SDM_HIP_CHECK(hipMemcpyAsync(y + c * m, p->y.p, m * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  }
  SDM_CATCH
}
int sdm_fwblkslv(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr, const sdm_int *perm,
                 sdm_int nsuper, const sdm_int *xsuper, sdm_int nrhs, const double *b, double *y) {
  return solve_common(true, m, Ljc, Lir, Lpr, perm, nsuper, xsuper, nrhs, b, y);
}
int sdm_bwblkslv(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr, const sdm_int *perm,
                 sdm_int nsuper, const sdm_int *xsuper, sdm_int nrhs, const double *b, double *y) {
  return solve_common(false, m, Ljc, Lir, Lpr, perm, nsuper, xsuper, nrhs, b, y);
}

// sparse right-hand sides: the pattern (Yjc,Yir) from symbfwblk is closed under the solve, so the
// dense solve restricted to it gives exactly the entries selfwsolve / selbwsolve define.
static int solve_sparse(bool fw, sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr,
                         const sdm_int *perm, sdm_int nsuper, const sdm_int *xsuper, sdm_int n, const sdm_int *Bjc,
                         const sdm_int *Bir, const double *Bpr, const sdm_int *Yjc, const sdm_int *Yir, double *Ypr) {
  SDM_TRY
  PlanGuard G; sdm_plan *p = G.p;
  std::vector<sdm_int> zj(m + 1, 0), idperm(m);
  for (sdm_int i = 0; i < m; i++) idperm[i] = i;
  // forward variant maps b through invperm == dense fwblkslv on a dense copy of b (fwblkslv.c:308-309);
  // backward variant uses no permutation at all (bwblkslv.c:279-291)
  plan_ok(sdm_plan_set_chol(p, m, Ljc, Lir, fw ? perm : idperm.data(), nsuper, xsuper, zj.data(), nullptr));
  chol_load_factor(p, Lpr);
  std::vector<double> col(m), out(m);
  for (sdm_int c = 0; c < n; c++) {
    std::fill(col.begin(), col.end(), 0.0);
    for (sdm_int t = Bjc[c]; t < Bjc[c + 1]; t++) col[Bir[t]] = Bpr[t];
    SDM_HIP_CHECK(hipMemcpyAsync(p->rhs.p, col.data(), m * sizeof(double), hipMemcpyHostToDevice, p->stream));
    plan_ok(fw ? sdm_plan_fwsolve(p) : sdm_plan_bwsolve(p));
    SDM_HIP_CHECK(hipMemcpyAsync(out.data(), p->y.p, m * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    for (sdm_int t = Yjc[c]; t < Yjc[c + 1]; t++) Ypr[t] = out[Yir[t]];
  }
  SDM_CATCH
}
int sdm_fwblkslv_sparse(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr, const sdm_int *perm,
                        sdm_int nsuper, const sdm_int *xsuper, sdm_int n, const sdm_int *Bjc, const sdm_int *Bir,
                        const double *Bpr, const sdm_int *Yjc, const sdm_int *Yir, double *Ypr) {
  return solve_sparse(true, m, Ljc, Lir, Lpr, perm, nsuper, xsuper, n, Bjc, Bir, Bpr, Yjc, Yir, Ypr);
}
int sdm_bwblkslv_sparse(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr, sdm_int nsuper,
                        const sdm_int *xsuper, sdm_int n, const sdm_int *Bjc, const sdm_int *Bir, const double *Bpr,
                        const sdm_int *Yjc, const sdm_int *Yir, double *Ypr) {
  return solve_sparse(false, m, Ljc, Lir, Lpr, nullptr, nsuper, xsuper, n, Bjc, Bir, Bpr, Yjc, Yir, Ypr);
}

// ---- invcholfac
int sdm_invcholfac(const sdm_cone *K, const double *u, const sdm_int *perm, double *y) {
  SDM_TRY
  std::vector<int> ns, p32; sdm_int lenud, plen;
  cone_blocks(K, ns, lenud, plen);
  if (lenud == 0) return 0;
  PlanGuard G; sdm_plan *p = G.p;
  DevBuf<double> du, dy; DevBuf<int> dp, dn, dpo; DevBuf<int64_t> doff;
  du.upload(u, (size_t)lenud); dy.alloc((size_t)lenud);
  if (perm) { perm32(perm, ns, p32); dp.upload(p32); }
  psd_invcholfac(p->stream, du.p, dy.p, perm ? dp.p : nullptr, ns, (int)K->rsdpN, dn, doff, dpo, false);
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  SDM_HIP_CHECK(hipMemcpy(y, dy.p, (size_t)lenud * sizeof(double), hipMemcpyDeviceToHost));
  SDM_CATCH
}

// ---- psdframeit / psdinvjmul in qrK's frames (sdm_cone.hip)
// the stream of the calling thread's psdframeit / psdinvjmul calls, created once: a new stream per call costs a new hardware queue, milliseconds
// against calls of a fraction of one (null where streams have no handles: the plan then makes its own)
static void *frame_stream() {
  static thread_local hipStream_t s = nullptr;
  if (!s && hipStreamCreate(&s) != hipSuccess) s = nullptr;
  return (void *)s;
}
static void h2d(double *d, const double *h, int64_t n) { SDM_HIP_CHECK(hipMemcpy(d, h, (size_t)n * sizeof(double), hipMemcpyHostToDevice)); }
static void d2h(double *h, const double *d, int64_t n) { SDM_HIP_CHECK(hipMemcpy(h, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost)); }
// How every frame / qrK call begins and ends.  K and frame_kind are checked and the orders of K's blocks are in ns; without PSD blocks there is
// nothing to do (p stays null: the caller returns); else no argument may be missing and the call has a plan on the thread's stream, p.
// the checks of K and frame_kind; ns = the orders of K's blocks; false: no PSD block has an entry
static bool frame_checks(const sdm_cone *K, int frame_kind, std::vector<int> &ns) {
  if (!K) throw std::runtime_error("K is null");
  if (frame_kind != SDM_FRAME_HOUSEHOLDER && frame_kind != SDM_FRAME_EXPLICIT)
    throw std::runtime_error("frame_kind must be SDM_FRAME_HOUSEHOLDER (0) or SDM_FRAME_EXPLICIT (1)");
  if (K->sdpN < 0 || K->rsdpN < 0 || K->rsdpN > K->sdpN) throw std::runtime_error("K: 0 <= rsdpN <= length(K.s) expected");
  sdm_int lenud, plen;
  cone_blocks(K, ns, lenud, plen);
  for (int n : ns) if (n < 0) throw std::runtime_error("K.s: negative order");
  return !std::all_of(ns.begin(), ns.end(), [](int n) { return n == 0; });
}
struct FrameCall {
  std::vector<int> ns;
  sdm_plan *p = nullptr;
  FrameCall(const char *who, const sdm_cone *K, int frame_kind, bool args_given) {
    if (!frame_checks(K, frame_kind, ns)) return;
    if (!args_given) throw std::runtime_error(std::string(who) + ": null argument");
    p = sdm_plan_create(0, frame_stream());
    if (!p) plan_ok(1);
  }
  ~FrameCall() { sdm_plan_destroy(p); }
  // the one synchronise of the call, then n doubles of the result d -> h
  void read_back(double *h, const double *d, int64_t n) { SDM_HIP_CHECK(hipStreamSynchronize(p->stream)); d2h(h, d, n); }
};
// the explicit frame on the device (qb): uploaded as it is, or expanded from the Householder form (staged in fr)
static void frame_upload(sdm_plan *p, const ConeTabs &T, const double *frms, int frame_kind, double *qb, double *fr) {
  if (frame_kind == SDM_FRAME_EXPLICIT) { h2d(qb, frms, T.lenud); return; }
  h2d(fr, frms, T.lenfr);
  cone_expand(p, T, fr, qb);
}
int sdm_set_frame_lds_budget(sdm_int bytes) {
  SDM_TRY
  cone_set_frame_lds_budget(bytes);
  SDM_CATCH
}
// (every call: one stream, ONE device allocation behind the block tables -- T.data, carved below -- and one synchronise before the read-back)
int sdm_psdframe_explicit(const sdm_cone *K, const double *frms, double *qb) {
  SDM_TRY
  FrameCall C("psdframe_explicit", K, SDM_FRAME_HOUSEHOLDER, frms && qb);
  if (!C.p) return 0;
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 1, 1, 0);
  double *dq = T.data, *df = dq + T.lenud;
  frame_upload(C.p, T, frms, SDM_FRAME_HOUSEHOLDER, dq, df);
  C.read_back(qb, dq, T.lenud);
  SDM_CATCH
}
int sdm_psdframeit(const sdm_cone *K, const double *lab, const double *frms, int frame_kind, double *x) {
  SDM_TRY
  FrameCall C("psdframeit", K, frame_kind, lab && frms && x);
  if (!C.p) return 0;
  const int hh = frame_kind == SDM_FRAME_HOUSEHOLDER ? 1 : 0;
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 2, hh, 1);
  double *dq = T.data, *dx = dq + T.lenud, *dl = dx + T.lenud, *df = dl + T.lenlab;
  h2d(dl, lab, T.lenlab);
  frame_upload(C.p, T, frms, frame_kind, dq, df);
  cone_frameit(C.p, T, dq, dl, dx);
  C.read_back(x, dx, T.lenud);
  SDM_CATCH
}
int sdm_psdinvjmul(const sdm_cone *K, const double *xlab, const double *frms, int frame_kind, const double *y, double *z) {
  SDM_TRY
  FrameCall C("psdinvjmul", K, frame_kind, xlab && frms && y && z);
  if (!C.p) return 0;
  const int hh = frame_kind == SDM_FRAME_HOUSEHOLDER ? 1 : 0;
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 5, hh, 1);
  double *dq = T.data, *dy = dq + T.lenud, *t1 = dy + T.lenud, *t2 = t1 + T.lenud, *dz = t2 + T.lenud, *dl = dz + T.lenud, *df = dl + T.lenlab;
  h2d(dl, xlab, T.lenlab); h2d(dy, y, T.lenud);
  frame_upload(C.p, T, frms, frame_kind, dq, df);
  cone_invjmul(C.p, T, dq, dl, dy, t1, t2, dz);
  C.read_back(z, dz, T.lenud);
  SDM_CATCH
}
// ---- qrK, the producer of those frames (sdm_qrk.hip); the call shape of the N5 entry points above
int sdm_set_qr_panel_lds_budget(sdm_int bytes) {
  SDM_TRY
  qrk_set_panel_lds_budget(bytes);
  SDM_CATCH
}
int sdm_qrk(const sdm_cone *K, const double *x, int frame_kind, double *q, double *r) {
  SDM_TRY
  FrameCall C("qrk", K, frame_kind, x && q);
  if (!C.p) return 0;
  QrkSteps S; qrk_plan(S, C.ns, (int)K->rsdpN);
  const int ex = frame_kind == SDM_FRAME_EXPLICIT ? 1 : 0;
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 1 + ex, 1, 0, S.words());
  double *dr = T.data, *dqb = dr + T.lenud, *dq = dr + (1 + ex) * T.lenud, *area = dq + T.lenfr;
  h2d(dr, x, T.lenud);
  qrk_run(C.p, T, S, area, dq, dr);
  if (ex) cone_expand(C.p, T, dq, dqb);
  C.read_back(q, ex ? dqb : dq, ex ? T.lenud : T.lenfr);
  if (r) d2h(r, dr, T.lenud);
  SDM_CATCH
}
// ---- urotorder, givensrot, sqrtinv (sdm_rot.hip); the call shape of the N5 / N6 entry points above
int sdm_set_rot_lds_budget(sdm_int bytes) {
  SDM_TRY
  rot_set_lds_budget(bytes);
  SDM_CATCH
}
int sdm_urotorder(const sdm_cone *K, const double *u, double maxu, const double *perm_in, double *u_out, double *perm_out, double *gjc, double *g,
                  sdm_int *g_len) {
  SDM_TRY
  if (!g_len) throw std::runtime_error("urotorder: null argument");
  *g_len = 0;
  std::vector<int> ns;
  if (!frame_checks(K, SDM_FRAME_HOUSEHOLDER, ns)) return 0;
  if (!(maxu == maxu)) throw std::runtime_error("urotorder: maxu is not a number");
  RotPlan S; urot_plan(S, ns, (int)K->rsdpN);
  FrameCall C("urotorder", K, SDM_FRAME_HOUSEHOLDER, u && u_out && perm_out && gjc && (g || S.gcap == 0));
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 2, 0, 3, 2 * S.gcap + S.words());
  double *du = T.data, *duo = du + T.lenud, *dpi = duo + T.lenud, *dpo = dpi + T.lenlab, *dgj = dpo + T.lenlab, *dgs = dgj + T.lenlab,
         *dgo = dgs + S.gcap, *area = dgo + S.gcap;
  h2d(du, u, T.lenud);
  if (perm_in) h2d(dpi, perm_in, T.lenlab);
  urot_run(C.p, T, S, area, du, duo, perm_in ? dpi : nullptr, dpo, dgj, dgs, dgo, maxu);
  C.read_back(gjc, dgj, T.lenlab);
  sdm_int len = 0, lo = 0;
  for (size_t b = 0; b < ns.size(); lo += ns[b], b++)
    if (ns[b] > 0) len += ((sdm_int)b < K->rsdpN ? 2 : 3) * (sdm_int)gjc[lo + ns[b] - 1];
  if (len < 0 || len > S.gcap) throw std::runtime_error("urotorder: rotation count out of range");
  d2h(perm_out, dpo, T.lenlab);
  if (len) d2h(g, dgo, len);
  d2h(u_out, duo, T.lenud);
  *g_len = len;
  SDM_CATCH
}
// gjc of every block: whole numbers that do not decrease, step k with at most n-1-k rotations (rows k .. k+m), all of them inside the g_len doubles
// of g.  gj32 = gjc as int32, goff = where every block's rotations begin in the compact g; returns the doubles of g they take
static sdm_int givens_counts(const sdm_cone *K, const std::vector<int> &ns, const double *gjc, sdm_int g_len, std::vector<int> &gj32,
                             std::vector<int64_t> &goff) {
  gj32.clear();
  goff.assign(ns.size(), 0);
  sdm_int inz = 0, lo = 0;
  for (size_t b = 0; b < ns.size(); lo += ns[b], b++) {
    const int n = ns[b];
    goff[b] = inz;
    for (int k = 0; k < n; k++) {
      const double v = gjc[lo + k];
      if (!(v >= 0.0 && v <= 2147483647.0)) throw std::runtime_error("givensrot: gjc out of range");
      gj32.push_back((int)v);
    }
    const int *gj = gj32.data() + lo;
    for (int k = 0; k + 1 < n; k++)
      if (gj[k + 1] < gj[k] || gj[k + 1] - gj[k] > n - 1 - k) throw std::runtime_error("givensrot: gjc is not a rotation count per step");
    if (n > 0) inz += ((sdm_int)b < K->rsdpN ? 2 : 3) * (sdm_int)gj[n - 1];
    if (inz > g_len) throw std::runtime_error("g size mismatch");       // givensrot.c:146, :156
  }
  return inz;
}
int sdm_givensrot(const sdm_cone *K, const double *gjc, const double *g, sdm_int g_len, const double *x, double *y) {
  SDM_TRY
  std::vector<int> ns;
  if (!frame_checks(K, SDM_FRAME_HOUSEHOLDER, ns)) return 0;
  if (!gjc || !x || !y || g_len < 0 || (!g && g_len > 0)) throw std::runtime_error("givensrot: null argument");
  std::vector<int> gj32;
  std::vector<int64_t> goff;
  const sdm_int inz = givens_counts(K, ns, gjc, g_len, gj32, goff);
  RotPlan S; givens_plan(S, ns, (int)K->rsdpN, goff);
  FrameCall C("givensrot", K, SDM_FRAME_HOUSEHOLDER, true);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 1, 0, 1, inz + S.words());
  double *dy = T.data, *dgj = dy + T.lenud, *dg = dgj + T.lenlab, *area = dg + inz;
  h2d(dy, x, T.lenud);
  SDM_HIP_CHECK(hipMemcpy(dgj, gj32.data(), gj32.size() * sizeof(int), hipMemcpyHostToDevice));
  if (inz) h2d(dg, g, inz);
  givens_run(C.p, T, S, area, dy, (const int *)dgj, dg);
  C.read_back(y, dy, T.lenud);
  SDM_CATCH
}
int sdm_sqrtinv(const sdm_cone *K, const double *q, const double *vlab, sdm_int vlab_len, double *y) {
  SDM_TRY
  std::vector<int> ns;
  const bool work = frame_checks(K, SDM_FRAME_HOUSEHOLDER, ns);
  sdm_int slen = 0;
  for (int n : ns) slen += n;
  const sdm_int skip = K->lpN + 2 * K->lorN;
  if (vlab_len != slen && vlab_len != skip + slen) throw std::runtime_error("v size mismatch");   // sqrtinv.c:120
  if (!work) return 0;
  FrameCall C("sqrtinv", K, SDM_FRAME_HOUSEHOLDER, q && vlab && y);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 2, 0, 1);
  double *dq = T.data, *dy = dq + T.lenud, *dv = dy + T.lenud;
  h2d(dq, q, T.lenud); h2d(dv, vlab + (vlab_len == slen ? 0 : skip), T.lenlab);
  sqrtinv_run(C.p, T, dq, dv, dy);
  C.read_back(y, dy, T.lenud);
  SDM_CATCH
}
// ---- triumtriu (sdm_cone.hip), and with it the whole PSD chain of updtransfo.m:99-108 as one call
int sdm_triumtriu(const sdm_cone *K, const double *x, const double *y, sdm_int len, double *z) {
  SDM_TRY
  std::vector<int> ns;
  const bool work = frame_checks(K, SDM_FRAME_HOUSEHOLDER, ns);
  sdm_int lenud, plen;
  cone_blocks(K, ns, lenud, plen);
  if (len < lenud) throw std::runtime_error("triumtriu: size mismatch");
  if (!work) return 0;
  FrameCall C("triumtriu", K, SDM_FRAME_HOUSEHOLDER, x && y && z);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 3, 0, 0);
  double *dx = T.data, *dy = dx + T.lenud, *dz = dy + T.lenud;
  h2d(dx, x + (len - lenud), T.lenud); h2d(dy, y + (len - lenud), T.lenud);    // triumtriu.m:50: the last lenud entries of both
  cone_triumtriu(C.p, T, dx, dy, dz);
  C.read_back(z, dz, T.lenud);
  SDM_CATCH
}
int sdm_updtransfo_psd(const sdm_cone *K, const double *ux, const double *u_in, const double *perm_in, const double *q, const double *vlab,
                       sdm_int vlab_len, double maxu, int frame_kind, double *u_out, double *perm_out, double *frame) {
  SDM_TRY
  std::vector<int> ns;
  const bool work = frame_checks(K, frame_kind, ns);
  sdm_int slen = 0;
  for (int n : ns) slen += n;
  const sdm_int skip = K->lpN + 2 * K->lorN;
  if (vlab_len != slen && vlab_len != skip + slen) throw std::runtime_error("v size mismatch");   // sqrtinv.c:120
  if (!work) return 0;
  if (!(maxu == maxu)) throw std::runtime_error("updtransfo_psd: maxu is not a number");
  const int rs = (int)K->rsdpN, ex = frame_kind == SDM_FRAME_EXPLICIT ? 1 : 0;
  RotPlan SU, SG; urot_plan(SU, ns, rs);
  givens_plan(SG, ns, rs, std::vector<int64_t>(ns.size(), 0));       // (sized here; planned again below, once gjc says where every block's rotations begin)
  QrkSteps SQ; qrk_plan(SQ, ns, rs);
  const int64_t wg = SG.words();
  FrameCall C("updtransfo_psd", K, frame_kind, ux && u_in && q && vlab && u_out && perm_out && frame);
  // six matrices: a = ux, later the result; b = u_in, later the explicit frame; c = ux u_in; d = urotorder's u; e = q, rotated in place; f = vinv, then r
  ConeTabs T; cone_tables(T, C.ns, rs, 6, 1, 5, 2 * SU.gcap + SU.words() + wg + SQ.words());
  double *da = T.data, *db = da + T.lenud, *dc = db + T.lenud, *dd = dc + T.lenud, *de = dd + T.lenud, *df = de + T.lenud, *dfr = df + T.lenud,
         *dpi = dfr + T.lenfr, *dpo = dpi + T.lenlab, *dgj = dpo + T.lenlab, *dgi = dgj + T.lenlab, *dv = dgi + T.lenlab, *dgs = dv + T.lenlab,
         *dgo = dgs + SU.gcap, *area_u = dgo + SU.gcap, *area_g = area_u + SU.words(), *area_q = area_g + wg;
  h2d(da, ux, T.lenud); h2d(db, u_in, T.lenud); h2d(de, q, T.lenud);
  if (perm_in) h2d(dpi, perm_in, T.lenlab);
  h2d(dv, vlab + (vlab_len == slen ? 0 : skip), T.lenlab);
  cone_triumtriu(C.p, T, da, db, dc);                                                                    // updtransfo.m:99
  urot_run(C.p, T, SU, area_u, dc, dd, perm_in ? dpi : nullptr, dpo, dgj, dgs, dgo, maxu);               // :100
  // the one transfer in the middle: gjc, which says how many rotations every step has (the host plans givensrot's strips on it)
  std::vector<double> gjc((size_t)T.lenlab);
  C.read_back(gjc.data(), dgj, T.lenlab);
  std::vector<int> gj32;
  std::vector<int64_t> goff;
  givens_counts(K, ns, gjc.data(), SU.gcap, gj32, goff);
  givens_plan(SG, ns, rs, goff);
  if (SG.words() != wg) throw std::runtime_error("updtransfo_psd: givensrot's plan changed size");
  SDM_HIP_CHECK(hipMemcpy(dgi, gj32.data(), gj32.size() * sizeof(int), hipMemcpyHostToDevice));
  givens_run(C.p, T, SG, area_g, de, (const int *)dgi, dgo);                                             // :102, g where urotorder left it
  sqrtinv_run(C.p, T, de, dv, df);                                                                       // :103
  qrk_run(C.p, T, SQ, area_q, dfr, df);                                                                  // :107
  cone_triumtriu(C.p, T, df, dd, da);                                                                    // :108
  if (ex) cone_expand(C.p, T, dfr, db);
  C.read_back(u_out, da, T.lenud);
  d2h(perm_out, dpo, T.lenlab);
  d2h(frame, ex ? db : dfr, ex ? T.lenud : T.lenfr);
  SDM_CATCH
}
// ---- psdfactor, psdinvscale (sdm_psdfact.hip), psdscale for a bare factor, and trydif.m:62-63 as one call; the call shape of N5 - N8
// the checks the four share, before anything touches a device: K, len >= lenud ("size mismatch"); false: no PSD block has an entry
static bool fact_checks(const char *who, const sdm_cone *K, sdm_int len, std::vector<int> &ns, sdm_int &lenud) {
  const bool work = frame_checks(K, SDM_FRAME_HOUSEHOLDER, ns);
  sdm_int plen;
  cone_blocks(K, ns, lenud, plen);
  if (len < lenud) throw std::runtime_error(std::string(who) + ": size mismatch");
  return work;
}
// where block `bad` begins in a lenud vector
static sdm_int fact_offset(const sdm_cone *K, const std::vector<int> &ns, int bad) {
  sdm_int o = 0;
  for (int b = 0; b < bad; b++) o += ((sdm_int)b < K->rsdpN ? 1 : 2) * (sdm_int)ns[b] * ns[b];
  return o;
}
int sdm_psdfactor(const sdm_cone *K, const double *x, sdm_int len, double *ux, int *ispos) {
  SDM_TRY
  std::vector<int> ns; sdm_int lenud;
  const bool work = fact_checks("psdfactor", K, len, ns, lenud);
  if (ispos) *ispos = 1;
  if (!work) return 0;
  FrameCall C("psdfactor", K, SDM_FRAME_HOUSEHOLDER, x && ux && ispos);
  PsdFactPlan S; psdfact_plan(S, C.ns, (int)K->rsdpN);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 1, 0, 0, S.words());
  double *da = T.data, *area = da + T.lenud;
  h2d(da, x + (len - lenud), T.lenud);                                  // psdfactor.m:55: the last lenud entries
  psdfactor_run(C.p, T, S, area, da);
  const int bad = psdfactor_first_bad(C.p, S, area);
  d2h(ux, da, T.lenud);
  if (bad >= 0) {                                                        // :68-71: `return` with ux zero from the failed block on
    const sdm_int o = fact_offset(K, ns, bad);
    std::fill(ux + o, ux + lenud, 0.0);
    *ispos = 0;
  }
  SDM_CATCH
}
int sdm_psdinvscale(const sdm_cone *K, const double *ud, const double *x, sdm_int len, double *y) {
  SDM_TRY
  std::vector<int> ns; sdm_int lenud;
  if (!fact_checks("psdinvscale", K, len, ns, lenud)) return 0;
  FrameCall C("psdinvscale", K, SDM_FRAME_HOUSEHOLDER, ud && x && y);
  PsdFactPlan S; psdfact_plan(S, C.ns, (int)K->rsdpN);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 2, 0, 0, S.words());
  double *du = T.data, *dy = du + T.lenud, *area = dy + T.lenud;
  h2d(du, ud, T.lenud); h2d(dy, x + (len - lenud), T.lenud);
  psdinvscale_run(C.p, T, S, area, du, dy);
  C.read_back(y, dy, T.lenud);
  SDM_CATCH
}
int sdm_psdscale(const sdm_cone *K, const double *ud, const double *x, sdm_int len, int transp, double *y) {
  SDM_TRY
  std::vector<int> ns; sdm_int lenud;
  if (!fact_checks("psdscale", K, len, ns, lenud)) return 0;
  FrameCall C("psdscale", K, SDM_FRAME_HOUSEHOLDER, ud && x && y);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 4, 0, 0);
  double *du = T.data, *dx = du + T.lenud, *dt = dx + T.lenud, *dy = dt + T.lenud;
  h2d(du, ud, T.lenud); h2d(dx, x + (len - lenud), T.lenud);
  pcg_psdscale_tabs(C.p, T.n, T.off, T.herm, T.items_full, T.nfull, transp ? 1 : 0, du, dx, dt, dy);
  SDM_HIP_CHECK(hipGetLastError());
  C.read_back(y, dy, T.lenud);
  SDM_CATCH
}
// trydif.m:62-63 on the device, shared by sdm_trydif_psd and sdm_wstruct_psd: x, z up; da = psdfactor(x), zero from a failed block on; ds = psdscale(da, z)
static void trydif_steps(FrameCall &C, const sdm_cone *K, const ConeTabs &T, const PsdFactPlan &S, double *area, const double *x, const double *z,
                         sdm_int len, sdm_int lenud, double *da, double *dz, double *dt, double *ds, int *ispos) {
  h2d(da, x + (len - lenud), T.lenud); h2d(dz, z + (len - lenud), T.lenud);
  psdfactor_run(C.p, T, S, area, da);                                                                    // trydif.m:62
  // the one transfer in the middle: the blocks' flags.  With a failed block ux is zero from it on before it scales z, as the two single calls have it
  const int bad = psdfactor_first_bad(C.p, S, area);
  if (bad >= 0) {
    const sdm_int o = fact_offset(K, C.ns, bad);
    SDM_HIP_CHECK(hipMemsetAsync(da + o, 0, (size_t)(lenud - o) * sizeof(double), C.p->stream));
    *ispos = 0;
  }
  pcg_psdscale_tabs(C.p, T.n, T.off, T.herm, T.items_full, T.nfull, 0, da, dz, dt, ds);                  // :63
  SDM_HIP_CHECK(hipGetLastError());
}
int sdm_trydif_psd(const sdm_cone *K, const double *x, const double *z, sdm_int len, double *ux, double *s, int *ispos) {
  SDM_TRY
  std::vector<int> ns; sdm_int lenud;
  const bool work = fact_checks("trydif_psd", K, len, ns, lenud);
  if (ispos) *ispos = 1;
  if (!work) return 0;
  FrameCall C("trydif_psd", K, SDM_FRAME_HOUSEHOLDER, x && z && ux && s && ispos);
  PsdFactPlan S; psdfact_plan(S, C.ns, (int)K->rsdpN);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 4, 0, 0, S.words());
  double *da = T.data, *dz = da + T.lenud, *dt = dz + T.lenud, *ds = dt + T.lenud, *area = ds + T.lenud;
  trydif_steps(C, K, T, S, area, x, z, len, lenud, da, dz, dt, ds, ispos);
  C.read_back(ux, da, T.lenud);
  d2h(s, ds, T.lenud);
  SDM_CATCH
}
// ---- psdeig and minpsdeig (sdm_psdeig.hip); the call shape of N9
static thread_local int g_eig_sweeps = 0;                               // the sweeps of the calling thread's last psdeig / minpsdeig call
static int eig_call(const char *who, const sdm_cone *K, const double *x, sdm_int len, double *lab, double *q, double *mineig, int *info) {
  std::vector<int> ns; sdm_int lenud;
  const bool work = fact_checks(who, K, len, ns, lenud);
  if (info) *info = -1;
  if (mineig) *mineig = HUGE_VAL;
  g_eig_sweeps = 0;
  if (!work) return 0;
  FrameCall C(who, K, SDM_FRAME_HOUSEHOLDER, x && info && (lab || mineig));
  PsdEigPlan S; psdeig_plan(S, C.ns, (int)K->rsdpN);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, q ? 3 : 2, 0, 1, S.words());
  double *dx = T.data, *db = dx + T.lenud, *dv = q ? db + T.lenud : nullptr, *dl = db + (q ? 2 : 1) * T.lenud, *area = dl + T.lenlab;
  h2d(dx, x + (len - lenud), T.lenud);                                  // psdeig.m:51: the last lenud entries
  *info = psdeig_run(C.p, T, S, area, dx, db, dv, dl, dx, mineig != nullptr, &g_eig_sweeps);   // (q over x: x is read by the first launch only)
  if (lab) d2h(lab, dl, T.lenlab);
  if (q) d2h(q, dx, T.lenud);
  if (mineig) d2h(mineig, area + S.o_min, 1);
  return 0;
}
int sdm_psdeig(const sdm_cone *K, const double *x, sdm_int len, double *lab, double *q, int *info) {
  SDM_TRY
  if (eig_call("psdeig", K, x, len, lab, q, nullptr, info)) return 1;
  SDM_CATCH
}
int sdm_minpsdeig(const sdm_cone *K, const double *x, sdm_int len, double *mineig, int *info) {
  SDM_TRY
  if (eig_call("minpsdeig", K, x, len, nullptr, nullptr, mineig, info)) return 1;
  SDM_CATCH
}
int sdm_psdeig_last_sweeps(void) { return g_eig_sweeps; }
// ---- psdjmul (sdm_cone.hip), and the two places of the loop that chained two of the calls above through the host as one call each
int sdm_psdjmul(const sdm_cone *K, const double *x, const double *y, sdm_int len, double *z) {
  SDM_TRY
  std::vector<int> ns; sdm_int lenud;
  if (!fact_checks("psdjmul", K, len, ns, lenud)) return 0;
  FrameCall C("psdjmul", K, SDM_FRAME_HOUSEHOLDER, x && y && z);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 3, 0, 0);
  double *dx = T.data, *dy = dx + T.lenud, *dz = dy + T.lenud;
  h2d(dx, x + (len - lenud), T.lenud); h2d(dy, y + (len - lenud), T.lenud);    // psdjmul.m:50: the last lenud entries of both
  cone_psdjmul(C.p, T, dx, dy, dz);
  C.read_back(z, dz, T.lenud);
  SDM_CATCH
}
// maxstep.m:63: psdinvscale's result stays on the device and is minpsdeig's input there
int sdm_maxstep_psd(const sdm_cone *K, const double *ud, const double *dx, sdm_int len, double *mineig, int *info) {
  SDM_TRY
  std::vector<int> ns; sdm_int lenud;
  const bool work = fact_checks("maxstep_psd", K, len, ns, lenud);
  if (info) *info = -1;
  if (mineig) *mineig = HUGE_VAL;
  g_eig_sweeps = 0;
  if (!work) return 0;
  FrameCall C("maxstep_psd", K, SDM_FRAME_HOUSEHOLDER, ud && dx && mineig && info);
  PsdFactPlan SF; psdfact_plan(SF, C.ns, (int)K->rsdpN);
  PsdEigPlan SE; psdeig_plan(SE, C.ns, (int)K->rsdpN);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 3, 0, 1, SF.words() + SE.words());
  double *du = T.data, *dy = du + T.lenud, *db = dy + T.lenud, *dl = db + T.lenud, *area_f = dl + T.lenlab, *area_e = area_f + SF.words();
  h2d(du, ud, T.lenud); h2d(dy, dx + (len - lenud), T.lenud);
  psdinvscale_run(C.p, T, SF, area_f, du, dy);
  *info = psdeig_run(C.p, T, SE, area_e, dy, db, nullptr, dl, dy, true, &g_eig_sweeps);
  d2h(mineig, area_e + SE.o_min, 1);
  SDM_CATCH
}
// widelen.m:101-104 / trydif.m:62-64: s stays on the device and is psdeig's input there (the values alone; psdeig_run does not write its x)
int sdm_wstruct_psd(const sdm_cone *K, const double *x, const double *z, sdm_int len, double *ux, double *s, double *lab, int *ispos, int *info) {
  SDM_TRY
  std::vector<int> ns; sdm_int lenud;
  const bool work = fact_checks("wstruct_psd", K, len, ns, lenud);
  if (ispos) *ispos = 1;
  if (info) *info = -1;
  g_eig_sweeps = 0;
  if (!work) return 0;
  FrameCall C("wstruct_psd", K, SDM_FRAME_HOUSEHOLDER, x && z && ux && s && lab && ispos && info);
  PsdFactPlan SF; psdfact_plan(SF, C.ns, (int)K->rsdpN);
  PsdEigPlan SE; psdeig_plan(SE, C.ns, (int)K->rsdpN);
  ConeTabs T; cone_tables(T, C.ns, (int)K->rsdpN, 5, 0, 1, SF.words() + SE.words());
  double *da = T.data, *dz = da + T.lenud, *dt = dz + T.lenud, *ds = dt + T.lenud, *db = ds + T.lenud, *dl = db + T.lenud, *area_f = dl + T.lenlab,
         *area_e = area_f + SF.words();
  trydif_steps(C, K, T, SF, area_f, x, z, len, lenud, da, dz, dt, ds, ispos);
  *info = psdeig_run(C.p, T, SE, area_e, ds, db, nullptr, dl, ds, false, &g_eig_sweeps);
  d2h(ux, da, T.lenud);
  d2h(s, ds, T.lenud);
  d2h(lab, dl, T.lenlab);
  SDM_CATCH
}
}  // extern "C"
