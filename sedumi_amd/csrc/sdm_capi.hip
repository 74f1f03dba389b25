// sdm_capi.hip -- extern "C" entry points of libsedumi_hip.so (include/sedumi_hip.h): the error state, the device calls and the plan tier
// (sdm_plan_*).  The stateless MEX equivalents are in sdm_gateways.hip, the cached ones in sdm_mexcache.hip.
#include "../../include/sedumi_hip.h"
#include "sdm_plan.h"
#include <algorithm>
#include <cstring>

namespace sdm {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
}  // namespace sdm
using namespace sdm;

// every read-back of a plan passes through here after its stream synchronise: a spin inside one of THIS plan's launches that gave up
// makes the results unusable -- of a factor launch: the plan is marked not factored; of a merged sweep launch (sdm_solve.hip: merged_wait):
// that solve's, the factor stays and the plan's next solves run unmerged (chol_wait_timeouts)
static const char *const FACTOR_TIMEOUT = "blkchol: a workgroup timed out waiting for another one inside a factor launch";
static void check_plan_health(sdm_plan *p) {
  const int t = chol_wait_timeouts(p);
  if (t & TMO_FACTOR) throw std::runtime_error(FACTOR_TIMEOUT);
  if (t & TMO_SWEEP) throw std::runtime_error("solve: a workgroup timed out waiting for another one inside a merged sweep launch (the factor stays; the next solves run unmerged)");
}
// the pivot parameters of a factorisation: blkchol.c:292-294 defaults, abstol >= 0 (blkchol.c:303)
static sdm_cholpars chol_pars(const sdm_cholpars *pars) {
  sdm_cholpars q = {1e-12, 5e2, 1e-20};
  if (pars) q = *pars;
  if (q.abstol < 0.0) q.abstol = 0.0;
  return q;
}
// the steps of a staged factorisation between sdm_plan_blkchol_begin and _end
static void require_begun(sdm_plan *p, const char *fn) {
  if (!p->has_chol) throw std::runtime_error(std::string(fn) + ": no symbolic factor set");
  if (!p->chol.begun) throw std::runtime_error(std::string(fn) + ": no factorisation begun (sdm_plan_blkchol_begin)");
}

extern "C" {

const char *sdm_last_error(void) { return g_err.c_str(); }
#ifdef SDM_EMU
const char *sdm_backend(void) { return "emu"; }
#else
const char *sdm_backend(void) { return "hip-gfx950"; }
#endif
int sdm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int sdm_set_device(int dev) {
  SDM_TRY
  SDM_HIP_CHECK(hipSetDevice(dev));
  SDM_CATCH
}

// ------------------------------------------------------------------ plan
sdm_plan *sdm_plan_create(int device, void *stream) {
  try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device available (libsedumi_hip has no CPU fallback)"); return nullptr; }
    SDM_HIP_CHECK(hipSetDevice(device));
    sdm_plan *p = new sdm_plan();
    p->device = device;
    if (stream) { p->stream = (hipStream_t)stream; p->own_stream = false; }
    else { SDM_HIP_CHECK(hipStreamCreate(&p->stream)); p->own_stream = true; }
    return p;
  } catch (const std::exception &e) { set_error(e.what()); return nullptr; }
}
void sdm_plan_destroy(sdm_plan *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  (void)hipStreamSynchronize(p->stream);
  chol_forget_plan(p);
  for (auto g : p->graphs) (void)hipGraphExecDestroy(g);
  for (int i = 0; i < 16; i++) { if (p->ev_begin[i]) (void)hipEventDestroy(p->ev_begin[i]); if (p->ev_end[i]) (void)hipEventDestroy(p->ev_end[i]); }
  if (p->own_stream && p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}
int sdm_plan_sync(sdm_plan *p) {
  SDM_TRY
  SDM_HIP_CHECK(hipSetDevice(p->device));
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  check_plan_health(p);
  SDM_CATCH
}

int sdm_plan_set_chol(sdm_plan *p, sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const sdm_int *perm,
                      sdm_int nsuper, const sdm_int *xsuper, const sdm_int *ADAjc, const sdm_int *ADAir) {
  SDM_TRY
  SDM_HIP_CHECK(hipSetDevice(p->device));
  p->dense = sdm::DensePlan();            // dense-column tables are sized for the factor they were set with: gone with it
  chol_build(p, m, Ljc, Lir, perm, nsuper, xsuper, ADAjc, ADAir);
  p->ada_jc.assign(ADAjc, ADAjc + m + 1);
  p->ada_ir.assign(ADAir, ADAir + ADAjc[m]);
  SDM_CATCH
}

int sdm_plan_set_ada(sdm_plan *p, sdm_int N, sdm_int m, const sdm_int *Ajc, const sdm_int *Air, const double *Apr,
                     const sdm_int *Ajc_psd, const sdm_cone *K, const sdm_int *qblkstart, const sdm_int *psd_blkstart,
                     const sdm_int *Qjc, const sdm_int *Qir) {
  SDM_TRY
  SDM_HIP_CHECK(hipSetDevice(p->device));
  if (!p->has_chol) throw std::runtime_error("sdm_plan_set_ada: call sdm_plan_set_chol first (it carries the ADA pattern)");
  if (m != p->chol.m) throw std::runtime_error("sdm_plan_set_ada: m mismatch");
  ada_build(p, N, m, Ajc, Air, Apr, Ajc_psd, K->lpN, K->lorN, K->sdpN, K->rsdpN, K->sdpNL, qblkstart,
            psd_blkstart, Qjc, Qir, p->ada_jc.data(), p->ada_ir.data());
  // host copy of At for the operators of sdm_pcg.hip (their device tables are built on first use)
  p->ada.h_Ajc.assign(Ajc, Ajc + m + 1); p->ada.h_Air.assign(Air, Air + Ajc[m]); p->ada.h_Apr.assign(Apr, Apr + Ajc[m]);
  p->ada.pcg_ready = false; p->ada.aden_n = 0;
  SDM_CATCH
}

static DevBuf<double> *plan_buf(sdm_plan *p, const char *name) {
  std::string s(name);
  if (s == "ada") return &p->ada_val;
  if (s == "absd") return &p->absd;
  if (s == "d") return &p->chol.d;
  if (s == "dsolve") return &p->chol.dsolve;
  if (s == "y") return &p->y;
  if (s == "rhs") return &p->rhs;
  if (s == "lpr") return &p->lpr;
  if (s == "udsqr") return &p->ada.udsqr;
  if (s == "u") { if (p->ada.ufac.n < (size_t)std::max<sdm_int>(p->ada.lenud, 1)) p->ada.ufac.alloc((size_t)std::max<sdm_int>(p->ada.lenud, 1)); return &p->ada.ufac; }
  if (s == "dl") return &p->ada.dl;
  if (s == "ddet") return &p->ada.ddet;
  if (s == "qpr") return &p->ada.qpr;
  if (s == "q1") return &p->ada.q1;
  if (s == "q2") return &p->ada.q2;
  if (s == "xN") { if (p->ada.xN.n == 0) throw std::runtime_error("buffer xN exists after the first sdm_plan_amul / vecsym / psdscale / pcg_init"); return &p->ada.xN; }
  if (s == "psd") { if (p->ada.psd.n == 0) throw std::runtime_error("buffer psd exists after sdm_plan_pcg_init"); return &p->ada.psd; }
  // sdm_plan_wrappcg: inputs (allocated on first use) and outputs (allocated by its first call)
  auto sized = [](DevBuf<double> &b, sdm_int n) -> DevBuf<double> * { if (b.n < (size_t)std::max<sdm_int>(n, 1)) b.alloc((size_t)std::max<sdm_int>(n, 1)); return &b; };
  if (s == "rv") return sized(p->ada.wp_rv, p->ada.N);
  if (s == "rb") return sized(p->ada.wp_rb, p->ada.m);
  if (s == "qauxdet") return sized(p->ada.qauxdet, p->ada.lorN);
  if (s == "qauxtr") return sized(p->ada.qauxtr, p->ada.lorN);
  if (s == "pcg_y" || s == "pcg_dx" || s == "pcg_r") {
    DevBuf<double> &b = s == "pcg_y" ? p->ada.wp_y : s == "pcg_dx" ? p->ada.wp_dx : p->ada.wp_r;
    if (b.n == 0) throw std::runtime_error("buffer " + s + " exists after the first sdm_plan_wrappcg");
    return &b;
  }
  if (s == "ad") return &p->dense.ad;      // dense columns Ad (m x nden, column major; deninfac.m:58-59)
  if (s == "lad") return &p->dense.lad;     // LAD = L \ Ad(perm,:) of the last sdm_plan_deninfac
  if (s == "dden") return &p->dense.dden;   // Ld of the last sdm_plan_deninfac
  // the arenas the multi-GPU layer exchanges slices of (sedumi_amd.dist.SeparatorShardedSolver)
  if (s == "fronts") return &p->chol.fronts;
  if (s == "wvec") return &p->chol.wvec;
  if (s == "xfin") return &p->chol.xfin;
  if (s == "ub") return &p->chol.ub;
  if (s == "panelrec") { if (p->chol.panelrec.n == 0) p->chol.panelrec.alloc((size_t)(4 * sdm::NB + 2 + sdm::NB * sdm::NB)); return &p->chol.panelrec; }
  throw std::runtime_error("unknown plan buffer: " + s);
}
void *sdm_plan_devptr(sdm_plan *p, const char *name, sdm_int *nelem) {
  try {
    DevBuf<double> *b = plan_buf(p, name);
    if (nelem) *nelem = (sdm_int)b->n;
    return b->p;
  } catch (const std::exception &e) { set_error(e.what()); return nullptr; }
}
int sdm_plan_upload(sdm_plan *p, const char *name, const double *src, sdm_int nelem) {
  SDM_TRY
  DevBuf<double> *b = plan_buf(p, name);
  if ((size_t)nelem > b->n) throw std::runtime_error(std::string("upload: too many elements for buffer ") + name);
  SDM_HIP_CHECK(hipMemcpyAsync(b->p, src, (size_t)nelem * sizeof(double), hipMemcpyHostToDevice, p->stream));
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  SDM_CATCH
}
int sdm_plan_download(sdm_plan *p, const char *name, double *dst, sdm_int nelem) {
  SDM_TRY
  DevBuf<double> *b = plan_buf(p, name);
  if (std::string(name) == "lpr") chol_extract(p, p->lpr.p);
  if ((size_t)nelem > b->n) throw std::runtime_error(std::string("download: too many elements for buffer ") + name);
  // small read-backs (the vectors a host-driven loop fetches a hundred times per iteration) through the plan's own pinned buffer: a copy into
  // pageable memory goes through the runtime's staging and took 37 us per call of the product driver, this one 12 (profiles/r08w_*)
  constexpr size_t DL_STAGE_BYTES = 64 * 1024;
  const size_t nbytes = (size_t)nelem * sizeof(double);
  if (nbytes > 0 && nbytes <= DL_STAGE_BYTES && !p->capturing) {
    p->dl_stage.ensure(DL_STAGE_BYTES / sizeof(int));
    SDM_HIP_CHECK(hipMemcpyAsync(p->dl_stage.p, b->p, nbytes, hipMemcpyDeviceToHost, p->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    memcpy(dst, p->dl_stage.p, nbytes);
  } else {
    SDM_HIP_CHECK(hipMemcpyAsync(dst, b->p, nbytes, hipMemcpyDeviceToHost, p->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  }
  check_plan_health(p);
  SDM_CATCH
}

int sdm_plan_getada(sdm_plan *p) {
  SDM_TRY
  if (!p->has_ada) throw std::runtime_error("sdm_plan_getada: no ADA data set");
  if (ada_lq_q(p, p->ada_val.p)) { ada_psd(p, p->ada_val.p, nullptr, false, true); return 0; }
  p->ada.zero_defer = true;                  // (a zero LP / Lorentz part may be cleared by the stage-1 launch of ada_psd: ada_zero_flush)
  try {
    ada_lq(p, p->ada_val.p, nullptr, false);
    ada_q(p, p->ada_val.p, nullptr, true);
    ada_psd(p, p->ada_val.p, nullptr, false);
  } catch (...) { p->ada.zero_defer = false; ada_zero_flush(p); throw; }
  p->ada.zero_defer = false;
  ada_zero_flush(p);
  SDM_CATCH
}
int sdm_plan_getdatq(sdm_plan *p) {
  SDM_TRY
  if (!p->has_ada) throw std::runtime_error("sdm_plan_getdatq: no ADA data set");
  ada_datq(p);
  SDM_CATCH
}
int sdm_plan_getada_cols(sdm_plan *p, sdm_int j0, sdm_int j1) {
  SDM_TRY
  if (!p->has_ada) throw std::runtime_error("sdm_plan_getada_cols: no ADA data set");
  if (j0 < 0 || j1 > p->ada.m || j0 > j1) throw std::runtime_error("sdm_plan_getada_cols: column range out of bounds");
  p->ada.col0 = j0; p->ada.col1 = j1;
  try {
    ada_lq(p, p->ada_val.p, nullptr, false);
    ada_q(p, p->ada_val.p, nullptr, true);
    ada_psd(p, p->ada_val.p, nullptr, false);
  } catch (...) { p->ada.col0 = 0; p->ada.col1 = p->ada.m; throw; }
  p->ada.col0 = 0; p->ada.col1 = p->ada.m;
  SDM_CATCH
}
int sdm_plan_copy(sdm_plan *p, const char *name, void *devptr, sdm_int offset, sdm_int nelem, int to_plan) {
  SDM_TRY
  DevBuf<double> *b = plan_buf(p, name);
  if (offset < 0 || nelem < 0 || (size_t)(offset + nelem) > b->n) throw std::runtime_error(std::string("sdm_plan_copy: range outside buffer ") + name);
  if (std::string(name) == "lpr" && !to_plan) chol_extract(p, p->lpr.p);
  if (to_plan) SDM_HIP_CHECK(hipMemcpyAsync(b->p + offset, devptr, (size_t)nelem * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  else SDM_HIP_CHECK(hipMemcpyAsync(devptr, b->p + offset, (size_t)nelem * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  check_plan_health(p);
  SDM_CATCH
}
// the whole factorisation, or (begin) its first step of three: sdm_plan_blkchol_begin / _levels / _end
static int plan_factor(sdm_plan *p, const sdm_cholpars *pars, int use_absd, bool begin) {
  SDM_TRY
  if (!p->has_chol) throw std::runtime_error(std::string(begin ? "sdm_plan_blkchol_begin" : "sdm_plan_blkchol") + ": no symbolic factor set");
  const sdm_cholpars q = chol_pars(pars);
  p->dense.factored = false;                        // the dense-column factors belong to the previous L, d
  (begin ? chol_begin : chol_factor)(p, q.canceltol, q.maxu, q.abstol, use_absd);
  SDM_CATCH
}
int sdm_plan_blkchol(sdm_plan *p, const sdm_cholpars *pars, int use_absd) { return plan_factor(p, pars, use_absd, false); }
int sdm_plan_blkchol_wait(sdm_plan *p, const sdm_cholpars *pars, int use_absd) {
  SDM_TRY
  for (int attempt = 0; ; attempt++) {
    plan_ok(sdm_plan_blkchol(p, pars, use_absd));
    SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    // (a factor time-out switches the plan to the launch-per-panel path; one of a merged sweep before it only switches merging off)
    if (!(chol_wait_timeouts(p) & TMO_FACTOR)) break;
    if (attempt == 1) throw std::runtime_error(FACTOR_TIMEOUT);
  }
  SDM_CATCH
}
// ---- the factorisation and the solve level by level (include/sedumi_hip.h: "Separator fronts across GPUs")
int sdm_plan_set_active_supernodes(sdm_plan *p, const int *active, sdm_int nsuper) {
  SDM_TRY
  p->chol.sn_active.assign(active ? active : nullptr, active ? active + nsuper : nullptr);
  for (auto &c : p->chol.sn_active) c = c ? 1 : 0;
  SDM_CATCH
}
int sdm_plan_front_layout(sdm_plan *p, sdm_int *nlevels, sdm_int *level, sdm_int *foff, sdm_int *fsize, sdm_int *woff, sdm_int *ms, sdm_int *first, sdm_int *ns) {
  SDM_TRY
  if (!p->has_chol) throw std::runtime_error("sdm_plan_front_layout: no symbolic factor set");
  const sdm::CholPlan &C = p->chol;
  if (nlevels) *nlevels = C.nlevels;
  for (sdm_int s = 0; s < C.nsuper; s++) {
    if (level) level[s] = C.sn_level[s];
    if (foff) foff[s] = C.sn_foff[s];
    if (fsize) fsize[s] = (sdm_int)C.sn_ld[s] * C.sn_ms[s];
    if (woff) woff[s] = C.sn_woff[s];
    if (ms) ms[s] = C.sn_ms[s];
    if (first) first[s] = C.sn_first[s];
    if (ns) ns[s] = C.sn_ns[s];
  }
  SDM_CATCH
}
int sdm_plan_blkchol_begin(sdm_plan *p, const sdm_cholpars *pars, int use_absd) { return plan_factor(p, pars, use_absd, true); }
// ---- one dense front factored block-column-cyclically by several ranks (include/sedumi_hip.h: "One front across GPUs")
int sdm_plan_blkchol_panels(sdm_plan *p, sdm_int l0, sdm_int l1, sdm_int pan0, sdm_int pan1, int world, int rank, int blk) {
  SDM_TRY
  require_begun(p, "sdm_plan_blkchol_panels");
  if (world < 1 || world > 255 || rank < 0 || rank >= world || blk < 1 || blk > 255) throw std::runtime_error("sdm_plan_blkchol_panels: need 1 <= world <= 255, 0 <= rank < world, 1 <= blk <= 255");
  if (world > 1 && p->chol.nsuper != 1) throw std::runtime_error("sdm_plan_blkchol_panels: block-cyclic ranks (world > 1) factor ONE dense front");
  for (int l = (int)std::max<sdm_int>(l0, 0); l < (int)std::min<sdm_int>(l1, p->chol.nlevels); l++)
    if (p->chol.lev_persist[l] && !p->chol.front_disabled)
      throw std::runtime_error("sdm_plan_blkchol_panels: the level is planned as ONE launch; call sdm_plan_set_one_launch_fronts(plan, 0) before sdm_plan_set_chol");
  const int own = world == 1 ? 0 : (world | rank << 8 | blk << 16);   // (k_ldl_panel: owns_col)
  chol_levels(p, (int)l0, (int)l1, false, own, (int)pan0, (int)std::min<sdm_int>(pan1, 1 << 30));
  SDM_CATCH
}
int sdm_plan_panel_record(sdm_plan *p, sdm_int panel, int unpack, sdm_int *front_offset, sdm_int *front_nelem) {
  SDM_TRY
  if (!p->has_chol) throw std::runtime_error("sdm_plan_panel_record: no symbolic factor set");
  const CholPlan &C = p->chol;
  if (C.nsuper != 1 || panel < 0 || panel * NB >= C.sn_ns[0]) throw std::runtime_error("sdm_plan_panel_record: one dense front, 0 <= panel < its panels");
  if (unpack >= 0) chol_panel_record(p, (int)panel, unpack);            // (unpack < 0: only the slice of "fronts" is asked for)
  const sdm_int k0 = panel * NB, kb = std::min<sdm_int>(NB, C.sn_ns[0] - k0);
  if (front_offset) *front_offset = C.sn_foff[0] + k0 * (sdm_int)C.sn_ld[0];
  if (front_nelem) *front_nelem = kb * (sdm_int)C.sn_ld[0];
  SDM_CATCH
}
int sdm_plan_blkchol_levels(sdm_plan *p, sdm_int l0, sdm_int l1, int extend_only) {
  SDM_TRY
  require_begun(p, "sdm_plan_blkchol_levels");
  chol_levels(p, (int)l0, (int)l1, extend_only != 0, /*own=*/0);
  SDM_CATCH
}
int sdm_plan_blkchol_end(sdm_plan *p) {
  SDM_TRY
  require_begun(p, "sdm_plan_blkchol_end");
  chol_end(p);
  SDM_CATCH
}
int sdm_plan_solve_levels(sdm_plan *p, int what, sdm_int l0, sdm_int l1) {
  SDM_TRY
  if (!p->factored) throw std::runtime_error("sdm_plan_solve_levels: no factor resident");
  if (p->dense.factored) throw std::runtime_error("sdm_plan_solve_levels: not with a resident dense-column factor");
  solve_levels(p, what, (int)l0, (int)l1);
  SDM_CATCH
}
int sdm_plan_load_factor(sdm_plan *p, const double *Lpr, const double *d) {
  SDM_TRY
  if (!p->has_chol) throw std::runtime_error("sdm_plan_load_factor: no symbolic factor set");
  SDM_HIP_CHECK(hipSetDevice(p->device));
  p->dense.factored = false;
  chol_load_factor(p, Lpr, d);
  SDM_CATCH
}
int sdm_plan_pivots(sdm_plan *p, sdm_int *nskip, sdm_int *skip_idx, double *skip_val, sdm_int *nadd,
                    sdm_int *add_idx, double *add_val) {
  SDM_TRY
  const sdm_int m = p->chol.m;
  std::vector<int> st(m);
  std::vector<double> val(m);
  SDM_HIP_CHECK(hipSetDevice(p->device));
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  check_plan_health(p);
  SDM_HIP_CHECK(hipMemcpy(st.data(), p->chol.pivstat.p, m * sizeof(int), hipMemcpyDeviceToHost));
  SDM_HIP_CHECK(hipMemcpy(val.data(), p->chol.pivval.p, m * sizeof(double), hipMemcpyDeviceToHost));
  sdm_int ns = 0, na = 0;
  for (sdm_int j = 0; j < m; j++) {
    if (st[j] == 1) { if (skip_idx) skip_idx[ns] = j; if (skip_val) skip_val[ns] = val[j]; ns++; }
    else if (st[j] == 2) { if (add_idx) add_idx[na] = j; if (add_val) add_val[na] = val[j]; na++; }
  }
  if (nskip) *nskip = ns;
  if (nadd) *nadd = na;
  SDM_CATCH
}
static int plan_solve(sdm_plan *p, int mode, const char *fn) {          // mode bits: 1 fw | 2 ./d | 4 bw (solve_run)
  SDM_TRY
  if (!p->factored) throw std::runtime_error(std::string(fn) + ": no factor resident");
  solve_run(p, p->rhs.p, p->y.p, mode);
  SDM_CATCH
}
int sdm_plan_fwsolve(sdm_plan *p) { return plan_solve(p, 1, "fwsolve"); }
int sdm_plan_bwsolve(sdm_plan *p) { return plan_solve(p, 4, "bwsolve"); }
int sdm_plan_ldlsolve(sdm_plan *p) { return plan_solve(p, 7, "ldlsolve"); }
int sdm_plan_set_growth_max(sdm_plan *p, double growth_max) {
  SDM_TRY
  if (!(growth_max >= 0.0)) throw std::runtime_error("growth_max must be >= 0");
  p->chol.growth_max = growth_max;
  SDM_CATCH
}
int sdm_plan_set_refinement(sdm_plan *p, int mode, double refine_max) {
  SDM_TRY
  if (mode < 0 || mode > 2) throw std::runtime_error("sdm_plan_set_refinement: mode must be 0, 1 or 2");
  if (!(refine_max >= 0.0)) throw std::runtime_error("sdm_plan_set_refinement: refine_max must be >= 0");
  p->chol.refine_mode = mode; p->chol.refine_max = refine_max;
  SDM_CATCH
}
int sdm_plan_set_one_launch_fronts(sdm_plan *p, int on) {
  SDM_TRY
  p->chol.front_off_req = !on;
  SDM_CATCH
}
int sdm_plan_set_tile_workgroups(sdm_plan *p, int n) {
  SDM_TRY
  if (n < 0) throw std::runtime_error("sdm_plan_set_tile_workgroups: n must be >= 0");
  p->chol.tile_wgs_req = n;
  SDM_CATCH
}
int sdm_plan_set_one_launch_inverse(sdm_plan *p, int on) {
  SDM_TRY
  p->chol.sprep_off = !on;
  SDM_CATCH
}
int sdm_plan_set_solve_width(sdm_plan *p, sdm_int width) {
  SDM_TRY
  if (width != 0 && (width < sdm::SBW_MIN || width > sdm::SBW_MAX || (width & (width - 1)) != 0))
    throw std::runtime_error("solve width must be 0 (automatic) or a power of two in 256 .. 2048");
  p->chol.sbw_req = (int)width;
  SDM_CATCH
}
int sdm_plan_get_solve_width(sdm_plan *p, sdm_int *width) {
  SDM_TRY
  if (!p->has_chol) throw std::runtime_error("sdm_plan_get_solve_width: no symbolic factor set");
  *width = p->chol.sbw;
  SDM_CATCH
}
int sdm_plan_solve_stats(sdm_plan *p, sdm_int *nblocks, sdm_int *nbad, double *max_growth) {
  SDM_TRY
  if (!p->has_chol) throw std::runtime_error("sdm_plan_solve_stats: no symbolic factor set");
  solve_stats(p, nblocks, nbad, max_growth);
  SDM_CATCH
}
// ---- the operators around the solves in wrapPcg.m / loopPcg.m
int sdm_plan_pcg_init(sdm_plan *p, sdm_int nden, const sdm_int *dense_cols, const double *denseA) {
  SDM_TRY
  if (!p->has_ada) throw std::runtime_error("sdm_plan_pcg_init: no problem data set (sdm_plan_set_ada)");
  SDM_HIP_CHECK(hipSetDevice(p->device));
  pcg_set_dense(p, nden, dense_cols, denseA);
  SDM_CATCH
}
int sdm_plan_amul(sdm_plan *p, int transp) {
  SDM_TRY
  if (!p->has_ada) throw std::runtime_error("sdm_plan_amul: no problem data set (sdm_plan_set_ada)");
  pcg_amul(p, transp);
  SDM_CATCH
}
int sdm_plan_vecsym(sdm_plan *p) {
  SDM_TRY
  if (!p->has_ada) throw std::runtime_error("sdm_plan_vecsym: no problem data set (sdm_plan_set_ada)");
  pcg_vecsym(p);
  SDM_CATCH
}
int sdm_plan_psdscale(sdm_plan *p, int transp, int use_perm) {
  SDM_TRY
  if (!p->has_ada) throw std::runtime_error("sdm_plan_psdscale: no problem data set (sdm_plan_set_ada)");
  pcg_psdscale(p, transp, use_perm != 0);
  SDM_CATCH
}
int sdm_plan_wrappcg(sdm_plan *p, const sdm_cgpars *cg, double y0, int use_rb, int use_perm, sdm_int *k, sdm_int *info) {
  SDM_TRY
  // every refusal before the first launch
  if (!cg) throw std::runtime_error("sdm_plan_wrappcg: no cgpars");
  if (!p->has_ada) throw std::runtime_error("sdm_plan_wrappcg: no problem data set (sdm_plan_set_ada)");
  if (!p->factored) throw std::runtime_error("sdm_plan_wrappcg: no factor resident");
  if (p->capturing) throw std::runtime_error("sdm_plan_wrappcg synchronises once per CG step: not inside a graph capture");
  if (p->ada.aden_n > 0 || p->dense.factored) throw std::runtime_error("sdm_plan_wrappcg: dense columns are not supported (sdm_plan_pcg_init with nden > 0 or a resident dense-column factor)");
  if (p->ada.lenud > 0 && p->ada.ufac.n < (size_t)p->ada.lenud) throw std::runtime_error("sdm_plan_wrappcg: PSD blocks need the scaling's \"u\" (upload it first)");
  if (use_perm && !p->ada.ic_has_perm) throw std::runtime_error("sdm_plan_wrappcg: use_perm without a resident pivot order (sdm_plan_invcholfac with perm)");
  if (p->ada.wp_rv.n < (size_t)std::max<sdm_int>(p->ada.N, 1)) throw std::runtime_error("sdm_plan_wrappcg: upload buffer \"rv\" first");
  if (use_rb && p->ada.wp_rb.n < (size_t)std::max<sdm_int>(p->ada.m, 1)) throw std::runtime_error("sdm_plan_wrappcg: upload buffer \"rb\" first (or use_rb = 0)");
  if (p->ada.lorN > 0 && (p->ada.qauxdet.n < (size_t)p->ada.lorN || p->ada.qauxtr.n < (size_t)p->ada.lorN))
    throw std::runtime_error("sdm_plan_wrappcg: Lorentz cones need \"qauxdet\" and \"qauxtr\" (d.auxdet, d.auxtr)");
  SDM_HIP_CHECK(hipSetDevice(p->device));
  pcg_wrap(p, cg, y0, use_rb != 0, use_perm != 0, k, info);
  check_plan_health(p);
  SDM_CATCH
}
// y(perm,perm) = u'u of every PSD block of the plan (invcholfac.c): from the resident "u" into "udsqr"
int sdm_plan_invcholfac(sdm_plan *p, const sdm_int *perm) {
  SDM_TRY
  AdaPlan &A = p->ada;
  if (A.lenud == 0) return 0;
  if (A.ufac.n < (size_t)A.lenud) throw std::runtime_error("invcholfac: upload buffer \"u\" first");
  std::vector<int> ns(A.psd_n.begin(), A.psd_n.end()), p32;
  if (perm) {
    // the permutation is staged in a plan-owned pinned buffer that outlives the call (the copy is asynchronous);
    // inside a graph capture the copy node would keep reading that buffer at every replay, so a NEW permutation
    // cannot be handed over there -- upload it before the capture
    if (p->capturing) throw std::runtime_error("sdm_plan_invcholfac: a permutation cannot be uploaded inside a graph capture (the captured copy would replay from the staging buffer)");
    perm32(perm, ns, p32);
    if (A.ic_perm.n < p32.size()) A.ic_perm.alloc(p32.size());
    A.ic_perm_host.ensure(p32.size());
    SDM_HIP_CHECK(hipStreamSynchronize(p->stream));                 // an earlier copy out of the staging buffer may be pending
    memcpy(A.ic_perm_host.p, p32.data(), p32.size() * sizeof(int));
    SDM_HIP_CHECK(hipMemcpyAsync(A.ic_perm.p, A.ic_perm_host.p, p32.size() * sizeof(int), hipMemcpyHostToDevice, p->stream));
    A.ic_has_perm = true;
  }
  const bool ready = A.ic_n.n == ns.size() && !ns.empty();           // block tables: once per plan (set_ada resets them)
  psd_invcholfac(p->stream, A.ufac.p, A.udsqr.p, perm ? A.ic_perm.p : nullptr, ns, (int)A.rsdpN, A.ic_n, A.ic_off, A.ic_poff, ready);
  SDM_CATCH
}
// ---- resident dense-column unit (deninfac.m:58-94)
int sdm_plan_set_dense(sdm_plan *p, sdm_int nden, const sdm_int *LADjc, const sdm_int *LADir, const sdm_int *dzjc, const sdm_int *dzir,
                       const sdm_int *colperm, const sdm_int *first) {
  SDM_TRY
  if (!p->has_chol) throw std::runtime_error("sdm_plan_set_dense: call sdm_plan_set_chol first");
  SDM_HIP_CHECK(hipSetDevice(p->device));
  dense_set(p, nden, LADjc, LADir, dzjc, dzir, colperm, first);
  SDM_CATCH
}
int sdm_plan_deninfac(sdm_plan *p, const double *smult, double maxuden, int *host_fallback) {
  SDM_TRY
  if (p->capturing) throw std::runtime_error("sdm_plan_deninfac synchronises (it reads the stability flag): not inside a graph capture");
  dense_factor(p, smult, maxuden, host_fallback);
  SDM_CATCH
}
int sdm_plan_lden(sdm_plan *p, sdm_int *betajc, double *beta, double *pv, sdm_int *pivperm, sdm_int *npivperm, sdm_int *dopiv, double *Ld) {
  SDM_TRY
  DensePlan &D = p->dense;
  if (!D.factored) throw std::runtime_error("sdm_plan_lden: no dense-column factor resident");
  dense_fetch_tables(p->stream, D);                                   // (lengths, row-order flags: device tables of the factorisation)
  const sdm_int nden = D.nden, nb = D.betajc[nden], np = D.permoff[nden];
  for (sdm_int k = 0; k <= nden; k++) betajc[k] = D.betajc[k];
  for (sdm_int k = 0; k < nden; k++) dopiv[k] = D.dopiv[k];
  if (nb) SDM_HIP_CHECK(hipMemcpy(beta, D.beta.p, nb * sizeof(double), hipMemcpyDeviceToHost));
  if (D.pnnz) SDM_HIP_CHECK(hipMemcpy(pv, D.p.p, D.pnnz * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<int> pp((size_t)std::max<sdm_int>(np, 1));
  if (np) SDM_HIP_CHECK(hipMemcpy(pp.data(), D.d_pivperm.p, np * sizeof(int), hipMemcpyDeviceToHost));
  for (sdm_int i = 0; i < np; i++) pivperm[i] = pp[i];
  *npivperm = np;
  SDM_HIP_CHECK(hipMemcpy(Ld, D.dden.p, p->chol.m * sizeof(double), hipMemcpyDeviceToHost));
  SDM_CATCH
}
// ---- hipGraph capture of a launch-bound sequence of plan calls (e.g. one whole iteration unit): everything the plan
// enqueues on its stream between begin and end becomes one executable graph; replay costs one launch.
int sdm_plan_graph_begin(sdm_plan *p) {
  SDM_TRY
  if (p->capturing) throw std::runtime_error("graph capture already in progress");
  if (p->kprof.enabled) throw std::runtime_error("per-kernel timing must be off during graph capture");
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  SDM_HIP_CHECK(hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal));
  p->capturing = true;
  SDM_CATCH
}
int sdm_plan_graph_end(sdm_plan *p, int *graph_id) {
  SDM_TRY
  if (!p->capturing) throw std::runtime_error("no graph capture in progress");
  p->capturing = false;
  hipGraph_t g = nullptr;
  SDM_HIP_CHECK(hipStreamEndCapture(p->stream, &g));
  hipGraphExec_t ge = nullptr;
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  SDM_HIP_CHECK(e);
  p->graphs.push_back(ge);
  if (graph_id) *graph_id = (int)p->graphs.size() - 1;
  SDM_CATCH
}
int sdm_plan_graph_launch(sdm_plan *p, int graph_id) {
  SDM_TRY
  if (graph_id < 0 || graph_id >= (int)p->graphs.size()) throw std::runtime_error("unknown graph id");
  SDM_HIP_CHECK(hipGraphLaunch(p->graphs[graph_id], p->stream));
  SDM_CATCH
}

int sdm_plan_timer_begin(sdm_plan *p, int slot) {
  SDM_TRY
  if (slot < 0 || slot >= 16) throw std::runtime_error("timer slot out of range");
  if (!p->ev_begin[slot]) { SDM_HIP_CHECK(hipEventCreate(&p->ev_begin[slot])); SDM_HIP_CHECK(hipEventCreate(&p->ev_end[slot])); }
  SDM_HIP_CHECK(hipEventRecord(p->ev_begin[slot], p->stream));
  SDM_CATCH
}
int sdm_plan_timer_end(sdm_plan *p, int slot) {
  SDM_TRY
  if (slot < 0 || slot >= 16 || !p->ev_end[slot]) throw std::runtime_error("timer slot not started");
  SDM_HIP_CHECK(hipEventRecord(p->ev_end[slot], p->stream));
  SDM_CATCH
}
int sdm_plan_timer_ms(sdm_plan *p, int slot, float *ms) {
  SDM_TRY
  if (slot < 0 || slot >= 16 || !p->ev_end[slot]) throw std::runtime_error("timer slot not started");
  SDM_HIP_CHECK(hipEventSynchronize(p->ev_end[slot]));
  SDM_HIP_CHECK(hipEventElapsedTime(ms, p->ev_begin[slot], p->ev_end[slot]));
  SDM_CATCH
}

// per-kernel timing (HIP events around every launch of the plan while enabled)
int sdm_plan_kprof_enable(sdm_plan *p, int on) {
  SDM_TRY
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  for (auto &r : p->kprof.recs) { p->kprof.pool.push_back(r.a); p->kprof.pool.push_back(r.b); }
  p->kprof.recs.clear();
  p->kprof.enabled = on != 0;
  SDM_CATCH
}
int sdm_plan_kprof_get(sdm_plan *p, const char *kernel, sdm_int *calls, double *total_ms) {
  SDM_TRY
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  sdm_int n = 0; double tot = 0.0;
  for (auto &r : p->kprof.recs)
    if (std::string(r.name) == kernel) { float ms = 0; SDM_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b)); tot += ms; n++; }
  if (calls) *calls = n;
  if (total_ms) *total_ms = tot;
  SDM_CATCH
}
// writes "name:calls:ms;" records for every kernel seen into buf (truncated to buflen)
int sdm_plan_kprof_summary(sdm_plan *p, char *buf, sdm_int buflen) {
  SDM_TRY
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  std::vector<std::string> names; std::vector<sdm_int> cnt; std::vector<double> tot;
  for (auto &r : p->kprof.recs) {
    float ms = 0; SDM_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
    size_t i = 0; for (; i < names.size(); i++) if (names[i] == r.name) break;
    if (i == names.size()) { names.push_back(r.name); cnt.push_back(0); tot.push_back(0.0); }
    cnt[i]++; tot[i] += ms;
  }
  std::string out;
  for (size_t i = 0; i < names.size(); i++) out += names[i] + ":" + std::to_string(cnt[i]) + ":" + std::to_string(tot[i]) + ";";
  if (buflen > 0) { size_t n = std::min<size_t>(out.size(), (size_t)buflen - 1); memcpy(buf, out.data(), n); buf[n] = 0; }
  SDM_CATCH
}

}  // extern "C"
