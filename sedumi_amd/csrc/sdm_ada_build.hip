// sdm_ada_build.hip -- host-side planning of ADA' (sdm_ada.hip): every table its kernels read, computed once per solve from At, the cone
// and the ADA' pattern.  ada_build (at the end) is the sequence of the steps below.  No kernel is defined or launched here.
#include "sdm_plan.h"
#include <algorithm>

namespace sdm {
namespace {

// what ada_build is given (sdm_plan.h)
struct AdaIn {
  sdm_int m; const sdm_int *Ajc, *Air; const double *Apr; const sdm_int *Ajc_psd;
  sdm_int lpN, lorN, sdpN, rsdpN; const sdm_int *sdpNL, *qblkstart, *psd_blkstart, *Qjc, *Qir, *ADAjc, *ADAir;
  sdm_int psd_begin(sdm_int j) const { return sdpN > 0 ? Ajc_psd[j] : Ajc[j + 1]; }   // first PSD nonzero of column j of At
};
// the PSD nonzeros of At against the union patterns of their blocks
struct PsdPatterns {
  std::vector<int> Ablk, Aupos;             // per nonzero of At: its PSD block (-1: none) and its position in U_k
  std::vector<std::vector<int>> U;          // U_k: the rows of block k (from the block's start) that any constraint has, sorted
  std::vector<int64_t> uoff;                // offset of U_k in their concatenation; uoff[sdpN] = length of a full-length z vector
  sdm_int psdnnz = 0;
};
// the stage-1 tasks (constraint j, PSD block k), column by column, and the slots of each
struct Stage1Tasks {
  std::vector<int> t_col, t_blk, t_n, t_nslot, t_ulen, t_herm, s_col, order, order_xcd;
  std::vector<int64_t> t_slotptr, t_udoff, t_uoff, t_zoff, t_end, s_nzptr, c_taskptr, c_zlen;
};

// 64-bit host indices as the 32-bit ones the kernels read
void upload_narrow(DevBuf<int> &d, const sdm_int *h, sdm_int n) { std::vector<int> v((size_t)n); for (sdm_int t = 0; t < n; t++) v[t] = (int)h[t]; d.upload(v); }

// The block table (A.psd_n, psd_start, psd_udoff, maxn, lenud: host side, sdm_psd.hip and sdm_pcg.hip read it too) with its checks;
// per PSD nonzero of At its block and its position in the union pattern U_k (d_Ablk, d_Aupos: stage 2 and k_psd_direct; u_pos: stage 1)
PsdPatterns psd_patterns(AdaPlan &A, const AdaIn &in) {
  const sdm_int m = in.m, sdpN = in.sdpN;
  A.psd_n.assign(in.sdpNL, in.sdpNL + sdpN);
  A.psd_start.assign(in.psd_blkstart, in.psd_blkstart + sdpN + (sdpN > 0 ? 1 : 0));
  A.psd_udoff.assign(sdpN + 1, 0);
  A.maxn = 0;
  for (sdm_int k = 0; k < sdpN; k++) {
    const sdm_int n = in.sdpNL[k], len = (k < in.rsdpN ? 1 : 2) * n * n;
    if (in.psd_blkstart[k + 1] - in.psd_blkstart[k] != len) throw std::runtime_error("PSD block size / blkstart mismatch");
    A.psd_udoff[k + 1] = A.psd_udoff[k] + len;
    A.maxn = std::max<int>(A.maxn, (int)n);
  }
  A.lenud = A.psd_udoff[sdpN];
  PsdPatterns pt;
  pt.Ablk.assign((size_t)A.nnzA, -1); pt.Aupos.assign((size_t)A.nnzA, 0); pt.U.resize(sdpN);
  for (sdm_int j = 0; j < m; j++) {
    sdm_int k = 0;
    for (sdm_int t = in.psd_begin(j); t < in.Ajc[j + 1]; t++) {
      sdm_int r = in.Air[t];
      if (r < A.nlq) throw std::runtime_error("Ajc_psd points into the LP/Lorentz part");
      while (k < sdpN && r >= in.psd_blkstart[k + 1]) k++;
      if (k >= sdpN) throw std::runtime_error("At row index beyond the PSD blocks");
      pt.Ablk[t] = (int)k;
      pt.U[k].push_back((int)(r - in.psd_blkstart[k]));
    }
  }
  pt.uoff.assign(sdpN + 1, 0);
  for (sdm_int k = 0; k < sdpN; k++) {
    std::sort(pt.U[k].begin(), pt.U[k].end());
    pt.U[k].erase(std::unique(pt.U[k].begin(), pt.U[k].end()), pt.U[k].end());
    pt.uoff[k + 1] = pt.uoff[k] + (int64_t)pt.U[k].size();
  }
  for (sdm_int j = 0; j < m; j++)
    for (sdm_int t = in.psd_begin(j); t < in.Ajc[j + 1]; t++) {
      const std::vector<int> &Uk = pt.U[pt.Ablk[t]];
      int q = (int)(in.Air[t] - in.psd_blkstart[pt.Ablk[t]]);
      pt.Aupos[t] = (int)(std::lower_bound(Uk.begin(), Uk.end(), q) - Uk.begin());
      pt.psdnnz++;
    }
  return pt;
}

// One pass over the columns of At: the tasks of stage 1 (k_psd_stage1_mfma, k_psd_stage1; k_psd_direct reads some of the t_* too) with
// their slots, the tasks of every column (c_taskptr, c_zlen: stage 2), then the two dispatch orders of a launch over all tasks
Stage1Tasks stage1_tasks(AdaPlan &A, const AdaIn &in, const PsdPatterns &pt) {
  const sdm_int m = in.m;
  Stage1Tasks tk;
  tk.c_taskptr.assign(m + 1, 0); tk.c_zlen.assign(m + 1, 0);       // (c_zlen: length of z_j, all tasks of constraint j)
  A.zlen = 0; A.zmaxj = 0; A.one_task_per_col = true; A.s1_maxulen = 0;
  for (sdm_int j = 0; j < m; j++) {
    sdm_int t = in.psd_begin(j);
    while (t < in.Ajc[j + 1]) {
      int k = pt.Ablk[t];
      sdm_int te = t;
      while (te < in.Ajc[j + 1] && pt.Ablk[te] == k) te++;
      const sdm_int n = A.psd_n[k];
      const bool herm = k >= in.rsdpN;
      const int ulen = (int)pt.U[k].size();
      tk.t_col.push_back((int)j); tk.t_blk.push_back(k); tk.t_n.push_back((int)n); tk.t_herm.push_back(herm ? 1 : 0);
      tk.t_slotptr.push_back((int64_t)tk.s_col.size());
      tk.t_udoff.push_back(A.psd_udoff[k]); tk.t_uoff.push_back(pt.uoff[k]); tk.t_ulen.push_back(ulen);
      tk.t_zoff.push_back(A.zlen); A.zlen += ulen; tk.c_zlen[j] += ulen;
      A.s1_maxulen = std::max(A.s1_maxulen, ulen);
      // slots: distinct columns of X_jk (real part first, then imaginary part for Hermitian blocks)
      int nslot = 0; sdm_int prevcol = -1; int prevpart = -1;
      for (sdm_int u = t; u < te; u++) {
        sdm_int q = in.Air[u] - in.psd_blkstart[k];
        int part = q >= n * n ? 1 : 0;
        sdm_int col = (q - part * n * n) / n;
        if (col != prevcol || part != prevpart) {
          tk.s_col.push_back((int)(col + part * n)); tk.s_nzptr.push_back((int64_t)u);
          nslot++; prevcol = col; prevpart = part;
        }
      }
      tk.t_nslot.push_back(nslot);
      tk.t_end.push_back((int64_t)te);   // per task: the end of its last slot (a slot before the last ends where the next one begins)
      t = te;
    }
    tk.c_taskptr[j + 1] = (int64_t)tk.t_col.size();
    if (tk.c_taskptr[j + 1] - tk.c_taskptr[j] > 1) A.one_task_per_col = false;
    A.zmaxj = std::max<int64_t>(A.zmaxj, tk.c_zlen[j]);
  }
  tk.s_nzptr.push_back(A.nnzA);   // sentinel (only used through per-task end pointers)
  A.ntask = (sdm_int)tk.t_col.size();
  A.h_taskptr = tk.c_taskptr; A.col0 = 0; A.col1 = m;
  // nonzeros of a task, as the span from its first nonzero to the next task's (the last task: to the end of At).  Where LP / Lorentz
  // nonzeros or columns without a PSD part lie in between, the span counts them too: an upper bound, which is all its users need
  // (the cost order below, and s1_maxnz -> s1_nzcap: the LDS that stage 1 reserves for the nonzeros of the largest task)
  // dispatch order of the stage-1 tasks: decreasing cost (nonzeros x order + slots x order^2), so that the few heavy
  // constraints do not form the tail of the launch
  std::vector<double> cost((size_t)A.ntask);
  tk.order.resize((size_t)A.ntask);
  A.s1_maxnz = 0;
  for (sdm_int t = 0; t < A.ntask; t++) {
    const int64_t nz = (t + 1 < A.ntask ? tk.s_nzptr[tk.t_slotptr[t + 1]] : A.nnzA) - tk.s_nzptr[tk.t_slotptr[t]];
    A.s1_maxnz = std::max(A.s1_maxnz, nz);
    tk.order[t] = (int)t;
    cost[t] = (double)nz * tk.t_n[t] + (double)tk.t_nslot[t] * tk.t_n[t] * tk.t_n[t];
  }
  std::stable_sort(tk.order.begin(), tk.order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
  // the generic kernel's dispatch order when there are many blocks (64 x 200): the hardware deals consecutive workgroups to the 8 XCDs
  // in turn, and every task re-reads rows of its block's D_k through its XCD's L2 -- with the constraints in natural order every D_k
  // was fetched by all eight L2s (246 MB of HBM traffic per launch against the 20 MB of the D_k).  So: block k's tasks go to XCD k % 8,
  // workgroup 8 s + x takes the s-th task of XCD x's list (heaviest first inside a list); lists that run out leave their turns to the rest.
  if (in.sdpN >= 16 && A.ntask > 0) {
    constexpr int NX = 8;
    std::vector<std::vector<int>> lst(NX);
    for (int t : tk.order) lst[tk.t_blk[t] % NX].push_back(t);
    tk.order_xcd.reserve(tk.order.size());
    std::vector<size_t> pos(NX, 0);
    while (tk.order_xcd.size() < tk.order.size())
      for (int x = 0; x < NX; x++) if (pos[x] < lst[x].size()) tk.order_xcd.push_back(lst[x][pos[x]++]);
  }
  return tk;
}

// one record per column for the prologue of k_psd_stage2_ell, column x of the table being constraint order[x] (null: x itself):
//   c64[8 x + ..] = first task, first PSD nonzero, end of the column, source offset in zbuf of its first four tasks
//   c32[16 x + ..] = the column, number of tasks, destination offset in z of the first four, their lengths
void ell_column_records(const AdaIn &in, const Stage1Tasks &tk, const std::vector<int> &zd, const int *order, DevBuf<long long> &d64, DevBuf<int> &d32) {
  const sdm_int m = in.m;
  std::vector<long long> c64((size_t)std::max<sdm_int>(m, 1) * 8, 0);
  std::vector<int> c32((size_t)std::max<sdm_int>(m, 1) * 16, 0);
  for (sdm_int x = 0; x < m; x++) {
    const sdm_int j = order ? order[(size_t)x] : x;
    const int64_t tb = tk.c_taskptr[j], te = tk.c_taskptr[j + 1];
    c64[8 * x] = tb; c64[8 * x + 1] = in.Ajc_psd[j]; c64[8 * x + 2] = in.Ajc[j + 1];
    c32[16 * x] = (int)j; c32[16 * x + 1] = (int)(te - tb);
    for (int sg = 0; sg < 4 && tb + sg < te; sg++) {
      c64[8 * x + 3 + sg] = tk.t_zoff[(size_t)(tb + sg)]; c32[16 * x + 2 + sg] = zd[(size_t)(tb + sg)]; c32[16 * x + 6 + sg] = tk.t_ulen[(size_t)(tb + sg)];
    }
  }
  d64.upload(c64); d32.upload(c32);
}

// ---- stage-2 fast path (dense-ish ADA patterns): the PSD nonzeros of At re-packed for one-row-per-lane sweeps (k_psd_stage2_ell).
// Rows (constraints) are sorted by their number of PSD nonzeros and cut into groups of 64; a group stores its
// nonzeros interleaved (entry t of all 64 rows contiguous) and padded to the longest row of the group, so that
// every load of the sweep is one coalesced 512-byte line and no cross-lane reduction is needed.  All wavefronts of
// a workgroup share every group (interleaved slices of the entry range).
// Decides A.ell_ok and uploads everything that only this path reads (so: nothing where it is not taken).
void stage2_ell(AdaPlan &A, const AdaIn &in, const PsdPatterns &pt, const Stage1Tasks &tk) {
  const sdm_int m = in.m, *Ajc = in.Ajc, *Ajc_psd = in.Ajc_psd;
  A.ell_ok = false;
  // z_j is staged in LDS at FULL length (all blocks, zeros where constraint j has no nonzero): an entry of the ELL
  // copy then carries its final position uoff[k] + upos and the sweep needs one LDS gather per entry and column
  const int64_t zmax = pt.uoff[in.sdpN];
  A.zmax = zmax;
  const double dens = m > 0 ? (double)in.ADAjc[m] / ((double)m * (double)m) : 0.0;
  const size_t lds = (size_t)zmax * sizeof(double);
  if (!(in.sdpN > 0 && pt.psdnnz > 0 && dens >= 0.2 && lds <= 96 * 1024 && !A.thread_per_row)) return;   // very short rows: one pattern entry per work-item instead
  std::vector<int> order(m);
  for (sdm_int j = 0; j < m; j++) order[j] = (int)j;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return Ajc[a + 1] - Ajc_psd[a] > Ajc[b + 1] - Ajc_psd[b]; });
  const int ng = (int)((m + 63) / 64);
  std::vector<int> grow((size_t)ng * 64, -1), glen(ng);
  std::vector<int64_t> goff(ng + 1, 0);
  for (int g = 0; g < ng; g++) {
    int len = 0;
    for (int l = 0; l < 64 && g * 64 + l < m; l++) { const int i = order[g * 64 + l]; grow[g * 64 + l] = i; len = std::max<int>(len, (int)(Ajc[i + 1] - Ajc_psd[i])); }
    glen[g] = len; goff[g + 1] = goff[g] + len;
  }
  std::vector<int> zp((size_t)A.nnzA, 0);                         // position of a PSD nonzero's entry in the full-length z vector
  for (sdm_int i = 0; i < m; i++) for (sdm_int t = Ajc_psd[i]; t < Ajc[i + 1]; t++) zp[(size_t)t] = (int)(pt.uoff[pt.Ablk[t]] + pt.Aupos[t]);
  std::vector<int> zd(tk.t_blk.size());                           // and of a task's block
  for (size_t t = 0; t < tk.t_blk.size(); t++) zd[t] = (int)pt.uoff[tk.t_blk[t]];
  std::vector<double> gval((size_t)goff[ng] * 64, 0.0);
  std::vector<int> gbu((size_t)goff[ng] * 64, 0);                 // position in the full-length z vector (padding: 0 with value 0)
  for (int g = 0; g < ng; g++)
    for (int l = 0; l < 64; l++) {
      const int i = grow[g * 64 + l];
      if (i < 0) continue;
      for (sdm_int t = Ajc_psd[i]; t < Ajc[i + 1]; t++) {
        const size_t pos = (size_t)(goff[g] + (t - Ajc_psd[i])) * 64 + l;
        gval[pos] = in.Apr[t]; gbu[pos] = zp[(size_t)t];
      }
    }
  A.ell_ng = ng;
  A.g_row.upload(grow); A.g_len.upload(glen); A.g_off.upload(goff); A.g_val.upload(gval); A.g_bu.upload(gbu);
  { std::vector<int> pos((size_t)m); for (sdm_int p = 0; p < m; p++) pos[(size_t)order[p]] = (int)p; A.ell_pos.upload(pos); }
  A.ell_order.upload(order);
  A.ell_full = (in.ADAjc[m] == (sdm_int)m * m);                    // every column of the pattern full: (j, i) sits at ADAjc[i] + j
  A.d_uoff.upload(pt.uoff); A.d_Azpos.upload(zp); A.t_zdst.upload(zd);
  ell_column_records(in, tk, zd, nullptr, A.cdc64, A.cdc32);        // indexed by column
  ell_column_records(in, tk, zd, order.data(), A.cdp64, A.cdp32);   // and by ELL position
  A.ell_ok = true;
}

// ---- transposed-entry map of the ADA pattern (d_ADAT: k_symmetrize): for entry e=(i,j): find (j,i) by binary search in column i
std::vector<int> ada_transpose_map(const AdaIn &in) {
  const sdm_int m = in.m, *ADAjc = in.ADAjc, *ADAir = in.ADAir;
  std::vector<int> adaT((size_t)ADAjc[m], -1);
  for (sdm_int j = 0; j < m; j++)
    for (sdm_int e = ADAjc[j]; e < ADAjc[j + 1]; e++) {
      sdm_int i = ADAir[e];
      const sdm_int *b = ADAir + ADAjc[i], *en = ADAir + ADAjc[i + 1];
      const sdm_int *f = std::lower_bound(b, en, j);
      if (f != en && *f == j) adaT[e] = (int)(f - ADAir);
    }
  return adaT;
}

// ---- dense-column form of the LP / Lorentz part.  A sparse-sparse dot per ADA' entry (k_ada_spdot) is the right
// tool for sparse columns; when the columns are dense-ish (nb.mat: 66 %) the same sums are a weighted Gram matrix
// A' diag(dsqr) A, i.e. GEMM-shaped work for the matrix cores.  Static data (At) is expanded once here.
// Decides A.lq_dense / A.q_dense and uploads what k_gram_tile, k_q_densify and k_lq_q_prep read; released where not taken.
void lq_dense_forms(AdaPlan &A, const AdaIn &in) {
  const sdm_int m = in.m, lorN = in.lorN;
  sdm_int nz = 0;
  for (sdm_int j = 0; j < m; j++) nz += in.Ajc_psd[j] - in.Ajc[j];
  const double cells = (double)A.nlq * (double)m;
  A.lq_dense = A.nlq > 0 && m > 1 && nz > 0 && (double)nz >= 0.10 * cells && cells * 8.0 <= 1.0e9;
  A.q_dense = lorN > 0 && A.nnzQ > 0 && (double)A.nnzQ >= 0.10 * (double)lorN * (double)m && (double)lorN * m * 8.0 <= 1.0e9;
  if (A.lq_dense) {
    std::vector<double> D((size_t)A.nlq * (size_t)m, 0.0);
    for (sdm_int j = 0; j < m; j++)
      for (sdm_int t = in.Ajc[j]; t < in.Ajc_psd[j]; t++) D[(size_t)j * (size_t)A.nlq + (size_t)in.Air[t]] = in.Apr[t];
    A.Alq_d.upload(D);
  } else A.Alq_d.release();
  if (A.q_dense) {
    std::vector<int64_t> dst((size_t)A.nnzQ);
    for (sdm_int j = 0; j < m; j++)
      for (sdm_int t = in.Qjc[j]; t < in.Qjc[j + 1]; t++) dst[(size_t)t] = (int64_t)j * lorN + in.Qir[t];
    A.q_dst.upload(dst);
    A.Q_d.alloc((size_t)lorN * (size_t)m);
    if (A.lq_dense && (double)lorN * (double)m <= 1.6e7) {          // inverse map for the fused form (ada_lq_q)
      std::vector<int> src((size_t)lorN * (size_t)m, -1);
      for (sdm_int t = 0; t < A.nnzQ; t++) src[(size_t)dst[(size_t)t]] = (int)t;
      A.q_src.upload(src);
    } else A.q_src.release();
  } else { A.Q_d.release(); A.q_dst.release(); A.q_src.release(); }
  if (A.lq_dense || A.q_dense) {
    const int nt = (int)((m + TILE - 1) / TILE), T = nt * (nt + 1) / 2;
    const sdm_int rows = std::max(A.lq_dense ? A.nlq : 0, A.q_dense ? lorN : 0);
    A.gram_split = (int)std::max<sdm_int>(1, std::min<sdm_int>((rows + TILE - 1) / TILE, std::max(1, 512 / T)));
    A.gram_part.alloc((size_t)A.gram_split * (size_t)m * (size_t)m);
  } else A.gram_part.release();
}

// Everything every path reads goes to the device here: At, the patterns of DAt.q and ADA', the tables of the first two steps, the
// work arrays; then the LDS budget of stage 1
void upload_tables(AdaPlan &A, const AdaIn &in, const PsdPatterns &pt, const Stage1Tasks &tk, const std::vector<int> &adaT) {
  const sdm_int m = in.m, lorN = in.lorN, sdpN = in.sdpN;
  // ---- dsqr source codes (getada1.c:106-118): -1 -> dl[r];  -2-k -> -ddet[k];  k>=0 -> ddet[k]
  { std::vector<int> code((size_t)A.nlq, -1);
    for (sdm_int r = in.lpN; r < in.lpN + lorN && r < A.nlq; r++) code[r] = (int)(-2 - (r - in.lpN));
    for (sdm_int k = 0; k < lorN; k++)
      for (sdm_int r = in.qblkstart[k]; r < in.qblkstart[k + 1] && r < A.nlq; r++) code[r] = (int)k;
    A.dsqr_code.upload(code); }
  A.d_Ajc.upload(in.Ajc, (size_t)m + 1); A.d_Ajc_psd.upload(in.Ajc_psd, (size_t)m);
  upload_narrow(A.d_Air, in.Air, A.nnzA);
  A.d_Apr.upload(in.Apr, (size_t)A.nnzA);
  A.d_Ablk.upload(pt.Ablk); A.d_Aupos.upload(pt.Aupos);
  { std::vector<int64_t> v(m + 1, 0); if (lorN > 0) v.assign(in.Qjc, in.Qjc + m + 1); A.d_Qjc.upload(v); }
  upload_narrow(A.d_Qir, in.Qir, A.nnzQ);
  A.d_ADAjc.upload(in.ADAjc, (size_t)m + 1);
  upload_narrow(A.d_ADAir, in.ADAir, in.ADAjc[m]);
  A.d_ADAT.upload(adaT);
  { std::vector<int> upos((size_t)pt.uoff[sdpN]), urc(upos.size(), 0);   // urc: (r << 16) | c of a real block's target (k_psd_stage1_mfma: no division per target)
    for (sdm_int k = 0; k < sdpN; k++) std::copy(pt.U[k].begin(), pt.U[k].end(), upos.begin() + pt.uoff[k]);
    for (sdm_int k = 0; k < std::min(sdpN, in.rsdpN); k++) {
      const int n = (int)A.psd_n[k];
      if (n >= 65536) continue;
      for (size_t u = 0; u < pt.U[k].size(); u++) { const int q = pt.U[k][u], c = q / n, r = q - c * n; urc[(size_t)pt.uoff[k] + u] = (r << 16) | c; }
    }
    A.u_pos.upload(upos); A.u_rc.upload(urc); }
  A.t_col.upload(tk.t_col); A.t_blk.upload(tk.t_blk); A.t_n.upload(tk.t_n); A.t_nslot.upload(tk.t_nslot); A.t_ulen.upload(tk.t_ulen);
  A.t_herm.upload(tk.t_herm); A.t_order.upload(tk.order);
  if (tk.order_xcd.empty()) A.t_order_xcd.release(); else A.t_order_xcd.upload(tk.order_xcd);
  A.t_slotptr.upload(tk.t_slotptr); A.t_udoff.upload(tk.t_udoff); A.t_uoff.upload(tk.t_uoff); A.t_zoff.upload(tk.t_zoff);
  A.s_col.upload(tk.s_col); A.s_nzptr.upload(tk.s_nzptr); A.c_taskptr.upload(tk.c_taskptr); A.c_zlen.upload(tk.c_zlen);
  A.t_end.upload(tk.t_end);
  { std::vector<int64_t> v(A.psd_start.begin(), A.psd_start.end()); if (v.empty()) v.push_back(0); A.d_psd_start.upload(v); }
  { std::vector<int64_t> v(lorN + 1, A.nlq); for (sdm_int k = 0; k <= lorN && lorN > 0; k++) v[k] = in.qblkstart[k]; A.d_qblk.upload(v); }
  A.zbuf.alloc((size_t)std::max<int64_t>(A.zlen, 1));
  A.dsqr.alloc((size_t)std::max<sdm_int>(A.nlq, 1));
  A.dl.alloc((size_t)std::max<sdm_int>(in.lpN, 1)); A.ddet.alloc((size_t)std::max<sdm_int>(lorN, 1));
  A.qpr.alloc((size_t)std::max<sdm_int>(A.nnzQ, 1)); A.udsqr.alloc((size_t)std::max<sdm_int>(A.lenud, 1));
  A.q1.alloc((size_t)std::max<sdm_int>(lorN, 1));
  A.q2.alloc((size_t)std::max<sdm_int>(lorN > 0 ? in.qblkstart[lorN] - in.qblkstart[0] : 0, 1));
  A.symtmp.alloc((size_t)std::max<sdm_int>(in.ADAjc[m], 1));
  // LDS budget for stage 1: Y chunk of CC slots x n rows
  const size_t need = (size_t)(sdpN > in.rsdpN ? 4 : 2) * (size_t)A.maxn * sizeof(double);     // one slot: Y (+Yi) and D(col,:) (+Im)
  A.stage1_lds = std::max<size_t>(96 * 1024, need);
  if (A.stage1_lds > 136 * 1024) throw std::runtime_error("PSD block too large for the LDS-staged D*A*D kernel (n > 8700)");
}

}  // namespace

// ============================================================ host analysis
void ada_build(sdm_plan *P, sdm_int N, sdm_int m, const sdm_int *Ajc, const sdm_int *Air, const double *Apr, const sdm_int *Ajc_psd, sdm_int lpN,
               sdm_int lorN, sdm_int sdpN, sdm_int rsdpN, const sdm_int *sdpNL, const sdm_int *qblkstart, const sdm_int *psd_blkstart,
               const sdm_int *Qjc, const sdm_int *Qir, const sdm_int *ADAjc, const sdm_int *ADAir) {
  AdaPlan &A = P->ada;
  const AdaIn in = {m, Ajc, Air, Apr, Ajc_psd, lpN, lorN, sdpN, rsdpN, sdpNL, qblkstart, psd_blkstart, Qjc, Qir, ADAjc, ADAir};
  A.N = N; A.m = m; A.nnzA = Ajc[m]; A.lpN = lpN; A.lorN = lorN; A.sdpN = sdpN; A.rsdpN = rsdpN;
  A.ic_n.release(); A.ufac.release();                                // invcholfac tables belong to the old cone
  if (A.nnzA >= (sdm_int)1 << 31 || N >= (sdm_int)1 << 31) throw std::runtime_error("At too large for 32-bit row indices");
  A.nlq = sdpN > 0 ? psd_blkstart[0] : N;
  if (lorN > 0 && qblkstart[lorN] != A.nlq && sdpN > 0) throw std::runtime_error("qblkstart / psd_blkstart mismatch");
  const PsdPatterns pt = psd_patterns(A, in);
  A.thread_per_row = (m > 0 && pt.psdnnz / (double)m < 48.0);     // short rows: one pattern entry per work-item, else per wavefront
  A.nnz_lq = A.nnzA - pt.psdnnz;                                   // LP + Lorentz nonzeros of At
  A.nnzQ = lorN > 0 ? Qjc[m] : 0;
  A.lq_maxcol = 0; A.q_maxcol = 0;                                 // (longest columns: lanes per pattern entry of k_ada_spdot)
  for (sdm_int j = 0; j < m; j++) A.lq_maxcol = std::max<int64_t>(A.lq_maxcol, in.psd_begin(j) - Ajc[j]);
  for (sdm_int j = 0; j < m && lorN > 0; j++) A.q_maxcol = std::max<int64_t>(A.q_maxcol, Qjc[j + 1] - Qjc[j]);
  const Stage1Tasks tk = stage1_tasks(A, in, pt);
  stage2_ell(A, in, pt, tk);
  upload_tables(A, in, pt, tk, ada_transpose_map(in));
  lq_dense_forms(A, in);
  P->has_ada = true;
}

}  // namespace sdm
