// sdm_solve_inv.hip -- the EXPLICIT INVERSES of the diagonal super-blocks that the triangular solves (sdm_solve.hip) apply: built once per
// factorisation into the arena S (and its transposed copy ST) whose layout and work lists sdm_solve_build.hip plans:
//   * 128-column leaves: 32x32 by substitution in registers, then two levels of  X21 = -inv(C) B inv(A)  on the FP64
//     matrix cores, all inside one workgroup (k_sinv128);
//   * combine levels 256, 512, ... W: the same identity on 64x64 product tiles (k_stile), two dependent stages per
//     level (T = B inv(A), then X21 = -inv(C) T); small problems run all of it as ONE launch with completion
//     counters between the stages (k_sprep);
//   * fronts factored by one k_ldl_front launch: behind that launch, following its progress (k_sinv_follow; the body is in sdm_follow.h);
//   * fronts of several super-blocks: the transposed copy LT of the rows of L below each super-block (k_ltrans).
// The growth of every super-block, max|inv(L_PP)| * max|L_PP|, is measured here (sb_g) and decides in the sweeps how the block is applied.
#include "sdm_follow.h"
#include <algorithm>

namespace sdm {

// Leaves.  One workgroup per 128-column block h of a front, bottom-up, everything in LDS / registers:
//   32x32  each of the four wavefronts inverts one 32x32 unit lower triangular diagonal block by columns (lane j owns
//          column j of the inverse in registers; the entries of L come as broadcast LDS reads at compile-time offsets);
//   64x64  X10 = -inv(A11) (A10 inv(A00)) for the two 64-column blocks A and C (matrix cores, two wavefronts each);
//   128    X21 = -inv(C) (B inv(A)) on the FP64 matrix cores, B = L(C rows, A columns) requested at the very start.
// Results go to S; max|inv| and max|L| to sb_g (growth check).
template <bool WT>
__device__ __forceinline__ void sinv128_body(char *smem, const double *__restrict__ F, double *__restrict__ S, double *__restrict__ STr, const FrontTab &tab,
                                             const int *it, unsigned long long *sb_g, int W) {
  double *bufA = (double *)smem, *bufC = bufA + 64 * TP, *bufB = bufC + 64 * TP, *bufT = bufB + 64 * TP;
  const int s = it[0], h = it[1];
  const int ns = tab.ns[s], ld = tab.ld[s], sld = tab.sld[s];
  const double *Fs = F + tab.foff[s];
  const int k0 = 128 * h, nbA = min(64, ns - k0), nbC = max(0, min(64, ns - k0 - 64));
  const int Pb = k0 / W, kl = k0 - Pb * W;                          // super-block of the leaf, its first column inside it
  double *Ss = S + tab.soff[s] + (int64_t)Pb * W * sld;
  double *Ts = STr + tab.soff[s] + (int64_t)Pb * W * sld;           // the transposed copy: Ts[r*sld + c] = inverse(r, c)
  unsigned long long *gP = sb_g + 2 * (tab.sboff[s] + Pb);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double vB[SPT];
  SDM_PHASE_BEGIN();
  if (nbC > 0) stage_colmajor_load(vB, Fs + (int64_t)k0 * ld + k0 + 64, ld, nbC, 64, tid);     // B(row, k) = L(k0+64+row, k0+k)
  // raw strictly lower triangles, column-major: rawA[k*TP + i] = L(k0+i, k0+k) (bufT), rawC likewise (bufB); the
  // destination buffers start as zero
  double *rawA = bufT, *rawC = bufB;
  double lmx = 0.0;
  {
    double va[SPT], vc[SPT];
    const int i = tid & 63, kq = tid >> 6;
#pragma unroll
    for (int j = 0; j < SPT; j++) {
      const int k = kq + (ST / 64) * j;
      va[j] = Fs[(int64_t)(k0 + min(k, nbA - 1)) * ld + k0 + min(i, nbA - 1)];
      vc[j] = nbC > 0 ? Fs[(int64_t)(k0 + 64 + min(k, nbC - 1)) * ld + k0 + 64 + min(i, nbC - 1)] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < SPT; j++) {
      const int k = kq + (ST / 64) * j;
      const double a = (i > k && i < nbA) ? va[j] : 0.0, c = (i > k && i < nbC) ? vc[j] : 0.0;
      rawA[k * TP + i] = a; rawC[k * TP + i] = c;
      bufA[k * TP + i] = 0.0; bufC[k * TP + i] = 0.0;
      lmx = fmax(lmx, fmax(fabs(a), fabs(c)));
    }
  }
  __syncthreads();
  SDM_PHASE(0);
  inv64_pair(rawA, rawC, bufA, bufC, wave, lane, gP);
  SDM_PHASE(3);
  __syncthreads();                                                  // bufA = inv(A) (B operand), bufC = inv(C) (A operand); raw buffers free
  if (nbC > 0) lmx = fmax(lmx, stage_colmajor_store(bufB, vB, nbC, 64, tid));
  wave_atomic_max(gP + 1, lmx, lane);
  // inverses to S (lower triangles incl. the unit diagonal; the upper triangles of S are zero and stay zero)
  for (int e = tid; e < 64 * 64; e += ST) {
    const int i = e & 63, j = e >> 6;
    if (i >= j && i < nbA) { if (WT) sdm_store_wt(&Ss[(int64_t)(kl + j) * sld + kl + i], bufA[i * TP + j]); else Ss[(int64_t)(kl + j) * sld + kl + i] = bufA[i * TP + j]; }
    if (i >= j && i < nbC) { if (WT) sdm_store_wt(&Ss[(int64_t)(kl + 64 + j) * sld + kl + 64 + i], bufC[j * TP + i]); else Ss[(int64_t)(kl + 64 + j) * sld + kl + 64 + i] = bufC[j * TP + i]; }
  }
  for (int e = tid; e < 64 * 64; e += ST) {                           // transposed copy: consecutive work-items on consecutive columns j
    const int j = e & 63, i = e >> 6;
    if (i >= j && i < nbA) { if (WT) sdm_store_wt(&Ts[(int64_t)(kl + i) * sld + kl + j], bufA[i * TP + j]); else Ts[(int64_t)(kl + i) * sld + kl + j] = bufA[i * TP + j]; }
    if (i >= j && i < nbC) { if (WT) sdm_store_wt(&Ts[(int64_t)(kl + 64 + i) * sld + kl + 64 + j], bufC[j * TP + i]); else Ts[(int64_t)(kl + 64 + i) * sld + kl + 64 + j] = bufC[j * TP + i]; }
  }
  SDM_PHASE(4);
  if (nbC <= 0) return;
  __syncthreads();
  Acc22 acc;
  acc_zero(acc);
  mma_block(acc, bufB, bufA, wave, lane);                           // T = B inv(A)
  acc_to_lds_rowmajor(acc, bufT, wave, lane, 1.0);                  // bufT[k*TP + col] = T(k, col): a B operand
  __syncthreads();
  acc_zero(acc);
  mma_block(acc, bufC, bufT, wave, lane);                           // inv(C) T
  __syncthreads();                                                  // bufB is free: stage the result for coalesced stores
  acc_to_lds_rowmajor(acc, bufB, wave, lane, -1.0);
  __syncthreads();
  SDM_PHASE(5);
  const double gm = store_tile<WT>(Ss + (int64_t)kl * sld + kl + 64, sld, bufB, nbC, 64, tid);
  store_tile_T<WT>(Ts + (int64_t)(kl + 64) * sld + kl, sld, bufB, nbC, 64, tid);
  wave_atomic_max(gP, gm, lane);
  SDM_PHASE(6);
}
__global__ void __launch_bounds__(ST)
k_sinv128(const double *__restrict__ F, double *__restrict__ S, double *__restrict__ STr, FrontTab tab, const int *items, unsigned long long *sb_g, int W) {
  SDM_DYN_SMEM(smem);
  sinv128_body<false>(smem, F, S, STr, tab, items + 4 * blockIdx.x, sb_g, W);
}

// Combine levels.  Level lev joins the inverses of neighbouring column ranges of half width h = 128 << lev inside a
// super-block:  inv([A 0; B C]) = [inv(A) 0; -inv(C) B inv(A), inv(C)]  with A = columns a0 .. a0+h-1, C = the nc <= h
// columns behind them.  One 64x64 tile of one of the two products per item {s, Pb, lev, pair, I, J, stage, wait}:
//   stage 0  T(I, J)   =   sum_{K >= J} B(I, K) inv(A)(K, J)        B = L(C rows, A columns) from the factor; T into the scratch arena
//   stage 1  X21(I, J) = - sum_{K <= I} inv(C)(I, K) T(K, J)        into S
// (both triangular in K: only the 64-blocks that can be non-zero are multiplied).
template <bool WT>
__device__ __forceinline__ void stile_body(char *smem, const double *F, double *S, double *STr, double *T, const FrontTab &tab, const int *it,
                                           unsigned long long *sb_g, int W) {
  double *As = (double *)smem, *Bs = As + 64 * TP;
  const int s = it[0], Pb = it[1], lev = it[2], pi = it[3], I = it[4], J = it[5], stage = it[6];
  const int ns = tab.ns[s], ld = tab.ld[s], sld = tab.sld[s];
  const int P0 = Pb * W, nb = min(W, ns - P0);
  const int h = 128 << lev, a0 = pi * 2 * h, nc = min(h, nb - a0 - h);
  const double *Fs = F + tab.foff[s];
  double *Sb = S + tab.soff[s] + (int64_t)P0 * sld, *Tb = T + tab.soff[s] + (int64_t)P0 * sld;
  unsigned long long *gP = sb_g + 2 * (tab.sboff[s] + Pb);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double *Ap, *Bp; double *Cp;
  int64_t lda, ldb;
  const int arows = min(64, nc - 64 * I);
  int kvalid;
  if (stage == 0) {
    kvalid = h - 64 * J;
    Ap = Fs + (int64_t)(P0 + a0 + 64 * J) * ld + P0 + a0 + h + 64 * I; lda = ld;
    Bp = Sb + (int64_t)(a0 + 64 * J) * sld + a0 + 64 * J; ldb = sld;
    Cp = Tb + (int64_t)(a0 + 64 * J) * sld + a0 + h + 64 * I;
  } else {
    kvalid = min(64 * (I + 1), nc);
    Ap = Sb + (int64_t)(a0 + h) * sld + a0 + h + 64 * I; lda = sld;
    Bp = Tb + (int64_t)(a0 + 64 * J) * sld + a0 + h; ldb = sld;
    Cp = Sb + (int64_t)(a0 + 64 * J) * sld + a0 + h + 64 * I;
  }
  Acc22 acc;
  acc_zero(acc);
  double lmx = 0.0;
  double va[SPT], vb[SPT];
  SDM_PHASE_BEGIN();
  stage_colmajor_load<WT>(va, Ap, lda, arows, kvalid, tid);
  stage_transposed_load<WT>(vb, Bp, ldb, kvalid, 64, tid);
  for (int kb = 0; kb < kvalid; kb += 64) {
    lmx = fmax(lmx, stage_colmajor_store(As, va, arows, kvalid - kb, tid));
    stage_transposed_store(Bs, vb, kvalid - kb, 64, tid);
    __syncthreads();
    if (kb + 64 < kvalid) {                                          // next K block: loads in flight during the products
      stage_colmajor_load<WT>(va, Ap + (int64_t)(kb + 64) * lda, lda, arows, kvalid - kb - 64, tid);
      stage_transposed_load<WT>(vb, Bp + kb + 64, ldb, kvalid - kb - 64, 64, tid);
    }
    mma_block(acc, As, Bs, wave, lane);
    __syncthreads();
  }
  SDM_PHASE(8 + 4 * stage);
  if (stage == 0) wave_atomic_max(gP + 1, lmx, lane);                // max |L| over the off-diagonal blocks of the super-block
  acc_to_lds_rowmajor(acc, As, wave, lane, stage == 0 ? 1.0 : -1.0);
  __syncthreads();
  const double gm = store_tile<WT>(Cp, sld, As, arows, 64, tid);
  if (stage == 1) {
    store_tile_T<WT>(STr + tab.soff[s] + (int64_t)P0 * sld + (int64_t)(a0 + h + 64 * I) * sld + a0 + 64 * J, sld, As, arows, 64, tid);
    wave_atomic_max(gP, gm, lane);                                   // max |inverse|
  }
  SDM_PHASE(9 + 4 * stage);
}
__global__ void __launch_bounds__(ST)
k_stile(const double *F, double *S, double *STr, double *T, FrontTab tab, const int *items, unsigned long long *sb_g, int W) {
  SDM_DYN_SMEM(smem);
  stile_body<false>(smem, F, S, STr, T, tab, items + 8 * blockIdx.x, sb_g, W);
}

// ---- all of the above in ONE launch for problems whose items fit the device at once (k_sprep): workgroups take the
// items in the order leaves, level 0 stage T, level 0 stage X, level 1 stage T, ... and wait on per-super-block completion
// counters instead of on launch boundaries.  Producers store write-through and count after their stores are
// acknowledged; consumers poll relaxed and read with sc1 loads.
// cnt[SPREP_NCNT * sb + 0] = finished leaves, [1 + st] = finished tiles of stage st (zeroed with sb_g by k_prep_pivots).
__global__ void __launch_bounds__(ST)
k_sprep(const double *F, double *S, double *STr, double *T, FrontTab tab, const int *l_i128, int n_i128, const int *l_items,
        unsigned long long *sb_g, int *cnt, int W, int *tmo) {
  SDM_DYN_SMEM(smem);
  const int b = blockIdx.x;
  if (b < n_i128) {
    const int *it = l_i128 + 4 * b;
    sinv128_body<true>(smem, F, S, STr, tab, it, sb_g, W);
    prep_done(cnt + SPREP_NCNT * (tab.sboff[it[0]] + (128 * it[1]) / W));
    return;
  }
  const int *it = l_items + 8 * (b - n_i128);
  const int st = 2 * it[2] + it[6];
  int *c = cnt + SPREP_NCNT * (tab.sboff[it[0]] + it[1]);
  prep_wait(c + st, it[7], tmo);
  stile_body<true>(smem, F, S, STr, T, tab, it, sb_g, W);
  prep_done(c + st + 1);
}

// ---- the inverse of a whole front BEHIND its factorisation: the body is sinv_follow_body (sdm_follow.h); this kernel runs it where
// the k_ldl_front launch does not carry the follower's workgroups itself (the emulator; captured graphs of older plans)
__global__ void __launch_bounds__(ST)
k_sinv_follow(const double *F, const double *DT, double *S, double *STr, FrontTab tab, const int *list, int *front_cnt, const int *diag_cnt,
              unsigned long long *sb_g, int *tmo) {
  SDM_DYN_SMEM(smem);
  const FollowDesc fd = follow_desc(tab, list, (int)blockIdx.y);
  sinv_follow_body(smem, (int)blockIdx.x, fd, F, DT, S, STr, front_cnt, diag_cnt, sb_g, tmo);
}

// transposed copy of the rows of L below super-block Pb of a front (64x64 tiles through LDS): LT[r*W + c] = L((Pb+1) W + r, Pb W + c)
__global__ void __launch_bounds__(ST)
k_ltrans(const double *__restrict__ F, double *__restrict__ LT, FrontTab tab, const int *items, int W) {
  __shared__ double t[64][65];
  const int *it = items + 4 * blockIdx.x;
  const int s = it[0], Pb = it[1], I = it[2], J = it[3];
  const int ns = tab.ns[s], ld = tab.ld[s];
  const int R0 = (Pb + 1) * W, nr = ns - R0;
  const double *src = F + tab.foff[s] + (int64_t)(Pb * W + 64 * J) * ld + R0 + 64 * I;       // (row i, column c) at src[c*ld + i]
  double *dst = LT + tab.ltoff[s] + lt_boff(ns, W, Pb) + (int64_t)(64 * I) * W + 64 * J;
  const int tid = threadIdx.x, a = tid & 63, b = tid >> 6;
  const int nri = min(64, nr - 64 * I);
  for (int c = b; c < 64; c += ST / 64) t[c][a] = a < nri ? src[(int64_t)c * ld + a] : 0.0;
  __syncthreads();
  for (int i = b; i < 64; i += ST / 64) if (i < nri) dst[(int64_t)i * W + a] = t[a][i];
}

static void solve_attrs() {
#ifndef SDM_EMU
  static bool attr = false;
  if (!attr) {
    SDM_HIP_CHECK(hipFuncSetAttribute((const void *)k_sinv128, hipFuncAttributeMaxDynamicSharedMemorySize, (int)INV_LDS));
    SDM_HIP_CHECK(hipFuncSetAttribute((const void *)k_stile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TILE_LDS));
    SDM_HIP_CHECK(hipFuncSetAttribute((const void *)k_sprep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)INV_LDS));
    SDM_HIP_CHECK(hipFuncSetAttribute((const void *)k_sinv_follow, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TILE_LDS));
    attr = true;
  }
#endif
}
// does one workgroup of k_sinv_follow fit a compute unit of the current device?  (follow_decide, sdm_solve_build.hip; the emulator has no such limit)
bool solve_follow_fits() {
#ifdef SDM_EMU
  return true;
#else
  int per_cu = 0;
  solve_attrs();
  SDM_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_sinv_follow, ST, TILE_LDS));
  return per_cu >= 1;
#endif
}
// the inverses of the fronts of level l behind their factorisation: launched on stream st right after (next to) k_ldl_front
void solve_follow(sdm_plan *P, int l, hipStream_t st) {
  CholPlan &C = P->chol;
  solve_attrs();
  C.growth_used = C.growth_max;
  const int nfr = C.levptr[l + 1] - C.levptr[l];
  SDM_KLAUNCH_ON(P, st, k_sinv_follow, dim3(C.lev_followT[l], nfr), dim3(ST), TILE_LDS, C.fronts.p, C.frontsT.p, C.S.p, C.ST.p, front_tab(C),
                 C.d_levlist.p + C.levptr[l], C.front_cnt.p, C.diag_cnt.p, C.sb_g.p, C.tmo.dev());
}
void solve_prepare(sdm_plan *P, bool sb_g_is_zero) {
  CholPlan &C = P->chol;
  FrontTab tab = front_tab(C);
  solve_attrs();
  C.growth_used = C.growth_max;                                     // the solves decide with the bound in force here
  const size_t gw = (size_t)std::max(C.nsbtot, 1) * (2 + SPREP_NCNT / 2);
  if (!sb_g_is_zero)                                                // (a factorisation zeroes them in k_prep_pivots)
    SDM_HIP_CHECK(hipMemsetAsync(C.sb_g.p, 0, gw * sizeof(unsigned long long), P->stream));
  const int W = C.sbw;
  if (C.n_lt) SDM_KLAUNCH(P, k_ltrans, dim3(C.n_lt), dim3(ST), 0, C.fronts.p, C.LT.p, tab, C.l_lt.p, W);
  if (C.n_i128 == 0) return;
  if (C.n_i128 + C.n_items <= SPREP_MAX_ITEMS && !C.sprep_off) {    // everything resident at once: one launch, counters instead of boundaries
    // (the emulator, where the test asks for it: as on the device, its workgroups wait for each other's counters -- one process each)
    SDM_KLAUNCH_WAITING(P, 200, k_sprep, dim3(C.n_i128 + C.n_items), dim3(ST), INV_LDS, C.fronts.p, C.S.p, C.ST.p, C.Tarena.p, tab, C.l_i128.p, C.n_i128,
                        C.l_items.p, C.sb_g.p, (int *)(C.sb_g.p + 2 * std::max(C.nsbtot, 1)), W, C.tmo.dev());
    return;
  }
  SDM_KLAUNCH(P, k_sinv128, dim3(C.n_i128), dim3(ST), INV_LDS, C.fronts.p, C.S.p, C.ST.p, tab, C.l_i128.p, C.sb_g.p, W);
  for (int st = 0; st < 2 * SINV_MAXLEV; st++) {
    const int n = C.stage_ptr[st + 1] - C.stage_ptr[st];
    if (n > 0) SDM_KLAUNCH(P, k_stile, dim3(n), dim3(ST), TILE_LDS, C.fronts.p, C.S.p, C.ST.p, C.Tarena.p, tab, C.l_items.p + 8 * (size_t)C.stage_ptr[st], C.sb_g.p, W);
  }
}

// growth statistics of the last solve_prepare (host read-back; tests and bench reporting)
void solve_stats(sdm_plan *P, sdm_int *nblocks, sdm_int *nbad, double *max_growth) {
  CholPlan &C = P->chol;
  std::vector<unsigned long long> g((size_t)std::max(2 * C.nsbtot, 2));
  SDM_HIP_CHECK(hipStreamSynchronize(P->stream));
  SDM_HIP_CHECK(hipMemcpy(g.data(), C.sb_g.p, g.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  sdm_int bad = 0; double mx = 0.0;
  for (int i = 0; i < C.nsbtot; i++) {
    union { unsigned long long u; double d; } a, b; a.u = g[2 * i]; b.u = g[2 * i + 1];
    const double gr = a.d * b.d;
    if (!(gr <= C.growth_used)) bad++;
    if (gr > mx || gr != gr) mx = gr;
  }
  if (nblocks) *nblocks = C.nsbtot;
  if (nbad) *nbad = bad;
  if (max_growth) *max_growth = mx;
}

}  // namespace sdm

#if defined(SDM_PHASES) && !defined(SDM_EMU)
// tools-only build (python -m sedumi_amd.build --phases): read / reset the in-kernel phase clocks of this file
extern "C" int sdm_debug_phases_solve(unsigned long long *out32, int reset) {
  if (out32 && hipMemcpyFromSymbol(out32, HIP_SYMBOL(sdm_phase_acc), 32 * sizeof(unsigned long long)) != hipSuccess) return 1;
  if (reset) { unsigned long long z[32] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(sdm_phase_acc), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif
