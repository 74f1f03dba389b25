// sdm_cone_dev.h -- what the kernels over lists of PSD blocks share (sdm_cone.hip, sdm_psdfact.hip): the block tables as a kernel argument and
// the matrix-core blocking of a 64 x 64 output tile.
#pragma once
#include "sdm_plan.h"

namespace sdm {

struct ConeBlk { const int *n; const int64_t *off, *foff; const int *herm, *loff; };   // per block: order, offset in x / Qb, in frms, Hermitian?, offset in lab
inline ConeBlk cone_blk(const ConeTabs &T) { ConeBlk B; B.n = T.n; B.off = T.off; B.foff = T.foff; B.herm = T.herm; B.loff = T.loff; return B; }

// 64 x 64 output tiles, 4 wavefronts of 2 x 2 v_mfma_f64_16x16x4_f64 tiles each; operands staged in LDS as As[k][row], Bs[k][col], pitch CN_P.
// Entry r of acc.t[i][j] is (row, col) = (32 (wave & 1) + 16 i + (lane >> 4) + 4 r, 32 (wave >> 1) + 16 j + (lane & 15)) of the tile.
constexpr int CN_T = 256, CN_P = 65;
struct ConeAcc { sdm_double4 t[2][2]; };

__device__ __forceinline__ void cone_mma(ConeAcc &acc, const double *As, const double *Bs, int wave, int lane) {
  const int rb = 32 * (wave & 1) + (lane & 15), cb = 32 * (wave >> 1) + (lane & 15), kq = lane >> 4;
#pragma unroll 4
  for (int kk = 0; kk < 64; kk += 4) {
    const double a0 = As[(kk + kq) * CN_P + rb], a1 = As[(kk + kq) * CN_P + rb + 16];
    const double b0 = Bs[(kk + kq) * CN_P + cb], b1 = Bs[(kk + kq) * CN_P + cb + 16];
    acc.t[0][0] = SDM_MFMA_F64_16x16x4(a0, b0, acc.t[0][0]);
    acc.t[0][1] = SDM_MFMA_F64_16x16x4(a0, b1, acc.t[0][1]);
    acc.t[1][0] = SDM_MFMA_F64_16x16x4(a1, b0, acc.t[1][0]);
    acc.t[1][1] = SDM_MFMA_F64_16x16x4(a1, b1, acc.t[1][1]);
  }
}

}  // namespace sdm
