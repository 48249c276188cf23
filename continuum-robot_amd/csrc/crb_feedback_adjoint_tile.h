// crb_feedback_adjoint_tile.h -- the tile shape and the MFMA step the matrix products of the closed-loop adjoints share
// (crb_feedback_adjoint.h: the RK4 loop; crb_implicit_feedback_adjoint.h: the sampled-data implicit loop): 256 threads, a
// 32 x 32 output tile, each wave one 16 x 16 tile of v_mfma_f64_16x16x4_f64, K in steps of 32.  The LDS layouts and why they
// are what they are: crb_feedback_adjoint.h.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_generic.h"

namespace crb {

constexpr int FBA_T = 32;            // output tile edge and K step
constexpr int FBA_LDK = FBA_T + 2;   // doubles per row of a [row][k] tile
constexpr int FBA_LDM = FBA_T + 16;  // doubles per row of a [k][col] tile
constexpr int FBA_Q = FBA_T * FBA_T / 256;   // values of each operand a thread moves per K step

typedef MfmaOps<double>::acc_t fba_acc_t;

// the 8 MFMAs of one K step of a wave's 16 x 16 tile: A element (i, k) at As[i * SAM + k * SAK], B element (k, j) at Bs[k * FBA_LDM + j]
template <int SAM, int SAK>
__device__ __forceinline__ fba_acc_t fba_mma(const double* As, const double* Bs, int wm, int wn, int lane, fba_acc_t acc) {
    const double* Aw = As + (wm + (lane & 15)) * SAM + (lane >> 4) * SAK;
    const double* Bw = Bs + (lane >> 4) * FBA_LDM + wn + (lane & 15);
#pragma unroll
    for (int kk = 0; kk < FBA_T; kk += 4) acc = MfmaOps<double>::run(Aw[kk * SAK], Bw[kk * FBA_LDM], acc);
    return acc;
}

}  // namespace crb
