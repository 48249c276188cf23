// crb_feedback_adjoint_tile.h -- what the matrix products of the closed-loop adjoints on v_mfma_f64_16x16x4_f64 share between the
// RK4 loop's kernels (crb_feedback_adjoint.h) and the sampled-data implicit loop's (crb_implicit_feedback_adjoint.h): the tile
// shape, the MFMA step, and the whole tile loop of the transposed product
//     P = ubar_red . K                          [rows x n] . [n x 2n]   fba_transposed_product, rows = n_cot * B (cotangent c, beam b)
// to which a kernel adds how a row's ubar record is addressed and what its epilogue does with P.  The gain gradient
//     sum_b ubar_red,b (x) (r_b - x_red,b)      [n x B] . [B x 2n]      over one slice of the beams
// has the same design, its loop written out in each of its two kernels.
//
// Both follow crb_feedback_kernel (crb_feedback.h): 256 threads, a 32 x 32 output tile, each wave one 16 x 16 MFMA tile, K in
// steps of 32; the global loads of step s + 1 are issued before the MFMAs of step s and stored to LDS after them.  ONE LDS
// stage (two barriers per step), not two: a K step here is 8 MFMAs per wave against a gather whose latency is several times
// that, so what hides the latency is other workgroups -- at 21 - 25 KB of LDS six of them share a CU (measured at 2048 x 128
// elements: the transposed product 49 us against 73 with two stages; the gain gradient 74 us in six slices against 177 with
// two stages and one slice -- DESIGN 10).  For the same reason the gain gradient's beam reduction is split over blockIdx.y
// slices once the output tiles alone do not fill the chip (feedback_gain_grad_slices: a function of B and n only); the
// slices' partial tiles are summed in ascending order by crb_feedback_gain_reduce_kernel.
// Every load is unconditional: rows, columns and K indices out of range read a clamped address and are zeroed by a select (the
// transposed product's A rows out of range are never stored, and its K tail is zeroed on the gain side: a non-finite value of
// a row stays in that row).
// LDS tiles: [row][k] with 32 + 2 doubles per row where the global operand is contiguous along k (the gathered ubar of the
// transposed product), [k][col] with 32 + 16 doubles per row where it is contiguous along the output index (the gain, the
// state, ubar^T): lanes 0 .. 31 of a fragment read (two k rows of 16 columns) then touch each bank once.
// No atomics: every output element is owned by one lane of one workgroup, and the beam reduction of the gain gradient runs
// in ascending order inside a slice and over the slices, so the results are bitwise reproducible and do not depend on n_cot.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_feedback_adjoint_params.h"
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

// A thread's place in its workgroup's 32 x 32 output tile at (m0, n0): wave (wm, wn) / 16 of the 2 x 2, and the epilogue frame --
// entry reg of the lane's accumulator is the output's row row(reg), column j() (D row = (lane >> 4) + 4 reg, D col = lane & 15);
// either may lie past the output's edge.
struct FbaTile {
    int t, lane, m0, n0, wm, wn;
    __device__ __forceinline__ int j() const { return n0 + wn + (lane & 15); }
    __device__ __forceinline__ int row(int reg) const { return m0 + wm + MfmaOps<double>::row(lane, reg); }
};

// ---- the transposed product: the tile at (32 blockIdx.x, 32 blockIdx.y) of P = ubar_red . K
// LDS: As [32][FBA_LDK], Bs [32][FBA_LDM], roff_s [n]
__host__ __device__ constexpr size_t fba_product_lds_bytes(int n) {
    return size_t(FBA_T) * (FBA_LDK + FBA_LDM) * sizeof(double) + size_t(n) * sizeof(int32_t);
}

// a thread's place on the grid (ceil(rows / 32), ceil(2n / 32)): taken once per kernel, for the loop and the epilogue alike
__device__ __forceinline__ FbaTile fba_product_tile() {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * FBA_T, n0 = blockIdx.y * FBA_T;
    return {t, lane, m0, n0, (wave >> 1) * 16, (wave & 1) * 16};
}

// urow(m): the force record ubar of row m < p.rows.  Returns the wave's 16 x 16 tile; roff_s holds p.row_off on return.
template <class URow>
__device__ __forceinline__ fba_acc_t fba_transposed_product(const FbaParams& p, const FbaTile& w, double* As, double* Bs, int32_t* roff_s,
                                                            URow urow) {
    const int t = w.t, m0 = w.m0, n0 = w.n0;
    for (int k = t; k < p.n; k += 256) roff_s[k] = p.row_off[k];
    // loader: A column lc of rows lr + 8 q (contiguous along k); B column lc of K rows lr + 8 q (contiguous along j)
    const int lc = t & (FBA_T - 1), lr = t / FBA_T;
    const double* arow[FBA_Q];
#pragma unroll
    for (int q = 0; q < FBA_Q; ++q) {
        const int m = m0 + lr + 8 * q;
        arow[q] = urow(m < p.rows ? m : p.rows - 1);
    }
    const bool jok = n0 + lc < p.n2;
    const double* const bcol = p.gain + (jok ? n0 + lc : 0);
    __syncthreads();   // roff_s
    double ra[FBA_Q], rb[FBA_Q];
    auto fetch = [&](int k0) {
        const int ka = k0 + lc;
        const int ro = roff_s[ka < p.n ? ka : 0];
#pragma unroll
        for (int q = 0; q < FBA_Q; ++q) ra[q] = arow[q][ro];
#pragma unroll
        for (int q = 0; q < FBA_Q; ++q) {
            const int kb = k0 + lr + 8 * q;
            const double v = bcol[size_t(kb < p.n ? kb : 0) * p.n2];
            rb[q] = (kb < p.n && jok) ? v : 0.0;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < FBA_Q; ++q) {
            As[(lr + 8 * q) * FBA_LDK + lc] = ra[q];
            Bs[(lr + 8 * q) * FBA_LDM + lc] = rb[q];
        }
    };
    fba_acc_t acc = {0.0, 0.0, 0.0, 0.0};
    const int nsteps = (p.n + FBA_T - 1) / FBA_T;
    fetch(0);
    for (int s = 0; s < nsteps; ++s) {
        stash();
        __syncthreads();
        if (s + 1 < nsteps) fetch((s + 1) * FBA_T);   // (uniform; in flight during the MFMAs)
        acc = fba_mma<FBA_LDK, 1>(As, Bs, w.wm, w.wn, w.lane, acc);
        __syncthreads();   // (the next stash overwrites what this step read)
    }
    return acc;
}

}  // namespace crb
