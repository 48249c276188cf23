// crb_implicit_feedback_adjoint.h -- the sample-boundary arithmetic of the adjoint of the sampled-data implicit loop
// (crb_step_implicit_feedback_adjoint), on v_mfma_f64_16x16x4_f64.
//
// Forward, sample k:  u_k = f_held + K (r - x_k),  x_{k+1} = Phi(x_k, u_k)  (the sample's implicit steps, started from a^0 = 0).
// The implicit sweep over the sample's steps (crb_imp_adj_kernel, IADJ_BWD) turns lambda = dL/dx_{k+1} into
// lambda' = (dPhi/dx)^T lambda and ubar_k = (dPhi/du)^T lambda.  What is left at the boundary, rows = n_cot * B:
//     P = ubar_k,red . K        [rows x n] . [n x 2n]                              crb_imp_fb_boundary_kernel, once per sample
//     dL/dx_k = lambda' - P,   ref_bar += P,   f_held_bar += ubar_k
//     gain_bar += sum_b ubar_k,b (x) (r_b - x_k,b)   [n x B] . [B x 2n]            crb_imp_fb_gain_grad_kernel, once per segment
// Both follow the products of the RK4 loop's adjoint (crb_feedback_adjoint_tile.h: tile, LDS layouts, one LDS stage, unconditional
// clamped loads zeroed by selects, and the loop of the transposed product itself).
//
// The boundary kernel has its own epilogue on lambda in place and adds ubar_k to f_held_bar from the workgroups of the first
// column tile, which own their 32 rows: no operand passes through a zero-filled buffer.
//
// The gain gradient is batched over the samples of a checkpoint segment: at the sizes the loop is tuned at (64 beams) one
// sample's product is two K steps and a launch per sample would be all launch cost.  A workgroup owns one output tile of one
// cotangent (and one beam slice, feedback_gain_grad_slices); it walks the samples in sweep order, last first, reduces each
// over its beams in ascending order into a FRESH accumulator and adds that to a running tile, which starts from gain_bar (one
// slice) or from the slice's partial tile (several; zeroed at the start of the call, summed into gain_bar in ascending order
// by crb_feedback_gain_reduce_kernel at its end) and is written back when the launch ends.  The additions and their order are
// the same however the samples fall into segments: gain_bar does not depend on the checkpoint interval, bitwise.  r_b - x_k,b
// is formed in the loader from the segment's recomputed step-start states.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_feedback_adjoint_tile.h"
#include "crb_implicit_feedback_adjoint_launch.h"

namespace crb {

// P = ubar_red . K; lam -= P on the free-DOF entries of the state layout, ref_bar += P; blockIdx.y == 0: f_held_bar += ubar on
// the free-DOF entries of the rows of this tile.  Grid: (ceil(rows / 32), ceil(2n / 32)).
__global__ void __launch_bounds__(256) crb_imp_fb_boundary_kernel(const ImpFbAdjParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    double* const As = reinterpret_cast<double*>(crb_smem);            // [32][FBA_LDK]
    double* const Bs = As + FBA_T * FBA_LDK;                           // [32][FBA_LDM]
    int32_t* const roff_s = reinterpret_cast<int32_t*>(Bs + FBA_T * FBA_LDM);   // [n]
    const FbaTile w = fba_product_tile();
    // the force record of row m = (cotangent, beam) of this sample
    auto urow = [&](int m) {
        const int c = m / p.B;
        return p.ubar + size_t(c) * p.cot_stride + size_t(m - c * p.B) * p.u_stride;
    };
    const fba_acc_t acc = fba_transposed_product(p, w, As, Bs, roff_s, urow);
    // f_held_bar += ubar: the first column tile owns the force records of its rows (wave-uniform branch)
    if (p.f_held_bar && blockIdx.y == 0) {
        const int m0 = w.m0, mrows = min(FBA_T, p.rows - m0);
        for (int e = w.t; e < mrows * p.n; e += 256) {
            const int r = e / p.n, off = roff_s[e - r * p.n];
            double* const d = p.f_held_bar + size_t(m0 + r) * p.u_stride + off;
            *d = *d + urow(m0 + r)[off];
        }
    }
    const int j = w.j();
    if (j >= p.n2) return;
    const int coff = p.col_off[j];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int m = w.row(reg);
        if (m >= p.rows) continue;
        const size_t idx = size_t(m) * p.x_stride + coff;
        const double P = acc[reg];
        p.lam[idx] = p.lam[idx] - P;
        if (p.ref_bar) p.ref_bar[size_t(m) * p.n2 + j] += P;
    }
}

// The running tile of (cotangent c = blockIdx.z, slice z) += for every sample of the segment, last first, the reduction over
// the slice's beams of ubar_red[c][sample]^T . (ref - x_sample,red).  Grid: (ceil(n / 32), ceil(2n / 32) * p.slices, n_cot);
// slice z = blockIdx.y / ceil(2n / 32) takes a contiguous range of K steps (32 beams each).
template <bool HAS_REF>
__global__ void __launch_bounds__(256) crb_imp_fb_gain_grad_kernel(const ImpFbAdjParams p) {
    __shared__ __attribute__((aligned(16))) double As[FBA_T * FBA_LDM];   // [k = beam][i]
    __shared__ __attribute__((aligned(16))) double Bs[FBA_T * FBA_LDM];   // [k = beam][j]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tiles_n = (p.n2 + FBA_T - 1) / FBA_T, z = blockIdx.y / tiles_n;
    const int m0 = blockIdx.x * FBA_T, n0 = (blockIdx.y - z * tiles_n) * FBA_T;
    const size_t c = blockIdx.z;
    const int wm = (wave >> 1) * 16, wn = (wave & 1) * 16;
    // loader: output row / column lc of beams lr + 8 q
    const int lc = t & (FBA_T - 1), lr = t / FBA_T;
    const bool iok = m0 + lc < p.n, jok = n0 + lc < p.n2;
    const int jc = jok ? n0 + lc : 0;
    const int roff = p.row_off[iok ? m0 + lc : 0], coff = p.col_off[jc];
    const double *ub = nullptr, *xb = nullptr;   // this thread's ubar and state columns of the sample being reduced
    double ra[FBA_Q], rb[FBA_Q];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < FBA_Q; ++q) {
            const int b = k0 + lr + 8 * q;
            const bool bok = b < p.B;
            const size_t bc = size_t(bok ? b : p.B - 1);
            const double va = ub[bc * p.u_stride];
            const double vx = xb[bc * p.x_stride];
            const double vr = HAS_REF ? p.ref[bc * size_t(p.n2) + jc] : 0.0;
            ra[q] = (bok && iok) ? va : 0.0;
            rb[q] = (bok && jok) ? vr - vx : 0.0;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < FBA_Q; ++q) {
            As[(lr + 8 * q) * FBA_LDM + lc] = ra[q];
            Bs[(lr + 8 * q) * FBA_LDM + lc] = rb[q];
        }
    };
    // this lane's four entries of the running tile
    const int j = n0 + wn + (lane & 15);
    double* const dst = (p.slices > 1 ? p.partial + (c * size_t(p.slices) + size_t(z)) * size_t(p.n) * p.n2
                                      : p.gain_bar + c * size_t(p.n) * p.n2) + j;
    fba_acc_t run = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int i = m0 + wm + MfmaOps<double>::row(lane, reg);
        if (i < p.n && j < p.n2) run[reg] = dst[size_t(i) * p.n2];
    }
    // this slice's K steps (none for a slice past the end: its tile stays as it is)
    const int all_steps = (p.B + FBA_T - 1) / FBA_T, per_slice = (all_steps + p.slices - 1) / p.slices;
    const int s0 = z * per_slice, nsteps = min(per_slice, all_steps - s0);
    for (int js = p.n_samples - 1; js >= 0; --js) {
        ub = p.ubar + c * p.cot_stride + size_t(js) * p.sample_stride + roff;
        xb = p.xs + size_t(js) * p.xs_stride + coff;
        fba_acc_t acc = {0.0, 0.0, 0.0, 0.0};
        if (nsteps > 0) fetch(s0 * FBA_T);
        for (int s = 0; s < nsteps; ++s) {
            stash();
            __syncthreads();
            if (s + 1 < nsteps) fetch((s0 + s + 1) * FBA_T);   // (uniform; in flight during the MFMAs)
            acc = fba_mma<1, FBA_LDM>(As, Bs, wm, wn, lane, acc);
            __syncthreads();   // (the next stash overwrites what this step read)
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) run[reg] = run[reg] + acc[reg];
    }
    if (j >= p.n2) return;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int i = m0 + wm + MfmaOps<double>::row(lane, reg);
        if (i < p.n) dst[size_t(i) * p.n2] = run[reg];
    }
}

}  // namespace crb
