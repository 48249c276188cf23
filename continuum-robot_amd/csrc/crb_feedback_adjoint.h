// crb_feedback_adjoint.h -- the two matrix products of the adjoint of the closed-loop RK4 rollout (crb_step_rk4_feedback_adjoint)
// on v_mfma_f64_16x16x4_f64, and the vector kernels between its steps.
//
// The closed-loop right-hand side is F(x) = f(x, K (r - x) + d(t)); f is affine in u, so with (xbar, ubar) = crb_rhs_vjp(X, NULL,
// kbar) at a stage state X the cotangent of the stage is
//     s = xbar - P,   P = ubar_red . K          [rows x n] . [n x 2n]      (crb_feedback_transpose_kernel)
//     ref_bar += P,   gain_bar += sum_b ubar_red,b (x) (r_b - X_red,b)      [n x B] . [B x 2n]  (crb_feedback_gain_grad_kernel)
// rows = n_cot * B (cotangent c, beam b).  The tile, the LDS layouts, the clamped loads and why they are what they are, and the
// loop of the transposed product: crb_feedback_adjoint_tile.h.  Here a row's ubar is record m of one [rows] array, and the
// epilogue keeps the books of the RK4 stages.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_feedback_adjoint_launch.h"
#include "crb_feedback_adjoint_tile.h"
#include "crb_generic.h"

namespace crb {

// P = ubar_red . K; per free-DOF entry of the state layout: s = xbar - P, sum (+)= s, then seed = ca lam + cb s, or with
// p.last lam += sum; ref_bar += P.  Grid: (ceil(rows / 32), ceil(2n / 32)).
__global__ void __launch_bounds__(256) crb_feedback_transpose_kernel(const FeedbackAdjParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    double* const As = reinterpret_cast<double*>(crb_smem);            // [32][FBA_LDK]
    double* const Bs = As + FBA_T * FBA_LDK;                           // [32][FBA_LDM]
    int32_t* const roff_s = reinterpret_cast<int32_t*>(Bs + FBA_T * FBA_LDM);   // [n]
    const FbaTile w = fba_product_tile();
    const fba_acc_t acc = fba_transposed_product(p, w, As, Bs, roff_s, [&](int m) { return p.ubar + size_t(m) * p.u_stride; });
    const int j = w.j();
    if (j >= p.n2) return;
    const int coff = p.col_off[j];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int m = w.row(reg);
        if (m >= p.rows) continue;
        const size_t idx = size_t(m) * p.x_stride + coff;
        const double P = acc[reg];
        const double s = p.xbar[idx] - P;
        const double sm = p.first ? s : p.sum[idx] + s;
        if (p.last) {
            p.lam[idx] = p.lam[idx] + sm;
        } else {
            p.sum[idx] = sm;
            p.seed[idx] = p.ca * p.lam[idx] + p.cb * s;
        }
        if (p.ref_bar) p.ref_bar[size_t(m) * p.n2 + j] += P;
    }
}

// gain_bar[c] += ubar_red[c]^T . (ref - X_red): [n x B] . [B x 2n], the reduction over the beams of cotangent c = blockIdx.z.
// Grid: (ceil(n / 32), ceil(2n / 32) * p.slices, n_cot); slice z = blockIdx.y / ceil(2n / 32) takes a contiguous range of K steps.
// One slice adds its tile to gain_bar; several write it to partial[c][z][n][2n] for crb_feedback_gain_reduce_kernel.
template <bool HAS_REF>
__global__ void __launch_bounds__(256) crb_feedback_gain_grad_kernel(const FeedbackAdjParams p) {
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
    const double* const ub = p.ubar + c * size_t(p.B) * p.u_stride + roff;
    const double* const xb = p.xs + coff;
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
    fba_acc_t acc = {0.0, 0.0, 0.0, 0.0};
    // this slice's K steps (none for a slice past the end: it contributes a tile of zeros)
    const int all_steps = (p.B + FBA_T - 1) / FBA_T, per_slice = (all_steps + p.slices - 1) / p.slices;
    const int s0 = z * per_slice, nsteps = min(per_slice, all_steps - s0);
    if (nsteps > 0) fetch(s0 * FBA_T);
    for (int s = 0; s < nsteps; ++s) {
        stash();
        __syncthreads();
        if (s + 1 < nsteps) fetch((s0 + s + 1) * FBA_T);   // (uniform; in flight during the MFMAs)
        acc = fba_mma<1, FBA_LDM>(As, Bs, wm, wn, lane, acc);
        __syncthreads();   // (the next stash overwrites what this step read)
    }
    const int j = n0 + wn + (lane & 15);
    if (j >= p.n2) return;
    double* const dst = p.slices > 1 ? p.partial + (c * size_t(p.slices) + size_t(z)) * size_t(p.n) * p.n2
                                     : p.gain_bar + c * size_t(p.n) * p.n2;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int i = m0 + wm + MfmaOps<double>::row(lane, reg);
        if (i >= p.n) continue;
        double* const d = dst + size_t(i) * p.n2 + j;
        *d = p.slices > 1 ? acc[reg] : *d + acc[reg];
    }
}

// gain_bar[c][e] += partial[c][0][e] + ... + partial[c][slices - 1][e], in that order; total = n_cot * n * 2n entries
__global__ void crb_feedback_gain_reduce_kernel(double* gain_bar, const double* partial, size_t per_cot, int slices, size_t total) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t c = i / per_cot, e = i - c * per_cot;
    const double* src = partial + c * size_t(slices) * per_cot + e;
    double v = gain_bar[i];
    for (int z = 0; z < slices; ++z) v = v + src[size_t(z) * per_cot];
    gain_bar[i] = v;
}

// The start of a step of the backward sweep: the cotangent of the sample taken at the end of the step is added to lambda at
// entry rec_off of every row's state record (rec_bar [rows][rec_n], sample kr; nullptr: none), then seed = c lambda.
// total = rows * x_stride entries.
__global__ void crb_feedback_seed_kernel(double* lam, double* seed, size_t total, size_t x_stride, double c, const double* rec_bar,
                                         size_t rec_off, int rec_n, int kr) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= total) return;
    double v = lam[i];
    if (rec_bar) {   // (uniform)
        const size_t row = i / x_stride;
        if (i - row * x_stride == rec_off) {
            v = v + rec_bar[row * size_t(rec_n) + size_t(kr)];
            lam[i] = v;
        }
    }
    seed[i] = c * v;
}

// out[b][kr] = x[b][off] of the checkpoint pass's recording (out [B][rec_n])
__global__ void crb_feedback_record_kernel(const double* x, size_t x_stride, size_t off, int B, double* out, int rec_n, int kr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[size_t(b) * size_t(rec_n) + size_t(kr)] = x[size_t(b) * x_stride + off];
}

// u += held on the free-DOF entries of the force layout (the held disturbance of the differentiable closed loop, added to the
// feedback force of a stage); total = B * n entries
__global__ void crb_feedback_held_kernel(double* u, const double* held, const int32_t* row_off, int n, size_t u_stride, size_t total) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / size_t(n);
    const size_t at = b * u_stride + size_t(row_off[i - b * size_t(n)]);
    u[at] = u[at] + held[at];
}

}  // namespace crb
