// crb_implicit_feedback_tangent.h -- the sample-boundary arithmetic of the tangent of the sampled-data implicit loop
// (crb_step_implicit_feedback_tangent), on v_mfma_f64_16x16x4_f64.
//
// Forward, sample k:  u_k = f_held + K (r - x_k),  x_{k+1} = Phi(x_k, u_k)  (the sample's implicit steps, started from a^0 = 0).
// Its tangent per direction d:  du_k = df_held + K (dr - dx_k) + dK (r - x_k), then the tangent of Phi along (dx_k, du_k) -- one
// interval of crb_imp_jvp_kernel<double, true>, launched by the entry point after this kernel.  What the boundary computes,
// straight from the state layout and to the force layout (free DOFs only: constrained DOFs and padding are not written):
//     u [b, :]     = f_held[b, :]     + (r[b, :] - x_red[b, :]) . K^T                                  [B x 2n] . [2n x n], once
//     du[d, b, :]  = df_held[d, b, :] + (dr[d, b, :] - dx_red[d, b, :]) . K^T                          [n_dir B x 2n] . [2n x n]
//                                     + (r[b, :] - x_red[b, :]) . dK_d^T                               per direction, its own dK_d
//
// Tiling: that of the closed-loop adjoints' products (crb_feedback_adjoint_tile.h: 256 threads, a 32 x 32 output tile, each wave
// one 16 x 16 MFMA tile, K steps of 32, one LDS stage, the loads of step s + 1 in flight during the MFMAs of step s, every load
// unconditional from a clamped address and zeroed by a select).  Both operands are contiguous along the reduction index 2n in
// global memory (a state record through col_off, a gain row), so both LDS tiles are [row][k] with FBA_LDK doubles per row.
// A row tile is 32 beams of ONE direction (or of the base): a workgroup is (direction, beam tile, column tile), its accumulator
// takes the K steps of K (dr - dx) in ascending order and then, in the same accumulator, those of dK_d (r - x).  So
//   - every output element has one owner and one summation order, no atomics;
//   - nothing depends on n_dir or on which directions share a launch: D directions in one launch are bitwise D launches of one,
//     and u (the workgroups of the slot past the last direction) is the same arithmetic whatever n_dir is;
//   - with d_gain == nullptr the second pass is not run (no loads, no MFMAs); every other result is bitwise unchanged;
//   - a non-finite entry of a seed row or of a beam's state stays in that row: rows and K indices out of range are zeroed on
//     BOTH operands, and an MFMA row reads only its own A row.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_feedback_adjoint_tile.h"
#include "crb_implicit_feedback_tangent_launch.h"

namespace crb {

// LDS: As [32][FBA_LDK], Bs [32][FBA_LDK], coff_s [2n]
__host__ __device__ constexpr size_t fbt_lds_bytes(int n2) {
    return size_t(2) * FBA_T * FBA_LDK * sizeof(double) + size_t(n2) * sizeof(int32_t);
}

// the 8 MFMAs of one K step of a wave's 16 x 16 tile: A element (i, k) at As[i * FBA_LDK + k], B element (k, j) at Bs[j * FBA_LDK + k]
__device__ __forceinline__ fba_acc_t fbt_mma(const double* As, const double* Bs, int wm, int wn, int lane, fba_acc_t acc) {
    const double* Aw = As + (wm + (lane & 15)) * FBA_LDK + (lane >> 4);
    const double* Bw = Bs + (wn + (lane & 15)) * FBA_LDK + (lane >> 4);
#pragma unroll
    for (int kk = 0; kk < FBA_T; kk += 4) acc = MfmaOps<double>::run(Aw[kk], Bw[kk], acc);
    return acc;
}

// Grid: ((n_dir + 1) * ceil(B / 32), ceil(n / 32)); blockIdx.x / ceil(B / 32) is the direction, n_dir the base's slot.
__global__ void __launch_bounds__(256) crb_imp_fb_tangent_boundary_kernel(const ImpFbTanParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    double* const As = reinterpret_cast<double*>(crb_smem);            // [32][FBA_LDK]  rows = beams
    double* const Bs = As + FBA_T * FBA_LDK;                           // [32][FBA_LDK]  rows = output columns
    int32_t* const coff_s = reinterpret_cast<int32_t*>(Bs + FBA_T * FBA_LDK);   // [2n]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tiles_b = (p.B + FBA_T - 1) / FBA_T;
    const int d = blockIdx.x / tiles_b;
    const bool base = d == p.n_dir;   // (workgroup-uniform)
    const FbaTile w = {t, lane, (int(blockIdx.x) - d * tiles_b) * FBA_T, int(blockIdx.y) * FBA_T, (wave >> 1) * 16, (wave & 1) * 16};
    for (int k = t; k < p.n2; k += 256) coff_s[k] = p.col_off[k];
    // loader: k index lc of beams lr + 8 q (A) and of output columns lr + 8 q (B)
    const int lc = t & (FBA_T - 1), lr = t / FBA_T;
    size_t arow[FBA_Q], brow[FBA_Q];
    bool aok[FBA_Q], bok[FBA_Q];
#pragma unroll
    for (int q = 0; q < FBA_Q; ++q) {
        const int b = w.m0 + lr + 8 * q, i = w.n0 + lr + 8 * q;
        aok[q] = b < p.B;
        bok[q] = i < p.n;
        arow[q] = size_t(aok[q] ? b : p.B - 1);
        brow[q] = size_t(bok[q] ? i : 0) * p.n2;
    }
    __syncthreads();   // coff_s
    fba_acc_t acc = {0.0, 0.0, 0.0, 0.0};
    const int nsteps = (p.n2 + FBA_T - 1) / FBA_T;
    const int npass = (!base && p.d_gain) ? 2 : 1;
    for (int pass = 0; pass < npass; ++pass) {
        // pass 0: (dr_d - dx_d) . K^T, or for the base (r - x) . K^T; pass 1: (r - x) . dK_d^T
        const bool seed = pass == 0 && !base;
        const double* const xa = seed ? p.dx + size_t(d) * p.B * p.x_stride : p.x;
        const double* const ra = seed ? (p.d_ref ? p.d_ref + size_t(d) * p.B * p.n2 : nullptr) : p.ref;
        const double* const gm = pass == 1 ? p.d_gain + size_t(d) * p.n * p.n2 : p.gain;
        double va[FBA_Q], vb[FBA_Q];
        auto fetch = [&](int k0) {
            const int k = k0 + lc;
            const bool kok = k < p.n2;
            const int kc = kok ? k : 0, co = coff_s[kc];
#pragma unroll
            for (int q = 0; q < FBA_Q; ++q) {
                const double vx = xa[arow[q] * p.x_stride + co];
                const double vr = ra ? ra[arow[q] * p.n2 + kc] : 0.0;   // (uniform)
                va[q] = (aok[q] && kok) ? vr - vx : 0.0;
            }
#pragma unroll
            for (int q = 0; q < FBA_Q; ++q) {
                const double v = gm[brow[q] + kc];
                vb[q] = (bok[q] && kok) ? v : 0.0;
            }
        };
        auto stash = [&]() {
#pragma unroll
            for (int q = 0; q < FBA_Q; ++q) {
                As[(lr + 8 * q) * FBA_LDK + lc] = va[q];
                Bs[(lr + 8 * q) * FBA_LDK + lc] = vb[q];
            }
        };
        fetch(0);
        for (int s = 0; s < nsteps; ++s) {
            stash();
            __syncthreads();
            if (s + 1 < nsteps) fetch((s + 1) * FBA_T);   // (uniform; in flight during the MFMAs)
            acc = fbt_mma(As, Bs, w.wm, w.wn, lane, acc);
            __syncthreads();   // (the next stash overwrites what this step read)
        }
    }
    const int i = w.j();
    if (i >= p.n) return;
    const int off = p.row_off[i];
    const double* const held = base ? p.f_held : (p.df_held ? p.df_held + size_t(d) * p.B * p.u_stride : nullptr);
    double* const out = base ? p.u : p.du + size_t(d) * p.du_dir_stride;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int b = w.row(reg);
        if (b >= p.B) continue;
        const size_t idx = size_t(b) * p.u_stride + off;
        out[idx] = held ? held[idx] + acc[reg] : acc[reg];
    }
}

}  // namespace crb
