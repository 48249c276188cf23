// crb_feedback_adjoint_launch.h -- host entry of the closed-loop adjoint translation unit (crb_feedback_adjoint.hip): the
// kernels' parameter block and their launchers (the kernels themselves, crb_feedback_adjoint.h, are built in that unit alone).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crb_feedback_adjoint_params.h"

namespace crb {
// p.ubar: [rows][n_node][4], the stage's (df/du)^T kbar; p.lam: lambda+ (read; written by the step's last launch: lambda =
// lambda+ + sum); p.xs: the stage state
struct FeedbackAdjParams : FbaParams {
    const double* xbar;        // [rows][2][n_node][4]  (df/dx)^T kbar of the stage
    double* sum;               // [rows][2][n_node][4]  running sum of the step's stage cotangents
    double* seed;              // [rows][2][n_node][4]  the next stage's seed ca lambda+ + cb s
    double ca, cb;
    int first, last;           // the step's first launch (stage 4: sum = s) / last launch (stage 1: lam += sum)
};

// crb_feedback_transpose_kernel on a grid of ceil(rows / 32) x ceil(2n / 32) workgroups
hipError_t launch_feedback_transpose(const FeedbackAdjParams& p, hipStream_t st);
// crb_feedback_gain_grad_kernel on a grid of ceil(n / 32) x ceil(2n / 32) * slices x n_cot workgroups (p.rows = n_cot * p.B,
// slices = feedback_gain_grad_slices(p.B, p.n)), then with slices > 1 crb_feedback_gain_reduce_kernel over p.partial
hipError_t launch_feedback_gain_grad(const FeedbackAdjParams& p, hipStream_t st);
// crb_feedback_gain_reduce_kernel alone: gain_bar [n_cot][n][2n] += partial [n_cot][slices][n][2n], the slices in ascending order
hipError_t launch_feedback_gain_reduce(double* gain_bar, const double* partial, int n, int n_cot, int slices, hipStream_t st);
// crb_feedback_seed_kernel over total = rows * x_stride entries
hipError_t launch_feedback_seed(double* lam, double* seed, size_t total, size_t x_stride, double c, const double* rec_bar,
                                size_t rec_off, int rec_n, int kr, hipStream_t st);
// crb_feedback_record_kernel: out[b][kr] = x[b][off]
hipError_t launch_feedback_record(const double* x, size_t x_stride, size_t off, int B, double* out, int rec_n, int kr,
                                  hipStream_t st);
// crb_feedback_held_kernel: u[b][row_off[i]] += held[b][row_off[i]], i < n, b < B
hipError_t launch_feedback_held(double* u, const double* held, const int32_t* row_off, int n, int B, size_t u_stride, hipStream_t st);
}  // namespace crb
