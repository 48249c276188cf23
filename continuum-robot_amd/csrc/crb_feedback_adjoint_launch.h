// crb_feedback_adjoint_launch.h -- host entry of the closed-loop adjoint translation unit (crb_feedback_adjoint.hip): the
// kernels' parameter block and their launchers (the kernels themselves, crb_feedback_adjoint.h, are built in that unit alone).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace crb {
struct FeedbackAdjParams {
    const double* ubar;        // [rows][n_node][4]  (df/du)^T kbar of the stage, force layout
    const int32_t* col_off;    // [2n] offset of reduced state index j inside a beam's state record
    const int32_t* row_off;    // [n]  offset of reduced position index i inside a beam's force record
    int rows, B, n, n2;        // rows = n_cot * B, n2 = 2n
    size_t x_stride, u_stride;
    // crb_feedback_transpose_kernel
    const double* gain;        // [n][2n] row-major
    const double* xbar;        // [rows][2][n_node][4]  (df/dx)^T kbar of the stage
    double* lam;               // [rows][2][n_node][4]  lambda+ (read; written by the step's last launch: lambda = lambda+ + sum)
    double* sum;               // [rows][2][n_node][4]  running sum of the step's stage cotangents
    double* seed;              // [rows][2][n_node][4]  the next stage's seed ca lambda+ + cb s
    double* ref_bar;           // [rows][2n] reduced, accumulated, or nullptr
    double ca, cb;
    int first, last;           // the step's first launch (stage 4: sum = s) / last launch (stage 1: lam += sum)
    // crb_feedback_gain_grad_kernel
    const double* xs;          // [B][2][n_node][4] the stage state
    const double* ref;         // [B][2n] reduced, or nullptr (= 0)
    double* gain_bar;          // [n_cot][n][2n], accumulated
    double* partial;           // [n_cot][slices][n][2n] the slices' tiles (feedback_gain_grad_slices(B, n) > 1), else unused
    int slices;                // set by launch_feedback_gain_grad
};

// Slices the beam reduction of the gain gradient is split into: enough for 1536 workgroups (six per CU) per cotangent where
// the n x 2n output tiles alone give fewer, never more than the reduction has K steps of 32 beams.  A function of B and n
// only, so that the summation order -- and the result, bitwise -- does not depend on the number of cotangents.
inline int feedback_gain_grad_slices(int B, int n) {
    const int tiles = ((n + 31) / 32) * ((2 * n + 31) / 32), ksteps = (B + 31) / 32;
    const int want = (1536 + tiles - 1) / tiles;
    return want < ksteps ? want : ksteps;
}

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
