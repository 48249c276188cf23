// crb_implicit_feedback_adjoint_launch.h -- host entry of the translation unit that holds the sample-boundary kernels of the
// adjoint of the sampled-data implicit loop (crb_implicit_feedback_adjoint.hip): their parameter block and launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace crb {
struct ImpFbAdjParams {
    // ubar of cotangent c, sample slot s, beam b: ubar + c * cot_stride + s * sample_stride + b * u_stride (force layout).  The
    // boundary launch is handed the address of its own sample's slot; the gain gradient that of slot 0.
    const double* ubar;
    size_t cot_stride, sample_stride;
    const int32_t* col_off;    // [2n] offset of reduced state index j inside a beam's state record
    const int32_t* row_off;    // [n]  offset of reduced position index i inside a beam's force record
    int rows, B, n, n2;        // rows = n_cot * B, n2 = 2n
    size_t x_stride, u_stride;
    // crb_imp_fb_boundary_kernel
    const double* gain;        // [n][2n] row-major
    double* lam;               // [rows][2][n_node][4]  lambda' on entry, dL/dx_k on exit
    double* ref_bar;           // [rows][2n] reduced, accumulated, or nullptr
    double* f_held_bar;        // [rows][n_node][4] force layout, accumulated, or nullptr
    // crb_imp_fb_gain_grad_kernel
    const double* xs;          // [n_samples][B][2][n_node][4] at stride xs_stride: the state every sample of the segment was taken at
    size_t xs_stride;
    int n_samples;             // samples of the segment (slots 0 .. n_samples - 1, swept last first)
    const double* ref;         // [B][2n] reduced, or nullptr (= 0)
    double* gain_bar;          // [n_cot][n][2n], accumulated (one slice)
    double* partial;           // [n_cot][slices][n][2n] the slices' running tiles (several slices), else unused
    int slices;                // set by launch_imp_fb_gain_grad: feedback_gain_grad_slices(B, n)
};

// crb_imp_fb_boundary_kernel on a grid of ceil(rows / 32) x ceil(2n / 32) workgroups
hipError_t launch_imp_fb_boundary(const ImpFbAdjParams& p, hipStream_t st);
// crb_imp_fb_gain_grad_kernel on a grid of ceil(n / 32) x ceil(2n / 32) * slices x n_cot workgroups
hipError_t launch_imp_fb_gain_grad(const ImpFbAdjParams& p, hipStream_t st);
}  // namespace crb
