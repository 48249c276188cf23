// crb_implicit_feedback_adjoint_launch.h -- host entry of the translation unit that holds the sample-boundary kernels of the
// adjoint of the sampled-data implicit loop (crb_implicit_feedback_adjoint.hip): their parameter block and launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crb_feedback_adjoint_params.h"

namespace crb {
// p.ubar of cotangent c, sample slot s, beam b: ubar + c * cot_stride + s * sample_stride + b * u_stride.  The boundary launch
// is handed the address of its own sample's slot; the gain gradient that of slot 0.  p.lam: lambda' on entry, dL/dx_k on exit.
// p.xs: [n_samples][B][2][n_node][4] at stride xs_stride, the state every sample of the segment was taken at.
struct ImpFbAdjParams : FbaParams {
    size_t cot_stride, sample_stride;
    double* f_held_bar;        // [rows][n_node][4] force layout, accumulated, or nullptr
    size_t xs_stride;
    int n_samples;             // samples of the segment (slots 0 .. n_samples - 1, swept last first)
};

// crb_imp_fb_boundary_kernel on a grid of ceil(rows / 32) x ceil(2n / 32) workgroups
hipError_t launch_imp_fb_boundary(const ImpFbAdjParams& p, hipStream_t st);
// crb_imp_fb_gain_grad_kernel on a grid of ceil(n / 32) x ceil(2n / 32) * slices x n_cot workgroups
hipError_t launch_imp_fb_gain_grad(const ImpFbAdjParams& p, hipStream_t st);
}  // namespace crb
