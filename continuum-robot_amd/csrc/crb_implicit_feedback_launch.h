// crb_implicit_feedback_launch.h -- host entry of the sampled-data feedback translation unit (crb_implicit_feedback.hip): the FB
// instances of crb_implicit_kernel (crb_stiff.h).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_stiff.h"

namespace crb {
// the FB instances that are built: fp64, beams that live in one wave (at most 6 reduction levels of A), one wave per SIMD
constexpr bool implicit_feedback_built(int levels) { return levels >= 0 && levels <= 6; }
// dynamic LDS of an FB workgroup of NT threads carrying G beams of n free position DOFs: the exchange columns, the error rows,
// the transposed gain (and the product rows of the matrix-core form) -- the layout of crb_beam_kernel<..., FB>
constexpr size_t implicit_feedback_lds_bytes(int NT, int G, int n) { return fb_lds_bytes<double>(NT, G, n); }
// crb_implicit_kernel<double, levels, 64, 1, false, false, true> on `groups` workgroups of 64 threads with `smem` bytes of LDS
hipError_t launch_implicit_feedback(const KParams<double>& k, const StiffFbParams<double>& q, int levels, int groups, size_t smem,
                                    hipStream_t st);
}  // namespace crb
