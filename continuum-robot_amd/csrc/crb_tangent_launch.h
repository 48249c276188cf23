// crb_tangent_launch.h -- host entry of the tangent-linear translation unit (crb_tangent.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_tangent.h"

namespace crb {
// crb_jvp_kernel<double, MODE_RHS> on a grid of `groups` x `n_dir` workgroups of `threads` (<= TANGENT_MAX_NT) threads
hipError_t launch_jvp_rhs(const KParams<double>& k, const TangentParams<double>& q, int groups, int n_dir, int threads, hipStream_t st);
// crb_jvp_kernel<double, MODE_STEP>: k.n_steps RK4 steps of the base and of every direction
hipError_t launch_jvp_step(const KParams<double>& k, const TangentParams<double>& q, int groups, int n_dir, int threads, hipStream_t st);
}  // namespace crb
