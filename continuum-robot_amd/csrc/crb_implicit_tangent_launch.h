// crb_implicit_tangent_launch.h -- host entry of the implicit stepper's tangent translation unit (crb_implicit_tangent.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_implicit_tangent.h"

namespace crb {
// crb_imp_jvp_kernel<double, sched>: k.n_steps implicit steps (n_iter iterations each) of the base and of every direction, on a
// grid of `groups` x `n_dir` workgroups of `threads` (<= TANGENT_MAX_NT) threads; sched: k carries a control schedule
hipError_t launch_imp_jvp_step(const KParams<double>& k, const TangentParams<double>& q, int n_iter, bool sched, int groups, int n_dir,
                               int threads, hipStream_t st);
}  // namespace crb
