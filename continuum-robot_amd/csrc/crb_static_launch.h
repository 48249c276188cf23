// crb_static_launch.h -- host entry of the static-equilibrium translation unit (crb_static.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_static.h"

namespace crb {
// crb_tangent_kernel<T> on `groups` workgroups of `threads` (<= STATIC_MAX_NT) threads: the blocks of dk/dq into q.blocks
hipError_t launch_tangent(const KParams<double>& k, const StaticParams<double>& q, int groups, int threads, hipStream_t st);
hipError_t launch_tangent(const KParams<float>& k, const StaticParams<float>& q, int groups, int threads, hipStream_t st);
// crb_static_kernel: the static solve of every beam (k.levels = ALL reduction levels of the beam)
hipError_t launch_static(const KParams<double>& k, const StaticParams<double>& q, int groups, int threads, hipStream_t st);
}  // namespace crb
