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
// crb_static_sens_kernel<double, transpose, NR> on groups x ceil(q.n_dir / NR) workgroups: J^-1 (or J^-T) applied to q.n_dir
// right-hand sides at the positions of plane 0 of k.x (k.levels = ALL reduction levels).  NR = STATIC_SENS_NR directions per
// workgroup, 1 for fewer directions than that.  q.status, when given, is zeroed on the stream first.
constexpr int STATIC_SENS_NR = 4;
hipError_t launch_static_sens(const KParams<double>& k, const StaticSensParams<double>& q, bool transpose, int groups, int threads,
                              hipStream_t st);
}  // namespace crb
