// crb_tangent.hip -- the tangent-linear kernels (crb_tangent.h), one translation unit of their own.
#include "crb_tangent_launch.h"

namespace crb {
namespace {
template <int MODE>
hipError_t jvp_impl(const KParams<double>& k, const TangentParams<double>& q, int groups, int n_dir, int threads, hipStream_t st) {
    if (threads > TANGENT_MAX_NT || n_dir < 1 || n_dir > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((crb_jvp_kernel<double, MODE>), dim3(groups, n_dir), dim3(threads), tangent_lds_bytes<double>(threads), st, k, q);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_jvp_rhs(const KParams<double>& k, const TangentParams<double>& q, int groups, int n_dir, int threads, hipStream_t st) {
    return jvp_impl<MODE_RHS>(k, q, groups, n_dir, threads, st);
}
hipError_t launch_jvp_step(const KParams<double>& k, const TangentParams<double>& q, int groups, int n_dir, int threads, hipStream_t st) {
    return jvp_impl<MODE_STEP>(k, q, groups, n_dir, threads, st);
}
}  // namespace crb
