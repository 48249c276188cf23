// crb_implicit_tangent.hip -- the tangent of the implicit stepper (crb_implicit_tangent.h), one translation unit of its own.
#include "crb_implicit_tangent_launch.h"

namespace crb {
namespace {
template <bool SCHED>
hipError_t imp_jvp_impl(const KParams<double>& k, const TangentParams<double>& q, int n_iter, int groups, int n_dir, int threads,
                        hipStream_t st) {
    hipLaunchKernelGGL((crb_imp_jvp_kernel<double, SCHED>), dim3(groups, n_dir), dim3(threads), tangent_lds_bytes<double>(threads), st, k,
                       q, n_iter);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_imp_jvp_step(const KParams<double>& k, const TangentParams<double>& q, int n_iter, bool sched, int groups, int n_dir,
                               int threads, hipStream_t st) {
    if (threads > TANGENT_MAX_NT || n_dir < 1 || n_dir > 65535 || n_iter < 1) return hipErrorInvalidValue;
    return sched ? imp_jvp_impl<true>(k, q, n_iter, groups, n_dir, threads, st) : imp_jvp_impl<false>(k, q, n_iter, groups, n_dir, threads, st);
}
}  // namespace crb
