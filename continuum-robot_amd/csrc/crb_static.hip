// crb_static.hip -- the static-equilibrium kernels (crb_static.h), one translation unit of their own.
#include "crb_host.h"
#include "crb_static_launch.h"

namespace crb {
namespace {
template <typename T>
hipError_t tangent_impl(const KParams<T>& k, const StaticParams<T>& q, int groups, int threads, hipStream_t st) {
    if (threads > STATIC_MAX_NT) return hipErrorInvalidValue;
    const size_t lds = static_lds_bytes<T>(threads);
    if (hipError_t e = lds_opt_in(crb_tangent_kernel<T>, lds)) return e;
    hipLaunchKernelGGL((crb_tangent_kernel<T>), dim3(groups), dim3(threads), lds, st, k, q);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_tangent(const KParams<double>& k, const StaticParams<double>& q, int groups, int threads, hipStream_t st) {
    return tangent_impl<double>(k, q, groups, threads, st);
}
hipError_t launch_tangent(const KParams<float>& k, const StaticParams<float>& q, int groups, int threads, hipStream_t st) {
    return tangent_impl<float>(k, q, groups, threads, st);
}
hipError_t launch_static(const KParams<double>& k, const StaticParams<double>& q, int groups, int threads, hipStream_t st) {
    if (threads > STATIC_MAX_NT) return hipErrorInvalidValue;
    const size_t lds = static_lds_bytes<double>(threads);
    if (hipError_t e = lds_opt_in(crb_static_kernel<double>, lds)) return e;
    hipLaunchKernelGGL(crb_static_kernel<double>, dim3(groups), dim3(threads), lds, st, k, q);
    return hipGetLastError();
}
}  // namespace crb
