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
template <bool TRANSPOSE, int NR>
hipError_t sens_impl(const KParams<double>& k, const StaticSensParams<double>& q, int groups, int threads, hipStream_t st) {
    const size_t lds = static_lds_bytes<double>(threads, static_sens_xcols(NR));
    if (hipError_t e = lds_opt_in(crb_static_sens_kernel<double, TRANSPOSE, NR>, lds)) return e;
    hipLaunchKernelGGL((crb_static_sens_kernel<double, TRANSPOSE, NR>), dim3(groups, (q.n_dir + NR - 1) / NR), dim3(threads), lds,
                       st, k, q);
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
hipError_t launch_static_sens(const KParams<double>& k, const StaticSensParams<double>& q, bool transpose, int groups, int threads,
                              hipStream_t st) {
    if (threads > STATIC_MAX_NT || q.n_dir < 1 || q.n_dir > 65535) return hipErrorInvalidValue;
    if (q.status)
        if (hipError_t e = hipMemsetAsync(q.status, 0, size_t(k.B) * sizeof(int32_t), st)) return e;
    if (q.n_dir < STATIC_SENS_NR)   // (a lone direction does not pay for the wide exchange)
        return transpose ? sens_impl<true, 1>(k, q, groups, threads, st) : sens_impl<false, 1>(k, q, groups, threads, st);
    return transpose ? sens_impl<true, STATIC_SENS_NR>(k, q, groups, threads, st)
                     : sens_impl<false, STATIC_SENS_NR>(k, q, groups, threads, st);
}
}  // namespace crb
