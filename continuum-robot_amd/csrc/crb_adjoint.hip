// crb_adjoint.hip -- the adjoint kernels (crb_adjoint.h), one translation unit of their own.
#include "crb_adjoint_launch.h"
#include "crb_paramgrad.h"

namespace crb {
namespace {
template <int MODE>
hipError_t adj_impl(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads, hipStream_t st) {
    if (threads > ADJ_MAX_NT || n_cot < 1 || n_cot > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((crb_adj_kernel<double, MODE>), dim3(groups, n_cot), dim3(threads), adjoint_lds_bytes<double>(threads), st, k, q);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_adj_rhs(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads, hipStream_t st) {
    return adj_impl<ADJ_RHS>(k, q, groups, n_cot, threads, st);
}
hipError_t launch_adj_forward(const KParams<double>& k, const AdjParams<double>& q, int groups, int threads, hipStream_t st) {
    return adj_impl<ADJ_FWD>(k, q, groups, 1, threads, st);
}
hipError_t launch_adj_backward(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads, hipStream_t st) {
    return adj_impl<ADJ_BWD>(k, q, groups, n_cot, threads, st);
}
hipError_t launch_adj_backward_store(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads,
                                     hipStream_t st) {
    return adj_impl<ADJ_BWD_STORE>(k, q, groups, n_cot, threads, st);
}
hipError_t launch_param_grad(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads, hipStream_t st) {
    if (threads > ADJ_MAX_NT || n_cot < 1 || n_cot > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((crb_param_grad_kernel<double>), dim3(groups, n_cot), dim3(threads), adjoint_lds_bytes<double>(threads), st, k, q);
    return hipGetLastError();
}
hipError_t launch_static_param(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads,
                               hipStream_t st) {
    if (threads > ADJ_MAX_NT || n_cot < 1 || n_cot > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((crb_static_param_kernel<double>), dim3(groups, n_cot), dim3(threads), adjoint_lds_bytes<double>(threads), st, k, q);
    return hipGetLastError();
}
}  // namespace crb
