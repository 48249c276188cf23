// crb_implicit_adjoint.hip -- the implicit stepper's adjoint kernels (crb_implicit_adjoint.h), one translation unit of their own.
#include "crb_implicit_adjoint_launch.h"
#include "crb_implicit_paramgrad.h"

namespace crb {
namespace {
template <int MODE>
hipError_t imp_adj_impl(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups, int n_cot,
                        int threads, hipStream_t st) {
    if (threads > ADJ_MAX_NT || n_cot < 1 || n_cot > 65535 || iq.n_iter < 1) return hipErrorInvalidValue;
    const dim3 grid(groups, n_cot), block(threads);
    const size_t smem = adjoint_lds_bytes<double>(threads);
    // a control schedule (k.sched_*) runs the SCHED instances; calls without one run the instances they always did
    if (k.sched_stride) hipLaunchKernelGGL((crb_imp_adj_kernel<double, MODE, true>), grid, block, smem, st, k, q, iq);
    else hipLaunchKernelGGL((crb_imp_adj_kernel<double, MODE, false>), grid, block, smem, st, k, q, iq);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_imp_adj_checkpoint(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                     int threads, hipStream_t st) {
    return imp_adj_impl<IADJ_CKPT>(k, q, iq, groups, 1, threads, st);
}
hipError_t launch_imp_adj_segment(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                  int threads, hipStream_t st) {
    return imp_adj_impl<IADJ_SEG>(k, q, iq, groups, 1, threads, st);
}
hipError_t launch_imp_adj_segment_final(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq,
                                        int groups, int threads, hipStream_t st) {
    return imp_adj_impl<IADJ_SEG_FIN>(k, q, iq, groups, 1, threads, st);
}
hipError_t launch_imp_adj_backward(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                   int n_cot, int threads, hipStream_t st) {
    return imp_adj_impl<IADJ_BWD>(k, q, iq, groups, n_cot, threads, st);
}
hipError_t launch_imp_adj_backward_store(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq,
                                         int groups, int n_cot, int threads, hipStream_t st) {
    return imp_adj_impl<IADJ_BWD_STORE>(k, q, iq, groups, n_cot, threads, st);
}
hipError_t launch_imp_param_grad(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                 int n_cot, int threads, hipStream_t st) {
    if (threads > ADJ_MAX_NT || n_cot < 1 || n_cot > 65535 || iq.n_iter < 1) return hipErrorInvalidValue;
    const dim3 grid(groups, n_cot), block(threads);
    const size_t smem = adjoint_lds_bytes<double>(threads);
    if (k.sched_stride) hipLaunchKernelGGL((crb_imp_param_grad_kernel<double, true>), grid, block, smem, st, k, q, iq);
    else hipLaunchKernelGGL((crb_imp_param_grad_kernel<double, false>), grid, block, smem, st, k, q, iq);
    return hipGetLastError();
}
}  // namespace crb
