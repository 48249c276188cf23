// crb_implicit_feedback.hip -- the implicit stepper with zero-order-hold state feedback (crb_stiff.h, FB), one translation
// unit of its own.
#include "crb_implicit_feedback_launch.h"

#include "crb_host.h"

namespace crb {
namespace {
template <int LV>
hipError_t implicit_feedback_lv(const KParams<double>& k, const StiffFbParams<double>& q, int groups, size_t smem, hipStream_t st) {
    auto kernel = crb_implicit_kernel<double, LV, 64, 1, false, false, true>;
    if (hipError_t e = lds_opt_in(kernel, smem)) return e;
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(64), smem, st, k, q);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_implicit_feedback(const KParams<double>& k, const StiffFbParams<double>& q, int levels, int groups, size_t smem,
                                    hipStream_t st) {
    if (!implicit_feedback_built(levels) || groups < 1 || q.hold < 1 || k.lognw != 0 || !k.fb_gain || !k.red_map ||
        smem > size_t(160) * 1024 || smem < implicit_feedback_lds_bytes(64, k.G, k.n_red))
        return hipErrorInvalidValue;
    return with_int<0, 6>(levels, [&](auto lv) { return implicit_feedback_lv<lv>(k, q, groups, smem, st); });
}
}  // namespace crb
