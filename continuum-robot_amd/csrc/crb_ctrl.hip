// crb_ctrl.hip -- the step-size-controlled steppers (crb_ctrl.h), one translation unit of their own.
#include "crb_ctrl_launch.h"
#include "crb_host.h"

namespace crb {
hipError_t launch_gain_transpose(const double* K, double* Kt, int n, int rows, hipStream_t st) {
    if (n < 1 || rows < 2 * n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crb_gain_transpose_kernel<double>, dim3((rows + 31) / 32, (n + 31) / 32), dim3(256), 0, st, K, Kt, n, 2 * n, rows);
    return hipGetLastError();
}

hipError_t launch_controlled(const KParams<double>& k, const CtrlParams<double>& q, int levels, bool feedback, bool stream_gain, int lean_lognw,
                             bool grav, bool pack, int threads, size_t lds, hipStream_t st) {
    if (threads < 64 || threads > 256 || (threads & 63)) return hipErrorInvalidValue;
    if (stream_gain && (!feedback || !q.gain_t)) return hipErrorInvalidValue;
    if (lean_lognw >= 0 && threads != (64 << lean_lognw)) return hipErrorInvalidValue;
    if (pack && k.G < 2) return hipErrorInvalidValue;
#ifdef CRB_FAST_BUILD
    return hipErrorInvalidValue;
#else
    const bool lean_grav = grav && lean_lognw >= 0;   // (the general RHS reads gravity from its tables: one instance)
    return with_int<0, MAX_LV>(levels, [&](auto lv) { return with_int<-1, 2>(lean_lognw, [&](auto nw) { return with_bool(feedback, [&](auto fb) {
        return with_bool(lean_grav, [&](auto g) { return with_bool(pack, [&](auto pk) { return with_bool(stream_gain, [&](auto sg) {
            if constexpr (controlled_built(lv, fb, nw, g, pk, sg)) {
                constexpr auto kernel = crb_controlled_kernel<double, lv, fb, nw, g, pk, sg>;
                if (hipError_t e = lds_opt_in(kernel, lds)) return e;
                hipLaunchKernelGGL(kernel, dim3(pk ? (k.B + k.G - 1) / k.G : k.B), dim3(threads), lds, st, k, q);
                return hipGetLastError();
            } else {
                return hipErrorInvalidValue;
            }
        }); }); });
    }); }); });
#endif
}
}  // namespace crb
