// crb_implicit_feedback_adjoint.hip -- the sample-boundary kernels of the adjoint of the sampled-data implicit loop
// (crb_implicit_feedback_adjoint.h), one translation unit of their own.
#include "crb_implicit_feedback_adjoint.h"
#include "crb_host.h"

namespace crb {
hipError_t launch_imp_fb_boundary(const ImpFbAdjParams& p, hipStream_t st) {
    if (!p.ubar || !fba_shape_ok(p) || !p.gain || !p.lam) return hipErrorInvalidValue;
    const size_t smem = fba_product_lds_bytes(p.n);
    if (hipError_t e = lds_opt_in(crb_imp_fb_boundary_kernel, smem)) return e;
    const dim3 grid((p.rows + FBA_T - 1) / FBA_T, (p.n2 + FBA_T - 1) / FBA_T);
    hipLaunchKernelGGL(crb_imp_fb_boundary_kernel, grid, dim3(256), smem, st, p);
    return hipGetLastError();
}

hipError_t launch_imp_fb_gain_grad(const ImpFbAdjParams& p, hipStream_t st) {
    if (!p.ubar || !fba_shape_ok(p) || !p.xs || p.n_samples < 1) return hipErrorInvalidValue;
    ImpFbAdjParams q = p;
    q.slices = feedback_gain_grad_slices(p.B, p.n);
    if (q.slices > 1 ? !q.partial : !q.gain_bar) return hipErrorInvalidValue;
    const dim3 grid((p.n + FBA_T - 1) / FBA_T, ((p.n2 + FBA_T - 1) / FBA_T) * q.slices, p.rows / p.B);
    if (p.ref) hipLaunchKernelGGL(crb_imp_fb_gain_grad_kernel<true>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(crb_imp_fb_gain_grad_kernel<false>, grid, dim3(256), 0, st, q);
    return hipGetLastError();
}
}  // namespace crb
