// crb_implicit_feedback_tangent.hip -- the sample-boundary kernel of the tangent of the sampled-data implicit loop
// (crb_implicit_feedback_tangent.h), one translation unit of its own.
#include "crb_implicit_feedback_tangent.h"
#include "crb_host.h"

namespace crb {
hipError_t launch_imp_fb_tangent_boundary(const ImpFbTanParams& p, hipStream_t st) {
    if (p.B < 1 || p.n < 1 || p.n2 != 2 * p.n || p.n_dir < 1 || p.n_dir > 65535) return hipErrorInvalidValue;
    if (!p.col_off || !p.row_off || !p.gain || !p.x || !p.dx || !p.u || !p.du) return hipErrorInvalidValue;
    const size_t smem = fbt_lds_bytes(p.n2);
    if (hipError_t e = lds_opt_in(crb_imp_fb_tangent_boundary_kernel, smem)) return e;
    const long long gx = (long long)(p.n_dir + 1) * ((p.B + FBA_T - 1) / FBA_T);
    if (gx > 2147483647LL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (p.n + FBA_T - 1) / FBA_T);
    hipLaunchKernelGGL(crb_imp_fb_tangent_boundary_kernel, grid, dim3(256), smem, st, p);
    return hipGetLastError();
}
}  // namespace crb
