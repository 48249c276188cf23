// crb_feedback_adjoint.hip -- the closed-loop adjoint kernels (crb_feedback_adjoint.h), one translation unit of their own.
#include "crb_feedback_adjoint.h"
#include "crb_host.h"

namespace crb {
hipError_t launch_feedback_transpose(const FeedbackAdjParams& p, hipStream_t st) {
    if (!fba_shape_ok(p)) return hipErrorInvalidValue;
    const size_t smem = fba_product_lds_bytes(p.n);
    if (hipError_t e = lds_opt_in(crb_feedback_transpose_kernel, smem)) return e;
    const dim3 grid((p.rows + FBA_T - 1) / FBA_T, (p.n2 + FBA_T - 1) / FBA_T);
    hipLaunchKernelGGL(crb_feedback_transpose_kernel, grid, dim3(256), smem, st, p);
    return hipGetLastError();
}

hipError_t launch_feedback_gain_grad(const FeedbackAdjParams& p, hipStream_t st) {
    if (!fba_shape_ok(p)) return hipErrorInvalidValue;
    FeedbackAdjParams q = p;
    q.slices = feedback_gain_grad_slices(p.B, p.n);
    if (q.slices > 1 && !q.partial) return hipErrorInvalidValue;
    const int n_cot = p.rows / p.B;
    const dim3 grid((p.n + FBA_T - 1) / FBA_T, ((p.n2 + FBA_T - 1) / FBA_T) * q.slices, n_cot);
    if (p.ref) hipLaunchKernelGGL(crb_feedback_gain_grad_kernel<true>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(crb_feedback_gain_grad_kernel<false>, grid, dim3(256), 0, st, q);
    if (hipError_t e = hipGetLastError()) return e;
    return q.slices > 1 ? launch_feedback_gain_reduce(q.gain_bar, q.partial, p.n, n_cot, q.slices, st) : hipSuccess;
}

hipError_t launch_feedback_gain_reduce(double* gain_bar, const double* partial, int n, int n_cot, int slices, hipStream_t st) {
    if (!gain_bar || !partial || n < 1 || n_cot < 1 || slices < 1) return hipErrorInvalidValue;
    const size_t per_cot = size_t(n) * size_t(2 * n), total = per_cot * size_t(n_cot);
    hipLaunchKernelGGL(crb_feedback_gain_reduce_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, gain_bar, partial, per_cot,
                       slices, total);
    return hipGetLastError();
}

hipError_t launch_feedback_seed(double* lam, double* seed, size_t total, size_t x_stride, double c, const double* rec_bar,
                                size_t rec_off, int rec_n, int kr, hipStream_t st) {
    if (!total || !x_stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crb_feedback_seed_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, lam, seed, total, x_stride, c,
                       rec_bar, rec_off, rec_n, kr);
    return hipGetLastError();
}

hipError_t launch_feedback_record(const double* x, size_t x_stride, size_t off, int B, double* out, int rec_n, int kr,
                                  hipStream_t st) {
    hipLaunchKernelGGL(crb_feedback_record_kernel, dim3((B + 255) / 256), dim3(256), 0, st, x, x_stride, off, B, out, rec_n, kr);
    return hipGetLastError();
}

hipError_t launch_feedback_held(double* u, const double* held, const int32_t* row_off, int n, int B, size_t u_stride, hipStream_t st) {
    if (n < 1 || B < 1) return hipErrorInvalidValue;
    const size_t total = size_t(B) * size_t(n);
    hipLaunchKernelGGL(crb_feedback_held_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, u, held, row_off, n, u_stride,
                       total);
    return hipGetLastError();
}
}  // namespace crb
