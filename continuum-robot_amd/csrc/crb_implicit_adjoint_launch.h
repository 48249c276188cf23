// crb_implicit_adjoint_launch.h -- host entry of the implicit stepper's adjoint translation unit (crb_implicit_adjoint.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_implicit_adjoint.h"

namespace crb {
// crb_imp_adj_kernel<double, IADJ_CKPT>: k.n_steps implicit steps of k.x in place, (q, v, starting iterate) of every
// q.store_every-th step written to q.states; `groups` workgroups of `threads` (<= ADJ_MAX_NT) threads
hipError_t launch_imp_adj_checkpoint(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                     int threads, hipStream_t st);
// crb_imp_adj_kernel<double, IADJ_SEG>: the same steps from the checkpoint iq.start, every step's start state, iterates and clock
// written to q.states, iq.iters_out and q.clocks
hipError_t launch_imp_adj_segment(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                  int threads, hipStream_t st);
// crb_imp_adj_kernel<double, IADJ_SEG_FIN>: the same, the last step's final iterate also written to iq.fin_out
hipError_t launch_imp_adj_segment_final(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq,
                                        int groups, int threads, hipStream_t st);
// crb_imp_adj_kernel<double, IADJ_BWD>: the backward sweep over one segment of k.n_steps steps, for n_cot cotangents
hipError_t launch_imp_adj_backward(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                   int n_cot, int threads, hipStream_t st);
// crb_imp_adj_kernel<double, IADJ_BWD_STORE>: the same sweep, every iteration's masked gbar also written to iq.gbar
hipError_t launch_imp_adj_backward_store(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq,
                                         int groups, int n_cot, int threads, hipStream_t st);
// crb_imp_param_grad_kernel<double> (crb_implicit_paramgrad.h): the parameter sums of one segment of k.n_steps steps over q.work,
// iq.iters, iq.gbar and iq.fin_out
hipError_t launch_imp_param_grad(const KParams<double>& k, const AdjParams<double>& q, const ImpAdjParams<double>& iq, int groups,
                                 int n_cot, int threads, hipStream_t st);
}  // namespace crb
