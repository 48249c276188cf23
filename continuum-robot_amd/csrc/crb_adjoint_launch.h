// crb_adjoint_launch.h -- host entry of the adjoint translation unit (crb_adjoint.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_adjoint.h"

namespace crb {
// crb_adj_kernel<double, ADJ_RHS> on a grid of `groups` x `n_cot` workgroups of `threads` (<= ADJ_MAX_NT) threads
hipError_t launch_adj_rhs(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads, hipStream_t st);
// crb_adj_kernel<double, ADJ_FWD>: k.n_steps RK4 steps, the start state of every q.store_every-th written to q.states
hipError_t launch_adj_forward(const KParams<double>& k, const AdjParams<double>& q, int groups, int threads, hipStream_t st);
// crb_adj_kernel<double, ADJ_BWD>: the backward sweep over one segment of k.n_steps steps, for n_cot cotangents
hipError_t launch_adj_backward(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads, hipStream_t st);
// crb_adj_kernel<double, ADJ_BWD_STORE>: the same sweep, every stage's masked rbar also written to q.rbar
hipError_t launch_adj_backward_store(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads,
                                     hipStream_t st);
// crb_param_grad_kernel<double> (crb_paramgrad.h): the parameter sums of one segment of k.n_steps steps over q.work and q.rbar
hipError_t launch_param_grad(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads, hipStream_t st);
// crb_static_param_kernel<double> (crb_paramgrad.h): crb_static_vjp's parameter records from q.work (the state) and q.rbar (mu)
hipError_t launch_static_param(const KParams<double>& k, const AdjParams<double>& q, int groups, int n_cot, int threads,
                               hipStream_t st);
}  // namespace crb
