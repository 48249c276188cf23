// crb_implicit_paramgrad.h -- gradients of an implicit rollout with respect to the rod: stiffness scales per element, the drag
// factor per node and the gravity vector per segment (crb_step_implicit_adjoint_params), in crb_paramgrad.h's record.
//
// What is summed.  Iteration i of a step is a^{i+1} = Ainv (F(q_m, v_m; theta) + u + alpha K0(theta) a^i) with
// A = M + alpha K0(theta) (crb_implicit_adjoint.h), and the sweep forms gbar = Ainv^T abar of that iteration (the storing sweep
// crb_imp_adj_kernel<double, IADJ_BWD_STORE> wrote it masked to iq.gbar).  With dAinv = -Ainv (alpha dK0) Ainv -- the truncated
// reduction equals A^-1 to the unit roundoff by construction of the tables -- the iteration adds to the cotangent of theta
//     gbar^T dF/dtheta (q_m, v_m)   +   alpha gbar^T (dK0/dtheta) (a^i - a^{i+1})
//   - the first term is crb_paramgrad.h's sum (param_point_sums) with gbar in the place of rbar and (q_m, v_m) as the point;
//   - the second exists for sA and sI only (drag and gravity are not in K0): dK0/dsA d is imp_k0's element product
//     (imp_k0_elem) on the slot's pack with the EI entries zeroed, dK0/dsI d the same with the EA entries zeroed
//     (stiffness_part: the packs of the first term), d = a^i - a^{i+1} masked like a^i.  It vanishes as the iteration converges.
// a^{i+1} is the next stored iterate of the step, the next step's a^0, or after the segment's last step the record IADJ_SEG
// wrote to iq.fin_out.  At the first step of a schedule interval a^0 = 0 and its slot holds the final iterate of the step before
// (ImpAdjParams::fin_out): read as a^{i+1} there, replaced by 0 as a^i.
//
// Mapping, LDS, constrained DOFs and the accumulators: those of crb_param_grad_kernel.  A thread reads its own and its left
// neighbour's (q0, v0), iterates and gbar by plain global loads and rebuilds (q_m, v_m) by the forward's own operations; it
// walks the segment's steps and iterations in the sweep's order with five accumulators in registers, loaded from param_bar at
// the start of the segment and stored at its end: the result is the same additions in the same order for any `every`, and
// every cotangent (grid y) sums on its own.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_implicit_adjoint.h"
#include "crb_paramgrad.h"

namespace crb {

// p: A's launch block (p.dt = h, p.n_steps = steps of the segment, p.sched_hold with SCHED).  aq: gadj / gadj_beam, work (the
// steps' start states [n_steps][B][2][n_node][4]), step0, param_bar.  iq: iters, gbar, fin_out (read), n_iter.  Grid groups x
// n_cot, blockDim = the plan's NT, adjoint_lds_bytes<T>(NT) of LDS.
template <typename T, bool SCHED = false>
__global__ void __launch_bounds__(ADJ_MAX_NT) crb_imp_param_grad_kernel(const KParams<T> p, const AdjParams<T> aq,
                                                                        const ImpAdjParams<T> iq) {
    static_assert(sizeof(T) == 8, "the adjoint kernels are fp64");
    const AdjLds<T> L = carve_adjoint_lds<T>(blockDim.x);
    const int NT = L.NT;
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    const size_t d = blockIdx.y;
    const bool drag_on = (p.flags & 1u) != 0, grav_on = (p.flags & 2u) != 0, corrected = (p.flags & 4u) != 0;

    const SlotConst<T>* const slots = p.slot + size_t(tp.beam) * p.slot_stride;
    const SlotConst<T> sc = valid ? slots[tp.j] : padding_slot<T>();
    const bool has_l = valid && tp.j >= 1;
    T ml[3];   // the left neighbour's mask
#pragma unroll
    for (int c = 0; c < 3; ++c) ml[c] = has_l ? slots[tp.j - 1].mask[c] : T(0);
    const ElemCoef<T> eA = stiffness_part<T>(sc.elem, true), eI = stiffness_part<T>(sc.elem, false);
    AdjIdx<T> ix;
    adj_index<T>(p, aq, tp, sc, NT, ix);
    if (threadIdx.x == 0) L.base[ADJ_LDS_ZERO * NT] = T(0);   // (read after the barrier every gather follows)

    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t xoff = size_t(tp.beam) * 2 * plane + node * 4;
    const size_t state_sz = size_t(p.B) * 2 * plane, force_sz = size_t(p.B) * plane;
    const size_t uoff = size_t(tp.beam) * plane + node * 4;
    const size_t gb_stride = size_t(gridDim.y) * force_sz;   // one iteration of gbar, every cotangent
    const bool zero_node0 = p.off == 1 && tp.j == 0;         // node 0 (FIXED in every beam, no slot) is written zero
    T* const out = aq.param_bar + ((d * size_t(p.B) + tp.beam) * size_t(p.n_node) + node) * 8;
    const T hh = T(0.5 * p.dt), alpha = T(0.25 * p.dt * p.dt);

    T acc[5] = {T(0), T(0), T(0), T(0), T(0)};   // sA, sI, sD, gx, gy
    T an[3] = {T(0), T(0), T(0)}, anl[3] = {T(0), T(0), T(0)};   // a^{i+1} of this node and of its left neighbour, masked
    if (valid) {
#pragma unroll
        for (int c = 0; c < 5; ++c) acc[c] = out[c];
        const T* const f = iq.fin_out + uoff;
#pragma unroll
        for (int c = 0; c < 3; ++c) an[c] = f[c] * sc.mask[c];
        if (has_l)
#pragma unroll
            for (int c = 0; c < 3; ++c) anl[c] = f[c - 4] * ml[c];
    }

#pragma unroll 1
    for (int i = p.n_steps - 1; i >= 0; --i) {
        bool first = false;   // (the step opens a schedule interval: its a^0 is 0, its slot holds the step before's final iterate)
        if constexpr (SCHED) first = (aq.step0 + i) % p.sched_hold == 0;
        // qp = q0 + hh v0 of the two nodes, and this node's transverse velocity (drag reads nothing else of v_m)
        T qp[3] = {T(0), T(0), T(0)}, qpl[3] = {T(0), T(0), T(0)}, v0w = T(0);
        if (valid) {
            const T* const w = aq.work + size_t(i) * state_sz + xoff;
#pragma unroll
            for (int c = 0; c < 3; ++c) qp[c] = w[c] * sc.mask[c] + hh * (w[plane + c] * sc.mask[c]);
            v0w = w[plane + 1] * sc.mask[1];
            if (has_l)
#pragma unroll
                for (int c = 0; c < 3; ++c) qpl[c] = w[c - 4] * ml[c] + hh * (w[plane + c - 4] * ml[c]);
        }
#pragma unroll 1
        for (int it = iq.n_iter - 1; it >= 0; --it) {
            const size_t rec = size_t(i) * size_t(iq.n_iter) + size_t(it);
            T as[3] = {T(0), T(0), T(0)}, asl[3] = {T(0), T(0), T(0)};   // what the iterate's slot holds
            T gb[3] = {T(0), T(0), T(0)}, gl[3] = {T(0), T(0), T(0)};
            if (valid) {
                const T* const ai = iq.iters + rec * force_sz + uoff;
                const T* const gi = iq.gbar + rec * gb_stride + d * force_sz + uoff;
#pragma unroll
                for (int c = 0; c < 3; ++c) { as[c] = ai[c] * sc.mask[c]; gb[c] = gi[c]; }
                if (has_l)
#pragma unroll
                    for (int c = 0; c < 3; ++c) { asl[c] = ai[c - 4] * ml[c]; gl[c] = gi[c - 4]; }
            }
            const bool zero = SCHED && first && it == 0;
            T q[3], ql[3], dd[3], ddl[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const T a = zero ? T(0) : as[c], al = zero ? T(0) : asl[c];
                q[c] = qp[c] + alpha * a;
                ql[c] = qpl[c] + alpha * al;
                dd[c] = a - an[c];
                ddl[c] = al - anl[c];
                an[c] = as[c];
                anl[c] = asl[c];
            }
            const T vw = v0w + hh * (zero ? T(0) : as[1]);
            // the iteration matrix: alpha gbar^T (dK0/dsA, dK0/dsI) d on the element left of the node
            T kl[3], kr[3];
            imp_k0_elem<T>(eA, corrected, ddl, dd, kl, kr);
            acc[0] = acc[0] + alpha * (gl[0] * kl[0] + gl[1] * kl[1] + gl[2] * kl[2] + gb[0] * kr[0] + gb[1] * kr[1] + gb[2] * kr[2]);
            imp_k0_elem<T>(eI, corrected, ddl, dd, kl, kr);
            acc[1] = acc[1] + alpha * (gl[0] * kl[0] + gl[1] * kl[1] + gl[2] * kl[2] + gb[0] * kr[0] + gb[1] * kr[1] + gb[2] * kr[2]);
            // the right-hand side: crb_paramgrad.h's sums at (q_m, v_m)
            param_point_sums<T>(L, tp, sc, eA, eI, ix, q, ql, vw, gb, gl, drag_on, grav_on, corrected, acc);
        }
    }
    if (!valid) return;
#pragma unroll
    for (int c = 0; c < 5; ++c) out[c] = acc[c];
#pragma unroll
    for (int c = 5; c < 8; ++c) out[c] = T(0);
    if (zero_node0)
#pragma unroll
        for (int c = 0; c < 8; ++c) out[c - 8] = T(0);
}

}  // namespace crb
