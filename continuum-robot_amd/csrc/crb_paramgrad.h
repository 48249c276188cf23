// crb_paramgrad.h -- gradients of an RK4 rollout with respect to the rod: stiffness scales per element, the drag factor per
// node and the gravity vector per segment (crb_step_rk4_adjoint_params).
//
// What is summed.  The right-hand side r = u - k(q) + f_drag(v) + f_grav(q) is linear in every parameter that stays out of the
// mass matrix, so with rbar = M^-T lambda_v of a stage (the ub of adj_vjp, which the storing sweep crb_adj_kernel<double,
// ADJ_BWD_STORE> wrote masked to aq.rbar) the parameter gradient is a sum over stages of rbar dotted with forces:
//   - stiffness: k of the element left of node j is EA k_A(q) + EI k_I(q) for both element kinds (crb_math.h ElemCoef:
//     nonlinear c[1], c[2], c[4] ~ EA and c[3], c[5] ~ EI with c[0] = L fixed; linear c[0] ~ EA and c[1..4] ~ EI), so
//         sA_j += -<(rbar_{j-1}, rbar_j), elem_force(pack_A)(q_{j-1}, q_j)>,   sI_j the same with pack_I,
//     pack_A the slot's pack with the EI entries 0 and pack_I with the EA entries 0: gradients with respect to RELATIVE scales
//     of EA and EI at scale 1 (no division here); `corrected` as elem_force honours it;
//   - drag:      sD_j += rbar_{w,j} drag_force(sc.drag, v_w), relative to the node's factor too;
//   - gravity of segment j: gb = the rbar entries its two components landed on (the sg gathers of adj_vjp, GravAdj), phi
//     its averaged rotation (the fq gathers), (s, c) = sincos(phi):
//         gx_j += half_mass (c gb0 - s gb1),   gy_j += half_mass (s gb0 + c gb1),
//     left per slot: the caller sums over slots in an order of its own choosing.
// Constrained DOFs: rbar is stored masked and the stage points are masked on load, as in the sweep.
//
// Mapping.  make_topo's, on the sweep's grid groups x n_cot.  A thread reads its own and its left neighbour's stage point and
// rbar by plain global loads; only the gravity gathers, which follow the plan's tables wherever they point, go through an
// LDS copy of q and rbar (AdjLds rows, AdjIdx offsets).  The thread walks the segment's steps and stages in the sweep's order
// with five accumulators in registers, loaded from param_bar at the start of the segment and stored at its end: like
// f_held_bar, the result is the same additions in the same order for any `every`.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_adjoint.h"

namespace crb {

// the slot's coefficient pack with the bending (keep_axial) or the axial (!keep_axial) entries zeroed
template <typename T>
__device__ __forceinline__ ElemCoef<T> stiffness_part(const ElemCoef<T>& e, bool keep_axial) {
    ElemCoef<T> o = e;
    const bool nl = e.kind == KIND_NONLINEAR;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const bool axial = nl ? (i == 1 || i == 2 || i == 4) : (i == 0);
        const bool fixed = nl && i == 0;   // (L)
        if (!fixed && axial != keep_axial) o.c[i] = T(0);
    }
    return o;
}

// The sums above at one point, from values in registers: this node's and its left neighbour's position (q, ql; masked), this
// node's transverse velocity vw and the masked cotangents (rb, rl) of the two nodes.  Adds into acc = (sA, sI, sD, gx, gy) in
// the order the rollout kernel has always used.  Whole workgroup when grav_on (two barriers); drag_on false leaves sD alone.
template <typename T>
__device__ __forceinline__ void param_point_sums(const AdjLds<T>& L, const Topo& tp, const SlotConst<T>& sc, const ElemCoef<T>& eA,
                                                 const ElemCoef<T>& eI, const AdjIdx<T>& ix, const T (&q)[3], const T (&ql)[3], T vw,
                                                 const T (&rb)[3], const T (&rl)[3], bool drag_on, bool grav_on, bool corrected,
                                                 T (&acc)[5]) {
    const int NT = L.NT;
    T fl[3], fr[3];
    elem_force<T>(eA, ql, q, corrected, fl, fr);
    acc[0] = acc[0] - (rl[0] * fl[0] + rl[1] * fl[1] + rl[2] * fl[2] + rb[0] * fr[0] + rb[1] * fr[1] + rb[2] * fr[2]);
    elem_force<T>(eI, ql, q, corrected, fl, fr);
    acc[1] = acc[1] - (rl[0] * fl[0] + rl[1] * fl[1] + rl[2] * fl[2] + rb[0] * fr[0] + rb[1] * fr[1] + rb[2] * fr[2]);
    if (drag_on) acc[2] = acc[2] + rb[1] * drag_force<T>(sc.drag, vw);
    if (grav_on) {   // (workgroup-uniform)
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) { L.q[c * NT + tp.t] = q[c]; L.rb[c * NT + tp.t] = rb[c]; }
        __syncthreads();
        T gb[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) gb[m] = L.base[ix.sg[m][0]] + L.base[ix.sg[m][1]];
        const T phi = ix.phim * (L.base[ix.fq[0]] + L.base[ix.fq[1]]);
        T sn, cs;
        crb_sincos(phi, &sn, &cs);
        acc[3] = acc[3] + sc.half_mass * (cs * gb[0] - sn * gb[1]);
        acc[4] = acc[4] + sc.half_mass * (sn * gb[0] + cs * gb[1]);
    }
}

// One stage point of the sums above: the state record `w` (positions at w[c], velocities a `plane` further) and the masked
// rbar record `r` of this thread's node, both null-safe only through `valid`; the left neighbour's records lie one node
// (4 values) before.  Loads them and adds param_point_sums.
template <typename T>
__device__ __forceinline__ void param_stage_point(const AdjLds<T>& L, const Topo& tp, const SlotConst<T>& sc, const T (&ml)[3],
                                                  const ElemCoef<T>& eA, const ElemCoef<T>& eI, const AdjIdx<T>& ix, bool valid,
                                                  bool has_l, const T* w, const T* r, size_t plane, bool drag_on, bool grav_on,
                                                  bool corrected, T (&acc)[5]) {
    T q[3] = {T(0), T(0), T(0)}, ql[3] = {T(0), T(0), T(0)}, rb[3] = {T(0), T(0), T(0)}, rl[3] = {T(0), T(0), T(0)};
    T vw = T(0);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { q[c] = w[c] * sc.mask[c]; rb[c] = r[c]; }
        if (drag_on) vw = w[plane + 1] * sc.mask[1];
        if (has_l)
#pragma unroll
            for (int c = 0; c < 3; ++c) { ql[c] = w[c - 4] * ml[c]; rl[c] = r[c - 4]; }
    }
    param_point_sums<T>(L, tp, sc, eA, eI, ix, q, ql, vw, rb, rl, drag_on, grav_on, corrected, acc);
}

// crb_static_vjp's parameter records: one "stage point", the equilibrium itself.  aq.work = the state whose plane 0 holds q,
// aq.rbar = mu [n_cot][B][n_node][4] (masked, as crb_static_sens_kernel stores it), aq.param_bar written, not accumulated.  No
// drag term: the velocities of an equilibrium are zero whatever the state's second plane holds.  Grid and LDS as below.
template <typename T>
__global__ void __launch_bounds__(ADJ_MAX_NT) crb_static_param_kernel(const KParams<T> p, const AdjParams<T> aq) {
    static_assert(sizeof(T) == 8, "the adjoint kernels are fp64");
    const AdjLds<T> L = carve_adjoint_lds<T>(blockDim.x);
    const int NT = L.NT;
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    const size_t d = blockIdx.y;
    const bool grav_on = (p.flags & 2u) != 0, corrected = (p.flags & 4u) != 0;
    const SlotConst<T>* const slots = p.slot + size_t(tp.beam) * p.slot_stride;
    const SlotConst<T> sc = valid ? slots[tp.j] : padding_slot<T>();
    const bool has_l = valid && tp.j >= 1;
    T ml[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ml[c] = has_l ? slots[tp.j - 1].mask[c] : T(0);
    const ElemCoef<T> eA = stiffness_part<T>(sc.elem, true), eI = stiffness_part<T>(sc.elem, false);
    AdjIdx<T> ix;
    adj_index<T>(p, aq, tp, sc, NT, ix);
    if (threadIdx.x == 0) L.base[ADJ_LDS_ZERO * NT] = T(0);
    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t xoff = size_t(tp.beam) * 2 * plane + node * 4, uoff = size_t(tp.beam) * plane + node * 4;
    T acc[5] = {T(0), T(0), T(0), T(0), T(0)};
    param_stage_point<T>(L, tp, sc, ml, eA, eI, ix, valid, has_l, aq.work + xoff, aq.rbar + d * size_t(p.B) * plane + uoff, plane,
                         false, grav_on, corrected, acc);
    if (!valid) return;
    T* const out = aq.param_bar + ((d * size_t(p.B) + tp.beam) * size_t(p.n_node) + node) * 8;
#pragma unroll
    for (int c = 0; c < 5; ++c) out[c] = acc[c];
#pragma unroll
    for (int c = 5; c < 8; ++c) out[c] = T(0);
    if (p.off == 1 && tp.j == 0)
#pragma unroll
        for (int c = 0; c < 8; ++c) out[c - 8] = T(0);
}

// p: the plan's tables and shape, p.n_steps = steps of the segment.  aq: gadj / gadj_beam, work (stage points), rbar,
// param_bar.  Grid groups x n_cot, blockDim = the plan's NT, adjoint_lds_bytes<T>(NT) of LDS.
template <typename T>
__global__ void __launch_bounds__(ADJ_MAX_NT) crb_param_grad_kernel(const KParams<T> p, const AdjParams<T> aq) {
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
    const size_t state_sz = size_t(p.B) * 2 * plane;
    const size_t uoff = size_t(tp.beam) * plane + node * 4;
    const size_t rb_sz = size_t(gridDim.y) * size_t(p.B) * plane;   // one stage of rbar, every cotangent
    const bool zero_node0 = p.off == 1 && tp.j == 0;   // node 0 (FIXED in every beam, no slot) is written zero
    T* const out = aq.param_bar + ((d * size_t(p.B) + tp.beam) * size_t(p.n_node) + node) * 8;

    T acc[5] = {T(0), T(0), T(0), T(0), T(0)};   // sA, sI, sD, gx, gy
    if (valid)
#pragma unroll
        for (int c = 0; c < 5; ++c) acc[c] = out[c];

#pragma unroll 1
    for (int i = p.n_steps - 1; i >= 0; --i) {
#pragma unroll 1
        for (int s = 3; s >= 0; --s) {
            const size_t st = size_t(i) * 4 + size_t(s);
            param_stage_point<T>(L, tp, sc, ml, eA, eI, ix, valid, has_l, aq.work + st * state_sz + xoff,
                                 aq.rbar + st * rb_sz + d * size_t(p.B) * plane + uoff, plane, drag_on, grav_on, corrected, acc);
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
