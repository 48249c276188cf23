// crb_implicit_adjoint.h -- reverse-mode derivative of the implicit fixed-step stepper (crb_step_implicit_checkpoint,
// crb_step_implicit_adjoint): the exact discrete adjoint of the map crb_step_implicit COMPUTES (crb_stiff.h: the implicit
// midpoint rule with a fixed number of modified-Newton iterations on A = M + alpha K0), not of the converged rule.
//
// Forward, per step, from (q0, v0) and the starting iterate a^0 (the previous step's final iterate; 0 at the first step of a
// call), alpha = h^2 / 4, hh = h / 2, qp = q0 + hh v0, u = f_held (+ amp on the impulse DOF while t + h/2 < duration):
//     for i = 0 .. n_iter-1:   q_m = qp + alpha a^i,  v_m = v0 + hh a^i,   a^{i+1} = Ainv (F(q_m, v_m) + u + alpha K0 a^i)
//     a = a^{n_iter},   q1 = q0 + h v0 + 2 alpha a,   v1 = v0 + h a;   the next step starts from a.
// Ainv is the plan's truncated cyclic reduction of A with the levels the stepper keeps for this h.  The launch's KParams carry
// A's tables, strides and level count where the RK4 adjoint carries M's, so that adj_accel (Ainv(u' - k(q) + f_drag + f_grav)
// with u' = u + alpha K0 a^i) and adj_vjp (Ainv^T and the transposed Jacobian of F) of crb_adjoint.h apply as they are.
//
// Reverse, given (qbar1, vbar1) and the carry cbar (the cotangent of the next step's starting iterate; 0 at the last step):
//     abar = 2 alpha qbar1 + h vbar1 + cbar,   qbar0 = qbar1,   vbar0 = h qbar1 + vbar1,   qpbar = vpbar = 0
//     for i = n_iter-1 .. 0:   gbar = Ainv^T abar;   ubar += gbar (f_held_bar; amp_bar on the impulse DOF while the step's
//         midpoint clock is < duration);   (qmbar, vmbar) = (dF/dq, dF/dv)^T gbar at that iterate's (q_m, v_m);
//         qpbar += qmbar,  vpbar += vmbar;   abar = alpha qmbar + hh vmbar + alpha K0^T gbar
//     cbar = abar (handed to the previous step; dropped at step 0 of the call, whose a^0 = 0 is a constant)
//     qbar0 += qpbar,   vbar0 += hh qpbar + vpbar
// K0^T gbar (imp_k0t) is the transpose of what imp_k0 applies in the forward pass: elem_force_linear on the elements' linear
// coefficient packs, with the unsymmetric axial block of the shipped nonlinear element (whose left-node row has no u2 term).
//
// Modes.  IADJ_CKPT: the forward pass from p.x (advanced in place), writing (q, v, starting iterate) of every store_every-th
// step to the checkpoints [n_seg][B][3][n_node][4].  IADJ_SEG: the same arithmetic from one checkpoint, writing per step of
// the segment its (q0, v0), its iterates a^0 .. a^{n_iter-1} and its clock.  IADJ_BWD: the sweep back over one segment for
// every cotangent (grid y); lambda, cbar and the input cotangents stay in registers across the segment, cbar passes from one
// segment's launch to the next through `carry`.  The sums are the same additions in the same order for any segment length
// and any number of cotangents: the gradient does not depend on either, bitwise.  No floating-point atomics.
// The parameter path (crb_implicit_paramgrad.h) runs two variants compiled in by the mode, so that the three modes above stay the
// code they were: IADJ_SEG_FIN, the recompute that also keeps the final iterate of the segment's last step, and IADJ_BWD_STORE,
// the sweep that also stores every iteration's masked gbar (one store per iteration, the lane address formed once).
// Mapping, LDS and constrained DOFs: those of crb_adjoint.h.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_adjoint.h"

namespace crb {

// IADJ_BWD_STORE: IADJ_BWD that also writes every iteration's masked gbar for crb_imp_param_grad_kernel (crb_implicit_paramgrad.h)
// IADJ_SEG_FIN: IADJ_SEG that also writes the final iterate of the segment's last step, which the same kernel needs
enum : int { IADJ_CKPT = 0, IADJ_SEG = 1, IADJ_BWD = 2, IADJ_BWD_STORE = 3, IADJ_SEG_FIN = 4 };

// The implicit launches' own fields, next to KParams<T> (A's tables in pcr_levels / pcr_final, p.dt = h) and AdjParams<T>
// (gadj, states / clocks / store_every / write_back, work / work_clock, lam / amp_bar / f_bar, step0 with their meanings there;
// states of IADJ_SEG and work of IADJ_BWD are [n_steps][B][2][n_node][4]).
template <typename T>
struct ImpAdjParams {
    const T* start;   // IADJ_SEG: [B][3][n_node][4] the checkpoint the segment starts from
    T* iters_out;     // IADJ_SEG: [n_steps][n_iter][B][n_node][4] the iterates a^0 .. a^{n_iter-1} of every step
    const T* iters;   // IADJ_BWD: the same
    T* carry;         // IADJ_BWD: [n_cot][B][n_node][4] cbar at the segment's first step, written; read when carry_in
    int carry_in;     // IADJ_BWD: 0 for the call's last segment (cbar = 0)
    int n_iter;
    // the parameter path (last, so that the fields above keep their kernel-argument offsets)
    T* gbar;          // IADJ_BWD_STORE: [n_steps][n_iter][n_cot][B][n_node][4] the masked gbar = Ainv^T abar of every iteration
    T* fin_out;       // IADJ_SEG_FIN: [B][n_node][4] the final iterate a^{n_iter} of the segment's last step.  With a schedule
                      //  the mode also moves the final iterate of every step an interval ends on INSIDE the segment into the
                      //  slot of the next step's a^0 (a constant 0, which IADJ_BWD_STORE and the reduction put back); the
                      //  reduction reads the record
};

// (kl, kr) = the left-node and right-node halves of K0's element block on (zl, a): elem_force_linear on the element's linear
// coefficient pack, with the axial block [[c0, -s c0], [-c0, c0]] (s = 0 for the shipped nonlinear element, whose f1 has no u2 term)
template <typename T>
__device__ __forceinline__ void imp_k0_elem(const ElemCoef<T>& e, bool corrected, const T zl[3], const T a[3], T kl[3], T kr[3]) {
    T lin[5] = {T(0), T(0), T(0), T(0), T(0)};
    elem_linear_coefs<T>(e.c, e.kind, lin);
    elem_force_linear<T>(lin, zl, a, kl, kr);
    if (e.kind == KIND_NONLINEAR && !corrected) kl[0] = lin[0] * zl[0];   // tangent of the shipped f1: no u2 term
}

// out = K0 a of this thread's node: the element left of the node on (a_{j-1}, a_j) by elem_force_linear (its right-node half
// stays, its left-node half goes left through LDS).  Whole workgroup; uses the reduction exchange rows of AdjLds.
template <typename T>
__device__ __forceinline__ void imp_k0(const AdjLds<T>& L, const Topo& tp, const JvpConst<T>& k, const T a[3], T out[3]) {
    const int NT = L.NT;
    const bool has_l = tp.j >= 1, has_r = tp.j + 1 < tp.S;
    const int tl = has_l ? tp.thread_of(tp.j - 1) : tp.t, tr = has_r ? tp.thread_of(tp.j + 1) : tp.t;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) L.r[c * NT + tp.t] = a[c];
    __syncthreads();
    T zl[3], kl[3], kr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) zl[c] = has_l ? L.r[c * NT + tl] : T(0);
    imp_k0_elem<T>(k.sc.elem, k.corrected, zl, a, kl, kr);
#pragma unroll
    for (int c = 0; c < 3; ++c) L.r[(3 + c) * NT + tp.t] = kl[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = kr[c] + (has_r ? L.r[(3 + c) * NT + tr] : T(0));
}

// out = K0^T w of this thread's node.  The bending blocks of the element are symmetric (K12 = K21^T, crb_math.h), so
// elem_force_linear on (w_{j-1}, w_j) is their transpose too; the axial block [[c0, -s c0], [-c0, c0]] (s = 0 for the shipped
// nonlinear element) transposes to a left-node half c0 (w_{j-1} - w_j) and a right-node half c0 (w_j - s w_{j-1}).
template <typename T>
__device__ __forceinline__ void imp_k0t(const AdjLds<T>& L, const Topo& tp, const JvpConst<T>& k, const T w[3], T out[3]) {
    const int NT = L.NT;
    const bool has_l = tp.j >= 1, has_r = tp.j + 1 < tp.S;
    const int tl = has_l ? tp.thread_of(tp.j - 1) : tp.t, tr = has_r ? tp.thread_of(tp.j + 1) : tp.t;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) L.r[c * NT + tp.t] = w[c];
    __syncthreads();
    T wl[3], lin[5] = {T(0), T(0), T(0), T(0), T(0)}, ol[3], orr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) wl[c] = has_l ? L.r[c * NT + tl] : T(0);
    elem_linear_coefs<T>(k.sc.elem.c, k.sc.elem.kind, lin);
    elem_force_linear<T>(lin, wl, w, ol, orr);
    if (k.sc.elem.kind == KIND_NONLINEAR && !k.corrected) orr[0] = lin[0] * w[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) L.r[(3 + c) * NT + tp.t] = ol[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = orr[c] + (has_r ? L.r[(3 + c) * NT + tr] : T(0));
}

// SCHED: a control schedule (crb_input_schedule; KParams sched_*, AdjParams fbar_cot_stride as in crb_adj_kernel) -- a
// compile-time axis, so that the unscheduled instances stay the code they were.  A scheduled call is the chain of one call per
// interval: at an interval's first step the forward modes reload uh and reset the starting iterate to 0 BEFORE that step's
// checkpoint / start-state store, and the sweep drops cbar there, stores the interval's force cotangent and takes up the
// record of the interval below.
template <typename T, int MODE, bool SCHED = false>
__global__ void __launch_bounds__(ADJ_MAX_NT) crb_imp_adj_kernel(const KParams<T> p, const AdjParams<T> aq, const ImpAdjParams<T> iq) {
    static_assert(sizeof(T) == 8, "the adjoint kernels are fp64");
    const AdjLds<T> L = carve_adjoint_lds<T>(blockDim.x);
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    const size_t d = blockIdx.y;

    JvpConst<T> k;
    jvp_load_const<T>(p, tp, k);   // (p.pcr_levels / p.pcr_final: the tables of A)
    const SlotConst<T>& sc = k.sc;
    AdjIdx<T> ix;
    adj_index<T>(p, aq, tp, sc, L.NT, ix);
    if (threadIdx.x == 0) L.base[ADJ_LDS_ZERO * L.NT] = T(0);

    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t xoff = size_t(tp.beam) * 2 * plane + node * 4;
    const size_t coff = size_t(tp.beam) * 3 * plane + node * 4;   // checkpoints: (q, v, starting iterate)
    const size_t state_sz = size_t(p.B) * 2 * plane, force_sz = size_t(p.B) * plane;
    const size_t uoff = size_t(tp.beam) * plane + node * 4;
    const size_t loff = d * state_sz + xoff, luoff = d * force_sz + uoff;
    const size_t fboff = SCHED ? d * aq.fbar_cot_stride + uoff : luoff;   // f_bar ([n_cot][n_intervals][B][n_node][4] with a schedule)
    const bool zero_node0 = p.off == 1 && tp.j == 0;
    T uh[3] = {T(0), T(0), T(0)};
    T amp = T(0);
    bool imp_here = false;
    if (valid) {
        if (p.u_held)
#pragma unroll
            for (int c = 0; c < 3; ++c) uh[c] = p.u_held[uoff + c];
        if (p.amp && tp.j == (p.imp_node_b ? p.imp_node_b[tp.beam] - p.off : p.imp_slot)) {
            amp = p.amp[tp.beam];
            imp_here = true;
        }
    }
    const T h = T(p.dt), hh = T(0.5 * p.dt), alpha = T(0.25 * p.dt * p.dt), alpha2 = T(0.5 * p.dt * p.dt);

    constexpr bool SEG = MODE == IADJ_SEG || MODE == IADJ_SEG_FIN;
    if (MODE == IADJ_CKPT || SEG) {
        T x[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, am[3] = {T(0), T(0), T(0)};
        if (valid) {
            if (SEG) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    x[c] = iq.start[coff + c] * sc.mask[c];
                    x[3 + c] = iq.start[coff + plane + c] * sc.mask[c];
                    am[c] = iq.start[coff + 2 * plane + c] * sc.mask[c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) { x[c] = p.x[xoff + c] * sc.mask[c]; x[3 + c] = p.x[xoff + plane + c] * sc.mask[c]; }
            }
        }
        double tc = p.t0;
        // SCHED: steps until the next interval's force takes uh's place (the host hands every launch the interval and the phase
        // it starts in), and this node's record of the current interval
        int sched_left = SCHED ? p.sched_first : -1;
        const T* sched_u = p.u_held + uoff;
        for (int step = 0; step < p.n_steps; ++step) {
            bool moved = false;   // (IADJ_SEG_FIN: the slot of this step's a^0 holds the previous step's final iterate)
            if constexpr (SCHED) {
                if (sched_left == 0) {   // (wave-uniform)
                    sched_left = p.sched_hold;
                    sched_u += p.sched_stride;
                    if (MODE == IADJ_SEG_FIN) {
                        moved = true;
                        if (valid) {
                            T* const io = iq.iters_out + size_t(step) * size_t(iq.n_iter) * force_sz + uoff;
#pragma unroll
                            for (int c = 0; c < 3; ++c) io[c] = am[c];
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (valid) uh[c] = sched_u[c];
                        am[c] = T(0);   // the interval starts as a call does: a^0 = 0 (what is stored below)
                    }
                }
                --sched_left;
            }
            if (SEG) {   // the step's start state and clock
                if (valid) {
                    T* const so = aq.states + size_t(step) * state_sz + xoff;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { so[c] = x[c]; so[plane + c] = x[3 + c]; }
                }
                if (aq.clocks && blockIdx.x == 0 && threadIdx.x == 0) aq.clocks[step] = tc;
            } else if (step % aq.store_every == 0 && valid) {   // the checkpoint pass: segment starts
                T* const so = aq.states + size_t(step / aq.store_every) * 3 * force_sz + coff;
#pragma unroll
                for (int c = 0; c < 3; ++c) { so[c] = x[c]; so[plane + c] = x[3 + c]; so[2 * plane + c] = am[c]; }
                so[3] = T(0);
                so[plane + 3] = T(0);
                so[2 * plane + 3] = T(0);
                if (zero_node0)
#pragma unroll
                    for (int c = 0; c < 4; ++c) { so[c - 4] = T(0); so[plane + c - 4] = T(0); so[2 * plane + c - 4] = T(0); }
            }
            const double tm = __dadd_rn(tc, 0.5 * p.dt);
            const T av = tm < p.duration ? amp : T(0);
            T uadd[3], qp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uadd[c] = uh[c] + ((c == p.imp_dof) ? av : T(0));
                qp[c] = x[c] + hh * x[3 + c];
            }
#pragma unroll 1
            for (int it = 0; it < iq.n_iter; ++it) {
                if (SEG && valid && !(moved && it == 0)) {
                    T* const io = iq.iters_out + (size_t(step) * size_t(iq.n_iter) + size_t(it)) * force_sz + uoff;
#pragma unroll
                    for (int c = 0; c < 3; ++c) io[c] = am[c];
                }
                T qm[3], vm[3], ka[3], u2[3], an[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { qm[c] = qp[c] + alpha * am[c]; vm[c] = x[3 + c] + hh * am[c]; }
                imp_k0<T>(L, tp, k, am, ka);
#pragma unroll
                for (int c = 0; c < 3; ++c) u2[c] = uadd[c] + alpha * ka[c];
                adj_accel<T>(p, L, tp, k, ix, qm, vm, u2, an);
#pragma unroll
                for (int c = 0; c < 3; ++c) am[c] = an[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[c] = x[c] + h * x[3 + c] + alpha2 * am[c];
                x[3 + c] = x[3 + c] + h * am[c];
            }
            tc = __dadd_rn(tc, p.dt);
            if (p.rec_out && valid && (step + 1) % p.rec_every == 0 && (step + 1) / p.rec_every <= p.rec_n) {
                const size_t kr = size_t((step + 1) / p.rec_every - 1);
                if (p.rec_slot == REC_ALL_SLOTS) {
                    T* const ro = p.rec_out + kr * state_sz + xoff;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { ro[c] = x[c]; ro[plane + c] = x[3 + c]; }
                    ro[3] = T(0);
                    ro[plane + 3] = T(0);
                } else if (tp.j == p.rec_slot) {
                    T rv = T(0);
#pragma unroll
                    for (int c = 0; c < 6; ++c)
                        if (c == p.rec_comp) rv = x[c];
                    p.rec_out[size_t(tp.beam) * p.rec_n + kr] = rv;
                }
            }
        }
        if (MODE == IADJ_CKPT && aq.write_back && valid)
#pragma unroll
            for (int c = 0; c < 3; ++c) { p.x[xoff + c] = x[c]; p.x[xoff + plane + c] = x[3 + c]; }
        if (MODE == IADJ_SEG_FIN && valid) {
            T* const fo = iq.fin_out + uoff;
#pragma unroll
            for (int c = 0; c < 3; ++c) fo[c] = am[c];
            fo[3] = T(0);
        }
        return;
    }

    // ---- IADJ_BWD, IADJ_BWD_STORE
    T lam[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, fb[3] = {T(0), T(0), T(0)}, cb[3] = {T(0), T(0), T(0)};
    T ab = T(0);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lam[c] = aq.lam[loff + c] * sc.mask[c];
            lam[3 + c] = aq.lam[loff + plane + c] * sc.mask[c];
            if (aq.f_bar) fb[c] = aq.f_bar[fboff + c];
            if (iq.carry_in) cb[c] = iq.carry[luoff + c] * sc.mask[c];
        }
        if (aq.amp_bar && imp_here) ab = aq.amp_bar[d * size_t(p.B) + tp.beam];
    }
    // this lane's addresses of the sweep's buffers, formed once and held in vector registers (crb_adj_kernel)
    T* lam_p = aq.lam + loff;
    T* fb_p = (aq.f_bar && valid) ? aq.f_bar + fboff : nullptr;
    T* ab_p = (aq.amp_bar && imp_here) ? aq.amp_bar + d * size_t(p.B) + tp.beam : nullptr;
    T* cb_p = iq.carry + luoff;
    const T* it_p = iq.iters + uoff;
    const T* rec_p = nullptr;
    if (p.rec_out)
        rec_p = p.rec_slot == REC_ALL_SLOTS ? p.rec_out + d * size_t(p.rec_n) * state_sz + xoff
                                            : p.rec_out + (d * size_t(p.B) + tp.beam) * size_t(p.rec_n);
    asm volatile("" : "+v"(lam_p), "+v"(fb_p), "+v"(ab_p), "+v"(rec_p), "+v"(cb_p), "+v"(it_p));
    T* gb_p = nullptr;                                         // (IADJ_BWD_STORE: this lane's gbar record of iteration 0 of step 0)
    const size_t gb_stride = size_t(gridDim.y) * force_sz;     //  and the stride from one iteration to the next
    if (MODE == IADJ_BWD_STORE) {
        gb_p = iq.gbar + luoff;
        asm volatile("" : "+v"(gb_p));
    }
#pragma unroll 1
    for (int i = p.n_steps - 1; i >= 0; --i) {
        const int kstep = aq.step0 + i;
        int idof = p.imp_dof, rslot = p.rec_slot, rcomp = p.rec_comp, imp = imp_here ? 1 : 0;
        asm volatile("" : "+s"(idof), "+s"(rslot), "+s"(rcomp), "+v"(imp));
        // the cotangent of the sample taken at the end of this step
        if (p.rec_out && valid && (kstep + 1) % p.rec_every == 0 && (kstep + 1) / p.rec_every <= p.rec_n) {
            const size_t kr = size_t((kstep + 1) / p.rec_every - 1);
            if (rslot == REC_ALL_SLOTS) {
                const T* const rb = rec_p + kr * state_sz;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    lam[c] = lam[c] + rb[c] * sc.mask[c];
                    lam[3 + c] = lam[3 + c] + rb[plane + c] * sc.mask[c];
                }
            } else if (tp.j == rslot) {
                const T rv = rec_p[kr];
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    if (c == rcomp) lam[c] = lam[c] + rv * sc.mask[c % 3];
            }
        }
        const double tc = aq.work_clock[i];
        const bool on = __dadd_rn(tc, 0.5 * p.dt) < p.duration;
        T x0[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, qp[3];
        if (valid) {
            const T* const w = aq.work + size_t(i) * state_sz + xoff;
#pragma unroll
            for (int c = 0; c < 3; ++c) { x0[c] = w[c] * sc.mask[c]; x0[3 + c] = w[plane + c] * sc.mask[c]; }
        }
        T abar[3], qpb[3] = {T(0), T(0), T(0)}, vpb[3] = {T(0), T(0), T(0)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            qp[c] = x0[c] + hh * x0[3 + c];
            abar[c] = alpha2 * lam[c] + h * lam[3 + c] + cb[c];
        }
#pragma unroll 1
        for (int it = iq.n_iter - 1; it >= 0; --it) {
            JvpConst<T> kk = k;
            AdjIdx<T> ixx = ix;
            opaque_consts<T>(kk, ixx);
            T a[3] = {T(0), T(0), T(0)}, qm[3], vm[3];
            if (valid) {
                const T* const ai = it_p + (size_t(i) * size_t(iq.n_iter) + size_t(it)) * force_sz;
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = ai[c] * sc.mask[c];
            }
            if constexpr (SCHED && MODE == IADJ_BWD_STORE) {   // an interval's a^0 is 0, whatever its slot holds (iq.fin_out)
                int hold = p.sched_hold;
                asm volatile("" : "+s"(hold));
                if (it == 0 && kstep % hold == 0)
#pragma unroll
                    for (int c = 0; c < 3; ++c) a[c] = T(0);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { qm[c] = qp[c] + alpha * a[c]; vm[c] = x0[3 + c] + hh * a[c]; }
            const T zero3[3] = {T(0), T(0), T(0)};
            T qb[3], vb[3], gb[3], kt[3];
            adj_vjp<T>(p, L, tp, kk, ixx, qm, vm, zero3, abar, qb, vb, gb);
#pragma unroll
            for (int c = 0; c < 3; ++c) { qb[c] = qb[c] * sc.mask[c]; vb[c] = vb[c] * sc.mask[c]; gb[c] = gb[c] * sc.mask[c]; }
            if (MODE == IADJ_BWD_STORE && valid) {
                T* const go = gb_p + (size_t(i) * size_t(iq.n_iter) + size_t(it)) * gb_stride;
#pragma unroll
                for (int c = 0; c < 3; ++c) go[c] = gb[c];
                go[3] = T(0);
            }
            imp_k0t<T>(L, tp, kk, gb, kt);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                fb[c] = fb[c] + gb[c];
                qpb[c] = qpb[c] + qb[c];
                vpb[c] = vpb[c] + vb[c];
                abar[c] = (alpha * qb[c] + hh * vb[c] + alpha * kt[c]) * sc.mask[c];
            }
            if (imp && on) {
                T ui = T(0);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c == idof) ui = gb[c];
                ab = ab + ui;
            }
        }
        bool first = kstep == 0;   // (step 0 of the call starts from the constant a^0 = 0 ...
        if constexpr (SCHED) {     //  ... and so does the first step of every interval)
            int hold = p.sched_hold;
            asm volatile("" : "+s"(hold));
            first = kstep % hold == 0;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cb[c] = first ? T(0) : abar[c];
            const T lq = lam[c];
            lam[c] = lq + qpb[c];
            lam[3 + c] = (h * lq + lam[3 + c]) + (hh * qpb[c] + vpb[c]);
        }
        // SCHED: the step just swept was its interval's first, and the launch goes on below it -- this interval's sum is
        // complete: store it, move the lane address down one interval and take up the record there (accumulated: a later
        // segment may have left a partial sum), as crb_adj_kernel does
        if constexpr (SCHED) {
            if (i > 0 && first && fb_p) {
#pragma unroll
                for (int c = 0; c < 3; ++c) fb_p[c] = fb[c];
                fb_p -= p.sched_stride;
#pragma unroll
                for (int c = 0; c < 3; ++c) fb[c] = fb_p[c];
            }
        }
    }
    if (!valid) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) { lam_p[c] = lam[c]; lam_p[plane + c] = lam[3 + c]; cb_p[c] = cb[c]; }
    cb_p[3] = T(0);
    if (zero_node0)
#pragma unroll
        for (int c = 0; c < 4; ++c) { lam_p[c - 4] = T(0); lam_p[plane + c - 4] = T(0); }
    if (fb_p)
#pragma unroll
        for (int c = 0; c < 3; ++c) fb_p[c] = fb[c];
    if (ab_p) *ab_p = ab;
}

}  // namespace crb
