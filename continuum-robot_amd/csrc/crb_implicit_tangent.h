// crb_implicit_tangent.h -- forward-mode derivative of the implicit fixed-step stepper (crb_step_implicit_tangent): the exact
// tangent of the map crb_step_implicit COMPUTES (crb_stiff.h: the implicit midpoint rule with a fixed number of
// modified-Newton iterations on A = M + alpha K0), in crb_implicit_adjoint.h's statement of it -- not of the converged rule.
//
// Per step, from (q0, v0), the starting iterate a^0 and their tangents (dq0, dv0, da^0), alpha = h^2 / 4, hh = h / 2,
// u = f_held (+ amp on the impulse DOF while t + h/2 < duration), du = df_held (+ d_amp there):
//     qp = q0 + hh v0,                       dqp = dq0 + hh dv0
//     for i = 0 .. n_iter-1:
//         q_m = qp + alpha a^i,   v_m = v0 + hh a^i,     dq_m = dqp + alpha da^i,   dv_m = dv0 + hh da^i
//         (a^{i+1}, da^{i+1}) = jvp_accel(q_m, dq_m, v_m, dv_m, u + alpha K0 a^i, du + alpha K0 da^i)
//     q1 = q0 + h v0 + 2 alpha a,   v1 = v0 + h a      (the same two lines on the tangents)
// jvp_accel (crb_tangent.h) evaluates Ainv(F(q, v) + u') and its tangent on dual numbers: the launch's KParams carry A's
// tables, strides and level count where the RK4 tangent carries M's (as the implicit adjoint's do), read from global memory
// at each level, so one instance serves every level count.  a^0 and da^0 are the previous step's final iterate and its
// tangent, 0 at the first step of a call; with a schedule (SCHED) both are 0 again at the first step of every interval, where
// uh and duh are reloaded: a scheduled call is the chain of one call per interval, as in crb_imp_adj_kernel.
//
// K0 a and K0 da (imp_k0_pair) are imp_k0's arithmetic (crb_implicit_adjoint.h) on the value and the tangent in ONE
// exchange through the reduction rows r0 / r1 of TangentLds.
//
// Mapping, LDS, direction in blockIdx.y, constants and constrained DOFs: those of crb_jvp_kernel<MODE_STEP>.  Instance d = 0
// writes the base back; with n_dir > 1 every instance reads the base from a copy made before the launch.  fp64, beams of up
// to 256 thread-carried nodes.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_tangent.h"

namespace crb {

// ka = K0 a and kda = K0 da of this thread's node: the element left of the node on (a_{j-1}, a_j) by elem_force_linear (its
// right-node half stays, its left-node half goes left through LDS), value in rows 0..2 and tangent in rows 3..5 of r0 (the
// iterates) and r1 (the left-node halves).  Whole workgroup.
template <typename T>
__device__ __forceinline__ void imp_k0_pair(const TangentLds<T>& L, const Topo& tp, const JvpConst<T>& k, const T a[3], const T da[3],
                                            T ka[3], T kda[3]) {
    const int NT = L.NT;
    const bool has_l = tp.j >= 1, has_r = tp.j + 1 < tp.S;
    const int tl = has_l ? tp.thread_of(tp.j - 1) : tp.t, tr = has_r ? tp.thread_of(tp.j + 1) : tp.t;
    __syncthreads();   // (the last level of the previous solve may still be reading r0 / r1)
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.r0[c * NT + tp.t] = a[c]; L.r0[(3 + c) * NT + tp.t] = da[c]; }
    __syncthreads();
    T zl[3], dzl[3], lin[5] = {T(0), T(0), T(0), T(0), T(0)}, kl[3], kr[3], dkl[3], dkr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        zl[c] = has_l ? L.r0[c * NT + tl] : T(0);
        dzl[c] = has_l ? L.r0[(3 + c) * NT + tl] : T(0);
    }
    elem_linear_coefs<T>(k.sc.elem.c, k.sc.elem.kind, lin);
    elem_force_linear<T>(lin, zl, a, kl, kr);
    elem_force_linear<T>(lin, dzl, da, dkl, dkr);
    if (k.sc.elem.kind == KIND_NONLINEAR && !k.corrected) {   // tangent of the shipped f1: no u2 term
        kl[0] = lin[0] * zl[0];
        dkl[0] = lin[0] * dzl[0];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.r1[c * NT + tp.t] = kl[c]; L.r1[(3 + c) * NT + tp.t] = dkl[c]; }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ka[c] = kr[c] + (has_r ? L.r1[c * NT + tr] : T(0));
        kda[c] = dkr[c] + (has_r ? L.r1[(3 + c) * NT + tr] : T(0));
    }
}

// n_steps implicit steps of the base (written back by d == 0) and of its tangent d (in place).  p: A's tables in pcr_levels /
// pcr_final, p.dt = h.  SCHED: a control schedule (KParams sched_*, TangentParams du_dir_stride), a compile-time axis.
template <typename T, bool SCHED>
__global__ void __launch_bounds__(TANGENT_MAX_NT) crb_imp_jvp_kernel(const KParams<T> p, const TangentParams<T> tq, const int n_iter) {
    static_assert(sizeof(T) == 8, "the tangent kernels are fp64");
    const TangentLds<T> L = carve_tangent_lds<T>(blockDim.x);
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    const size_t d = blockIdx.y;

    JvpConst<T> k;
    jvp_load_const<T>(p, tp, k);   // (p.pcr_levels / p.pcr_final: the tables of A)
    const SlotConst<T>& sc = k.sc;

    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t xoff = size_t(tp.beam) * 2 * plane + node * 4;            // the base's record
    const size_t dxoff = d * size_t(p.B) * 2 * plane + xoff;              // this direction's record
    const size_t uoff = size_t(tp.beam) * plane + node * 4;
    const size_t duoff = d * (tq.du_dir_stride ? tq.du_dir_stride : size_t(p.B) * plane) + uoff;
    T x[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, dx[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    T uh[3] = {T(0), T(0), T(0)}, duh[3] = {T(0), T(0), T(0)};
    T amp = T(0), damp = T(0);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = tq.x0[xoff + c] * sc.mask[c];
            x[3 + c] = tq.x0[xoff + plane + c] * sc.mask[c];
            dx[c] = tq.dx[dxoff + c] * sc.mask[c];
            dx[3 + c] = tq.dx[dxoff + plane + c] * sc.mask[c];
            if (p.u_held) uh[c] = p.u_held[uoff + c];
            if (tq.du_held) duh[c] = tq.du_held[duoff + c] * sc.mask[c];
        }
        if (p.amp && tp.j == (p.imp_node_b ? p.imp_node_b[tp.beam] - p.off : p.imp_slot)) {
            amp = p.amp[tp.beam];
            if (tq.d_amp) damp = tq.d_amp[d * size_t(p.B) + tp.beam];
        }
    }
    const T h = T(p.dt), hh = T(0.5 * p.dt), alpha = T(0.25 * p.dt * p.dt), alpha2 = T(0.5 * p.dt * p.dt);

    T am[3] = {T(0), T(0), T(0)}, dam[3] = {T(0), T(0), T(0)};
    double tc = p.t0;
    // SCHED: steps until the next interval's force (and its tangent) take over
    int sched_left = SCHED ? p.sched_first : -1;
    size_t sched_off = 0;
    for (int step = 0; step < p.n_steps; ++step) {
        if constexpr (SCHED) {
            if (sched_left == 0) {   // (wave-uniform)
                sched_left = p.sched_hold;
                sched_off += p.sched_stride;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (valid) {
                        uh[c] = p.u_held[sched_off + uoff + c];
                        if (tq.du_held) duh[c] = tq.du_held[sched_off + duoff + c] * sc.mask[c];
                    }
                    am[c] = T(0);   // the interval starts as a call does: a^0 = 0, da^0 = 0
                    dam[c] = T(0);
                }
            }
            --sched_left;
        }
        const double tm = __dadd_rn(tc, 0.5 * p.dt);
        const bool on = tm < p.duration;
        const T av = on ? amp : T(0), dav = on ? damp : T(0);
        T uadd[3], duadd[3], qp[3], dqp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uadd[c] = uh[c] + ((c == p.imp_dof) ? av : T(0));
            duadd[c] = duh[c] + ((c == p.imp_dof) ? dav : T(0));
            qp[c] = x[c] + hh * x[3 + c];
            dqp[c] = dx[c] + hh * dx[3 + c];
        }
#pragma unroll 1
        for (int it = 0; it < n_iter; ++it) {
            T qm[3], vm[3], dqm[3], dvm[3], ka[3], dka[3], u2[3], du2[3], an[3], dan[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                qm[c] = qp[c] + alpha * am[c];
                vm[c] = x[3 + c] + hh * am[c];
                dqm[c] = dqp[c] + alpha * dam[c];
                dvm[c] = dx[3 + c] + hh * dam[c];
            }
            imp_k0_pair<T>(L, tp, k, am, dam, ka, dka);
#pragma unroll
            for (int c = 0; c < 3; ++c) { u2[c] = uadd[c] + alpha * ka[c]; du2[c] = duadd[c] + alpha * dka[c]; }
            jvp_accel<T>(p, L, tp, k, qm, dqm, vm, dvm, u2, du2, an, dan);
#pragma unroll
            for (int c = 0; c < 3; ++c) { am[c] = an[c]; dam[c] = dan[c]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = x[c] + h * x[3 + c] + alpha2 * am[c];
            x[3 + c] = x[3 + c] + h * am[c];
            dx[c] = dx[c] + h * dx[3 + c] + alpha2 * dam[c];
            dx[3 + c] = dx[3 + c] + h * dam[c];
        }
        tc = __dadd_rn(tc, p.dt);
    }
    if (!valid) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) { tq.dx[dxoff + c] = dx[c]; tq.dx[dxoff + plane + c] = dx[3 + c]; }
    if (d == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { p.x[xoff + c] = x[c]; p.x[xoff + plane + c] = x[3 + c]; }
        mark_nonfinite<T>(p, tp.beam, x, x + 3);
    }
}

}  // namespace crb
