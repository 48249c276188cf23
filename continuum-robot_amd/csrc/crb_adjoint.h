// crb_adjoint.h -- reverse-mode derivatives (vector-Jacobian products) of the right-hand side and of the fused RK4 rollout
// (crb_rhs_vjp, crb_step_rk4_checkpoint, crb_step_rk4_adjoint).
//
// What is differentiated.  ADJ_RHS: f(x, u) = [v ; M^-1 r], r = u - k(q) + f_drag(v) + f_grav(q), the RHS of crb_rhs; for a
// cotangent lambda = [lq ; lv] per node:
//     rbar = M^-T lv          ubar = rbar          qbar = -(dk/dq)^T rbar + (dg/dq)^T rbar          vbar = lq + (dd/dv)^T rbar
// ADJ_BWD: the transpose of the discrete map of crb_step_rk4 -- classical RK4 steps, the same stage times, clock and impulse
// window -- swept backward over a segment of steps whose stage points a forward pass (ADJ_FWD) has recomputed.  Like the
// tangent kernels (crb_tangent.h) these are the derivatives of what the steppers COMPUTE, transposed exactly:
//   - M^-T is the transpose of the plan's TRUNCATED reduction (`levels`), not the forward solve again (the truncated operator
//     is not symmetric): y = F^T lv, then for l = levels-1 .. 0, stride s = 2^l,  y_j += A_{j+s}^T y_{j+s} + C_{j-s}^T y_{j-s}
//     with the neighbours' multipliers of that level (each thread forms A_j^T y_j and C_j^T y_j from its own row and hands
//     them to slots j - s and j + s through LDS, under the range conditions the forward level used);
//   - element forces: the 6 x 6 element Jacobian of elem_force, column by column on dual numbers (the passes of
//     elem_tangent), dotted with -(rbar_{j-1}, rbar_j); the node-j half stays, the node-(j-1) half goes left through LDS;
//   - drag: diagonal on the w DOF (drag_force on a dual velocity);
//   - gravity: the table's gathers become gathers over inverse index lists (GravAdj, built on the host from the plan's own
//     tables): segment s sums the rbar entries its force landed on, turns them into phibar through d g / d phi, and every
//     rotation DOF sums the phibar of the segments that averaged it -- wherever the table points (PINNED roots included);
//   - constrained DOFs: zero on load (lambda) and on store (xbar, ubar); node 0 of off == 1 plans is written zero.
// No floating-point atomics: every sum has a fixed order, so results are bitwise reproducible.
//
// The RK4 step in reverse.  x+ = x + dt/6 (k1 + 2 k2 + 2 k3 + k4); given lambda+:
//     s4 = J4^T(dt/6 l+),  s3 = J3^T(dt/3 l+ + dt s4),  s2 = J2^T(dt/3 l+ + dt/2 s3),  s1 = J1^T(dt/6 l+ + dt/2 s2)
//     lambda = l+ + s1 + s2 + s3 + s4
// J_s^T is the VJP at stage point s, as the recompute pass (ADJ_FWD, values only) wrote it.  The
// input cotangent of stage s is its ubar: it adds to f_held_bar, and to amp_bar on the impulse DOF while the stage time is
// < duration.  Cotangents of recorded samples are added to lambda when the sweep reaches the end of the step that took them.
//
// Checkpointing (crbeam.hip).  ADJ_FWD with store_every = `every` writes the state at every segment start (the checkpoint
// pass); per segment, last to first, ADJ_FWD with stage_pts rewrites the four stage points of every step of the segment and
// the steps' clocks into `work`, and ADJ_BWD sweeps the segment for all cotangents.  Both forward passes are the same kernel (the same
// arithmetic), and the sweep keeps lambda and the input cotangents in registers, loaded at the start of a segment and
// stored at its end, so the sums are the same additions in the same order for any `every`: the gradient does not depend on
// it, bitwise.
//
// Mapping.  That of crb_tangent.h: one thread per node slot (make_topo), short beams packed G to a wave, up to 4 waves (256
// thread-carried nodes) per beam; the cotangent index is the grid's second dimension, every instance reads the shared stage
// points and keeps its own cotangent, so D cotangents in one launch are bitwise D launches of one.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_tangent.h"

namespace crb {

constexpr int ADJ_MAX_NT = 256;
constexpr int GRAV_SEG_FANIN = 2;   // node DOFs one component of a segment's gravity lands on (fan-in of the reversed gathers)
constexpr int GRAV_PHI_FANIN = 2;   // segments whose rotation average reads one DOF
// ADJ_BWD_STORE: ADJ_BWD that also writes every stage's masked rbar for crb_param_grad_kernel (crb_paramgrad.h)
enum : int { ADJ_RHS = 0, ADJ_FWD = 1, ADJ_BWD = 2, ADJ_BWD_STORE = 3 };

// Inverse gravity lists of one slot (host-built: crb_plan_get_grav_transpose).  -1 = no entry; entries in ascending order.
struct GravAdj {
    int32_t seg[2][GRAV_SEG_FANIN];         // as segment s, per component (0 axial / 1 transverse) of its force: slot * 4 + dof
                                            //  of every node DOF that component adds to
    int32_t phi[3][GRAV_PHI_FANIN];         // per DOF of this slot: (segment << 1) | half of the segments whose rotation reads
                                            //  it (half: the segment averages two rotations)
};

// The launch's reverse-mode pointers, next to the KParams<T> of the base (x, u_held, amp, impulse and record fields).
template <typename T>
struct AdjParams {
    const GravAdj* gadj;        // [n_tab][S] inverse gravity lists
    const int32_t* gadj_beam;   // [B] list set of each beam, or nullptr (set 0 for every beam)
    // ADJ_RHS
    const T* lam_in;            // [n_cot][B][2][n_node][4] cotangent of xdot
    T* xbar;                    // [n_cot][B][2][n_node][4]
    T* ubar;                    // [n_cot][B][n_node][4] or nullptr
    // ADJ_FWD: the checkpoint pass writes the state at the start of step k to states[k / store_every] when
    // k % store_every == 0; the recompute (stage_pts) writes every step's four stage points to states[k][s] ([n_steps][4][B][2]
    // [n_node][4]) and its clock to clocks[k]; p.x advances in place when write_back
    T* states;
    double* clocks;
    int store_every;
    int stage_pts;
    int write_back;
    // ADJ_BWD
    const T* work;              // [n_steps][4][B][2][n_node][4] the stage points of every step of the segment
    const double* work_clock;   // [n_steps] the steps' clocks
    T* lam;                     // [n_cot][B][2][n_node][4] in place
    T* amp_bar;                 // [n_cot][B] or nullptr
    T* f_bar;                   // [n_cot][B][n_node][4] or nullptr
    int step0;                  // index of the segment's first step in the rollout (record cotangents)
    // ADJ_BWD_STORE writes, crb_param_grad_kernel reads (last, so that the fields above keep their kernel-argument offsets)
    T* rbar;                    // [n_steps][4][n_cot][B][n_node][4] the masked rbar = M^-T lambda_v of every stage of the segment
    T* param_bar;               // [n_cot][B][n_node][8] crb_param_grad_kernel's accumulators (crb_param_cotangent)
    // control schedule (KParams sched_stride / sched_hold): f_bar is [n_cot][n_intervals][B][n_node][4] and points at the
    // interval of the segment's LAST step; fbar_cot_stride = elements from one cotangent's records to the next (0 = B * n_node * 4)
    size_t fbar_cot_stride;
};

// LDS: q [3][NT], rbar [3][NT], element left halves / element forces [3][NT], segment gravity / phibar [2][NT], reduction
// exchange [6][NT] (the value solve double-buffers its 3 rows in it), then one cell that holds 0.
template <typename T>
struct AdjLds {
    T* q;
    T* rb;
    T* eh;
    T* g;
    T* r;
    T* base;   // the LDS base: the gravity gathers address it by offset (AdjIdx)
    int NT;
};
constexpr int ADJ_LDS_Q = 0, ADJ_LDS_RB = 3, ADJ_LDS_G = 9, ADJ_LDS_ZERO = 17;   // row offsets (times NT) of AdjLds
template <typename T>
__host__ __device__ constexpr size_t adjoint_lds_bytes(int NT) {
    return (size_t(17) * size_t(NT) + 1) * sizeof(T);
}
template <typename T>
__device__ __forceinline__ AdjLds<T> carve_adjoint_lds(int NT) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    T* b = reinterpret_cast<T*>(crb_smem);
    AdjLds<T> l;
    l.NT = NT;
    l.q = b;
    l.rb = b + 3 * NT;
    l.eh = b + 6 * NT;
    l.g = b + 9 * NT;
    l.r = b + 11 * NT;
    l.base = b;
    return l;
}

// The gravity gathers of a thread as LDS offsets, resolved once per launch: an absent entry reads the zero cell, so the
// gathers need no per-entry branch (whose lane masks the compiler would otherwise keep, loop-invariant, in scalar registers).
template <typename T>
struct AdjIdx {
    int fq[2];      // forward: the rotations segment j averages (q rows)
    int fg[3][2];   // forward: the segment gravity components DOF c sums (g rows, segA / segB)
    int sg[2][2];   // reverse: the rbar entries component 0 / 1 of segment j's gravity landed on (rb rows)
    int sp[3][2];   // reverse: the phibar of the segments that read DOF c (g row 0)
    T phim;         // 0.5 when segment j averages two rotations, else 1
    int half;       // bit 2 c + i: entry sp[c][i] has the weight 0.5 (else 1)
};
template <typename T>
__device__ __forceinline__ void adj_index(const KParams<T>& p, const AdjParams<T>& aq, const Topo& tp, const SlotConst<T>& sc,
                                          int NT, AdjIdx<T>& ix) {
    const int Z = ADJ_LDS_ZERO * NT;
    const bool on = tp.valid && (p.flags & 2u);
    GravAdj ga;
    if (on) ga = aq.gadj[(aq.gadj_beam ? size_t(aq.gadj_beam[tp.beam]) : size_t(0)) * size_t(p.S) + tp.j];
    const int ia = on ? sc.grav.phiA : -1, ib = on ? sc.grav.phiB : -1;
    ix.fq[0] = ia >= 0 ? ADJ_LDS_Q * NT + (ia & 3) * NT + tp.thread_of(ia >> 2) : Z;
    ix.fq[1] = ib >= 0 ? ADJ_LDS_Q * NT + (ib & 3) * NT + tp.thread_of(ib >> 2) : Z;
    ix.phim = ib >= 0 ? T(0.5) : T(1);
    ix.half = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int go = sc.grav.comp[c];
        const int sa = on ? sc.grav.segA[c] : -1, sb = on ? sc.grav.segB[c] : -1;
        ix.fg[c][0] = sa >= 0 ? (ADJ_LDS_G + go) * NT + tp.thread_of(sa) : Z;
        ix.fg[c][1] = sb >= 0 ? (ADJ_LDS_G + go) * NT + tp.thread_of(sb) : Z;
#pragma unroll
        for (int i = 0; i < GRAV_PHI_FANIN; ++i) {
            const int en = on ? ga.phi[c][i] : -1;
            ix.sp[c][i] = en >= 0 ? ADJ_LDS_G * NT + tp.thread_of(en >> 1) : Z;
            if (en >= 0 && (en & 1)) ix.half |= 1 << (2 * c + i);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < GRAV_SEG_FANIN; ++i) {
            const int en = on ? ga.seg[m][i] : -1;
            ix.sg[m][i] = en >= 0 ? (ADJ_LDS_RB + (en & 3)) * NT + tp.thread_of(en >> 2) : Z;
        }
}

// a = M^-1(u - k(q) + f_drag(v) + f_grav(q)) of this thread's node, values only (the forward arithmetic of the adjoint).
// Whole workgroup.
template <typename T>
__device__ __forceinline__ void adj_accel(const KParams<T>& p, const AdjLds<T>& L, const Topo& tp, const JvpConst<T>& k,
                                          const AdjIdx<T>& ix, const T q[3], const T v[3], const T u[3], T a[3]) {
    const int NT = L.NT;
    const SlotConst<T>& sc = k.sc;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) L.q[c * NT + tp.t] = q[c];
    __syncthreads();
    const bool has_l = tp.j >= 1, has_r = tp.j + 1 < tp.S;
    const int tl = has_l ? tp.thread_of(tp.j - 1) : tp.t;
    T ql[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ql[c] = has_l ? L.q[c * NT + tl] : T(0);
    T fl[3], fr[3];
    elem_force<T>(sc.elem, ql, q, k.corrected, fl, fr);
    T gseg[2] = {T(0), T(0)};
    if (k.grav_on) {
        const T phi = ix.phim * (L.base[ix.fq[0]] + L.base[ix.fq[1]]);
        gravity_segment<T>(phi, k.gx, k.gy, sc.half_mass, gseg);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) L.eh[c * NT + tp.t] = fl[c];
    if (k.grav_on) { L.g[tp.t] = gseg[0]; L.g[NT + tp.t] = gseg[1]; }
    __syncthreads();
    const int tr = has_r ? tp.thread_of(tp.j + 1) : tp.t;
    T r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = u[c] - (fr[c] + (has_r ? L.eh[c * NT + tr] : T(0)));
    if (k.drag_on) r[1] = r[1] + drag_force<T>(sc.drag, v[1]);
    if (k.grav_on) {
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = r[c] + L.base[ix.fg[c][0]] + L.base[ix.fg[c][1]];
    }
    for (int l = 0; l < p.levels; ++l) {
        T* const buf = (l & 1) ? L.r + 3 * NT : L.r;
#pragma unroll
        for (int c = 0; c < 3; ++c) buf[c * NT + tp.t] = r[c];
        __syncthreads();
        const int s = 1 << l;
        const bool lo = tp.j - s >= 0, hi = tp.j + s < tp.S;
        const int tlo = lo ? tp.thread_of(tp.j - s) : tp.t, thi = hi ? tp.thread_of(tp.j + s) : tp.t;
        T lov[3], hiv[3], cf[PCR_LEVEL_VALS];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lov[c] = lo ? buf[c * NT + tlo] : T(0);
            hiv[c] = hi ? buf[c * NT + thi] : T(0);
        }
        const T* src = k.lv + size_t(l) * size_t(p.S) * PCR_LEVEL_VALS;
#pragma unroll
        for (int i = 0; i < PCR_LEVEL_VALS; ++i) cf[i] = tp.valid ? src[i] : T(0);
        pcr_apply_level<T>(cf, lov, hiv, r);
    }
    pcr_apply_final<T>(k.fin, r, a);
}

// out[s] = sum_rows K[row][s] w[row] for the element Jacobian K = d[fl; fr] / d[ql; qr] and w = [wl; wr]: the six dual passes
// of elem_tangent, each column dotted with w as it comes out (the 6 x 6 matrix is never held).
template <typename T>
__device__ __forceinline__ void elem_vjp(const ElemCoef<T>& e, const T ql[3], const T qr[3], bool corrected, const T wl[3],
                                         const T wr[3], T out[6]) {
    typedef Dual<T> D;
    ElemCoef<D> ed;
    ed.kind = e.kind;
    ed.pad = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) ed.c[i] = D(e.c[i], T(0));
#pragma unroll 1
    for (int s = 0; s < 6; ++s) {
        D dl[3], dr[3], gl[3], gr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dl[c] = D(ql[c], s == c ? T(1) : T(0));
            dr[c] = D(qr[c], s == 3 + c ? T(1) : T(0));
        }
        elem_force<D>(ed, dl, dr, corrected, gl, gr);
        const T o = gl[0].d * wl[0] + gl[1].d * wl[1] + gl[2].d * wl[2] + gr[0].d * wr[0] + gr[1].d * wr[1] + gr[2].d * wr[2];
#pragma unroll
        for (int c = 0; c < 6; ++c)
            if (c == s) out[c] = o;
    }
}

// (qbar, vbar, ubar) = J^T (lq, lv) at the point (q, v) of this thread's node; lq / lv masked by the caller, the outputs are
// not masked.  Whole workgroup.
template <typename T>
__device__ __forceinline__ void adj_vjp(const KParams<T>& p, const AdjLds<T>& L, const Topo& tp, const JvpConst<T>& k,
                                        const AdjIdx<T>& ix, const T q[3], const T v[3], const T lq[3], const T lv[3], T qb[3],
                                        T vb[3], T ub[3]) {
    const int NT = L.NT;
    const SlotConst<T>& sc = k.sc;
    // -- 1. rbar = M^-T lv: the final block transposed, then the levels in reverse with the neighbours' multipliers
    T y[3];
    y[0] = k.fin[0] * lv[0];
    y[1] = k.fin[1] * lv[1] + k.fin[3] * lv[2];
    y[2] = k.fin[2] * lv[1] + k.fin[4] * lv[2];
    __syncthreads();
    for (int l = p.levels - 1; l >= 0; --l) {
        T* const buf = L.r;
        const T* src = k.lv + size_t(l) * size_t(p.S) * PCR_LEVEL_VALS;
        T cf[PCR_LEVEL_VALS];
#pragma unroll
        for (int i = 0; i < PCR_LEVEL_VALS; ++i) cf[i] = tp.valid ? src[i] : T(0);
        // A_j^T y_j (for slot j - s) and C_j^T y_j (for slot j + s): pcr_apply_level's A = [a0; a2 a3; a4 a5], C = [c1; c6 c7; c8 c9]
        buf[tp.t] = cf[0] * y[0];
        buf[NT + tp.t] = cf[2] * y[1] + cf[4] * y[2];
        buf[2 * NT + tp.t] = cf[3] * y[1] + cf[5] * y[2];
        buf[3 * NT + tp.t] = cf[1] * y[0];
        buf[4 * NT + tp.t] = cf[6] * y[1] + cf[8] * y[2];
        buf[5 * NT + tp.t] = cf[7] * y[1] + cf[9] * y[2];
        __syncthreads();
        const int s = 1 << l;
        const bool lo = tp.j - s >= 0, hi = tp.j + s < tp.S;
        const int tlo = lo ? tp.thread_of(tp.j - s) : tp.t, thi = hi ? tp.thread_of(tp.j + s) : tp.t;
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c] = y[c] + (hi ? buf[c * NT + thi] : T(0)) + (lo ? buf[(3 + c) * NT + tlo] : T(0));
        __syncthreads();
    }

    // -- 2. the element left of the node on -(rbar_{j-1}, rbar_j); gravity of segment j back to its rotation
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.q[c * NT + tp.t] = q[c]; L.rb[c * NT + tp.t] = y[c]; }
    __syncthreads();
    const bool has_l = tp.j >= 1, has_r = tp.j + 1 < tp.S;
    const int tl = has_l ? tp.thread_of(tp.j - 1) : tp.t, tr = has_r ? tp.thread_of(tp.j + 1) : tp.t;
    T ql[3], rl[3], e[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ql[c] = has_l ? L.q[c * NT + tl] : T(0);
        rl[c] = has_l ? L.rb[c * NT + tl] : T(0);
    }
    elem_vjp<T>(sc.elem, ql, q, k.corrected, rl, y, e);
#pragma unroll
    for (int c = 0; c < 3; ++c) L.eh[c * NT + tp.t] = e[c];
    if (k.grav_on) {
        T gb[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) gb[m] = L.base[ix.sg[m][0]] + L.base[ix.sg[m][1]];
        const T phi = ix.phim * (L.base[ix.fq[0]] + L.base[ix.fq[1]]);
        T gs[2], dg[2];
        gravity_segment<T>(phi, k.gx, k.gy, sc.half_mass, gs);
        gravity_segment_dphi<T>(gs, dg);
        L.g[tp.t] = gb[0] * dg[0] + gb[1] * dg[1];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) qb[c] = -e[3 + c] - (has_r ? L.eh[c * NT + tr] : T(0));
    if (k.grav_on) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < GRAV_PHI_FANIN; ++i) {
                const T w = T(1) - T(0.5) * T((ix.half >> (2 * c + i)) & 1);
                qb[c] = qb[c] + w * L.base[ix.sp[c][i]];
            }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { vb[c] = lq[c]; ub[c] = y[c]; }
    if (k.drag_on) {
        const Dual<T> dd = drag_force<Dual<T>>(Dual<T>(sc.drag, T(0)), Dual<T>(v[1], T(1)));
        vb[1] = vb[1] + dd.d * y[1];
    }
}

// One RK4 step of the values, x in place (the forward arithmetic of the adjoint: crb_jvp_kernel's step without the tangent).
template <typename T>
__device__ __forceinline__ void adj_rk4_step(const KParams<T>& p, const AdjLds<T>& L, const Topo& tp, const JvpConst<T>& k,
                                             const AdjIdx<T>& ix, const T uh[3], T amp, double tc, T x[6], T* stage_out,
                                             size_t stage_stride) {
    const T dt = T(p.dt), hdt = T(0.5 * p.dt), dt6 = T(p.dt / 6.0);
    const double t_half = __dadd_rn(tc, 0.5 * p.dt), t_full = __dadd_rn(tc, p.dt);
    T acc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    T xs[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) xs[c] = x[c];
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        const double ts = (s == 0) ? tc : ((s == 3) ? t_full : t_half);
        const T av = ts < p.duration ? amp : T(0);
        T uadd[3], a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) uadd[c] = uh[c] + ((c == p.imp_dof) ? av : T(0));
        if (stage_out) {   // (ADJ_FWD's recompute: the stage points the backward sweep linearises about)
            T* const so = stage_out + size_t(s) * stage_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) { so[c] = xs[c]; so[size_t(p.n_node) * 4 + c] = xs[3 + c]; }
        }
        adj_accel<T>(p, L, tp, k, ix, xs, xs + 3, uadd, a);
        const T w = (s == 0 || s == 3) ? T(1) : T(2);
        const T cs = (s == 2) ? dt : hdt;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T kq = xs[3 + c], kv = a[c];
            acc[c] += w * kq;
            acc[3 + c] += w * kv;
            xs[c] = x[c] + cs * kq;
            xs[3 + c] = x[3 + c] + cs * kv;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) x[c] += dt6 * acc[c];
}

// The per-launch constants of a thread, made opaque to the optimiser at the top of a loop body: otherwise everything the
// four VJPs of a step derive from them (dual seeds, lane masks, table offsets) is hoisted out of the sweep's loops and kept
// live across them, past the register file.
template <typename T>
__device__ __forceinline__ void opaque_consts(JvpConst<T>& k, AdjIdx<T>& ix) {
#pragma unroll
    for (int i = 0; i < 6; ++i) asm volatile("" : "+v"(k.sc.elem.c[i]));
#pragma unroll
    for (int i = 0; i < 5; ++i) asm volatile("" : "+v"(k.fin[i]));
    asm volatile("" : "+v"(k.sc.drag), "+v"(k.sc.half_mass), "+v"(ix.phim), "+v"(ix.half));
    asm volatile("" : "+v"(ix.fq[0]), "+v"(ix.fq[1]));
#pragma unroll
    for (int c = 0; c < 3; ++c) asm volatile("" : "+v"(ix.fg[c][0]), "+v"(ix.fg[c][1]), "+v"(ix.sp[c][0]), "+v"(ix.sp[c][1]));
    asm volatile("" : "+v"(ix.sg[0][0]), "+v"(ix.sg[0][1]), "+v"(ix.sg[1][0]), "+v"(ix.sg[1][1]));
}

// ADJ_RHS: xdot = f(x, u) (instance 0, when p.out is set), xbar[d] = J_x^T lam[d], ubar[d] = J_u^T lam[d].
// ADJ_FWD: p.n_steps RK4 steps from p.x with checkpoints / per-step start states (one instance per beam).
// ADJ_BWD: the sweep of one segment of p.n_steps steps back over aq.work, lam[d] and the input cotangents in place.  fp64 only.
// ADJ_BWD_STORE: the same sweep, the same arithmetic; each stage's masked ub also goes to aq.rbar (component 3 = 0).
template <typename T, int MODE>
__global__ void __launch_bounds__(ADJ_MAX_NT) crb_adj_kernel(const KParams<T> p, const AdjParams<T> aq) {
    static_assert(sizeof(T) == 8, "the adjoint kernels are fp64");
    const AdjLds<T> L = carve_adjoint_lds<T>(blockDim.x);
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    const size_t d = blockIdx.y;

    JvpConst<T> k;
    jvp_load_const<T>(p, tp, k);
    const SlotConst<T>& sc = k.sc;
    AdjIdx<T> ix;
    adj_index<T>(p, aq, tp, sc, L.NT, ix);
    if (threadIdx.x == 0) L.base[ADJ_LDS_ZERO * L.NT] = T(0);   // (read after the barrier every gather follows)

    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t xoff = size_t(tp.beam) * 2 * plane + node * 4;
    const size_t state_sz = size_t(p.B) * 2 * plane;
    const size_t loff = d * state_sz + xoff;
    const size_t uoff = size_t(tp.beam) * plane + node * 4;
    const size_t luoff = d * size_t(p.B) * plane + uoff;                                                 // ubar, rbar
    const size_t fboff = d * (aq.fbar_cot_stride ? aq.fbar_cot_stride : size_t(p.B) * plane) + uoff;    // f_bar
    const bool zero_node0 = p.off == 1 && tp.j == 0;   // node 0 (FIXED in every beam, no slot) is written zero
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

    if (MODE == ADJ_RHS) {
        T x[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, lam[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
        if (valid)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[c] = p.x[xoff + c] * sc.mask[c];
                x[3 + c] = p.x[xoff + plane + c] * sc.mask[c];
                lam[c] = aq.lam_in[loff + c] * sc.mask[c];
                lam[3 + c] = aq.lam_in[loff + plane + c] * sc.mask[c];
            }
        if (d == 0 && p.out) {   // (workgroup-uniform: every instance of the grid row takes the same branch)
            T a[3];
            adj_accel<T>(p, L, tp, k, ix, x, x + 3, uh, a);
            if (valid) {
                T* const xo = p.out + xoff;
#pragma unroll
                for (int c = 0; c < 3; ++c) { xo[c] = x[3 + c]; xo[plane + c] = a[c]; }
                xo[3] = T(0);
                xo[plane + 3] = T(0);
                if (zero_node0)
#pragma unroll
                    for (int c = 0; c < 4; ++c) { xo[c - 4] = T(0); xo[plane + c - 4] = T(0); }
            }
        }
        T qb[3], vb[3], ub[3];
        adj_vjp<T>(p, L, tp, k, ix, x, x + 3, lam, lam + 3, qb, vb, ub);
        if (!valid) return;
        T* const o = aq.xbar + loff;
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[c] = qb[c] * sc.mask[c]; o[plane + c] = vb[c] * sc.mask[c]; }
        o[3] = T(0);
        o[plane + 3] = T(0);
        if (zero_node0)
#pragma unroll
            for (int c = 0; c < 4; ++c) { o[c - 4] = T(0); o[plane + c - 4] = T(0); }
        if (aq.ubar) {
            T* const uo = aq.ubar + luoff;
#pragma unroll
            for (int c = 0; c < 3; ++c) uo[c] = ub[c] * sc.mask[c];
            uo[3] = T(0);
            if (zero_node0)
#pragma unroll
                for (int c = 0; c < 4; ++c) uo[c - 4] = T(0);
        }
        return;
    }

    if (MODE == ADJ_FWD) {
        T x[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
        if (valid)
#pragma unroll
            for (int c = 0; c < 3; ++c) { x[c] = p.x[xoff + c] * sc.mask[c]; x[3 + c] = p.x[xoff + plane + c] * sc.mask[c]; }
        double tc = p.t0;
        // control schedule: steps until the next interval's force takes uh's place (the host hands every launch the interval
        // and the phase it starts in); never 0 without a schedule.  One scalar and the lane's address stay live across a step.
        int sched_left = p.sched_stride ? p.sched_first : -1;
        const T* sched_u = p.u_held + uoff;
        asm volatile("" : "+v"(sched_u));
        for (int step = 0; step < p.n_steps; ++step) {
            if (sched_left == 0) {   // (wave-uniform)
                sched_left = p.sched_hold;
                sched_u += p.sched_stride;
                if (valid)
#pragma unroll
                    for (int c = 0; c < 3; ++c) uh[c] = sched_u[c];
            }
            --sched_left;
            T* stage_out = nullptr;
            if (aq.stage_pts) {   // the recompute: every step's four stage points, states[step][s]
                if (valid) stage_out = aq.states + size_t(step) * 4 * state_sz + xoff;
                if (aq.clocks && blockIdx.x == 0 && threadIdx.x == 0) aq.clocks[step] = tc;
            } else if (step % aq.store_every == 0) {   // the checkpoint pass: segment starts
                const size_t k_st = size_t(step / aq.store_every);
                if (valid) {
                    T* const so = aq.states + k_st * state_sz + xoff;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { so[c] = x[c]; so[plane + c] = x[3 + c]; }
                    so[3] = T(0);
                    so[plane + 3] = T(0);
                }
                if (aq.clocks && blockIdx.x == 0 && threadIdx.x == 0) aq.clocks[k_st] = tc;
            }
            adj_rk4_step<T>(p, L, tp, k, ix, uh, amp, tc, x, stage_out, state_sz);
            tc = __dadd_rn(tc, p.dt);
            if (p.rec_out && valid && (step + 1) % p.rec_every == 0 && (step + 1) / p.rec_every <= p.rec_n) {
                const size_t kr = size_t((step + 1) / p.rec_every - 1);
                if (p.rec_slot == REC_ALL_SLOTS) {
                    T* const ro = p.rec_out + kr * state_sz + xoff;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { ro[c] = x[c]; ro[plane + c] = x[3 + c]; }
                } else if (tp.j == p.rec_slot) {
                    T rv = T(0);
#pragma unroll
                    for (int c = 0; c < 6; ++c)
                        if (c == p.rec_comp) rv = x[c];
                    p.rec_out[size_t(tp.beam) * p.rec_n + kr] = rv;
                }
            }
        }
        if (aq.write_back && valid)
#pragma unroll
            for (int c = 0; c < 3; ++c) { p.x[xoff + c] = x[c]; p.x[xoff + plane + c] = x[3 + c]; }
        return;
    }

    // ---- ADJ_BWD
    T lam[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, fb[3] = {T(0), T(0), T(0)};
    T ab = T(0);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lam[c] = aq.lam[loff + c] * sc.mask[c];
            lam[3 + c] = aq.lam[loff + plane + c] * sc.mask[c];
            if (aq.f_bar) fb[c] = aq.f_bar[fboff + c];
        }
        if (aq.amp_bar && imp_here) ab = aq.amp_bar[d * size_t(p.B) + tp.beam];
    }
    // this lane's addresses of the sweep's uniform-base buffers, formed once and held in vector registers (as scalars they
    // stay live across the sweep next to its loop constants, past the scalar register file)
    T* lam_p = aq.lam + loff;
    T* fb_p = (aq.f_bar && valid) ? aq.f_bar + fboff : nullptr;
    T* ab_p = (aq.amp_bar && imp_here) ? aq.amp_bar + d * size_t(p.B) + tp.beam : nullptr;
    const T* rec_p = nullptr;
    if (p.rec_out)
        rec_p = p.rec_slot == REC_ALL_SLOTS ? p.rec_out + d * size_t(p.rec_n) * state_sz + xoff
                                            : p.rec_out + (d * size_t(p.B) + tp.beam) * size_t(p.rec_n);
    asm volatile("" : "+v"(lam_p), "+v"(fb_p), "+v"(ab_p), "+v"(rec_p));
    T* rb_p = nullptr;                                                    // (ADJ_BWD_STORE: this lane's rbar record of stage 0)
    const size_t rb_stride = size_t(gridDim.y) * size_t(p.B) * plane;     //  and the stride from one stage to the next
    if (MODE == ADJ_BWD_STORE) {
        rb_p = aq.rbar + luoff;
        asm volatile("" : "+v"(rb_p));
    }
    const T dt = T(p.dt), hdt = T(0.5 * p.dt), dt3 = T(p.dt / 3.0), dt6 = T(p.dt / 6.0);
#pragma unroll 1
    for (int i = p.n_steps - 1; i >= 0; --i) {
        const int kstep = aq.step0 + i;
        // (the launch's selectors, opaque per step: their compare masks are formed where they are used, not kept live)
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
        const double t_half = __dadd_rn(tc, 0.5 * p.dt), t_full = __dadd_rn(tc, p.dt);
        // the stages in reverse: kbar_s, s_s = J_s^T kbar_s; lambda = l+ + s1 + s2 + s3 + s4
        T sum[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, sb[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, kb[6], ub[3];
#pragma unroll 1
        for (int s = 3; s >= 0; --s) {
            const T wl = (s == 0 || s == 3) ? dt6 : dt3;
            const T ws = (s == 2) ? dt : hdt;
#pragma unroll
            for (int c = 0; c < 6; ++c) kb[c] = (s == 3) ? wl * lam[c] : wl * lam[c] + ws * sb[c];
            JvpConst<T> kk = k;
            AdjIdx<T> ixx = ix;
            opaque_consts<T>(kk, ixx);
            T xs[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
            if (valid) {
                const T* const w = aq.work + (size_t(i) * 4 + size_t(s)) * state_sz + xoff;
#pragma unroll
                for (int c = 0; c < 3; ++c) { xs[c] = w[c] * sc.mask[c]; xs[3 + c] = w[plane + c] * sc.mask[c]; }
            }
            adj_vjp<T>(p, L, tp, kk, ixx, xs, xs + 3, kb, kb + 3, sb, sb + 3, ub);
#pragma unroll
            for (int c = 0; c < 3; ++c) { sb[c] = sb[c] * sc.mask[c]; sb[3 + c] = sb[3 + c] * sc.mask[c]; }
#pragma unroll
            for (int c = 0; c < 6; ++c) sum[c] = (s == 3) ? sb[c] : sum[c] + sb[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) fb[c] = fb[c] + ub[c] * sc.mask[c];
            if (MODE == ADJ_BWD_STORE && valid) {
                T* const ro = rb_p + (size_t(i) * 4 + size_t(s)) * rb_stride;
#pragma unroll
                for (int c = 0; c < 3; ++c) ro[c] = ub[c] * sc.mask[c];
                ro[3] = T(0);
            }
            const double ts = (s == 0) ? tc : ((s == 3) ? t_full : t_half);
            if (imp && ts < p.duration) {
                T ui = T(0);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c == idof) ui = ub[c] * sc.mask[c];
                ab = ab + ui;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) lam[c] = lam[c] + sum[c];
        // control schedule: the step just swept was its interval's first, and the launch goes on below it -- this interval's
        // sum is complete: store it, move the lane address down one interval and take up the record there (accumulated: a
        // later segment may have left a partial sum)
        int hold = p.sched_hold;
        asm volatile("" : "+s"(hold));
        if (p.sched_stride && i > 0 && kstep % hold == 0 && fb_p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) fb_p[c] = fb[c];
            fb_p -= p.sched_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) fb[c] = fb_p[c];
        }
    }
    if (!valid) return;
    T* const lo = lam_p;
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = lam[c]; lo[plane + c] = lam[3 + c]; }
    if (zero_node0)
#pragma unroll
        for (int c = 0; c < 4; ++c) { lo[c - 4] = T(0); lo[plane + c - 4] = T(0); }
    if (fb_p)
#pragma unroll
        for (int c = 0; c < 3; ++c) fb_p[c] = fb[c];
    if (ab_p) *ab_p = ab;
}

}  // namespace crb
