// crb_tangent.h -- forward-mode derivatives (Jacobian-vector products) of the right-hand side and of the fused RK4
// rollout (crb_rhs_jvp, crb_step_rk4_tangent).
//
// What is differentiated.  MODE_RHS: f(x, u) = [v ; M^-1(-k(q) + f_drag(v) + f_grav(q) + u)], the RHS of crb_rhs, along
// (dx, du).  MODE_STEP: the discrete map of crb_step_rk4 -- n_steps classical RK4 steps, the same stage times and clock
// (t <- t + dt), the same impulse window -- along (dx(0), d amp, d f_held).  Both are the derivative of what the steppers
// COMPUTE: the mass solve applies the plan's truncated reduction (`levels`, not `levels_full`) with the same multipliers to
// the value and to the tangent, so the tangent of a rollout is the exact derivative of the rollout's own arithmetic.
//
// How.  Dual numbers (crb_math.h: Dual): every node carries q + eps dq and v + eps dv.
//   - element forces: ONE elem_force<Dual<T>> pass on the seeded positions of the node and its left neighbour (their
//     tangents exchanged through LDS with the values: 6 values per node);
//   - drag -c v|v| on the dual v (crb_abs on Dual);
//   - gravity on the dual phi read through the plan's gravity index table (crb_sincos on Dual).  Every entry of the table
//     is followed, wherever it points: with a PINNED root the reduced-index quirk makes the phi row of node i depend on the
//     rotation of slot i + 2 -- outside the +-1 band that crb_static.h's iteration matrix keeps, but part of this tangent;
//   - the held-force tangent d f_held and the impulse tangent d amp (on the impulse's DOF, inside its time window);
//   - constrained DOFs: zero in both parts (masked on load; their rows are zero in every multiplier of the solve).
//
// Mapping.  One thread per node slot (make_topo: beams of fewer than 64 slots packed G to a wave, longer ones one beam per
// workgroup of up to 4 waves, 256 thread-carried nodes).  The direction index is the grid's second dimension: instance
// (d, b) carries beam b's base state AND its tangent d -- every instance recomputes the base trajectory with identical
// arithmetic, and only d == 0 writes it back (MODE_STEP reads the base from a copy made before the launch when n_dir > 1,
// so that instance 0's store cannot reach another instance's load).  One direction per instance keeps the registers at
// about twice the plain stepper's; D directions in one launch are bitwise the same as D launches of one.
// Every neighbour exchange goes through LDS (the mapping of crb_static.h: packed or multi-wave alike); the multipliers of
// the reduction are read from the plan's tables at each use (they are shared by the value and the tangent).
//
// Registers.  The translation unit is compiled with -mllvm -disable-machine-licm (Makefile): otherwise the ~30 fp64
// literals of the dual element polynomial and of sincos are hoisted out of the RK4 loop into scalar register pairs, which
// then overflow the scalar file (23 - 34 SGPRs spilled to VGPR lanes, 255 VGPRs).  Without the hoisting MODE_STEP takes
// 240 VGPRs and MODE_RHS 136, no spills, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_static.h"

namespace crb {

constexpr int TANGENT_MAX_NT = 256;

// Tangent pointers of a launch, next to the KParams<T> of the base (whose argument layout stays as it is).  Directions are
// the leading index: [n_dir][B][...] in the layouts of the base.
template <typename T>
struct TangentParams {
    const T* x0;        // MODE_STEP: the base state at the start of the launch, read by every instance ([B][2][n_node][4])
    T* dx;              // [n_dir][B][2][n_node][4]: MODE_STEP the tangent, propagated in place; MODE_RHS read only
    T* dxdot;           // MODE_RHS: [n_dir][B][2][n_node][4] tangent of the RHS
    const T* du_held;   // [n_dir][B][n_node][4] tangent of the held force, or nullptr (= 0)
    const T* d_amp;     // [n_dir][B] tangent of the impulse amplitude, or nullptr (= 0)
    size_t du_dir_stride;   // elements from one direction of du_held to the next; 0 = B * n_node * 4.  With a control schedule
                            //  (KParams sched_*) du_held is [n_dir][n_intervals][B][n_node][4] and switches with u_held
};

// LDS: q + eps dq [6][NT], element halves [6][NT], segment gravity [4][NT], reduction exchange r0 / r1 [6][NT] each.
// Rows: value components first, then tangent components.
template <typename T>
struct TangentLds {
    T* q;
    T* f;
    T* g;
    T* r0;
    T* r1;
    int NT;
};
template <typename T>
__host__ __device__ constexpr size_t tangent_lds_bytes(int NT) {
    return size_t(28) * size_t(NT) * sizeof(T);
}
template <typename T>
__device__ __forceinline__ TangentLds<T> carve_tangent_lds(int NT) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    T* b = reinterpret_cast<T*>(crb_smem);
    TangentLds<T> l;
    l.NT = NT;
    l.q = b;
    l.f = b + 6 * NT;
    l.g = b + 12 * NT;
    l.r0 = b + 16 * NT;
    l.r1 = b + 22 * NT;
    return l;
}

// Per-thread constants of a launch, resolved once: the slot's constants, the beam's gravity vector, the final block of the
// reduction and where the slot's level multipliers start.
template <typename T>
struct JvpConst {
    SlotConst<T> sc;
    T gx, gy;
    T fin[5];
    const T* lv;
    bool drag_on, grav_on, corrected;
};
template <typename T>
__device__ __forceinline__ void jvp_load_const(const KParams<T>& p, const Topo& tp, JvpConst<T>& k) {
    SlotConst<T>& sc = k.sc;
    k.drag_on = (p.flags & 1u) != 0;
    k.grav_on = (p.flags & 2u) != 0;
    k.corrected = (p.flags & 4u) != 0;
    k.gx = p.gx;
    k.gy = p.gy;
    if (p.gvec) { k.gx = p.gvec[2 * size_t(tp.beam)]; k.gy = p.gvec[2 * size_t(tp.beam) + 1]; }   // (per-beam ForceParams)
    k.lv = p.pcr_levels + size_t(tp.beam) * p.lv_stride + size_t(tp.j) * PCR_LEVEL_VALS;
    if (tp.valid) {
        sc = p.slot[size_t(tp.beam) * p.slot_stride + tp.j];
        const T* f = p.pcr_final + size_t(tp.beam) * p.fin_stride + size_t(tp.j) * PCR_FINAL_VALS;
#pragma unroll
        for (int i = 0; i < 5; ++i) k.fin[i] = f[i];
    } else {   // padding thread: an isolated dummy node, all coefficients 0
        sc = padding_slot<T>();
#pragma unroll
        for (int i = 0; i < 5; ++i) k.fin[i] = T(0);
    }
}

// a and da: the acceleration M^-1(-k(q) + f_drag(v) + f_grav(q) + u) of this thread's node and its tangent along
// (dq, dv, du).  Whole workgroup: every thread calls it the same number of times (the barriers inside are workgroup-wide).
template <typename T>
__device__ __forceinline__ void jvp_accel(const KParams<T>& p, const TangentLds<T>& L, const Topo& tp, const JvpConst<T>& k,
                                          const T q[3], const T dq[3], const T v[3], const T dv[3], const T u[3], const T du[3],
                                          T a[3], T da[3]) {
    typedef Dual<T> D;
    const int NT = L.NT;
    const bool drag_on = k.drag_on, grav_on = k.grav_on, corrected = k.corrected;
    const SlotConst<T>& sc = k.sc;

    // -- 1. q + eps dq of every node; the left node's into the element
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.q[c * NT + tp.t] = q[c]; L.q[(3 + c) * NT + tp.t] = dq[c]; }
    __syncthreads();
    const bool has_l = tp.j >= 1, has_r = tp.j + 1 < tp.S;
    const int tl = has_l ? tp.thread_of(tp.j - 1) : tp.t;
    D ql[3], qd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ql[c] = has_l ? D(L.q[c * NT + tl], L.q[(3 + c) * NT + tl]) : D();
        qd[c] = D(q[c], dq[c]);
    }
    ElemCoef<D> ed;
    ed.kind = sc.elem.kind;
    ed.pad = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) ed.c[i] = D(sc.elem.c[i], T(0));
    D fl[3], fr[3];
    elem_force<D>(ed, ql, qd, corrected, fl, fr);

    // segment gravity on the dual rotation(s) the table names (any slot of the beam: no band)
    D gseg[2];
    if (grav_on && sc.half_mass != T(0)) {
        const int ia = sc.grav.phiA, ib = sc.grav.phiB;
        D phi;
        if (ia >= 0) {
            const int ta = tp.thread_of(ia >> 2), ca = ia & 3;
            phi = D(L.q[ca * NT + ta], L.q[(3 + ca) * NT + ta]);
        }
        if (ib >= 0) {
            const int tb = tp.thread_of(ib >> 2), cb = ib & 3;
            phi = D(T(0.5), T(0)) * (phi + D(L.q[cb * NT + tb], L.q[(3 + cb) * NT + tb]));
        }
        gravity_segment<D>(phi, D(k.gx, T(0)), D(k.gy, T(0)), D(sc.half_mass, T(0)), gseg);
    }

    // -- 2. the right neighbour's left-node half and the segment gravity
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.f[c * NT + tp.t] = fl[c].v; L.f[(3 + c) * NT + tp.t] = fl[c].d; }
    if (grav_on) {
        L.g[tp.t] = gseg[0].v;
        L.g[NT + tp.t] = gseg[1].v;
        L.g[2 * NT + tp.t] = gseg[0].d;
        L.g[3 * NT + tp.t] = gseg[1].d;
    }
    __syncthreads();
    const int tr = has_r ? tp.thread_of(tp.j + 1) : tp.t;
    D r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const D fnext = has_r ? D(L.f[c * NT + tr], L.f[(3 + c) * NT + tr]) : D();
        r[c] = D(u[c], du[c]) - (fr[c] + fnext);
    }
    if (drag_on) r[1] = r[1] + drag_force<D>(D(sc.drag, T(0)), D(v[1], dv[1]));
    if (grav_on) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int segs[2] = {sc.grav.segA[c], sc.grav.segB[c]};
            const int go = sc.grav.comp[c];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (segs[s] < 0) continue;
                const int ts = tp.thread_of(segs[s]);
                r[c] = r[c] + D(L.g[go * NT + ts], L.g[(2 + go) * NT + ts]);
            }
        }
    }

    // -- 3. M^-1 by the plan's (truncated) cyclic reduction: the same multipliers on the value and the tangent
    T rv[3], rd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { rv[c] = r[c].v; rd[c] = r[c].d; }
    for (int l = 0; l < p.levels; ++l) {
        T* const buf = (l & 1) ? L.r1 : L.r0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { buf[c * NT + tp.t] = rv[c]; buf[(3 + c) * NT + tp.t] = rd[c]; }
        __syncthreads();
        const int s = 1 << l;
        const bool lo = tp.j - s >= 0, hi = tp.j + s < tp.S;
        const int tlo = lo ? tp.thread_of(tp.j - s) : tp.t, thi = hi ? tp.thread_of(tp.j + s) : tp.t;
        T lov[3], hiv[3], lod[3], hid[3], cf[PCR_LEVEL_VALS];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lov[c] = lo ? buf[c * NT + tlo] : T(0);
            lod[c] = lo ? buf[(3 + c) * NT + tlo] : T(0);
            hiv[c] = hi ? buf[c * NT + thi] : T(0);
            hid[c] = hi ? buf[(3 + c) * NT + thi] : T(0);
        }
        const T* src = k.lv + size_t(l) * size_t(p.S) * PCR_LEVEL_VALS;
#pragma unroll
        for (int i = 0; i < PCR_LEVEL_VALS; ++i) cf[i] = tp.valid ? src[i] : T(0);
        pcr_apply_level<T>(cf, lov, hiv, rv);
        pcr_apply_level<T>(cf, lod, hid, rd);
    }
    pcr_apply_final<T>(k.fin, rv, a);
    pcr_apply_final<T>(k.fin, rd, da);
}

// MODE_RHS: xdot = f(x, u) (d == 0, when p.out is set) and dxdot[d] = df/dx dx[d] + df/du du[d].
// MODE_STEP: n_steps RK4 steps of the base (written back by d == 0) and of its tangent d (in place).  fp64 only.
template <typename T, int MODE>
__global__ void __launch_bounds__(TANGENT_MAX_NT) crb_jvp_kernel(const KParams<T> p, const TangentParams<T> tq) {
    static_assert(sizeof(T) == 8, "the tangent kernels are fp64");
    static_assert(MODE == MODE_RHS || MODE == MODE_STEP, "MODE_RHS or MODE_STEP");
    const TangentLds<T> L = carve_tangent_lds<T>(blockDim.x);
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    const size_t d = blockIdx.y;

    JvpConst<T> k;
    jvp_load_const<T>(p, tp, k);
    const SlotConst<T>& sc = k.sc;

    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t xoff = size_t(tp.beam) * 2 * plane + node * 4;            // the base's record
    const size_t dxoff = d * size_t(p.B) * 2 * plane + xoff;              // this direction's record
    const size_t uoff = size_t(tp.beam) * plane + node * 4;
    const size_t duoff = d * (tq.du_dir_stride ? tq.du_dir_stride : size_t(p.B) * plane) + uoff;
    const T* const xin = (MODE == MODE_STEP) ? tq.x0 : p.x;
    T x[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, dx[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    T uh[3] = {T(0), T(0), T(0)}, duh[3] = {T(0), T(0), T(0)};
    T amp = T(0), damp = T(0);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = xin[xoff + c] * sc.mask[c];
            x[3 + c] = xin[xoff + plane + c] * sc.mask[c];
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

    if (MODE == MODE_RHS) {
        T a[3], da[3];
        jvp_accel<T>(p, L, tp, k, x, dx, x + 3, dx + 3, uh, duh, a, da);
        if (!valid) return;
        T* const o = tq.dxdot + dxoff;
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[c] = dx[3 + c]; o[plane + c] = da[c]; }
        o[3] = T(0);
        o[plane + 3] = T(0);
        if (p.off == 1 && tp.j == 0)   // node 0 (FIXED in every beam, no slot): zero
#pragma unroll
            for (int c = 0; c < 4; ++c) { o[c - 4] = T(0); o[plane + c - 4] = T(0); }
        if (d == 0 && p.out) {
            T* const xo = p.out + xoff;
#pragma unroll
            for (int c = 0; c < 3; ++c) { xo[c] = x[3 + c]; xo[plane + c] = a[c]; }
            xo[3] = T(0);
            xo[plane + 3] = T(0);
            if (p.off == 1 && tp.j == 0)
#pragma unroll
                for (int c = 0; c < 4; ++c) { xo[c - 4] = T(0); xo[plane + c - 4] = T(0); }
        }
        return;
    }

    // ---- classical RK4 on (x, dx): crb_beam_kernel's MODE_STEP with the tangent alongside
    const T dt = T(p.dt), hdt = T(0.5 * p.dt), dt6 = T(p.dt / 6.0);
    double tc = p.t0;
    // control schedule: steps until the next interval's force (and its tangent) take over; never 0 without a schedule
    int sched_left = p.sched_stride ? p.sched_first : -1;
    size_t sched_off = 0;
    for (int step = 0; step < p.n_steps; ++step) {
        if (sched_left == 0) {   // (wave-uniform)
            sched_left = p.sched_hold;
            sched_off += p.sched_stride;
            if (valid)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    uh[c] = p.u_held[sched_off + uoff + c];
                    if (tq.du_held) duh[c] = tq.du_held[sched_off + duoff + c] * sc.mask[c];
                }
        }
        --sched_left;
        const double t_half = __dadd_rn(tc, 0.5 * p.dt), t_full = __dadd_rn(tc, p.dt);
        T acc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, dacc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
        T xs[6], dxs[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) { xs[c] = x[c]; dxs[c] = dx[c]; }
#pragma unroll 1
        for (int s = 0; s < 4; ++s) {
            const double ts = (s == 0) ? tc : ((s == 3) ? t_full : t_half);
            const bool on = ts < p.duration;
            const T av = on ? amp : T(0), dav = on ? damp : T(0);
            T uadd[3], duadd[3], a[3], da[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uadd[c] = uh[c] + ((c == p.imp_dof) ? av : T(0));
                duadd[c] = duh[c] + ((c == p.imp_dof) ? dav : T(0));
            }
            jvp_accel<T>(p, L, tp, k, xs, dxs, xs + 3, dxs + 3, uadd, duadd, a, da);
            const T w = (s == 0 || s == 3) ? T(1) : T(2);
            const T cs = (s == 2) ? dt : hdt;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const T kq = xs[3 + c], kv = a[c], dkq = dxs[3 + c], dkv = da[c];
                acc[c] += w * kq;
                acc[3 + c] += w * kv;
                dacc[c] += w * dkq;
                dacc[3 + c] += w * dkv;
                xs[c] = x[c] + cs * kq;
                xs[3 + c] = x[3 + c] + cs * kv;
                dxs[c] = dx[c] + cs * dkq;
                dxs[3 + c] = dx[3 + c] + cs * dkv;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) { x[c] += dt6 * acc[c]; dx[c] += dt6 * dacc[c]; }
        tc = t_full;
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
