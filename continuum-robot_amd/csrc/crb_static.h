// crb_static.h -- static equilibrium and tangent stiffness of every beam of an ensemble (crb_solve_static,
// crb_tangent_stiffness), and the sensitivities of that equilibrium (crb_static_jvp, crb_static_vjp: the end of this file).
//
// Residual.  r(q) = k(q) - g(q) - u with the velocities zero (drag vanishes): the force balance whose zero is a rest shape,
// i.e. the q at which crb_rhs returns zero acceleration.  k and g are evaluated per node exactly as the RHS kernels do
// (crb_generic.h): the element LEFT of a node in its thread, the right neighbour's left-node half through LDS, segment
// gravity with the reference's reduced-index table (gravity_forces.py:97-146).
//
// Tangent.  J = dr/dq is block tridiagonal over the nodes, 3 x 3 blocks on [u, w, phi] (A = coupling to the node on the
// left, B = own, C = right).  The element tangent comes from elem_force on dual numbers (crb_math.h: elem_tangent) and
// is assembled like the mass matrix (mass_add_as_left_elem / mass_add_as_right_elem): a node's own element contributes
// K22 to B and K21 to A, the element on its right (its right neighbour's) K11 to B and K12 to C.  Gravity adds -dg/dq:
// segment s's force depends on the rotation(s) its table entry phiA / phiB names.  For a FIXED root (the plain cantilever)
// those lie on slots s and s + 1, inside the +-1 band of every node the segment loads.  A PINNED root (and any other
// constraint that removes a number of DOFs that is no multiple of three ahead of a segment) shifts the reduced indexing, and
// the row of node i then depends on a source two or more slots away: such terms fall outside the band and are left out of
// the ITERATION matrix only (the residual keeps them; Newton converges linearly instead of quadratically there -- they are
// O(rho A L g), against the element stiffness).  The plan builder records whether a plan has such terms
// (gravity_out_of_band): the sensitivities at the end of this file, for which the tangent must be exact, refuse it.
// Constrained DOFs get identity rows and columns.
//
// Newton homotopy from the initial guess q0:  H(q, lam) = r(q) - (1 - lam) r(q0),  lam = 0 -> 1 in load_steps equal
// increments; an increment that does not converge within max_iter Newton steps is halved (q back to the start of the
// increment), up to STATIC_HALVINGS times in a row and never below nominal / 2^STATIC_HALVINGS, then the beam fails (-1).
// After an accepted increment the next one doubles back towards the nominal size.  A beam whose residual is affine in q
// (all-linear elements, no gravity) takes one increment.
// Termination: every accepted increment advances lam by at least nominal / 2^STATIC_HALVINGS (or ends the path), so a beam
// accepts at most 2^STATIC_HALVINGS load_steps + 1 increments, with at most STATIC_HALVINGS + 1 attempts of at most
// max_iter + 1 evaluations between two of them.  (Without the floor, a beam whose residual floor rises above rtol part-way
// along the path -- a limit point, or rounding at large deformations -- creeps towards that point with increments that
// shrink without bound: succeed at d, fail at 2 d, halve, succeed at d / 2, ... and never ends.)
// Convergence: |H|inf <= rtol max(|k(q)|inf, |g(q) + u|inf) + atol per beam.
//
// Solve.  Each Newton step solves J dq = H by block cyclic reduction in registers + LDS, all ceil(log2 S) levels, after a
// symmetric Jacobi scaling D J D (d = |J_kk|^-1/2: the blocks mix EA/L, 12EI/L^3 and 4EI/L).  Every level normalises the
// node row by its pivoted block inverse (crb_math.h: row3_normalise / row3_level), so the neighbours' diagonal blocks need
// not be exchanged: 21 values per node and level.
//
// Mapping.  make_topo (crb_generic.h): beams of fewer than 64 slots packed G to a wave, longer ones one
// beam per workgroup of up to 4 waves (256 thread-carried nodes).  The whole solve is one launch; every beam keeps its own
// increment / iteration state (uniform over its threads: all of them reduce the same norms), a beam that has converged or
// failed is switched off by predication, and a workgroup leaves when all of its beams are done.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_generic.h"

namespace crb {

constexpr int STATIC_MAX_NT = 256;
constexpr int STATIC_HALVINGS = 6;
constexpr int STATIC_RED_SLOTS = 65;   // per-beam reduction words: up to 64 beams of a wave + one for padding threads

template <typename T>
struct StaticParams {
    T* blocks;            // crb_tangent_kernel: [B][n_node][3][3][3] (left / own / right block, row-major)
    int load_steps, max_iter;
    double rtol, atol;
    int32_t* iters;       // [B]: Newton steps used, -1 not converged, -2 non-finite
    T* residual;          // [B] final |H|inf / max(|k|inf, |g + u|inf), or null
};

// LDS: q [3][NT], exchange [21][NT] (element halves + tangent blocks, then the reduction's rows), gravity [2][NT],
// per-beam reduction words
template <typename T>
struct StaticLds {
    T* q;
    T* x;
    T* g;
    unsigned long long* red;
    int NT;
};
// (xcols: columns of the exchange buffer; crb_static_sens_kernel carries 18 + 3 NR per level)
template <typename T>
__host__ __device__ constexpr size_t static_lds_bytes(int NT, int xcols = 21) {
    return size_t(5 + xcols) * size_t(NT) * sizeof(T) + size_t(STATIC_RED_SLOTS) * 4 * sizeof(unsigned long long);
}
template <typename T>
__device__ __forceinline__ StaticLds<T> carve_static_lds(int NT, int xcols = 21) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    StaticLds<T> l;
    l.NT = NT;
    l.q = reinterpret_cast<T*>(crb_smem);
    l.x = l.q + 3 * NT;
    l.g = l.x + xcols * NT;
    l.red = reinterpret_cast<unsigned long long*>(crb_smem + size_t(5 + xcols) * NT * sizeof(T));
    return l;
}

// Per-thread constants: the slot table, the left neighbour's mask and, per DOF and gravity segment, the rotation sources
// (phiA / phiB of that segment's table entry) of the gravity derivative.
template <typename T>
struct StaticConst {
    SlotConst<T> sc;
    T maskL[3];
    int16_t src[3][2][2];   // [dof][segA / segB][phiA / phiB]: (slot * 4 + dof) or -1
};
template <typename T>
__device__ __forceinline__ void static_load_const(const KParams<T>& p, const Topo& tp, StaticConst<T>& k) {
    SlotConst<T>& sc = k.sc;
    for (int c = 0; c < 3; ++c) {
        k.maskL[c] = T(0);
        for (int s = 0; s < 2; ++s) k.src[c][s][0] = k.src[c][s][1] = -1;
    }
    if (tp.valid) {
        const SlotConst<T>* st = p.slot + size_t(tp.beam) * p.slot_stride;
        sc = st[tp.j];
        if (tp.j >= 1)
            for (int c = 0; c < 3; ++c) k.maskL[c] = st[tp.j - 1].mask[c];
        for (int c = 0; c < 3; ++c) {
            const int sa = sc.grav.segA[c], sb = sc.grav.segB[c];
            if (sa >= 0) { k.src[c][0][0] = st[sa].grav.phiA; k.src[c][0][1] = st[sa].grav.phiB; }
            if (sb >= 0) { k.src[c][1][0] = st[sb].grav.phiA; k.src[c][1][1] = st[sb].grav.phiB; }
        }
    } else {
        sc = padding_slot<T>();
    }
}

// a += v at column d (0..2) of row r of a 3 x 3 block, d only known at run time: a select per column (no indexed registers)
template <typename T>
__device__ __forceinline__ void block_add(T (&M)[9], int r, int d, T v) {
#pragma unroll
    for (int c = 0; c < 3; ++c) M[3 * r + c] += (c == d) ? v : T(0);
}

// k(q), g(q) and the blocks of J = dk/dq - GRAV * dg/dq at this thread's node.  Whole workgroup (two barriers; the
// exchange buffer is free again when it returns).
template <typename T, bool GRAV>
__device__ __forceinline__ void static_eval(const KParams<T>& p, const StaticLds<T>& L, const Topo& tp, const StaticConst<T>& k,
                                            const T q[3], T kq[3], T gq[3], T (&A)[9], T (&B)[9], T (&C)[9]) {
    const int NT = L.NT;
    const SlotConst<T>& sc = k.sc;
    const bool corrected = (p.flags & 4u) != 0;
    const bool grav = GRAV && (p.flags & 2u) != 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) L.q[c * NT + tp.t] = q[c];
    __syncthreads();
    const bool has_l = tp.j >= 1, has_r = tp.j + 1 < tp.S;
    T ql[3];
    const int tl = has_l ? tp.thread_of(tp.j - 1) : tp.t;
#pragma unroll
    for (int c = 0; c < 3; ++c) ql[c] = has_l ? L.q[c * NT + tl] : T(0);
    T K[6][6], fl[3], fr[3];
    elem_tangent<T>(sc.elem, ql, q, corrected, K, fl, fr);
    T gseg[2] = {T(0), T(0)};
    if (grav && sc.half_mass != T(0)) {
        const int ia = sc.grav.phiA, ib = sc.grav.phiB;
        T phi = T(0);
        if (ia >= 0) phi = L.q[(ia & 3) * NT + tp.thread_of(ia >> 2)];
        if (ib >= 0) phi = T(0.5) * (phi + L.q[(ib & 3) * NT + tp.thread_of(ib >> 2)]);
        T gx = p.gx, gy = p.gy;
        if (p.gvec) { gx = p.gvec[2 * size_t(tp.beam)]; gy = p.gvec[2 * size_t(tp.beam) + 1]; }
        gravity_segment<T>(phi, gx, gy, sc.half_mass, gseg);
    }
    // publish the left-node half of this node's element (force, K11, K12) for the node on the left
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        L.x[r * NT + tp.t] = fl[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            L.x[(3 + 3 * r + c) * NT + tp.t] = K[r][c] * k.maskL[c];
            L.x[(12 + 3 * r + c) * NT + tp.t] = K[r][3 + c] * sc.mask[c];
        }
    }
    if (grav) { L.g[tp.t] = gseg[0]; L.g[NT + tp.t] = gseg[1]; }
    __syncthreads();
    const int tr = has_r ? tp.thread_of(tp.j + 1) : tp.t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        kq[r] = fr[r] + (has_r ? L.x[r * NT + tr] : T(0));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[3 * r + c] = K[3 + r][c] * k.maskL[c];
            B[3 * r + c] = K[3 + r][3 + c] * sc.mask[c] + (has_r ? L.x[(3 + 3 * r + c) * NT + tr] : T(0));
            C[3 * r + c] = has_r ? L.x[(12 + 3 * r + c) * NT + tr] : T(0);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) gq[c] = T(0);
    if (grav) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int segs[2] = {sc.grav.segA[c], sc.grav.segB[c]};
            const int go = sc.grav.comp[c];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (segs[s] < 0) continue;
                const int ts = tp.thread_of(segs[s]);
                const T g2[2] = {L.g[ts], L.g[NT + ts]};
                gq[c] += g2[go];
                T dg[2];
                gravity_segment_dphi<T>(g2, dg);
                const int ia = k.src[c][s][0], ib = k.src[c][s][1];
                const T w = (ia >= 0 && ib >= 0) ? T(0.5) : T(1);
                const int srcs[2] = {ia, ib};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if (srcs[e] < 0) continue;
                    const int off = (srcs[e] >> 2) - tp.j, d = srcs[e] & 3;
                    const T v = -w * dg[go];   // J = dk/dq - dg/dq
                    if (off == -1) block_add<T>(A, c, d, v);
                    else if (off == 0) block_add<T>(B, c, d, v);
                    else if (off == 1) block_add<T>(C, c, d, v);
                    // (|off| > 1: PINNED-root indexing, outside the band -- left out of the iteration matrix, see the top)
                }
            }
        }
    }
    // constrained rows: identity
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const bool fr_ = sc.mask[r] != T(0);
        kq[r] *= sc.mask[r];
        gq[r] *= sc.mask[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[3 * r + c] = fr_ ? A[3 * r + c] : T(0);
            C[3 * r + c] = fr_ ? C[3 * r + c] : T(0);
            B[3 * r + c] = fr_ ? B[3 * r + c] : (r == c ? T(1) : T(0));
        }
    }
    __syncthreads();   // (the exchange buffer is rewritten by the next caller)
}

// crb_tangent_kernel: the blocks of dk/dq at the positions of plane 0 of p.x, into sp.blocks [B][n_node][3][3][3].
template <typename T>
__global__ void __launch_bounds__(STATIC_MAX_NT) crb_tangent_kernel(const KParams<T> p, const StaticParams<T> sp) {
    const StaticLds<T> L = carve_static_lds<T>(blockDim.x);
    int g;
    const Topo tp = make_topo<T>(p, g);
    StaticConst<T> k;
    static_load_const<T>(p, tp, k);
    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    T q[3] = {T(0), T(0), T(0)};
    if (tp.valid)
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = p.x[size_t(tp.beam) * 2 * plane + node * 4 + c] * k.sc.mask[c];
    T kq[3], gq[3], A[9], B[9], C[9];
    static_eval<T, false>(p, L, tp, k, q, kq, gq, A, B, C);
    if (!tp.valid) return;
    T* o = sp.blocks + (size_t(tp.beam) * p.n_node + node) * 27;
#pragma unroll
    for (int e = 0; e < 9; ++e) { o[e] = A[e]; o[9 + e] = B[e]; o[18 + e] = C[e]; }
    if (p.off == 1 && tp.j == 0) {   // node 0 (FIXED in every beam, no slot): an identity row
        T* o0 = sp.blocks + size_t(tp.beam) * p.n_node * 27;
#pragma unroll
        for (int e = 0; e < 27; ++e) o0[e] = (e >= 9 && e < 18 && (e - 9) % 4 == 0) ? T(1) : T(0);
    }
}

// per-beam maxima of four non-negative values (fp64 bit patterns order as unsigned integers; a NaN comes out on top).
// Whole workgroup.  `slot` = the beam's words.
__device__ __forceinline__ void beam_max4(unsigned long long* slot, const Topo& tp, const double v[4], double out[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicMax(slot + k, (unsigned long long)__double_as_longlong(v[k]));
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = __longlong_as_double((long long)slot[k]);
    __syncthreads();
    if (tp.j == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) slot[k] = 0ull;   // (the next use is at least one barrier away)
}

// Solves the node rows of the workgroup (J dq = H, one row per thread) by block cyclic reduction: symmetric Jacobi scaling,
// `levels` levels, final block inverse.  Whole workgroup; X = the exchange buffer [21][NT].
__device__ __forceinline__ void static_solve(const Topo& tp, double* X, int NT, int levels, Row3& w, double x[3]) {
    // -- D J D, d = |J_kk|^-1/2 (1 where the diagonal is zero or not finite)
    double d[3], dl[3], dh[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = fabs(w.B[4 * c]);
        d[c] = (a > 0.0 && a < INFINITY) ? 1.0 / sqrt(a) : 1.0;
        X[c * NT + tp.t] = d[c];
    }
    __syncthreads();
    {
        const bool hl = tp.j >= 1, hh = tp.j + 1 < tp.S;
        const int tl = hl ? tp.thread_of(tp.j - 1) : tp.t, th = hh ? tp.thread_of(tp.j + 1) : tp.t;
#pragma unroll
        for (int c = 0; c < 3; ++c) { dl[c] = hl ? X[c * NT + tl] : 1.0; dh[c] = hh ? X[c * NT + th] : 1.0; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        w.r[r] *= d[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) { w.A[3 * r + c] *= d[r] * dl[c]; w.B[3 * r + c] *= d[r] * d[c]; w.C[3 * r + c] *= d[r] * dh[c]; }
    }
    // -- reduction levels
    for (int l = 0; l < levels; ++l) {
        const int s = 1 << l;
        row3_normalise(w);
#pragma unroll
        for (int e = 0; e < 9; ++e) { X[e * NT + tp.t] = w.A[e]; X[(9 + e) * NT + tp.t] = w.C[e]; }
#pragma unroll
        for (int e = 0; e < 3; ++e) X[(18 + e) * NT + tp.t] = w.r[e];
        __syncthreads();
        const bool lo = tp.j - s >= 0, hi = tp.j + s < tp.S;
        const int tl = lo ? tp.thread_of(tp.j - s) : tp.t, th = hi ? tp.thread_of(tp.j + s) : tp.t;
        double loA[9], loC[9], lor[3], hiA[9], hiC[9], hir[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            loA[e] = lo ? X[e * NT + tl] : 0.0;
            loC[e] = lo ? X[(9 + e) * NT + tl] : 0.0;
            hiA[e] = hi ? X[e * NT + th] : 0.0;
            hiC[e] = hi ? X[(9 + e) * NT + th] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) { lor[e] = lo ? X[(18 + e) * NT + tl] : 0.0; hir[e] = hi ? X[(18 + e) * NT + th] : 0.0; }
        __syncthreads();
        Row3 o;
        row3_level(w, loA, loC, lor, hiA, hiC, hir, o);
        w = o;
    }
    double Bi[9];
    inv3<double>(w.B, Bi);
    mulv3<double>(Bi, w.r, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] *= d[c];
}

// crb_static_kernel: the whole static solve of every beam in one launch (see the top of this file).  fp64 only.
template <typename T>
__global__ void __launch_bounds__(STATIC_MAX_NT, 1) crb_static_kernel(const KParams<T> p, const StaticParams<T> sp) {
    static_assert(sizeof(T) == 8, "the static solve is fp64 (Row3, the reduction's rows, are fp64)");
    const int NT = blockDim.x;
    const StaticLds<T> L = carve_static_lds<T>(NT);
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    StaticConst<T> k;
    static_load_const<T>(p, tp, k);
    unsigned long long* const red = L.red + 4 * g;
    for (int i = tp.t; i < STATIC_RED_SLOTS * 4; i += NT) L.red[i] = 0ull;
    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t xoff = size_t(tp.beam) * 2 * plane + node * 4;
    T q[3] = {0.0, 0.0, 0.0}, uh[3] = {0.0, 0.0, 0.0};
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            q[c] = p.x[xoff + c] * k.sc.mask[c];
            if (p.u_held) uh[c] = p.u_held[size_t(tp.beam) * plane + node * 4 + c];
        }
    }
    __syncthreads();   // (reduction words zeroed)

    // r(q0), and whether the beam's residual is affine in q (all-linear elements, no gravity): one increment then
    T r0[3];
    Row3 w;
    double nrm[4];
    {
        T kq[3], gq[3];
        static_eval<T, true>(p, L, tp, k, q, kq, gq, w.A, w.B, w.C);
#pragma unroll
        for (int c = 0; c < 3; ++c) r0[c] = kq[c] - gq[c] - uh[c] * k.sc.mask[c];
        const bool nonaffine = valid && (k.sc.elem.kind == KIND_NONLINEAR || ((p.flags & 2u) && k.sc.half_mass != 0.0));
        const double v[4] = {0.0, 0.0, 0.0, nonaffine ? 1.0 : 0.0};
        beam_max4(red, tp, v, nrm);
    }
    const double nominal = (nrm[3] != 0.0) ? 1.0 / double(sp.load_steps) : 1.0;
    const double dlam_min = nominal * (1.0 / double(1 << STATIC_HALVINGS));
    double lam = 0.0, dlam = nominal, resid = 0.0;
    int halv = 0, it = 0, total = 0, state = 0;   // state: 0 running, 1 converged, -1 not converged, -2 non-finite
    T qs[3] = {q[0], q[1], q[2]};
    for (;;) {
        const bool act = valid && state == 0;
        if (!__syncthreads_or(act)) break;
        const double lt = (dlam >= 1.0 - lam) ? 1.0 : lam + dlam;
        T kq[3], gq[3], H[3];
        static_eval<T, true>(p, L, tp, k, q, kq, gq, w.A, w.B, w.C);
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T gu = gq[c] + uh[c] * k.sc.mask[c];
            H[c] = kq[c] - gu - (1.0 - lt) * r0[c];
            v[0] = fmax(v[0], fabs(H[c]));
            v[1] = fmax(v[1], fabs(kq[c]));
            v[2] = fmax(v[2], fabs(gu));
            bad = bad || !isfinite(H[c]);
        }
        if (bad) v[0] = __longlong_as_double(0x7ff8000000000000ll);   // (fmax drops a NaN operand: a positive NaN tops the max)
        beam_max4(red, tp, v, nrm);
        bool step = false;
        if (act) {
            const double scale = fmax(nrm[1], nrm[2]);
            const bool finite = isfinite(nrm[0]);
            resid = scale > 0.0 ? nrm[0] / scale : nrm[0];
            if (!finite && it == 0) {
                state = -2;   // at an accepted iterate: the input itself is not finite
            } else if (finite && nrm[0] <= sp.rtol * scale + sp.atol) {
                lam = lt;
                it = 0;
                halv = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) qs[c] = q[c];
                if (lam >= 1.0) state = 1;
                else dlam = fmin(fmin(2.0 * dlam, nominal), 1.0 - lam);
            } else if (!finite || it >= sp.max_iter) {
                if (++halv > STATIC_HALVINGS || 0.5 * dlam < dlam_min) {
                    state = -1;
                } else {
                    dlam *= 0.5;
                    it = 0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c] = qs[c];
                }
            } else {
                step = true;
            }
        }
        if (__syncthreads_or(step)) {
            if (step) {
#pragma unroll
                for (int c = 0; c < 3; ++c) w.r[c] = H[c];
            } else {   // a beam that does not step this round solves an identity system
#pragma unroll
                for (int e = 0; e < 9; ++e) { w.A[e] = 0.0; w.C[e] = 0.0; w.B[e] = (e % 4 == 0) ? 1.0 : 0.0; }
                w.r[0] = w.r[1] = w.r[2] = 0.0;
            }
            double dq[3];
            static_solve(tp, L.x, NT, p.levels, w, dq);
            if (step) {
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c] -= dq[c] * k.sc.mask[c];
                ++it;
                ++total;
            }
        }
    }
    if (!valid) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) { p.x[xoff + c] = q[c]; p.x[xoff + plane + c] = 0.0; }
    p.x[xoff + 3] = 0.0;
    p.x[xoff + plane + 3] = 0.0;
    if (tp.j == 0) {
        if (p.off == 1)   // node 0 (FIXED in every beam, no slot): zero as well
#pragma unroll
            for (int c = 0; c < 4; ++c) { p.x[xoff - 4 + c] = 0.0; p.x[xoff - 4 + plane + c] = 0.0; }
        sp.iters[tp.beam] = state == 1 ? total : state;
        if (sp.residual) sp.residual[tp.beam] = resid;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Sensitivities of the equilibrium (crb_static_jvp, crb_static_vjp).  With R(q; u, theta) = k(q) - g(q) - u = 0 the implicit
// function theorem gives dq = J^-1 du and, for a cotangent qbar = dL/dq, mu = J^-T qbar = dL/du; dL/dtheta = mu . dr/dtheta
// with r = u - k + g is crb_paramgrad.h's stage sum at the one point q (crb_static_param_kernel).  J is static_eval's exact
// tangent (the plan builder refuses the plans whose gravity couplings fall outside its band); it does not depend on u.
//
// crb_static_sens_kernel<T, TRANSPOSE, NR>: grid groups x ceil(n_dir / NR), crb_static_kernel's mapping and tables.  One
// tangent evaluation and, per pass, one Jacobi scaling and the matrix part of every reduction level serve NR right-hand
// sides; the exchange carries 18 + 3 NR columns per level.  Two passes: the solve and one refinement step on b - J x.  TRANSPOSE turns the node row (A_j, B_j, C_j) of J into that of J^T,
// ((C_{j-1})^T, B_j^T, (A_{j+1})^T), by one exchange of A and C.  Right-hand sides past n_dir (the tail chunk) are zero and
// store nothing.  Everything that crosses lanes is a select on `inside the beam`, never a 0 / 1 factor: a beam whose q is not
// finite leaves the beams that share its wave bitwise alone.
template <typename T>
struct StaticSensParams {
    const T* rhs;       // [n_dir][B][n_node][4]: du, or qbar
    T* sol;             // [n_dir][B][n_node][4]: dq = J^-1 du, or mu = J^-T qbar (component 3, constrained DOFs: 0)
    int n_dir;
    int32_t* status;    // [B] zeroed before the launch: -2 where a component of a direction is not finite; or null
};
__host__ __device__ constexpr int static_sens_xcols(int NR) { return 18 + 3 * NR > 21 ? 18 + 3 * NR : 21; }

// static_solve for NR right-hand sides: r[k] in, x[k] out; A, B, C are consumed.  Whole workgroup; X = [18 + 3 NR][NT].
template <int NR>
__device__ __forceinline__ void static_solve_multi(const Topo& tp, double* X, int NT, int levels, double (&A)[9], double (&B)[9],
                                                   double (&C)[9], double (&r)[NR][3], double (&x)[NR][3]) {
    double d[3], dl[3], dh[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = fabs(B[4 * c]);
        d[c] = (a > 0.0 && a < INFINITY) ? 1.0 / sqrt(a) : 1.0;
        X[c * NT + tp.t] = d[c];
    }
    __syncthreads();
    {
        const bool hl = tp.j >= 1, hh = tp.j + 1 < tp.S;
        const int tl = hl ? tp.thread_of(tp.j - 1) : tp.t, th = hh ? tp.thread_of(tp.j + 1) : tp.t;
#pragma unroll
        for (int c = 0; c < 3; ++c) { dl[c] = hl ? X[c * NT + tl] : 1.0; dh[c] = hh ? X[c * NT + th] : 1.0; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < NR; ++k) r[k][i] *= d[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) { A[3 * i + c] *= d[i] * dl[c]; B[3 * i + c] *= d[i] * d[c]; C[3 * i + c] *= d[i] * dh[c]; }
    }
    for (int l = 0; l < levels; ++l) {
        const int s = 1 << l;
        double Bi[9];
        row3_normalise_matrix(A, B, C, Bi);
#pragma unroll
        for (int k = 0; k < NR; ++k) row3_normalise_rhs(Bi, r[k]);
#pragma unroll
        for (int e = 0; e < 9; ++e) { X[e * NT + tp.t] = A[e]; X[(9 + e) * NT + tp.t] = C[e]; }
#pragma unroll
        for (int k = 0; k < NR; ++k)
#pragma unroll
            for (int e = 0; e < 3; ++e) X[(18 + 3 * k + e) * NT + tp.t] = r[k][e];
        __syncthreads();
        const bool lo = tp.j - s >= 0, hi = tp.j + s < tp.S;
        const int tl = lo ? tp.thread_of(tp.j - s) : tp.t, th = hi ? tp.thread_of(tp.j + s) : tp.t;
#pragma unroll
        for (int k = 0; k < NR; ++k) {   // (the right-hand sides first: they read the row's A and C of before the level)
            double lor[3], hir[3], o[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                lor[e] = lo ? X[(18 + 3 * k + e) * NT + tl] : 0.0;
                hir[e] = hi ? X[(18 + 3 * k + e) * NT + th] : 0.0;
            }
            row3_level_rhs(A, C, r[k], lor, hir, o);
#pragma unroll
            for (int e = 0; e < 3; ++e) r[k][e] = o[e];
        }
        double loA[9], loC[9], hiA[9], hiC[9], oA[9], oC[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            loA[e] = lo ? X[e * NT + tl] : 0.0;
            loC[e] = lo ? X[(9 + e) * NT + tl] : 0.0;
            hiA[e] = hi ? X[e * NT + th] : 0.0;
            hiC[e] = hi ? X[(9 + e) * NT + th] : 0.0;
        }
        __syncthreads();
        row3_level_matrix(A, C, loA, loC, hiA, hiC, oA, B, oC);
#pragma unroll
        for (int e = 0; e < 9; ++e) { A[e] = oA[e]; C[e] = oC[e]; }
    }
    double Bi[9];
    inv3<double>(B, Bi);
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        mulv3<double>(Bi, r[k], x[k]);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[k][c] *= d[c];
    }
}

template <typename T, bool TRANSPOSE, int NR>
__global__ void __launch_bounds__(STATIC_MAX_NT) crb_static_sens_kernel(const KParams<T> p, const StaticSensParams<T> sp) {
    static_assert(sizeof(T) == 8, "the static sensitivities are fp64 (the reduction's rows are fp64)");
    const int NT = blockDim.x;
    const StaticLds<T> L = carve_static_lds<T>(NT, static_sens_xcols(NR));
    int g;
    const Topo tp = make_topo<T>(p, g);
    const bool valid = tp.valid;
    StaticConst<T> k;
    static_load_const<T>(p, tp, k);
    unsigned long long* const red = L.red + 4 * g;
    for (int i = tp.t; i < STATIC_RED_SLOTS * 4; i += NT) L.red[i] = 0ull;   // (static_eval's barriers come before its use)
    const size_t plane = size_t(p.n_node) * 4, node = size_t(tp.j + p.off);
    const size_t voff = size_t(tp.beam) * plane + node * 4;
    const int d0 = int(blockIdx.y) * NR;
    bool fr[3];
    T q[3] = {0.0, 0.0, 0.0};
    double r[NR][3], x[NR][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        fr[c] = valid && k.sc.mask[c] != T(0);
        if (fr[c]) q[c] = p.x[size_t(tp.beam) * 2 * plane + node * 4 + c];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            r[i][c] = 0.0;
            if (fr[c] && d0 + i < sp.n_dir) r[i][c] = sp.rhs[size_t(d0 + i) * size_t(p.B) * plane + voff + c];
        }
    }
    double A[9], B[9], C[9];
    {
        T kq[3], gq[3];
        static_eval<T, true>(p, L, tp, k, q, kq, gq, A, B, C);
    }
    if (TRANSPOSE) {
        double* const X = L.x;
#pragma unroll
        for (int e = 0; e < 9; ++e) { X[e * NT + tp.t] = A[e]; X[(9 + e) * NT + tp.t] = C[e]; }
        __syncthreads();
        const bool hl = tp.j >= 1, hh = tp.j + 1 < tp.S;
        const int tl = hl ? tp.thread_of(tp.j - 1) : tp.t, th = hh ? tp.thread_of(tp.j + 1) : tp.t;
        double own[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                A[3 * i + c] = hl ? X[(9 + 3 * c + i) * NT + tl] : 0.0;   // (C_{j-1})^T
                C[3 * i + c] = hh ? X[(3 * c + i) * NT + th] : 0.0;       // (A_{j+1})^T
                own[3 * i + c] = B[3 * c + i];
            }
#pragma unroll
        for (int e = 0; e < 9; ++e) B[e] = own[e];
        __syncthreads();
    }
    // The solve, then ONE step of iterative refinement with the unscaled row: block cyclic reduction takes no pivots across
    // blocks, and on tangents of condition 1e8 .. 1e10 its error reached twice LAPACK's own; the residual b - J x in fp64 and a
    // second pass bring it to LAPACK's level.
    double A0[9], B0[9], C0[9], r0[NR][3];
#pragma unroll
    for (int e = 0; e < 9; ++e) { A0[e] = A[e]; B0[e] = B[e]; C0[e] = C[e]; }
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) r0[i][c] = r[i][c];
    static_solve_multi<NR>(tp, L.x, NT, p.levels, A, B, C, r, x);
    {
        double* const X = L.x;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) X[(3 * i + c) * NT + tp.t] = x[i][c];
        __syncthreads();
        const bool hl = tp.j >= 1, hh = tp.j + 1 < tp.S;
        const int tl = hl ? tp.thread_of(tp.j - 1) : tp.t, th = hh ? tp.thread_of(tp.j + 1) : tp.t;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            double xl[3], xh[3], a[3], b[3], c3[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xl[c] = hl ? X[(3 * i + c) * NT + tl] : 0.0;
                xh[c] = hh ? X[(3 * i + c) * NT + th] : 0.0;
            }
            mulv3<double>(A0, xl, a);
            mulv3<double>(B0, x[i], b);
            mulv3<double>(C0, xh, c3);
#pragma unroll
            for (int c = 0; c < 3; ++c) r[i][c] = r0[i][c] - a[c] - b[c] - c3[c];
        }
        __syncthreads();
    }
    {
        double dx[NR][3];
        static_solve_multi<NR>(tp, L.x, NT, p.levels, A0, B0, C0, r, dx);
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) x[i][c] += dx[i][c];
    }
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const bool on = valid && d0 + i < sp.n_dir;
        T* const o = sp.sol + size_t(d0 + i) * size_t(p.B) * plane + voff;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = fr[c] ? x[i][c] : 0.0;
            bad = bad || (on && !isfinite(v));
            if (on) o[c] = v;
        }
        if (on) {
            o[3] = 0.0;
            if (p.off == 1 && tp.j == 0)   // node 0 (FIXED in every beam, no slot): zero
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c - 4] = 0.0;
        }
    }
    atomicMax(red, bad ? 1ull : 0ull);
    __syncthreads();
    if (valid && tp.j == 0 && sp.status && red[0] != 0ull) sp.status[tp.beam] = -2;
}

}  // namespace crb
