// crb_blocked.h -- the mass solve of the register-blocked lean stepper (crb_step_lean_kernel<..., NPL = 4>): a 256-slot
// beam lives in ONE wave, lane l owning slots 4l .. 4l+3.  Slots 4l .. 4l+2 are a lane's interior nodes, slot 4l+3 its
// separator.  Per right-hand side r (M x = r, M block tridiagonal per node: axial scalar + (w, phi) 2x2):
//   1. y = A_II^-1 r_I          the lane's 3-node interior, exactly (block Thomas with precomputed factors)
//   2. g = r_s - A_s y_2 - C_s y_0(lane+1)                      the separator right-hand side (one exchange)
//   3. S x_s = g                the separator Schur system (one row per lane) by cyclic reduction at lane strides
//                               1, 2, 4, ..., truncated where the multipliers fall below the unit roundoff (pick_levels)
//   4. x_I = y - W_L x_s(lane-1) - W_R x_s                       back substitution (one exchange)
// For a uniform beam every interior block, A_s, C_s, W_L and W_R are the same in every lane (lane 0's W_L only ever meets
// the fixed root's x_s = 0, lane 63's C_s the 0 shifted in past the wave's end), so they are ONE table of wave-uniform
// constants; only the separator system's multipliers differ near the beam's ends and are stored per lane.
// blocked_factor builds both in fp64 and refuses a beam whose interior constants are not bitwise uniform.
// CRB_BLK_TWIST: step 1 twisted about the lane's centre node.  The blocked stepper only takes beams of equal elements, and
// their consistent mass matrix is mirror symmetric: every interior diagonal block B is diagonal (the +-22L terms of the two
// adjoining elements cancel) and C = J A J with J = diag(1, -1) on (w, phi).  Then the centre pivot
// Dc = B1 - A1 B0^-1 C0 - C1 B2^-1 A2 is diagonal too (the off-diagonal parts of its two products are mirror images), and
//   t0 = B^-1 r0, t2 = B^-1 r2;  z1 = r1 - (A1 B^-1) r0 - (C1 B^-1) r2;  y1 = Dc^-1 z1;  y0 = t0 - (B^-1 C0) y1;  y2 = t2 - (B^-1 A2) y1
// is 29 multiplies and multiply-adds of depth three against block Thomas's 35 of depth five (blk_twist_interior_solve).
// blocked_mirrored checks the structure bitwise; blocked_factor builds this form's constants for node blocks that have it, and a
// plan whose blocks lack it runs the block-Thomas instance.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "crb_math.h"

#ifndef CRB_BLK_TWIST
#define CRB_BLK_TWIST 1
#endif

namespace crb {

constexpr int BLK_NPL = 4;                 // nodes per lane
constexpr int BLK_LANES = 64;
constexpr int BLK_S = BLK_NPL * BLK_LANES; // slots of a beam the blocked stepper carries
constexpr int BLK_MAX_LV = 6;              // log2(BLK_LANES): the exact separator reduction
// A node block as 5 values: [axial, ww, wp, pw, pp] (the 2x2 row-major, as PCR_LEVEL_VALS' halves)
constexpr int BLK_PACK = 5;
// wave-uniform table: the interior's block-Thomas factors L1, L2 (forward), inv(D0..D2), U0 = inv(D0) C0, U1 = inv(D1) C1,
// then W_L[0..2], W_R[0..2], A_s, C_s
enum : int {
    BU_L1 = 0, BU_L2 = 5, BU_D0 = 10, BU_D1 = 15, BU_D2 = 20, BU_U0 = 25, BU_U1 = 30,
    BU_WL = 35, BU_WR = 50, BU_AS = 65, BU_CS = 70, BU_N = 76   // (75 values, padded to 16 bytes)
};
// per-lane separator table: `levels` level records of PCR_LEVEL_VALS, then the final inverse (5); stored value-major
// [value][lane] so that a wave reads one value of every lane with one conflict-free access
__host__ __device__ constexpr int blk_sep_vals(int levels) { return levels * PCR_LEVEL_VALS + BLK_PACK; }
// plans of nonlinear elements: the folded force constants (crb_math.h: elem_fold_build, FK_N values) follow the separator
// tables of the plan's `levels` in the blocked table buffer
__host__ __device__ constexpr int blk_fold_offset(int levels) { return BU_N + blk_sep_vals(levels) * BLK_LANES; }
// ... and behind them the constants of the form that shares the membrane combinations (elem_share_build, SK_N values)
__host__ __device__ constexpr int blk_share_offset(int levels) { return blk_fold_offset(levels) + FK_N; }

// The twisted form's wave-uniform table (CRB_BLK_TWIST), behind the constants of the shared form whatever the element kind:
// P = A1 B^-1, Q = C1 B^-1 (into z1), U = B^-1 C0, V = B^-1 A2 (back into y0, y2), the diagonals of B^-1 and Dc^-1
// [axial, w, phi], then W_L, W_R, A_s, C_s as in the table above.  It is stored as the kernel's registers read it: entry k
// at [k], BT_TAB = BLK_TAB_REGS * BLK_TAB_ROW values, zero behind BT_N.
enum : int {
    BT_P = 0, BT_Q = 5, BT_U = 10, BT_V = 15, BT_BI = 20, BT_DI = 23, BT_WL = 26, BT_WR = 41, BT_AS = 56, BT_CS = 61, BT_N = 66,
    BT_TAB = 80
};
__host__ __device__ constexpr int blk_twist_offset(int levels) { return blk_share_offset(levels) + SK_N; }

// The wave-uniform table as the kernel holds it: BLK_TAB_REGS fp64 registers per lane, constant k in lane k % BLK_TAB_ROW of
// EVERY 16-lane row of register k / BLK_TAB_ROW (a DPP row broadcast reads inside the reader's own row, so each of the four
// rows of a wave carries the whole table); the slots past the table repeat its zero pad.
constexpr int BLK_TAB_ROW = 16;
constexpr int BLK_TAB_REGS = (BU_N + BLK_TAB_ROW - 1) / BLK_TAB_ROW;   // 5
static_assert(BT_N <= BU_N && BT_TAB == BLK_TAB_REGS * BLK_TAB_ROW, "the twisted table fills the same registers");
__host__ __device__ constexpr int blk_tab_index(int reg, int lane) {   // the table entry that `lane` holds in register `reg`
    return BLK_TAB_ROW * reg + (lane & (BLK_TAB_ROW - 1)) < BU_N - 1 ? BLK_TAB_ROW * reg + (lane & (BLK_TAB_ROW - 1)) : BU_N - 1;
}

#if defined(__HIPCC__)
// ---- multiply-adds whose wave-uniform constant is a DPP row broadcast of the register table: no load, no SGPR, no wait.
// gfx950 has exactly one fp64 arithmetic instruction with a DPP source, the VOP2 v_fmac_f64 (d += src0 * src1, src0 through
// row_newbcast:N = lane N of the reader's row, sign by the source modifier); v_mov_b64 has the same source for a plain copy.
// The asm is not volatile: it is a pure function of its operands, the compiler may schedule and hoist it.  The compiler
// does not see the DPP in it and inserts no wait states for one: `tab` must have been written long before (lean_blocked_body).
// acc -= u[OFF] * x
template <int OFF, typename T>
__device__ __forceinline__ void blk_bc_fnma(const T (&tab)[BLK_TAB_REGS], T x, T& acc) {
    static_assert(OFF >= 0 && OFF < BU_N, "table offset");
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(acc) : "v"(tab[OFF / BLK_TAB_ROW]), "v"(x), "n"(OFF % BLK_TAB_ROW));
#else
    acc -= tab[OFF / BLK_TAB_ROW] * x;
#endif
}
// acc += u[OFF] * x
template <int OFF, typename T>
__device__ __forceinline__ void blk_bc_fma(const T (&tab)[BLK_TAB_REGS], T x, T& acc) {
    static_assert(OFF >= 0 && OFF < BU_N, "table offset");
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(acc) : "v"(tab[OFF / BLK_TAB_ROW]), "v"(x), "n"(OFF % BLK_TAB_ROW));
#else
    acc += tab[OFF / BLK_TAB_ROW] * x;
#endif
}
// u[OFF] in every lane (for the few products that head a sum: only the multiply-ADD has the broadcast form)
template <int OFF, typename T>
__device__ __forceinline__ T blk_bc_copy(const T (&tab)[BLK_TAB_REGS]) {
    static_assert(OFF >= 0 && OFF < BU_N, "table offset");
#if defined(__HIP_DEVICE_COMPILE__)
    T d;
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(tab[OFF / BLK_TAB_ROW]), "n"(OFF % BLK_TAB_ROW));
    return d;
#else
    return tab[OFF / BLK_TAB_ROW];
#endif
}
// o -= u[OFF .. OFF+4] v, the roundings of blk_sub_mul below: each component one chain of fused multiply-adds
template <int OFF, typename T>
__device__ __forceinline__ void blk_bc_sub_mul(const T (&tab)[BLK_TAB_REGS], const T v[3], T o[3]) {
    blk_bc_fnma<OFF + 0>(tab, v[0], o[0]);
    blk_bc_fnma<OFF + 1>(tab, v[1], o[1]);
    blk_bc_fnma<OFF + 2>(tab, v[2], o[1]);
    blk_bc_fnma<OFF + 3>(tab, v[1], o[2]);
    blk_bc_fnma<OFF + 4>(tab, v[2], o[2]);
}
// o += u[OFF .. OFF+4] v
template <int OFF, typename T>
__device__ __forceinline__ void blk_bc_add_mul(const T (&tab)[BLK_TAB_REGS], const T v[3], T o[3]) {
    blk_bc_fma<OFF + 0>(tab, v[0], o[0]);
    blk_bc_fma<OFF + 1>(tab, v[1], o[1]);
    blk_bc_fma<OFF + 2>(tab, v[2], o[1]);
    blk_bc_fma<OFF + 3>(tab, v[1], o[2]);
    blk_bc_fma<OFF + 4>(tab, v[2], o[2]);
}
#endif

// ---- apply a 5-pack to a 3-vector [u, w, phi]
// (P: a plain or a constant-address-space pointer)
template <typename T, typename P = const T*>
__host__ __device__ __forceinline__ void blk_mul(P m, const T v[3], T o[3]) {
    o[0] = m[0] * v[0];
    o[1] = m[1] * v[1] + m[2] * v[2];
    o[2] = m[3] * v[1] + m[4] * v[2];
}
// o -= m v
template <typename T, typename P = const T*>
__host__ __device__ __forceinline__ void blk_sub_mul(P m, const T v[3], T o[3]) {
    o[0] = o[0] - m[0] * v[0];
    o[1] = o[1] - m[1] * v[1] - m[2] * v[2];
    o[2] = o[2] - m[3] * v[1] - m[4] * v[2];
}
// y = A_II^-1 r for the three interior nodes of a lane (u: the wave-uniform table)
template <typename T, typename P = const T*>
__host__ __device__ __forceinline__ void blk_interior_solve(P u, const T r[][3], T y[3][3]) {
    T z1[3] = {r[1][0], r[1][1], r[1][2]}, z2[3] = {r[2][0], r[2][1], r[2][2]};
    blk_sub_mul<T, P>(u + BU_L1, r[0], z1);
    blk_sub_mul<T, P>(u + BU_L2, z1, z2);
    blk_mul<T, P>(u + BU_D2, z2, y[2]);
    blk_mul<T, P>(u + BU_D1, z1, y[1]);
    blk_sub_mul<T, P>(u + BU_U1, y[2], y[1]);
    blk_mul<T, P>(u + BU_D0, r[0], y[0]);
    blk_sub_mul<T, P>(u + BU_U0, y[1], y[0]);
}
// the same about the lane's centre node (w: the twisted table; needs the mirror structure, blocked_factor)
template <typename T, typename P = const T*>
__host__ __device__ __forceinline__ void blk_twist_interior_solve(P w, const T r[][3], T y[3][3]) {
    T z1[3] = {r[1][0], r[1][1], r[1][2]};
    blk_sub_mul<T, P>(w + BT_P, r[0], z1);
    blk_sub_mul<T, P>(w + BT_Q, r[2], z1);
    for (int c = 0; c < 3; ++c) {
        y[0][c] = w[BT_BI + c] * r[0][c];
        y[2][c] = w[BT_BI + c] * r[2][c];
        y[1][c] = w[BT_DI + c] * z1[c];
    }
    blk_sub_mul<T, P>(w + BT_U, y[1], y[0]);
    blk_sub_mul<T, P>(w + BT_V, y[1], y[2]);
}

// ---- host-side factorisation (plan time, fp64)
struct Blk2 {   // one node block: axial scalar + 2x2
    double ax = 0.0, m[4] = {0.0, 0.0, 0.0, 0.0};
};
inline Blk2 b2_mul(const Blk2& a, const Blk2& b) {
    Blk2 r;
    r.ax = a.ax * b.ax;
    mul2(a.m, b.m, r.m);
    return r;
}
inline Blk2 b2_sub(const Blk2& a, const Blk2& b) {
    Blk2 r;
    r.ax = a.ax - b.ax;
    for (int k = 0; k < 4; ++k) r.m[k] = a.m[k] - b.m[k];
    return r;
}
inline Blk2 b2_inv(const Blk2& a) {
    Blk2 r;
    r.ax = 1.0 / a.ax;
    inv2(a.m, r.m);
    return r;
}
inline void b2_store(const Blk2& a, double* o) {
    o[0] = a.ax;
    for (int k = 0; k < 4; ++k) o[1 + k] = a.m[k];
}
inline Blk2 b2_diag(const NodeBlocks& n) { Blk2 r; r.ax = n.b_ax; for (int k = 0; k < 4; ++k) r.m[k] = n.B[k]; return r; }
inline Blk2 b2_left(const NodeBlocks& n) { Blk2 r; r.ax = n.a_ax; for (int k = 0; k < 4; ++k) r.m[k] = n.A[k]; return r; }
inline Blk2 b2_right(const NodeBlocks& n) { Blk2 r; r.ax = n.c_ax; for (int k = 0; k < 4; ++k) r.m[k] = n.C[k]; return r; }

// The interior constants of lane `l` of `blk` (the 256 node rows of M) into u[BU_N].
inline void blocked_lane_constants(const NodeBlocks* blk, int l, double* u) {
    const NodeBlocks* n = blk + BLK_NPL * l;
    const Blk2 B0 = b2_diag(n[0]), C0 = b2_right(n[0]), A1 = b2_left(n[1]), B1 = b2_diag(n[1]), C1 = b2_right(n[1]),
               A2 = b2_left(n[2]), B2 = b2_diag(n[2]);
    const Blk2 D0i = b2_inv(B0);
    const Blk2 L1 = b2_mul(A1, D0i);
    const Blk2 D1i = b2_inv(b2_sub(B1, b2_mul(L1, C0)));
    const Blk2 L2 = b2_mul(A2, D1i);
    const Blk2 D2i = b2_inv(b2_sub(B2, b2_mul(L2, C1)));
    const Blk2 U0 = b2_mul(D0i, C0), U1 = b2_mul(D1i, C1);
    std::memset(u, 0, sizeof(double) * BU_N);
    b2_store(L1, u + BU_L1); b2_store(L2, u + BU_L2);
    b2_store(D0i, u + BU_D0); b2_store(D1i, u + BU_D1); b2_store(D2i, u + BU_D2);
    b2_store(U0, u + BU_U0); b2_store(U1, u + BU_U1);
    // W_L = A_II^-1 [A_0; 0; 0] and W_R = A_II^-1 [0; 0; C_2], by the same elimination applied to block columns
    const Blk2 Afirst = b2_left(n[0]), Clast = b2_right(n[2]);
    {
        const Blk2 z0 = Afirst, z1 = b2_sub(Blk2(), b2_mul(L1, z0)), z2 = b2_sub(Blk2(), b2_mul(L2, z1));
        const Blk2 w2 = b2_mul(D2i, z2), w1 = b2_sub(b2_mul(D1i, z1), b2_mul(U1, w2)), w0 = b2_sub(b2_mul(D0i, z0), b2_mul(U0, w1));
        b2_store(w0, u + BU_WL); b2_store(w1, u + BU_WL + 5); b2_store(w2, u + BU_WL + 10);
    }
    {
        const Blk2 w2 = b2_mul(D2i, Clast), w1 = b2_sub(Blk2(), b2_mul(U1, w2)), w0 = b2_sub(Blk2(), b2_mul(U0, w1));
        b2_store(w0, u + BU_WR); b2_store(w1, u + BU_WR + 5); b2_store(w2, u + BU_WR + 10);
    }
    b2_store(b2_left(n[3]), u + BU_AS);
    b2_store(b2_right(n[3]), u + BU_CS);
}

// The mirror structure of lane `l`'s interior, bitwise: every B diagonal, every C = J A J, and the blocks that the twisted
// form takes as one (B0 = B2, A1 = A2, C0 = C1) equal.
inline bool blocked_lane_mirrored(const NodeBlocks* blk, int l) {
    const NodeBlocks* n = blk + BLK_NPL * l;
    for (int k = 0; k < 3; ++k) {
        const double jaj[4] = {n[k].A[0], -n[k].A[1], -n[k].A[2], n[k].A[3]};
        if (n[k].B[1] != 0.0 || n[k].B[2] != 0.0) return false;
        if (l == 0 && k == 0) continue;   // (the node at the fixed root has no left coupling; the form takes none of it)
        if (n[k].c_ax != n[k].a_ax) return false;
        for (int i = 0; i < 4; ++i)
            if (n[k].C[i] != jaj[i]) return false;
    }
    return n[0].b_ax == n[2].b_ax && n[0].B[0] == n[2].B[0] && n[0].B[3] == n[2].B[3] && n[1].a_ax == n[2].a_ax &&
           std::memcmp(n[1].A, n[2].A, sizeof(n[1].A)) == 0 && std::memcmp(n[0].C, n[1].C, sizeof(n[0].C)) == 0;
}
inline bool blocked_mirrored(const NodeBlocks* blk) {   // every lane of the 256 node rows
    for (int l = 0; l < BLK_LANES; ++l)
        if (!blocked_lane_mirrored(blk, l)) return false;
    return true;
}
// The twisted table of lane `l` (mirrored, above) into w[BT_TAB]; u: the lane's constants of blocked_lane_constants, whose
// W_L, W_R, A_s, C_s it carries over.
inline void blocked_twist_constants(const NodeBlocks* blk, int l, const double* u, double* w) {
    const NodeBlocks* n = blk + BLK_NPL * l;
    Blk2 Bi;   // B^-1, a diagonal's reciprocals
    Bi.ax = 1.0 / n[0].b_ax; Bi.m[0] = 1.0 / n[0].B[0]; Bi.m[3] = 1.0 / n[0].B[3];
    const Blk2 C0 = b2_right(n[0]), A1 = b2_left(n[1]), B1 = b2_diag(n[1]), C1 = b2_right(n[1]), A2 = b2_left(n[2]);
    const Blk2 Pm = b2_mul(A1, Bi), Qm = b2_mul(C1, Bi);
    // the off-diagonals of the two products are mirror images: they cancel, exactly so in Dc
    const Blk2 Dc = b2_sub(b2_sub(B1, b2_mul(Pm, C0)), b2_mul(Qm, A2));
    std::memset(w, 0, sizeof(double) * BT_TAB);
    b2_store(Pm, w + BT_P); b2_store(Qm, w + BT_Q);
    b2_store(b2_mul(Bi, C0), w + BT_U); b2_store(b2_mul(Bi, A2), w + BT_V);
    w[BT_BI] = Bi.ax; w[BT_BI + 1] = Bi.m[0]; w[BT_BI + 2] = Bi.m[3];
    w[BT_DI] = 1.0 / Dc.ax; w[BT_DI + 1] = 1.0 / Dc.m[0]; w[BT_DI + 2] = 1.0 / Dc.m[3];
    std::memcpy(w + BT_WL, u + BU_WL, sizeof(double) * 15);
    std::memcpy(w + BT_WR, u + BU_WR, sizeof(double) * 15);
    std::memcpy(w + BT_AS, u + BU_AS, sizeof(double) * BLK_PACK);
    std::memcpy(w + BT_CS, u + BU_CS, sizeof(double) * BLK_PACK);
}

// Builds the blocked solve's tables from the 256 node rows of M (Lc: the length that scales rotations in the level norms,
// as pick_levels uses).  u[BU_N]: the wave-uniform constants; sep[blk_sep_vals(BLK_MAX_LV)][64]: the separator tables of the
// returned level count (levels past it are left 0); norms[BLK_MAX_LV]: each level's largest multiplier.  Returns the
// separator levels the solve needs in fp64, or -1 when the interior constants are not bitwise uniform over the lanes.
// tw (optional): the twisted table [BT_TAB], for node blocks that are mirrored (blocked_mirrored).
inline int blocked_factor(const NodeBlocks* blk, double Lc, double* u, double* sep, double* norms, double* tw = nullptr) {
    blocked_lane_constants(blk, 1, u);
    double v[BU_N];
    for (int l = 0; l < BLK_LANES; ++l) {
        if (l == 1) continue;
        blocked_lane_constants(blk, l, v);
        // lane 0's W_L multiplies the fixed root (0); lane 63's C_s must be 0 (the tip)
        for (int k = 0; k < BU_N; ++k) {
            const bool skip = (l == 0 && k >= BU_WL && k < BU_WL + 15) || (l == BLK_LANES - 1 && k >= BU_CS && k < BU_CS + 5);
            if (!skip && std::memcmp(&v[k], &u[k], sizeof(double)) != 0) return -1;
            if (l == BLK_LANES - 1 && k >= BU_CS && k < BU_CS + 5 && v[k] != 0.0) return -1;
        }
    }
    if (tw) {
        blocked_twist_constants(blk, 1, u, tw);
        double x[BT_TAB];
        for (int l = 0; l < BLK_LANES; ++l) {   // (the interior blocks themselves, as the constants above)
            blocked_twist_constants(blk, l, u, x);
            if (std::memcmp(x, tw, sizeof(double) * BT_WL) != 0) return -1;
        }
    }
    // the separator Schur system, one row per lane:  -A_s W_L2 x_s(l-1) + (B_s - A_s W_R2 - C_s W_L0) x_s(l) - C_s W_R0 x_s(l+1)
    auto pk = [&](int off) { Blk2 r; r.ax = u[off]; for (int k = 0; k < 4; ++k) r.m[k] = u[off + 1 + k]; return r; };
    const Blk2 As = pk(BU_AS), WL0 = pk(BU_WL), WL2 = pk(BU_WL + 10), WR0 = pk(BU_WR), WR2 = pk(BU_WR + 10);
    NodeBlocks cur[BLK_LANES], nxt[BLK_LANES];
    for (int l = 0; l < BLK_LANES; ++l) {
        const NodeBlocks& s = blk[BLK_NPL * l + 3];
        const Blk2 Cs = b2_right(s);
        const Blk2 Bh = b2_sub(b2_sub(b2_diag(s), b2_mul(As, WR2)), b2_mul(Cs, WL0));
        const Blk2 Ah = l > 0 ? b2_sub(Blk2(), b2_mul(As, WL2)) : Blk2();
        const Blk2 Ch = l + 1 < BLK_LANES ? b2_sub(Blk2(), b2_mul(Cs, WR0)) : Blk2();
        NodeBlocks& o = cur[l];
        o.a_ax = Ah.ax; o.b_ax = Bh.ax; o.c_ax = Ch.ax;
        for (int k = 0; k < 4; ++k) { o.A[k] = Ah.m[k]; o.B[k] = Bh.m[k]; o.C[k] = Ch.m[k]; }
    }
    static_assert(BLK_MAX_LV * PCR_LEVEL_VALS + BLK_PACK == blk_sep_vals(BLK_MAX_LV), "separator table size");
    std::memset(sep, 0, sizeof(double) * size_t(blk_sep_vals(BLK_MAX_LV)) * BLK_LANES);
    // every level's multipliers and rows; the count is decided afterwards, the final inverse is of the rows after it
    std::vector<NodeBlocks> rowbuf(size_t(BLK_MAX_LV + 1) * BLK_LANES);
    auto rows = [&](int lv) { return rowbuf.data() + size_t(lv) * BLK_LANES; };
    std::memcpy(rows(0), cur, sizeof(cur));
    std::vector<double> lvbuf(size_t(BLK_MAX_LV) * BLK_LANES * PCR_LEVEL_VALS);
    auto lvv = [&](int lv, int l) { return lvbuf.data() + (size_t(lv) * BLK_LANES + l) * PCR_LEVEL_VALS; };
    for (int lv = 0; lv < BLK_MAX_LV; ++lv) {
        const int st = 1 << lv;
        norms[lv] = 0.0;
        for (int l = 0; l < BLK_LANES; ++l) {
            const bool lo = l - st >= 0, hi = l + st < BLK_LANES;
            PcrLevel P;
            pcr_factor_level(rows(lv)[l], rows(lv)[lo ? l - st : l], lo, rows(lv)[hi ? l + st : l], hi, P, nxt[l]);
            const double n = pcr_level_norm(P, Lc);
            norms[lv] = n > norms[lv] ? n : norms[lv];
            double* o = lvv(lv, l);
            o[0] = P.al_ax; o[1] = P.ga_ax;
            for (int k = 0; k < 4; ++k) { o[2 + k] = P.al[k]; o[6 + k] = P.ga[k]; }
        }
        std::memcpy(rows(lv + 1), nxt, sizeof(nxt));
    }
    int used = BLK_MAX_LV;
    while (used > 0 && norms[used - 1] < std::ldexp(1.0, -53)) --used;
    for (int lv = 0; lv < used; ++lv)
        for (int l = 0; l < BLK_LANES; ++l)
            for (int k = 0; k < PCR_LEVEL_VALS; ++k) sep[size_t(lv * PCR_LEVEL_VALS + k) * BLK_LANES + l] = lvv(lv, l)[k];
    for (int l = 0; l < BLK_LANES; ++l) {
        const Blk2 fin = b2_inv(b2_diag(rows(used)[l]));
        double f[BLK_PACK];
        b2_store(fin, f);
        for (int k = 0; k < BLK_PACK; ++k) sep[size_t(used * PCR_LEVEL_VALS + k) * BLK_LANES + l] = f[k];
    }
    return used;
}

// Host restatement of the kernel's solve (fp64, lanes run one after another; a lane shift past the wave's end reads 0, as
// the DPP moves with bound_ctrl do): x = M^-1 r for r, x of [256][3].  The test suite checks it against a dense solve.
// tw: the twisted table, for the interiors solved about their centre nodes (CRB_BLK_TWIST) instead of by block Thomas.
inline void blocked_solve_host(const double* u, const double* sep, int levels, const double* r, double* x, const double* tw = nullptr) {
    double y[BLK_LANES][3][3], g[BLK_LANES][3];
    for (int l = 0; l < BLK_LANES; ++l) {
        double ri[3][3];
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) ri[k][c] = r[(BLK_NPL * l + k) * 3 + c];
        if (tw) blk_twist_interior_solve<double>(tw, ri, y[l]);
        else blk_interior_solve<double>(u, ri, y[l]);
    }
    for (int l = 0; l < BLK_LANES; ++l) {
        const double zero[3] = {0.0, 0.0, 0.0};
        const double* y0r = l + 1 < BLK_LANES ? y[l + 1][0] : zero;
        for (int c = 0; c < 3; ++c) g[l][c] = r[(BLK_NPL * l + 3) * 3 + c];
        blk_sub_mul<double>(u + BU_AS, y[l][2], g[l]);
        blk_sub_mul<double>(u + BU_CS, y0r, g[l]);
    }
    for (int lv = 0; lv < levels; ++lv) {
        const int st = 1 << lv;
        double ng[BLK_LANES][3];
        for (int l = 0; l < BLK_LANES; ++l) {
            double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0}, cf[PCR_LEVEL_VALS];
            for (int c = 0; c < 3; ++c) {
                if (l - st >= 0) lo[c] = g[l - st][c];
                if (l + st < BLK_LANES) hi[c] = g[l + st][c];
                ng[l][c] = g[l][c];
            }
            for (int k = 0; k < PCR_LEVEL_VALS; ++k) cf[k] = sep[size_t(lv * PCR_LEVEL_VALS + k) * BLK_LANES + l];
            pcr_apply_level<double>(cf, lo, hi, ng[l]);
        }
        std::memcpy(g, ng, sizeof(g));
    }
    double xs[BLK_LANES][3];
    for (int l = 0; l < BLK_LANES; ++l) {
        double f[BLK_PACK];
        for (int k = 0; k < BLK_PACK; ++k) f[k] = sep[size_t(levels * PCR_LEVEL_VALS + k) * BLK_LANES + l];
        pcr_apply_final<double>(f, g[l], xs[l]);
    }
    for (int l = 0; l < BLK_LANES; ++l) {
        const double zero[3] = {0.0, 0.0, 0.0};
        const double* xl = l > 0 ? xs[l - 1] : zero;
        for (int k = 0; k < 3; ++k) {
            double* o = x + (BLK_NPL * l + k) * 3;
            for (int c = 0; c < 3; ++c) o[c] = y[l][k][c];
            blk_sub_mul<double>(u + BU_WL + 5 * k, xl, o);
            blk_sub_mul<double>(u + BU_WR + 5 * k, xs[l], o);
        }
        for (int c = 0; c < 3; ++c) x[(BLK_NPL * l + 3) * 3 + c] = xs[l][c];
    }
}

}  // namespace crb
