// crb_lean.h -- the lean kernels: fused multi-step RK4 stepper (the headline path), lean RHS, one-stage kernel
// of the stage-split stepper.  Register-resident solve tables, merged exchange rounds, DPP lane shifts.
#pragma once
#include <hip/hip_runtime.h>

#include "crb_blocked.h"
#include "crb_generic.h"

namespace crb {

// ------------------------------------------------------------------ lean fused stepper
// crb_step_lean_kernel: the stepper for plans without gravity and calls without a held input
// (BASELINE configs 3/4), one beam per workgroup of NW = 2^LOGNW waves, everything compile-time:
//   * exchange rounds merged.  Positions of the NEXT stage are known when a stage starts
//     (q_next = x_q + c*v_stage), so they ride on this stage's force exchange instead of costing a
//     round of their own; the force exchange itself is merged with cyclic-reduction level 0: a
//     thread publishes {q_next, p = u - f_right + drag, f_left} once and rebuilds r of both
//     neighbours from what it reads (r_{i-1} = p_{i-1} - f_left_i, r_{i+1} = p_{i+1} - f_left_{i+2}).
//     Rounds per RHS: 1 + (LV-1) instead of 2 + LV; barriers: max(LOGNW,1) [0 for one wave].
//   * round A moves 16-byte LDS words (record = 10 fp64 / 12 fp32 values per thread, padded so
//     that ds_read/write_b128 are bank-conflict free); lane +-1 shifts use DPP wave_shr/wave_shl
//     (no LDS round trip), larger lane shifts ds_bpermute.
template <typename T>
struct LeanRec {                    // fp32: [qn0 qn1 qn2 - | p0 p1 p2 - | fl0 fl1 fl2 -]   (fp64: columns, see the stepper)
    static constexpr int N = sizeof(T) == 8 ? 10 : 12;   // 80 B / 48 B: conflict-free 16-byte accesses
    static constexpr int V = 16 / sizeof(T);              // values per 16-byte LDS word
};
template <typename T>
__host__ __device__ constexpr size_t lean_lds_bytes(int NT, int lognw) {
    // round A records (+1 all-zero "no neighbour" record; double-buffered when round A is the only
    // barrier round) + SoA buffers (+1 zero column) of the cross-wave levels 1..lognw-1
    // (fp32: the cross-wave levels move one 16-byte record [r0 r1 r2 -] per thread instead of three 4-byte columns)
    return sizeof(T) * (size_t(NT + 1) * LeanRec<T>::N * (lognw == 1 ? 2 : 1) +
                        (sizeof(T) == 4 ? 4 : 3) * size_t(NT + 1) * size_t(lognw > 1 ? lognw - 1 : 0));
}

// wave_shr:1 / wave_shl:1 with bound_ctrl: a lane without a source lane reads 0 and no "old" value has
// to be materialised first (update_dpp(0, ..) costs one extra v_mov per DPP).
__device__ __forceinline__ double dpp_from_lower(double x) {  // value held by lane-1 (0 into lane 0)
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x138, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double dpp_from_higher(double x) {  // value held by lane+1 (0 into lane 63)
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x130, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float dpp_from_lower(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_from_higher(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x130, 0xf, 0xf, true));
}
// Value of lane-D / lane+D of the same wave.  D <= DPP_MAX: chained DPP wave shifts (VALU, no
// LDS round trip; lanes shifted in from outside the wave read 0).  Larger D: ds_bpermute; a lane
// index outside the wave wraps to some lane of the SAME beam -- callers only ever multiply such
// a value by a multiplier that is exactly 0 (no neighbour at that stride).
constexpr int LEAN_DPP_MAX = 4;   // lane shifts up to this distance are chained DPP moves, larger ones ds_bpermute
// wave priorities per phase of a stage (s_setprio; -1 = leave unchanged): element force 0, exchanges and the cross-wave
// level 2, in-wave levels 1 -- the two workgroups of a CU then interleave force arithmetic with the other's exchange
// latency (+10 %).  fp32 plans (four waves per SIMD, LDS-issue-limited) want the priority to RISE through the stage and
// drop at its end (config 4: +3.7 % over the fp64 values; the fp64 stepper is indifferent to those or slower).
constexpr int P_FORCE = 0, P_XCHG = 2, P_L1 = -1, P_TAIL = 1, P_FIN = -1;
constexpr int P32_L1 = 3, P32_TAIL = 3, P32_FIN = 0;
#define CRB_SETPRIO(v) do { if ((v) >= 0) __builtin_amdgcn_s_setprio((v) < 0 ? 0 : (v)); } while (0)
template <typename T, int D>
__device__ __forceinline__ T lane_lower(T x, int lane) {
    if (D <= LEAN_DPP_MAX) {
#pragma unroll
        for (int i = 0; i < D; ++i) x = dpp_from_lower(x);
        return x;
    }
    return __shfl(x, lane - D, 64);
}
template <typename T, int D>
__device__ __forceinline__ T lane_higher(T x, int lane) {
    if (D <= LEAN_DPP_MAX) {
#pragma unroll
        for (int i = 0; i < D; ++i) x = dpp_from_higher(x);
        return x;
    }
    return __shfl(x, lane + D, 64);
}

// Reduction levels 1..LV-1 and the final block inverse of the lean kernels, given r after level 0.
// Levels whose stride stays inside the workgroup's waves-per-beam interleave (l < LOGNW) go through LDS
// columns + a barrier, the others are in-wave lane shifts.  A missing neighbour contributes through a
// multiplier that is exactly 0, so whatever finite value the shift returns there is harmless.
// ISOLATE (packed beams: several beams share the wave): what a lane shift drags across a beam boundary is replaced
// by 0 with a select -- a multiplier of exactly 0 would turn a neighbouring beam's Inf/NaN into NaN here, and
// the reference's beams are independent (a diverged beam must not take its wave-mates with it).
// RECB (fp32 stepper): a cross-wave level is ONE 16-byte store and two 16-byte loads per thread instead of 3 + 6
// 4-byte ones -- the fp32 stepper runs four waves per SIMD and is limited by LDS instruction issue, not by bytes.
template <typename T, int LV, int LOGNW, bool ISOLATE = false, bool RECB = false>
__device__ __forceinline__ void lean_reduce_tail(const SolveCoef<T, LV>& cf, T* ldsB, int t, int lane, int j, int S,
                                                 bool valid, T r[3], T a[3]) {
    constexpr int NW = 1 << LOGNW, NT = 64 << LOGNW, NULLT = NT;
    auto thread_of = [](int jj) { return ((jj & (NW - 1)) << 6) | (jj >> LOGNW); };
    T rlo[3], rhi[3];
#pragma unroll
    for (int l = 1; l < LV; ++l) {
        if (l < LOGNW) {  // another wave holds the neighbour: LDS + barrier
            if (l == 1) CRB_SETPRIO(sizeof(T) == 4 ? P32_L1 : P_L1);
            const int st = 1 << l;
            const int tl = (valid && j - st >= 0) ? thread_of(j - st) : NULLT;
            const int th = (valid && j + st < S) ? thread_of(j + st) : NULLT;
            if constexpr (RECB) {
                typedef T rec4 __attribute__((ext_vector_type(4)));
                rec4* buf = reinterpret_cast<rec4*>(ldsB) + size_t(l - 1) * (NT + 1);
                buf[t] = rec4{r[0], r[1], r[2], T(0)};
                __syncthreads();
                const rec4 lo = buf[tl], hi = buf[th];
#pragma unroll
                for (int c = 0; c < 3; ++c) { rlo[c] = lo[c]; rhi[c] = hi[c]; }
            } else {
                T* buf = ldsB + size_t(l - 1) * 3 * (NT + 1);
                buf[t] = r[0]; buf[(NT + 1) + t] = r[1]; buf[2 * (NT + 1) + t] = r[2];
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 3; ++c) { rlo[c] = buf[c * (NT + 1) + tl]; rhi[c] = buf[c * (NT + 1) + th]; }
            }
        } else {
            if (l == LOGNW) CRB_SETPRIO(sizeof(T) == 4 ? P32_TAIL : P_TAIL);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                switch (l - LOGNW) {
                    case 0: rlo[c] = lane_lower<T, 1>(r[c], lane); rhi[c] = lane_higher<T, 1>(r[c], lane); break;
                    case 1: rlo[c] = lane_lower<T, 2>(r[c], lane); rhi[c] = lane_higher<T, 2>(r[c], lane); break;
                    case 2: rlo[c] = lane_lower<T, 4>(r[c], lane); rhi[c] = lane_higher<T, 4>(r[c], lane); break;
                    case 3: rlo[c] = lane_lower<T, 8>(r[c], lane); rhi[c] = lane_higher<T, 8>(r[c], lane); break;
                    case 4: rlo[c] = lane_lower<T, 16>(r[c], lane); rhi[c] = lane_higher<T, 16>(r[c], lane); break;
                    default: rlo[c] = lane_lower<T, 32>(r[c], lane); rhi[c] = lane_higher<T, 32>(r[c], lane); break;
                }
            }
            if (ISOLATE) {
                const int st = 1 << l;
                const bool lo_ok = valid && j - st >= 0, hi_ok = valid && j + st < S;
#pragma unroll
                for (int c = 0; c < 3; ++c) { rlo[c] = lo_ok ? rlo[c] : T(0); rhi[c] = hi_ok ? rhi[c] : T(0); }
            }
        }
        pcr_apply_level<T>(cf.lv[l], rlo, rhi, r);
    }
    CRB_SETPRIO(sizeof(T) == 4 ? P32_FIN : P_FIN);
    pcr_apply_final<T>(cf.fin, r, a);
}

template <typename T, int LV, int LOGNW, int EM>
__device__ __forceinline__ void lean_rhs(const ElemCoef<T>& ec, T dragc, bool corrected, const SolveCoef<T, LV>& cf, T* lds3, int t,
                                         int lane, int j, int S, bool valid, const T sq[3], const T sv[3], const T uadd[3], T a[3]) {
    constexpr int NW = 1 << LOGNW, NT = 64 << LOGNW, NULLT = NT;
    T* const ldsQ = lds3;                           // [3][NT+1]  stage positions
    T* const ldsA = lds3 + 3 * size_t(NT + 1);      // [6][NT+1]  p0..2, fl0..2
    T* const ldsB = lds3 + 9 * size_t(NT + 1);      // [LOGNW-1][3][NT+1]
    auto thread_of = [](int jj) { return ((jj & (NW - 1)) << 6) | (jj >> LOGNW); };
    const int t_l1 = (valid && j >= 1) ? thread_of(j - 1) : NULLT;
    const int t_r1 = (valid && j + 1 < S) ? thread_of(j + 1) : NULLT;
    const int t_r2 = (valid && j + 2 < S) ? thread_of(j + 2) : NULLT;
    // -- the left neighbour's position (its own exchange: stage states are arbitrary combinations here)
    T qL[3];
    if (LOGNW == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) qL[c] = lane_lower<T, 1>(sq[c], lane);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) ldsQ[size_t(c) * (NT + 1) + t] = sq[c];
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) qL[c] = ldsQ[size_t(c) * (NT + 1) + t_l1];
    }
    T fl[3], fr[3];
    if (EM == EM_NONLINEAR) elem_force_nonlinear<T>(ec.c, qL, sq, false, fl, fr);
    else if (EM == EM_LINEAR) elem_force_linear<T>(ec.c, qL, sq, fl, fr);
    else elem_force<T>(ec, qL, sq, corrected, fl, fr);
    T pp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pp[c] = uadd[c] - fr[c];
    pp[1] += drag_force<T>(dragc, sv[1]);
    // -- merged exchange round {p, fl} + level 0.  The barrier of the q exchange above orders the previous
    //    call's reads of these columns before this call's writes (and vice versa for the q columns).
    T r[3], rlo[3], rhi[3];
    if (LOGNW == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r[c] = pp[c] - lane_higher<T, 1>(fl[c], lane);   // (one wave: r first, then ITS neighbours -- see the stepper)
            rlo[c] = lane_lower<T, 1>(r[c], lane);
            rhi[c] = lane_higher<T, 1>(r[c], lane);
        }
    } else {
        auto col = [&](int k, int th) -> T& { return ldsA[size_t(k) * (NT + 1) + th]; };
#pragma unroll
        for (int c = 0; c < 3; ++c) { col(c, t) = pp[c]; col(3 + c, t) = fl[c]; }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rlo[c] = col(c, t_l1) - fl[c];
            r[c] = pp[c] - col(3 + c, t_r1);
            rhi[c] = col(c, t_r1) - col(3 + c, t_r2);
        }
    }
    pcr_apply_level<T>(cf.lv[0], rlo, rhi, r);
    lean_reduce_tail<T, LV, LOGNW>(cf, ldsB, t, lane, j, S, valid, r, a);
}

// ------------------------------------------------------------------ register-blocked lean stepper (NPL = 4)
// crb_step_lean_kernel<double, LS, 2, false, EM, false, false, false, 4>: fp64 beams of exactly 256 slots with one table set
// and one element kind whose mass matrix is uniform (crbeam.hip: blocked_step_ok).  One WAVE per beam, lane l owning slots
// 4l .. 4l+3: the mass solve and the exchanges scale with the lane boundaries, not with the nodes (crb_blocked.h):
//   exchanges per stage: q of lane-1's last node (the next stage's rides on this one), the left half of the lane's first element
//   back to lane-1, y_0 of lane+1, the separator levels at lane strides 1 and 2 and x_s of lane-1 by DPP lane shifts; the third
//   separator level (stride 4) through the wave's own LDS strip [3][4 + 64 + 4] (3 ds_write_b64 + 6 ds_read_b64 at immediate
//   offsets instead of 24 DPP moves; the pads, zeroed once, are the 0 that a bound_ctrl shift brings in past the root and the
//   tip, so the results are bitwise those of the shifts).  No barrier in the step loop: a wave's LDS accesses execute in order.
//   A workgroup is four independent beam walkers.  The first two rounds are off the stage's dependent chain, and were still
//   slower through strips of their own (3 ds_write_b64 + 3 ds_read_b64 each, at -1 / +1 column, reads behind the writes;
//   measured, DESIGN.md §4, three rounds: +0.15 .. 0.18 us per step for the q round alone, +0.12 .. 0.24 for the left half
//   alone, +0.36 .. 0.46 for both, with 24 / 24 / 48 v_mov_b32_dpp fewer per step): not taken.
// The solve's 75 wave-uniform constants (the interior's factors, W_L / W_R, A_s / C_s) sit in five fp64 registers per lane,
// loaded once per launch: constant k in lane k % 16 of every 16-lane row of register k / 16 (crb_blocked.h: BLK_TAB_*).  The 66
// multiply-adds per stage that use one take it as the DPP row-broadcast source of v_fmac_f64 (blk_bc_fma / blk_bc_fnma: no
// load, no SGPR, no wait); the nine products that head a sum multiply by a copy made before the walk loop (blk_bc_copy, 18
// registers).  Read as scalar loads pack by pack they were 31 of the stage's 38 s_load and 15 of its 21 full lgkmcnt(0) drains,
// each exposing most of a scalar load's latency on the wave's serial chain; held in SGPRs they overflow the scalar file.  Each sum keeps
// the order the compiler gave the scalar-operand form, so the results are bitwise those of blk_interior_solve's roundings.
// Checked in the ISA of this kernel (a DPP inside asm gets no wait states from the compiler): the five table pairs and the
// nine copies are written by nothing but their loads / moves ahead of the walk loop; no VALU instruction of the step loop
// writes EXEC (no v_cmpx, no v_readlane into it); the step loop has 264 v_fmac_f64_dpp per step and no scalar load of the table.
// The element pack, the drag factor and the launch parameters stay scalar loads through the kernarg pointer laundered per
// stage (they feed VOP3 instructions); the per-lane separator tables sit in LDS (shared by the four waves, [value pair][lane]
// records) and are read level by level.  LS = separator levels.
// Measured at 4096 x 256: 549 vector instructions per beam and stage against 868 (4 waves x 217), 16.3 against
// 27.1 us per step with every level by DPP; the strip takes that to 501 and 16.53 to 16.15 us per step (strides 2 and 4 through
// the strip: 477 and 16.17).  The impulse behind scalar branches instead of a selector FMA per component, and RK4 sums started by
// stage 0: 410 -> 393 executed fp64 instructions per stage, no SGPR spill left (52 before), 16.25 -> 15.41 us per step (the shipped
// library against its parent's, one box, alternating); 210 VGPRs, no scratch, two waves per SIMD.  DESIGN.md §4 has the
// stage's fp64 budget per phase.  The uniform constants as row broadcasts and the first level's table read under the interior
// solve: 38 -> 7.5 scalar loads and 21 -> 6.5 full drains per stage, 238 VGPRs, 15.21 -> 15.00 us per step (-1.35 %; the
// broadcasts alone -0.7 %), outputs bitwise equal (DESIGN.md §4 has the probe of the instruction and the variants).
// The nonlinear instance takes the element's axial pair regrouped (crb_math.h: elem_force_nonlinear_regrouped): an element
// hands out f2 = cA1 E and cA1 W with f1 + f2 = cA1 W, a node's axial right-hand side is (f2(k+1) - f2(k)) - cA1 W(k+1), and
// only the lane's first element forms f1 = cA1 W - f2 itself, for lane-1's last node.  10 fp64 instructions per element and
// node instead of 14 in the source, 1617 -> 1557 emitted per step (15 per stage), 240 VGPRs, 98 SGPRs, no spill, no scratch;
// the roundings of the axial right-hand side change in order (not in number or size), so this instance is no longer bitwise
// its parent's -- it agrees with it, with the one-node-per-lane stepper and with the oracle to rounding (DESIGN.md §4 has
// the figures).  The linear instance and every other kernel keep their code line for line.
// The element polynomials are evaluated in chord-relative variables (crb_math.h: elem_force_nonlinear_chord; e = s - 2 dw,
// d, dw, L du: the monomials that cancel between s^2, p and s dw are never formed), and RK4 carries the positions on the
// accelerations (crb_math.h: Rk4Pos): q_2 and q + dt v at the top of stage 0, then one multiply-add of dt^2/4, dt^2/2, dt^2/6
// times the stage's acceleration per position, so the stage velocities of u and phi and the sum accq are gone; the drag's
// stage velocity of w is the only one formed, and the next stage's positions are known at the top of each stage as before
// (the last node's still rides the q exchange).  The state between steps is (xq, xv) and nothing else, unscaled, so chunked
// launches stay bitwise.  1557 -> 1498 fp64 instructions per step (chord forces alone 1513, the RK4 form alone 1542), VALU
// 2101 -> 2032, 250 VGPRs, 90 SGPRs, no spill, no scratch; the linear instance takes the RK4 form too (238 VGPRs, 58 SGPRs).
// Outputs agree with the parent's to rounding.  CRB_BLK_CHORD / CRB_BLK_RK4_POS (=0 in the tuning build)
// switch either item off for timing.
// The nonlinear instance evaluates the element polynomials with the pack's prefactors folded into their coefficients
// (crb_math.h: elem_force_nonlinear_folded): the blocked stepper only takes plans of 256 equal elements, so phi L, L du, 3 e
// and the products with cA1, cA3, cD3, cA4, cD4 are one number per plan, multiplied into 30 constants when the plan is built
// (elem_fold_build, each rounded once) and stored behind the blocked tables (crb_blocked.h: blk_fold_offset).  A stage reads
// them as scalar loads in the batch that read the element pack, which they replace (three s_load_dwordx16, one x8, one x4
// under the stage's one wait; the four constants that head a sum take a v_mov_b64 each per stage, since an instruction has one
// scalar operand).  41 fp64 instructions per element; 1498 -> 1386 per step (add +48: sigma and delta are additions now,
// phi L +- was fused; mul -112, FMA -48), VALU 2032 -> 1928, 256 VGPRs, 100 SGPRs, no spill, no scratch, two waves per SIMD;
// the compiler no longer holds the chord form's rationals in SGPR pairs across the loop.  Outputs agree with the parent's to
// rounding (DESIGN.md §4 has the timings of this build, of its parent and of the tuning build with CRB_BLK_FOLD=0, the chord
// form, and the counters).  The linear instance is untouched.
// The folded polynomials now share the membrane strain's two combinations (crb_math.h: elem_force_nonlinear_shared): the du
// and dw^2 coefficients of f2, of both factors of f3, of X's eps factor and of Rf are pairwise proportional, so A1 = dw^2 - 2 L du
// and A2 = dw^2 - (2 L / 3) du are formed once per element (one multiply-add each) and the five sums lose a term each: 38
// fp64 instructions per element against 41, 27 plan constants (elem_share_build, behind the folded ones: crb_blocked.h,
// blk_share_offset) against 30; 1386 -> 1338 fp64 instructions per step, VALU 1928 -> 1880.  u2 LT is contracted into the
// axial right-hand side's subtractions (no bare multiply is left of it).  The five sums of two products are explicit fused
// multiply-adds, so that their roundings do not depend on the code around the call.
// The constants are requested ONE STAGE AHEAD (CRB_BLK_CONST_AHEAD): once before the step loop, then after each stage's
// right-hand side for the next stage (stage 3: for the next step's stage 0), where the last instruction that reads them is
// behind and the whole mass solve and the RK4 ends, which need no scalar register, lie ahead; they land under the solve's
// first LDS wait instead of being waited for at the stage's top.  With that, what else a stage read at its top -- the
// impulse window's end and component, the drag factor, the constants' address -- is read once per beam and held over the
// step loop (CRB_BLK_HOLD_PARAMS): seven scalar registers, live in the force block either way, which is where the scalar
// file is fullest.  A stage's top has no scalar load and no wait: per step 87 -> 71 s_load (20 of them the four requests),
// 108 -> 95 s_waitcnt, 256 VGPRs, 97 SGPRs, no spill, no scratch, two waves per SIMD.  The values are the same numbers, so
// the outputs are bitwise those of a build with both switches off (checked with bench.py --dump-outputs).  DESIGN.md §4
// has the timings of the four variants, of this build and of its parent, and the counters.  CRB_BLK_SHARE /
// CRB_BLK_CONST_AHEAD / CRB_BLK_HOLD_PARAMS (=0 in the tuning build) switch each off; with all three off the unit's
// code is the parent's line for line.
// Two pieces of the stage's vector work that is no arithmetic are gone, neither changing a computed value.
// CRB_BLK_F3_PLUS: the right transverse half is carried as +f3 through the impulse block (its dof-1 line adds amp; (f3 + amp)
// is exactly -(-f3 - amp)) instead of being stored as -f3 -- an in/out operand of the block, so the negation was materialised
// as a v_xor_b32 and a v_mov_b32 per node -- and negated again in the right-hand side; node k's transverse right-hand side
// stands directly behind its block, as the last reader of the f3 that the next block takes in/out, so that no copy is made
// either.  CRB_BLK_SEP_ADDR: the separator tables are read at immediate offsets from this lane's LDS byte address, formed once
// per launch and laundered in place per level, instead of through a laundered lane index that was scaled again at every level.
// Step loop of the tuning build, per step (parent / F3_PLUS alone / SEP_ADDR alone / both): VALU 1634 / 1602 / 1614 / 1582,
// v_xor_b32 16 / 0 / 16 / 0, v_mov_b32_e32 20 / 4 / 16 / 0, v_lshl_add_u32 16 / 16 / 0 / 0, fp64 1322 and v_mov_b32_dpp 240 in
// each; VGPRs 256 / 252 / 256 / 252, 103 SGPRs as the assembler totals them, no spill, no scratch.  The linear instance: VALU 1198
// -> 1146 (v_xor_b32 20 -> 4, v_mov_b32_e32 24 -> 4, v_lshl_add_u32 16 -> 0), fp64 893 and its mix unchanged, 238 -> 236 VGPRs.
// Measured (tuning builds, one box, alternating, three rounds): 12.121 / 12.125 / 12.106 us per step with neither,
// 12.083 / 12.116 / 12.071 and 12.092 / 12.089 / 12.078 with one, 12.032 / 12.041 / 12.023 with both: -0.7 % for the pair, which
// is more than three round-to-round spreads; either item alone is not.  The whole library against its parent's on another
// box: 12.167 / 12.187 / 12.191 against 12.263 / 12.301 / 12.260 (-0.8 %, below in every round, short of three of the parent's
// spreads there), 13.55 against 13.79 at 20 steps per launch, 1.206 against 1.222 ms per 100-step launch in the kernel trace:
// about a fifth of what 52 of 1634 issue slots project.  Outputs are bitwise the parent's, config 3 (state and
// clock) and the linear instance.  With both switches off (=0 in the tuning build) the unit's code is the parent's line for line.
// Two changes that rest on the mirror symmetry of a mass matrix of equal elements and on the linearity of the separator's
// right-hand side; both change roundings, neither the number of fp64 operations outside the interior solve.
// CRB_BLK_TWIST (crb_blocked.h): a lane's nodes 0 and 2 are eliminated into its centre node instead of swept 0 -> 1 -> 2 and back:
// every interior B is diagonal, C = J A J, so the centre pivot is diagonal too and the solve is 29 fp64 instructions of depth
// three against 35 of depth five, with six broadcast copies (B^-1, Dc^-1) against nine.  It is the instance TW = true
// (crb_step_lean_twist_kernel), which a plan runs when its node blocks have the structure bitwise; the device assembly leaves a
// rounding residue in B's off-diagonals at some element lengths (0.3 / 256 and 0.0731 / 256 among the suite's; 0.25 / 256 and
// 1 / 256 have none), and those plans run TW = false.  crb_plan_get_blocked_form reports the choice.
// CRB_BLK_ONE_RIGHT: the left halves of lane+1's first element enter nothing but the separator's right-hand side g, as C_s y_0 of
// lane+1 does, so lane+1 forms h = fl[0] + C_s y_0 (the same five multiply-adds, on fl[0] instead of on g) and ONE shift brings
// hR: g = (-fr[3] [+ drag]) - A_s y_2 - hR.  The impulse on the axial dof of a lane's last node lands on the local f2(3); the
// axial and moment components of g's local part are carried negated until the subtraction of hR, where the sign is a source
// modifier (formed as -fr they cost a v_xor_b32 each).  Lane 63 is shifted a 0, as before.
// Step loop of the tuning build, per step (neither / TWIST alone / ONE_RIGHT alone / both): VALU 1582 / 1558 / 1562 / 1538, fp64
// 1322 / 1298 / 1322 / 1298 (v_fmac_f64_dpp 264 / 240 / 264 / 240, every other fp64 opcode unchanged), v_mov_b32_dpp 240 / 240 /
// 216 / 216, v_mov_b64 17 / 17 / 21 / 21, s_waitcnt 52 / 50 / 51 / 48, s_nop 25 / 27 / 30 / 29, LDS and scalar loads unchanged;
// VGPRs 252 / 246 / 252 / 246, 103 SGPRs, no spill, no scratch, two waves per SIMD.  (Counted from the step loop's header label
// to its backward branch, which gives the s_waitcnt 52 and s_nop 25 that DESIGN.md §4 records for the parent; "neither" is the
// parent's assembly byte for byte.)
// The linear instance takes neither (taken, it has VALU 1146 -> 1102, fp64 893 -> 869, 236 -> 228 VGPRs): its output is held to
// its parent's bit for bit by the suite (tests/test_blocked_folded_forces.py), so its code stays line for line.  With both
// switches off (=0 in the tuning build) the unit's code is the parent's line for line.  DESIGN.md §4 has the timings.
// The next beam's state is not prefetched as in the one-node-per-lane
// form: four nodes' records are 48 more registers than the budget of two waves per SIMD holds.
#ifndef CRB_BLK_CHORD
#define CRB_BLK_CHORD 1
#endif
#ifndef CRB_BLK_FOLD
#define CRB_BLK_FOLD 1
#endif
#ifndef CRB_BLK_SHARE
#define CRB_BLK_SHARE 1
#endif
#ifndef CRB_BLK_CONST_AHEAD
#define CRB_BLK_CONST_AHEAD 1
#endif
#ifndef CRB_BLK_HOLD_PARAMS
#define CRB_BLK_HOLD_PARAMS 1
#endif
#ifndef CRB_BLK_RK4_POS
#define CRB_BLK_RK4_POS 1
#endif
#ifndef CRB_BLK_F3_PLUS
#define CRB_BLK_F3_PLUS 1
#endif
#ifndef CRB_BLK_SEP_ADDR
#define CRB_BLK_SEP_ADDR 1
#endif
#ifndef CRB_BLK_ONE_RIGHT
#define CRB_BLK_ONE_RIGHT 1
#endif
constexpr int BLK_STRIP_PAD = 4;   // the stride of the separator level that goes through the wave's LDS strip (the third)
constexpr int BLK_STRIP_W = BLK_STRIP_PAD + BLK_LANES + BLK_STRIP_PAD;
// dynamic LDS of the blocked stepper: the separator tables (value pairs per lane), then per wave a strip [3][W] of fp64
__host__ __device__ constexpr size_t blk_lds_bytes(int ls) {
    return size_t(blk_sep_vals(ls) + 1) / 2 * 2 * BLK_LANES * sizeof(double) + size_t(4) * 3 * BLK_STRIP_W * sizeof(double);
}
// TW: the instance whose interiors are solved about their centre nodes (crb_step_lean_twist_kernel below; plans whose node
// blocks have the mirror structure, crb_blocked.h: blocked_mirrored)
template <typename T, int LS, int EM, bool TW, typename KPT>
__device__ __forceinline__ void lean_blocked_body(KPT kp) {
    static_assert(sizeof(T) == 8, "the blocked stepper is fp64");
    static_assert(LS == 3 && (1 << (LS - 1)) == BLK_STRIP_PAD, "the strip carries the third separator level, stride 4");
    constexpr int NP = BLK_NPL, NV = blk_sep_vals(LS), NV2 = (NV + 1) / 2;
    // the nonlinear element's axial pair regrouped (crb_math.h: elem_force_nonlinear_regrouped), 10 fp64 instructions per element
    // and node instead of 14; the literal polynomial (-DCRB_LITERAL_POLY=1) has no such form
    constexpr bool REGROUP = EM == EM_NONLINEAR && !CRB_LITERAL_POLY;
    // tuning-build switches (make fast EXTRA=-D...=0): the chord-relative element polynomials (crb_math.h:
    // elem_force_nonlinear_chord) instead of elem_force_nonlinear_regrouped, and the RK4 positions carried on the
    // accelerations (crb_math.h: Rk4Pos) instead of on stage velocities of every component
    constexpr bool CHORD = CRB_BLK_CHORD, RKPOS = CRB_BLK_RK4_POS;
    // the element polynomials with the pack's prefactors folded into their coefficients (crb_math.h: elem_force_nonlinear_folded;
    // the plan's FK_N constants behind the blocked tables, crb_blocked.h: blk_fold_offset) instead of the chord form
    constexpr bool FOLD = REGROUP && CRB_BLK_FOLD;
    // the folded form with the membrane combinations A1, A2 formed once (crb_math.h: elem_force_nonlinear_shared; the plan's
    // SK_N constants behind the folded ones, crb_blocked.h: blk_share_offset) instead of the folded form; without
    // CRB_BLK_FOLD the switch does nothing
    constexpr bool SHARE = FOLD && CRB_BLK_SHARE;
    constexpr int NK = SHARE ? int(SK_N) : int(FK_N);
    // the polynomial constants requested one stage ahead, after the previous stage's right-hand side, instead of at the
    // stage's top (the same loads of the same values: outputs are bitwise those of the build without)
    constexpr bool AHEAD = FOLD && CRB_BLK_CONST_AHEAD;
    // ... and what else a stage reads by scalar loads (the impulse window's end and component, the drag factor, the constants'
    // address) read once per beam and held over the step loop, so that a stage's top has no scalar load and no wait at all:
    // with the constants arriving under the solve these seven registers no longer push anything out of the scalar file
    // (needs CRB_BLK_CONST_AHEAD)
    constexpr bool HOLD = AHEAD && CRB_BLK_HOLD_PARAMS;
    // the stage's vector work that is no arithmetic (neither item changes a computed value):
    // +f3 carried through the impulse block as the right transverse half, instead of -f3 negated again in the right-hand side
    constexpr bool F3PLUS = CRB_BLK_F3_PLUS && (REGROUP || EM == EM_LINEAR);
    // the separator tables read at immediate offsets from this lane's LDS byte address, laundered per level in place,
    // instead of through the laundered lane index (a new index every time, scaled again every time)
    constexpr bool SEPADDR = CRB_BLK_SEP_ADDR;
    // the lane's interior solved about its centre node (crb_blocked.h: blk_twist_interior_solve; the plan's twisted table behind
    // the shared form's constants, blk_twist_offset) instead of by block Thomas: 29 fp64 instructions against 35, depth 3 against 5
    constexpr bool TWIST = TW;
    // the two things a stage fetches from lane+1 -- the left halves of its first element, which enter nothing but the separator's
    // right-hand side, and its y_0 -- in ONE exchange: lane+1 forms h = fl[0] + C_s y_0, and g = (-fr[3] [+ drag]) - A_s y_2 - hR
    // (tip: lane 63 is shifted a 0, and C_s there only ever met a 0.  Written for the +f3 form, CRB_BLK_F3_PLUS.
    //  The linear instance keeps both exchanges: its code, and with it its output, stays its parent's bit for bit)
    constexpr bool ONER = CRB_BLK_ONE_RIGHT && F3PLUS && REGROUP;
    static_assert(!TW || EM == EM_NONLINEAR, "the twisted instance is built for the nonlinear element");
    // the table offsets of the form at hand
    constexpr int O_WL = TWIST ? int(BT_WL) : int(BU_WL), O_WR = TWIST ? int(BT_WR) : int(BU_WR),
                  O_AS = TWIST ? int(BT_AS) : int(BU_AS), O_CS = TWIST ? int(BT_CS) : int(BU_CS);
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) SlotConst<T>* CS;
    typedef const __attribute__((address_space(4))) T* CK;
#define CRB_BFRESH(ptr) asm volatile("" : "+s"(ptr))
#else
    typedef const SlotConst<T>* CS;
    typedef const T* CK;
#define CRB_BFRESH(ptr) (void)(ptr)
#endif
    typedef T rec4 __attribute__((ext_vector_type(4)));
    typedef T pair2 __attribute__((ext_vector_type(2)));
    KParams<T> p = *(const KParams<T>*)(kp);
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    pair2* const sepL = reinterpret_cast<pair2*>(crb_smem);   // [NV2][64]
    T* const strips = reinterpret_cast<T*>(sepL + NV2 * 64);    // [4 waves][3][BLK_STRIP_W]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // (wave-uniform to the compiler: the walk below is scalar)
    {   // the separator tables, [value][lane] in the plan, value pairs per lane here
        const T* src = p.blocked + BU_N;
        for (int i = t; i < NV2 * 64; i += 256) {
            const int v = 2 * (i >> 6), l = i & 63;
            sepL[i] = pair2{src[size_t(v) * 64 + l], v + 1 < NV ? src[size_t(v + 1) * 64 + l] : T(0)};
        }
        // the strips' pads: a neighbour past either end of the beam reads 0, as a DPP shift with bound_ctrl does
        for (int i = t; i < 4 * 3 * BLK_STRIP_W; i += 256) {
            const int k = i % BLK_STRIP_W;
            if (k < BLK_STRIP_PAD || k >= BLK_STRIP_PAD + BLK_LANES) strips[i] = T(0);
        }
    }
    // this wave's strip at its lane's column (volatile: the compiler sees a level's reads as other addresses than this lane's
    // store and would hoist them; a wave's LDS accesses execute in order, so the order is all that is needed -- no wait)
#if defined(__HIP_DEVICE_COMPILE__)
    typedef volatile __attribute__((address_space(3))) T* SP;   // (spelled out: a volatile access keeps a generic pointer flat)
#else
    typedef volatile T* SP;
#endif
    const SP strip = (SP)(strips + wave * 3 * BLK_STRIP_W + BLK_STRIP_PAD + lane);
    // SEPADDR: this lane's column of the separator tables, value pair v at sepc[v * 64]
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(3))) pair2* SEPC;
#else
    typedef const pair2* SEPC;
#endif
    [[maybe_unused]] SEPC sepc = (SEPC)(sepL + lane);
    // the wave-uniform table, once per launch: constant k in lane k % 16 of every row of tab[k / 16] (crb_blocked.h), and
    // broadcast copies of the nine constants that multiply without adding (the first product of each blk_mul sum)
    T tab[BLK_TAB_REGS];
#pragma unroll
    for (int i = 0; i < BLK_TAB_REGS; ++i)
        tab[i] = TWIST ? p.blocked[blk_twist_offset(LS) + BLK_TAB_ROW * i + (lane & (BLK_TAB_ROW - 1))] : p.blocked[blk_tab_index(i, lane)];
    // (TWIST: six copies, cD0 = the diagonal of B^-1 and cD1 = that of Dc^-1; there is no cD2)
    constexpr int O_C0u = TWIST ? int(BT_BI) : int(BU_U0), O_C0w = TWIST ? BT_BI + 1 : BU_D0 + 2, O_C0p = TWIST ? BT_BI + 2 : BU_D0 + 4;
    constexpr int O_C1u = TWIST ? int(BT_DI) : int(BU_U1), O_C1w = TWIST ? BT_DI + 1 : BU_D1 + 2, O_C1p = TWIST ? BT_DI + 2 : BU_D1 + 4;
    [[maybe_unused]] T cD2[3] = {T(0), T(0), T(0)};
    if constexpr (!TWIST) { cD2[0] = blk_bc_copy<BU_D2>(tab); cD2[1] = blk_bc_copy<BU_D2 + 2>(tab); cD2[2] = blk_bc_copy<BU_D2 + 4>(tab); }
    const T cD1[3] = {blk_bc_copy<O_C1u>(tab), blk_bc_copy<O_C1w>(tab), blk_bc_copy<O_C1p>(tab)};
    const T cD0[3] = {blk_bc_copy<O_C0u>(tab), blk_bc_copy<O_C0w>(tab), blk_bc_copy<O_C0p>(tab)};
    __syncthreads();   // (the only barrier: the waves walk over their beams independently from here on)
    const int n_groups = (p.B + 3) / 4;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        CRB_BFRESH(kp);
        p = *(const KParams<T>*)(kp);
        const int beam = grp * 4 + wave;
        if (beam >= p.B) continue;   // (wave-uniform)
        const size_t plane = size_t(p.n_node) * 4;
        const size_t xoff = size_t(beam) * 2 * plane + size_t(NP * lane + p.off) * 4;
        T xq[NP][3], xv[NP][3];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const rec4 a = *reinterpret_cast<const rec4*>(p.x + xoff + 4 * k), b = *reinterpret_cast<const rec4*>(p.x + xoff + plane + 4 * k);
#pragma unroll
            for (int c = 0; c < 3; ++c) { xq[k][c] = a[c]; xv[k][c] = b[c]; }
        }
        T amp = T(0);
        int kimp = -1;   // impulse node of the beam: slot 4 lane + kimp (wave-uniform)
        if (p.amp) {
            const int js = p.imp_node_b ? p.imp_node_b[beam] - p.off : p.imp_slot;
            if (js >= 0 && js < BLK_S) {
                kimp = js & (NP - 1);
                if (lane == js / NP) amp = p.amp[beam];
            }
        }
        T qL[3];   // q of lane-1's last node (the fixed root: 0 into lane 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) qL[c] = dpp_from_lower(xq[NP - 1][c]);
        const T dt = T(p.dt), hdt = T(0.5 * p.dt), dt6 = T(p.dt / 6.0);
        [[maybe_unused]] const T c6 = T(p.dt * p.dt / 6.0), c4 = T(0.25 * p.dt * p.dt), c2 = T(0.5 * p.dt * p.dt);   // (RKPOS)
        double tc = p.t0;
        // RKPOS: sq is the stage's positions, rk the next stage's and the running sums, sv[.][1] the stage velocity of w (the
        // only one a force reads: the drag); xv is updated by stage 3 itself.  Otherwise accq / sv carry every component
        [[maybe_unused]] T accq[NP][3], accv[NP][3];
        T sq[NP][3], sv[NP][3];
        [[maybe_unused]] Rk4Pos<T> rk[NP][3];
        // AHEAD: the polynomial constants, requested here for the first stage and after each stage's right-hand side for the next
        [[maybe_unused]] T fk_ahead[NK];
        [[maybe_unused]] CK FC_held = nullptr;
        [[maybe_unused]] double dur_held = 0.0;
        [[maybe_unused]] int dof_held = 0;
        [[maybe_unused]] T dragc_held = T(0);
        if constexpr (AHEAD) {
            const CK FC = (CK)p.blocked + (SHARE ? blk_share_offset(LS) : blk_fold_offset(LS));
#pragma unroll
            for (int i = 0; i < NK; ++i) fk_ahead[i] = FC[i];
            if constexpr (HOLD) {
                FC_held = FC;
                dur_held = p.duration;
                dof_held = p.imp_dof;
                const T drag_all = ((CS)p.slot)->drag;
                dragc_held = (p.flags & 1u) ? drag_all : T(0);
            }
        }
        for (int step = 0; step < p.n_steps; ++step) {
            double t_half, t_full;
            {
                KPT ks = kp;
                CRB_BFRESH(ks);
                const double hstep = (*(const KParams<T>*)(ks)).dt;
                t_half = __dadd_rn(tc, 0.5 * hstep);
                t_full = __dadd_rn(tc, hstep);
            }
#pragma unroll
            for (int k = 0; k < NP; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) { sq[k][c] = xq[k][c]; sv[k][c] = xv[k][c]; }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                // (without HOLD, what a stage needs of the launch parameters is re-read through the laundered kernarg pointer:
                //  held across the loop next to constants loaded at the stage's top, it pushed them out of the scalar file)
                KPT ks = kp;
                CRB_BFRESH(ks);
                const KParams<T>& q = *(const KParams<T>*)(ks);
                const double ts = (s == 0) ? tc : ((s == 3) ? t_full : t_half);
                const bool imp_on = ts < (HOLD ? dur_held : q.duration);
                const T w = (s == 0 || s == 3) ? T(1) : T(2);
                const T cs = (s == 2) ? dt : hdt;
                const CS SC = (CS)q.slot;
                [[maybe_unused]] T ec[6];
                [[maybe_unused]] T fk_stage[NK];
                [[maybe_unused]] T* const fk = AHEAD ? fk_ahead : fk_stage;
                [[maybe_unused]] CK FCn = nullptr;   // (AHEAD: where the request after the right-hand side reads)
                if constexpr (FOLD) {
                    const CK FC = (CK)q.blocked + (SHARE ? blk_share_offset(LS) : blk_fold_offset(LS));
                    if constexpr (AHEAD) FCn = HOLD ? FC_held : FC;
                    else {
#pragma unroll
                        for (int i = 0; i < NK; ++i) fk[i] = FC[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 6; ++i) ec[i] = SC->elem.c[i];
                }
                const T drag_all = SC->drag;   // (loaded whatever the flag: a load under a branch costs a wait of its own)
                const T dragc = HOLD ? dragc_held : ((q.flags & 1u) ? drag_all : T(0));
                // -- positions of the next stage: the last node's ride on this stage's q exchange
                [[maybe_unused]] T qn3[3];
                T qLn[3];
                if constexpr (RKPOS) {
                    if (s == 0) {
#pragma unroll
                        for (int k = 0; k < NP; ++k)
#pragma unroll
                            for (int c = 0; c < 3; ++c) rk4_begin<T>(rk[k][c], xq[k][c], xv[k][c], hdt, dt);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) qLn[c] = dpp_from_lower(rk[NP - 1][c].next);
                } else {
#pragma unroll
                    for (int k = 0; k < NP; ++k)
#pragma unroll
                        for (int c = 0; c < 3; ++c) accq[k][c] = (s == 0) ? sv[k][c] : accq[k][c] + w * sv[k][c];   // (stage 0 starts the sum: no 0 + x)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        qn3[c] = (s == 3) ? (xq[NP - 1][c] + dt6 * accq[NP - 1][c]) : (xq[NP - 1][c] + cs * sv[NP - 1][c]);
                        qLn[c] = dpp_from_lower(qn3[c]);
                    }
                }
                // -- the four elements left of this lane's nodes (element k joins node k-1 -- lane-1's last for k = 0 -- and node k)
                CRB_SETPRIO(P_FORCE);
                T fl[NP][3], r[NP][3];
                T fr[NP][3];
                T f2[NP], cW[NP];   // (REGROUP: the axial pair as f2 and W, crb_math.h)
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    if constexpr (FOLD) {
                        ElemForceRegrouped<T> e;
                        if constexpr (SHARE) e = elem_force_nonlinear_shared<T, const T*>(fk, k ? sq[k - 1] : qL, sq[k]);
                        else e = elem_force_nonlinear_folded<T, const T*>(fk, k ? sq[k - 1] : qL, sq[k]);
                        f2[k] = e.f2; cW[k] = e.W;   // (W carries cA1)
                        fl[k][1] = e.f3; fr[k][1] = F3PLUS ? e.f3 : -e.f3; fl[k][2] = e.m_left; fr[k][2] = e.m_right;
                    } else if constexpr (REGROUP) {
                        const ElemForceRegrouped<T> e = CHORD ? elem_force_nonlinear_chord<T>(ec, k ? sq[k - 1] : qL, sq[k])
                                                              : elem_force_nonlinear_regrouped<T>(ec, k ? sq[k - 1] : qL, sq[k]);
                        f2[k] = e.f2; cW[k] = ec[1] * e.W;
                        fl[k][1] = e.f3; fr[k][1] = F3PLUS ? e.f3 : -e.f3; fl[k][2] = e.m_left; fr[k][2] = e.m_right;
                    } else if (EM == EM_NONLINEAR) elem_force_nonlinear<T>(ec, k ? sq[k - 1] : qL, sq[k], false, fl[k], fr[k]);
                    else {
                        elem_force_linear<T>(ec, k ? sq[k - 1] : qL, sq[k], fl[k], fr[k]);
                        if constexpr (F3PLUS) fr[k][1] = fl[k][1];   // (the linear element's right transverse half is -fl[1])
                    }
                }
                if constexpr (REGROUP) {
                    // the axial right-hand side less its last product, negated: fr[k][0] enters r as -fr[k][0] below, as the
                    // right half f2(k) does in the other form, so the impulse block acts on it with the same sign.  The last
                    // node's is the explicit left half f1 = cA1 W - f2 of lane+1's first element (one per lane, not four)
                    fl[0][0] = cW[0] - f2[0];
#pragma unroll
                    for (int k = 0; k + 1 < NP; ++k) fr[k][0] = f2[k] - f2[k + 1];
                    // (-f2(3) - this below: the impulse's -amp lands on either term alike.  ONER: f1 of lane+1 arrives inside hR in
                    //  the solve, and the impulse's -amp lands on the local f2(3), negated below)
                    fr[NP - 1][0] = ONER ? f2[NP - 1] : dpp_from_higher(fl[0][0]);
                }
                // -- the impulse: fr - amp on its one (node, dof), so that r = (amp - fr) - fl there and -fr - fl everywhere else
                //    (REGROUP, axial dof: fr[k][0] is the difference / the shifted-in f1 above, entering r with the same sign),
                //    instead of one r = sel * amp - fr per component (12 fp64 FMAs per stage for one lane's one component).  The
                //    selector is wave-uniform, so the choice is scalar compares and branches around ONE v_add_f64; they are
                //    written as an opaque block per node because a C++ branch here splits the stage's straight-line code, which
                //    the scheduler then no longer interleaves with the solve (measured: 50 spilled VGPRs).  No lane shift inside.
                //    After a compiler upgrade re-check with `make resource-usage`: this kernel at 0 SGPR spills, <= 256 VGPRs
                //    (252 with +f3 carried through this block, CRB_BLK_F3_PLUS; 256 without it, the ceiling of two waves per SIMD, where
                //    a compiler that needs one more register spills; 97 SGPRs allocated with the constants a stage ahead, 103 as the
                //    tool totals them), no scratch.  The block can go back to the C++ form of the host branch below once that no longer splits the
                //    schedule (same resource figures, same step time).
                {
                    const int kon = imp_on ? kimp : -1, dof = HOLD ? dof_held : q.imp_dof;
                    // (F3PLUS: the transverse left half of lane+1's first element, for the last node's right-hand side below)
                    [[maybe_unused]] T flR1 = T(0);
                    if constexpr (F3PLUS && !ONER) flR1 = dpp_from_higher(fl[0][1]);
#if defined(__HIP_DEVICE_COMPILE__)
                    // (SGN1: the sign of amp on the transverse dof -- "-" on fr[k][1] = -f3, "" on +f3 carried through, F3PLUS)
#define CRB_BLK_IMPULSE(SGN1)                                                                  \
                        asm volatile(                                                          \
                            "s_cmp_lg_u32 %[kon], %[k]\n\t"                                    \
                            "s_cbranch_scc1 2f\n\t"                                            \
                            "s_cmp_lg_u32 %[dof], 0\n\t"                                       \
                            "s_cbranch_scc1 0f\n\t"                                            \
                            "v_add_f64 %[f0], %[f0], -%[amp]\n"                                \
                            "0:\n\t"                                                           \
                            "s_cmp_lg_u32 %[dof], 1\n\t"                                       \
                            "s_cbranch_scc1 1f\n\t"                                            \
                            "v_add_f64 %[f1], %[f1], " SGN1 "%[amp]\n"                         \
                            "1:\n\t"                                                           \
                            "s_cmp_lg_u32 %[dof], 2\n\t"                                       \
                            "s_cbranch_scc1 2f\n\t"                                            \
                            "v_add_f64 %[f2], %[f2], -%[amp]\n"                                \
                            "2:"                                                               \
                            : [f0] "+v"(fr[k][0]), [f1] "+v"(fr[k][1]), [f2] "+v"(fr[k][2])    \
                            : [kon] "s"(kon), [dof] "s"(dof), [amp] "v"(amp), [k] "n"(k)       \
                            : "scc")
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        if constexpr (F3PLUS) {
                            // (node k's transverse right-hand side directly behind its block: it is the last reader of
                            //  fl[k + 1][1], the very f3 that the next block takes in/out -- dead by then, it needs no copy)
                            CRB_BLK_IMPULSE("");
                            r[k][1] = fr[k][1] + drag_force<T>(dragc, sv[k][1]);
                            if (k + 1 < NP || !ONER) r[k][1] -= (k + 1 < NP) ? fl[k + 1][1] : flR1;   // (ONER: the last node's is in hR)
                        } else CRB_BLK_IMPULSE("-");
                    }
#undef CRB_BLK_IMPULSE
#else
                    for (int k = 0; k < NP; ++k)
                        for (int c = 0; c < 3; ++c) {
                            const T ac = (kon == k && c == dof) ? amp : T(0);
                            if (F3PLUS && c == 1) fr[k][c] += ac;
                            else fr[k][c] -= ac;
                        }
                    if constexpr (F3PLUS)
                        for (int k = 0; k < NP; ++k) {
                            r[k][1] = fr[k][1] + drag_force<T>(dragc, sv[k][1]);
                            if (k + 1 < NP || !ONER) r[k][1] -= (k + 1 < NP) ? fl[k + 1][1] : flR1;
                        }
#endif
                }
                CRB_SETPRIO(P_TAIL);
                // -- right-hand side: the left half of the lane's first element belongs to lane-1's last node (0 past the tip)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (REGROUP && c == 0) {   // r_u[k] = (f2(k+1) - f2(k)) - cA1 W(k+1); the last node's -f2(3) - f1 of lane+1
#pragma unroll
                        for (int k = 0; k < NP; ++k) r[k][0] = (k + 1 < NP) ? (-fr[k][0] - cW[k + 1]) : (ONER ? fr[k][0] : (-f2[k] - fr[k][0]));   // (ONER: the last node's NEGATED, as its moment below: see the solve)
                        continue;
                    }
                    if (F3PLUS && c == 1) continue;   // (formed behind the impulse blocks, above)
                    const T flR = ONER ? T(0) : dpp_from_higher(fl[0][c]);   // (ONER: inside hR in the solve)
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        T h = -fr[k][c];
                        if (c == 1) h += drag_force<T>(dragc, sv[k][1]);
                        r[k][c] = (ONER && k + 1 == NP) ? ((c == 1) ? h : fr[k][c]) : h - ((k + 1 < NP) ? fl[k + 1][c] : flR);
                    }
                }
                // -- AHEAD: the polynomial constants of the NEXT stage (stage 3: of the next step's stage 0), requested where this
                //    stage's last use of them is behind: the request is tied to the finished right-hand side, the solve and the
                //    RK4 ends below need no scalar register, and the values land under them
                if constexpr (AHEAD) {
#if defined(__HIP_DEVICE_COMPILE__)
                    asm volatile("" : "+s"(FCn)
                                 : "v"(r[0][0]), "v"(r[0][1]), "v"(r[0][2]), "v"(r[1][0]), "v"(r[1][1]), "v"(r[1][2]),
                                   "v"(r[2][0]), "v"(r[2][1]), "v"(r[2][2]), "v"(r[3][0]), "v"(r[3][1]), "v"(r[3][2]));
#endif
#pragma unroll
                    for (int i = 0; i < NK; ++i) fk_ahead[i] = FCn[i];
                }
                // -- mass solve: interior, separator right-hand side, separator levels, back substitution.  Every wave-uniform
                //    constant is a row broadcast of `tab` inside a multiply-add (66 per stage), or one of the nine copies; each
                //    sum in the order the compiler contracts blk_interior_solve's (crb_blocked.h) with scalar operands: a blk_mul
                //    row is fma(m1, v1, m2 v2), and the axial row of a blk_mul / blk_sub_mul pair is fma(d, v, -(u w))
                T y[3][3], z1[3], g[3], y0R[3];
                [[maybe_unused]] T z2[3];
                // (the first separator level's table is requested here, under the interior solve, which has no wait of its own:
                //  what the reads are addressed by is laundered through the right-hand side, so that they are issued where the solve
                //  starts.  SEPADDR: that is the lane's table address, laundered in place -- the old value is dead, so nothing is
                //  copied or scaled again -- with every read at an immediate offset from it; otherwise the lane index)
                [[maybe_unused]] int li = lane;
                T cf0[PCR_LEVEL_VALS];
                auto sep_pair = [&](int v2) -> pair2 {
                    if constexpr (SEPADDR) return sepc[v2 * 64];
                    else return sepL[v2 * 64 + li];
                };
                if constexpr (SEPADDR) asm volatile("" : "+v"(sepc) : "v"(r[0][0]));
                else asm volatile("" : "+v"(li) : "v"(r[0][0]));
#pragma unroll
                for (int i = 0; i < PCR_LEVEL_VALS; i += 2) {
                    const pair2 e = sep_pair(i / 2);
                    cf0[i] = e[0]; cf0[i + 1] = e[1];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) { z1[c] = r[1][c]; if (!TWIST) z2[c] = r[2][c]; g[c] = r[NP - 1][c]; }
                if constexpr (TWIST) {
                    // z_1 = r_1 - (A1 B^-1) r_0 - (C1 B^-1) r_2; y_1 = Dc^-1 z_1; y_0 = B^-1 r_0 - (B^-1 C0) y_1; y_2 = B^-1 r_2 - (B^-1 A2) y_1
                    blk_bc_sub_mul<BT_P>(tab, r[0], z1);
                    blk_bc_sub_mul<BT_Q>(tab, r[2], z1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) { y[0][c] = cD0[c] * r[0][c]; y[2][c] = cD0[c] * r[2][c]; y[1][c] = cD1[c] * z1[c]; }
                    blk_bc_sub_mul<BT_U>(tab, y[1], y[0]);
                    blk_bc_sub_mul<BT_V>(tab, y[1], y[2]);
                } else {
                    blk_bc_sub_mul<BU_L1>(tab, r[0], z1);
                    blk_bc_sub_mul<BU_L2>(tab, z1, z2);
                    y[2][0] = cD2[0] * z2[0];                       // y_2 = D2 z_2
                    y[2][1] = cD2[1] * z2[2]; blk_bc_fma<BU_D2 + 1>(tab, z2[1], y[2][1]);
                    y[2][2] = cD2[2] * z2[2]; blk_bc_fma<BU_D2 + 3>(tab, z2[1], y[2][2]);
                    y[1][0] = -(cD1[0] * y[2][0]); blk_bc_fma<BU_D1>(tab, z1[0], y[1][0]);   // y_1 = D1 z_1 - U1 y_2
                    y[1][1] = cD1[1] * z1[2]; blk_bc_fma<BU_D1 + 1>(tab, z1[1], y[1][1]);
                    y[1][2] = cD1[2] * z1[2]; blk_bc_fma<BU_D1 + 3>(tab, z1[1], y[1][2]);
                    blk_bc_fnma<BU_U1 + 1>(tab, y[2][1], y[1][1]); blk_bc_fnma<BU_U1 + 2>(tab, y[2][2], y[1][1]);
                    blk_bc_fnma<BU_U1 + 3>(tab, y[2][1], y[1][2]); blk_bc_fnma<BU_U1 + 4>(tab, y[2][2], y[1][2]);
                    y[0][0] = -(cD0[0] * y[1][0]); blk_bc_fma<BU_D0>(tab, r[0][0], y[0][0]);   // y_0 = D0 r_0 - U0 y_1
                    y[0][1] = cD0[1] * r[0][2]; blk_bc_fma<BU_D0 + 1>(tab, r[0][1], y[0][1]);
                    y[0][2] = cD0[2] * r[0][2]; blk_bc_fma<BU_D0 + 3>(tab, r[0][1], y[0][2]);
                    blk_bc_fnma<BU_U0 + 1>(tab, y[1][1], y[0][1]); blk_bc_fnma<BU_U0 + 2>(tab, y[1][2], y[0][1]);
                    blk_bc_fnma<BU_U0 + 3>(tab, y[1][1], y[0][2]); blk_bc_fnma<BU_U0 + 4>(tab, y[1][2], y[0][2]);
                }
                if constexpr (ONER) {
                    // h = fl[0] + C_s y_0, what this lane owes the separator of lane-1; g (so far without the left halves of
                    // lane+1's first element) takes lane+1's whole in one exchange: the tip is shifted a 0
                    blk_bc_add_mul<O_CS>(tab, y[0], fl[0]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) y0R[c] = dpp_from_higher(fl[0][c]);
                    // (the axial and the moment component arrive negated -- a bare negation would be an instruction, inside the
                    //  last subtraction it is a source modifier -- so A_s y_2 is added to them; the roundings are the mirror images)
                    blk_bc_fma<O_AS + 0>(tab, y[2][0], g[0]);
                    blk_bc_fnma<O_AS + 1>(tab, y[2][1], g[1]);
                    blk_bc_fnma<O_AS + 2>(tab, y[2][2], g[1]);
                    blk_bc_fma<O_AS + 3>(tab, y[2][1], g[2]);
                    blk_bc_fma<O_AS + 4>(tab, y[2][2], g[2]);
                    g[0] = -g[0] - y0R[0];
                    g[1] = g[1] - y0R[1];
                    g[2] = -g[2] - y0R[2];
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) y0R[c] = dpp_from_higher(y[0][c]);
                    blk_bc_sub_mul<O_AS>(tab, y[2], g);
                    blk_bc_sub_mul<O_CS>(tab, y0R, g);
                }
#pragma unroll
                for (int l = 0; l < LS; ++l) {
                    // (the table address -- without SEPADDR the lane index -- is laundered through this level's input, so that
                    //  the table loads of the later levels are issued when they start instead of all at the top of the loop: the
                    //  tables would otherwise take 70 registers)
                    if constexpr (SEPADDR) asm volatile("" : "+v"(sepc) : "v"(g[0]));
                    else asm volatile("" : "+v"(li) : "v"(g[0]));
                    T cf[PCR_LEVEL_VALS];
#pragma unroll
                    for (int i = 0; i < PCR_LEVEL_VALS; i += 2) {
                        const int v = l * PCR_LEVEL_VALS + i;   // (even: PCR_LEVEL_VALS is)
                        if (l == 0) { cf[i] = cf0[i]; cf[i + 1] = cf0[i + 1]; continue; }
                        const pair2 e = sep_pair(v / 2);
                        cf[i] = e[0]; cf[i + 1] = e[1];
                    }
                    T glo[3], ghi[3];
                    if (l == 2) {   // stride 4 through the strip: 3 stores, 6 loads at immediate offsets
#pragma unroll
                        for (int c = 0; c < 3; ++c) strip[c * BLK_STRIP_W] = g[c];
#pragma unroll
                        for (int c = 0; c < 3; ++c) { glo[c] = strip[c * BLK_STRIP_W - 4]; ghi[c] = strip[c * BLK_STRIP_W + 4]; }
                    } else if (l == 1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) { glo[c] = lane_lower<T, 2>(g[c], lane); ghi[c] = lane_higher<T, 2>(g[c], lane); }
                    } else {
#pragma unroll
                        for (int c = 0; c < 3; ++c) { glo[c] = lane_lower<T, 1>(g[c], lane); ghi[c] = lane_higher<T, 1>(g[c], lane); }
                    }
                    pcr_apply_level<T>(cf, glo, ghi, g);
                }
                if constexpr (SEPADDR) asm volatile("" : "+v"(sepc) : "v"(g[0]));
                else asm volatile("" : "+v"(li) : "v"(g[0]));
                T fin[6], xs[3], xsL[3];
#pragma unroll
                for (int i = 0; i < 6; i += 2) {
                    const int v = LS * PCR_LEVEL_VALS + i;
                    const pair2 e = sep_pair(v / 2);
                    fin[i] = e[0]; fin[i + 1] = e[1];
                }
                pcr_apply_final<T>(fin, g, xs);
#pragma unroll
                for (int c = 0; c < 3; ++c) xsL[c] = dpp_from_lower(xs[c]);
                T a[NP][3];
#pragma unroll
                for (int k = 0; k < NP - 1; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) a[k][c] = y[k][c];
                static_assert(NP == 4, "three interior nodes, written out: the table offsets are template arguments");
                blk_bc_sub_mul<O_WL>(tab, xsL, a[0]);
                blk_bc_sub_mul<O_WR>(tab, xs, a[0]);
                blk_bc_sub_mul<O_WL + BLK_PACK>(tab, xsL, a[1]);
                blk_bc_sub_mul<O_WR + BLK_PACK>(tab, xs, a[1]);
                blk_bc_sub_mul<O_WL + 2 * BLK_PACK>(tab, xsL, a[2]);
                blk_bc_sub_mul<O_WR + 2 * BLK_PACK>(tab, xs, a[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) a[NP - 1][c] = xs[c];
                // -- RK4 bookkeeping
#pragma unroll
                for (int k = 0; k < NP; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if constexpr (RKPOS) {
                            sq[k][c] = rk[k][c].next;
                            if (s == 0) rk4_end0<T>(rk[k][c], a[k][c], c6, c4);
                            else if (s == 1) rk4_end1<T>(rk[k][c], a[k][c], c6, c2);
                            else if (s == 2) rk4_end2<T>(rk[k][c], a[k][c], c6);
                            else xv[k][c] = rk4_end3<T>(rk[k][c], xv[k][c], a[k][c], dt6);
                            if (c == 1 && s < 3) sv[k][1] = rk4_stage_velocity<T>(xv[k][1], cs, a[k][1]);
                        } else {
                            accv[k][c] = (s == 0) ? a[k][c] : accv[k][c] + w * a[k][c];
                            if (k == NP - 1) sq[k][c] = qn3[c];
                            else sq[k][c] = (s == 3) ? (xq[k][c] + dt6 * accq[k][c]) : (xq[k][c] + cs * sv[k][c]);
                            sv[k][c] = (s == 3) ? (xv[k][c] + dt6 * accv[k][c]) : (xv[k][c] + cs * a[k][c]);
                        }
                    }
#pragma unroll
                for (int c = 0; c < 3; ++c) qL[c] = qLn[c];
            }
#pragma unroll
            for (int k = 0; k < NP; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xq[k][c] = sq[k][c];
                    if (!RKPOS) xv[k][c] = sv[k][c];
                }
            tc = t_full;
            KPT kr_ = kp;
            CRB_BFRESH(kr_);
            const KParams<T>& pr = *(const KParams<T>*)(kr_);   // (re-read, as above)
            if (pr.rec_out && (step + 1) % pr.rec_every == 0) {
                const size_t kr = size_t((step + 1) / pr.rec_every - 1);
                if (pr.rec_slot == REC_ALL_SLOTS) {   // whole-state snapshot kr: every lane stores its nodes' records
                    T* snap = pr.rec_out + kr * size_t(pr.B) * 2 * plane + xoff;
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        *reinterpret_cast<rec4*>(snap + 4 * k) = rec4{xq[k][0], xq[k][1], xq[k][2], T(0)};
                        *reinterpret_cast<rec4*>(snap + plane + 4 * k) = rec4{xv[k][0], xv[k][1], xv[k][2], T(0)};
                    }
                } else if (pr.rec_slot >= 0 && lane == pr.rec_slot / NP) {
                    const int kk = pr.rec_slot & (NP - 1);
                    T val = xq[0][0];
#pragma unroll
                    for (int k = 0; k < NP; ++k)
#pragma unroll
                        for (int c = 0; c < 6; ++c)
                            val = (k == kk && c == pr.rec_comp) ? (c < 3 ? xq[k][c] : xv[k][c - 3]) : val;
                    pr.rec_out[size_t(beam) * pr.rec_n + kr] = val;
                }
            }
        }
        CRB_BFRESH(kp);
        p = *(const KParams<T>*)(kp);
        bool bad = false;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            *reinterpret_cast<rec4*>(p.x + xoff + 4 * k) = rec4{xq[k][0], xq[k][1], xq[k][2], T(0)};
            *reinterpret_cast<rec4*>(p.x + xoff + plane + 4 * k) = rec4{xv[k][0], xv[k][1], xv[k][2], T(0)};
#pragma unroll
            for (int c = 0; c < 3; ++c) bad = bad || !isfinite(xq[k][c]) || !isfinite(xv[k][c]);
        }
        if (p.status && bad) atomicCAS(p.status + beam, 0, p.status_value);
    }
#undef CRB_BFRESH
}

// Waves per SIMD the fp64 lean kernels are register-allocated for.  Two, except single-wave beams with gravity and 5 or
// more reduction levels: their working set does not fit 256 registers (18 .. 140 spilled VGPRs), and a beam that lives in
// ONE wave gains nothing from a second resident wave until the ensemble exceeds 1024 beams -- measured, spill-free at one
// wave per SIMD against two with spills: 1024 x 64 + gravity (BASELINE config 2) 3.27 against 4.13 us per step, 4096 x 64
// 11.4 against 11.6.  Beams of several waves keep two (their cross-wave exchanges need the second workgroup to hide the
// barrier latency: 4096 x 128 / x 256 + gravity take 32 / 70 us per step at one wave per SIMD against 21 / 39 at two, spills
// included).
__host__ __device__ constexpr int lean_minw_f64(int lv, int lognw, bool grav) { return (grav && lv >= 5 && lognw == 0) ? 1 : 2; }
// EM (EM_*): the element kind when the whole topology has one; the force evaluation is then straight-line
// code that the scheduler interleaves with the tail of the previous stage's reduction (measured +8 %
// over the per-lane branch of EM_MIXED; a wave-uniform run-time branch does not get it).
// HELD: a per-node input force held over the launch (zero-order-hold control, `u` of dynamic_system(t, x, u)
// as an array): three more registers and three more additions per stage, so it is its own instantiation.
// PACK (one-wave form only): beams with fewer than 64 slots, G = 64/S of them per wave (lane = g*S + j).  All
// exchanges stay DPP lane shifts; whatever a shift drags across a beam boundary is replaced by 0 with a SELECT (in
// round A and in every reduction level, lean_reduce_tail<..., ISOLATE>): a diverged wave-mate's Inf / NaN must not
// reach its neighbours through a 0 * NaN (the reference's beams are independent).
// FB (packed one-wave form): the state feedback u = K (r - x) inside every stage, as in crb_beam_kernel<..., FB> (crb_generic.h: gain
// in LDS, the product K e on the matrix cores for gains of 21 .. 32 rows) but around THIS kernel's right-hand side -- the
// general kernel's costs 4000 cycles per stage for a 10-element beam, this one's 1900.  One wave per SIMD (the gain's
// fragments take 64 more registers).
// NPL (nodes per lane): 1, or 4 for the register-blocked form above (LV is then its separator level count, LOGNW 2: four
// independent one-wave beams per workgroup).
template <typename T, int LV, int LOGNW, bool GRAV, int EM, bool HELD = false, bool PACK = false, bool FB = false, int NPL = 1>
// fp64: 2 waves/SIMD, 256 VGPRs hold the multipliers.  fp32: the headline shape (<= 4 levels, no gravity, no held
// input) fits 4 waves/SIMD (128 VGPRs; three 8-byte addresses spill, outside the step loop: config 4 runs 8.1e10
// element-steps/s at 4 waves against 6.6e10 at 3), the other fp32 instantiations keep 3 waves/SIMD (168 VGPRs)
__global__ void __launch_bounds__(64 << LOGNW, FB ? 1 : ((sizeof(T) == 4 && LOGNW <= 2) ? ((LV <= 4 && !GRAV && !HELD) ? 4 : 3) : lean_minw_f64(LV, LOGNW, GRAV)))
crb_step_lean_kernel(const KParams<T> p_formal) {
    // The launch parameters are read through the kernarg pointer, which is "laundered" (CRB_FRESH) at the top of
    // every beam and again after the step loop: what the beam prologue / epilogue need (pointers, strides, sizes) is
    // then re-read from the kernarg segment by a few scalar loads instead of staying live in SGPRs across the step
    // loop.  That loop keeps ~36 SGPRs of fp64 polynomial constants; with the walk-over-beams loop around it the
    // scalar file overflowed (28 spills) and the scheduler fell back to a serialised LDS schedule: 28.4 -> 32.4 us/step.
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) KParams<T>* KP;
    KP kp = (KP)__builtin_amdgcn_kernarg_segment_ptr();   // the explicit arguments start at offset 0 of the segment
    (void)p_formal;
#define CRB_FRESH(ptr) asm volatile("" : "+s"(ptr))
#define CRB_PARAMS(ptr) (*(const KParams<T>*)(ptr))
#else   // (host pass: only the stub is emitted; keep the body well-formed)
    const KParams<T>* kp = &p_formal;
#define CRB_FRESH(ptr) (void)(ptr)
#define CRB_PARAMS(ptr) (*(ptr))
#endif
    if constexpr (NPL > 1) {
        static_assert(NPL == BLK_NPL && LOGNW == 2 && !GRAV && !HELD && !PACK && !FB, "the blocked form is the plain 256-slot stepper");
        lean_blocked_body<T, LV, EM, false>(kp);
        return;
    }
    KParams<T> p = CRB_PARAMS(kp);
    static_assert(!PACK || LOGNW == 0, "packed beams live inside one wave");
    static_assert(!FB || (PACK && !HELD), "the feedback form is the packed one-wave stepper");
    static_assert(LV >= 1, "lean stepper needs at least one reduction level");
    constexpr int NW = 1 << LOGNW, NT = 64 << LOGNW, RN = LeanRec<T>::N;
    constexpr int NULLT = NT;  // index of the all-zero record / column: "no neighbour"
    // fp64 round A is laid out as 9 columns [qn0..2 p0..2 fl0..2][NT+1] moved by 8-byte accesses (a 16-byte LDS
    // store costs 13 cycles of the store path against 2 x 6 for two 8-byte ones); fp32 keeps 16-byte records
    constexpr bool SOA = sizeof(T) == 8;
    constexpr bool RECB = sizeof(T) == 4;   // cross-wave levels as 16-byte records (fp64: 32-byte records measured 4 % slower)
    auto recA = [](T* base, int th, int k) -> T& { return SOA ? base[size_t(k) * (NT + 1) + th] : base[size_t(th) * RN + k]; };
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    T* const ldsA = reinterpret_cast<T*>(crb_smem);
    T* const ldsB = ldsA + size_t(NT + 1) * RN * (LOGNW == 1 ? 2 : 1);  // [level-1][3][NT+1]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S;
    const int pg = PACK ? lane / S : 0;                         // beam of this lane inside the wave
    const int j = PACK ? lane - pg * S : ((lane << LOGNW) | wave);
    const bool has_slot = PACK ? (pg < p.G) : (j < S);          // this thread carries a slot (of some beam)
    auto thread_of = [](int jj) { return ((jj & (NW - 1)) << 6) | (jj >> LOGNW); };
    // LDS positions of the stride-1 / stride-2 neighbours (NULLT outside the beam)
    const int t_l1 = (has_slot && j >= 1) ? thread_of(j - 1) : NULLT;
    const int t_r1 = (has_slot && j + 1 < S) ? thread_of(j + 1) : NULLT;
    if (LOGNW > 0 && t == 0) {  // zero the "no neighbour" slots once
#pragma unroll
        for (int k = 0; k < RN; ++k) {
            recA(ldsA, NULLT, k) = T(0);
            if (LOGNW == 1) recA(ldsA + size_t(NT + 1) * RN, NULLT, k) = T(0);
        }
#pragma unroll
        for (int l = 1; l < LOGNW; ++l)
#pragma unroll
            for (int c = 0; c < (RECB ? 4 : 3); ++c)
                ldsB[RECB ? (size_t(l - 1) * (NT + 1) + NULLT) * 4 + c : (size_t(l - 1) * 3 + c) * (NT + 1) + NULLT] = T(0);
    }

    // ---- per-thread constants: element pack, drag factor, the thread's rows of the solve tables.  Plans whose
    // beams share one table set load them ONCE per workgroup; the workgroup then walks over its beams (the grid is
    // sized to what is resident, crb_lean.hip): at 4096 x 256 the table prologue is 112 KB per workgroup from L2,
    // 460 MB per launch if every beam's workgroup repeats it -- 43 us, the whole fixed cost of a launch.
    const bool shared_tables = p.slot_stride == 0 && p.lv_stride == 0 && p.fin_stride == 0;
    ElemCoef<T> ec;
    T dragc = T(0);
    SolveCoef<T, LV> cf;
    // GRAV: gravity on the canonical cantilever (only node 0 constrained), where the reference's reduced-index
    // addressing (gravity_forces.py:104-146) is nearest-neighbour: segment j averages the rotations of slots j
    // and j+1 (slot j alone at the tip) and loads slots j and j+1.  A thread evaluates segment j AND segment
    // j-1 itself (it knows phi of slots j-1, j, j+1), so gravity needs no exchange of its own.
    T hm_own = T(0), hm_left = T(0);
    auto load_tables = [&](int beam) {
        if (has_slot) {
            const SlotConst<T>* st = p.slot + size_t(beam) * p.slot_stride;
            const SlotConst<T>& sc = st[j];
            ec = sc.elem;
            dragc = (p.flags & 1u) ? sc.drag : T(0);
            if (GRAV) { hm_own = sc.half_mass; hm_left = j >= 1 ? st[j - 1].half_mass : T(0); }
#pragma unroll
            for (int l = 0; l < LV; ++l) {
                const T* src = p.pcr_levels + size_t(beam) * p.lv_stride + (size_t(l) * size_t(S) + size_t(j)) * PCR_LEVEL_VALS;
#pragma unroll
                for (int k = 0; k < PCR_LEVEL_VALS; ++k) cf.lv[l][k] = src[k];
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) cf.fin[k] = p.pcr_final[size_t(beam) * p.fin_stride + size_t(j) * PCR_FINAL_VALS + k];
        } else {
            ec = padding_slot<T>().elem;
#pragma unroll
            for (int l = 0; l < LV; ++l)
#pragma unroll
                for (int k = 0; k < PCR_LEVEL_VALS; ++k) cf.lv[l][k] = T(0);
#pragma unroll
            for (int k = 0; k < 5; ++k) cf.fin[k] = T(0);
        }
    };
    if (shared_tables) load_tables(0);
    // FB: the gain (transposed) and the stage's error vectors of the wave's beams live in LDS (the one-wave form uses none otherwise)
    const int fb_n = FB ? p.n_red : 0, fb_n2 = 2 * fb_n, fb_n2p = fb_padded(fb_n2), fb_G = FB ? p.G : 0;
    T* const fbx = reinterpret_cast<T*>(crb_smem);        // [G][2n padded]
    T* const fbK = fbx + size_t(fb_G) * fb_n2p;           // [2n padded][n]
    T* const fbu = fbK + size_t(fb_n2p) * fb_n;           // [G][FBM_UPAD]
    const bool fb_mfma = FB && fb_on_matrix_cores(fb_G, fb_n);
    T fb_af[FBM_MT][FBM_KS];
    if (FB) {
        for (int idx = t; idx < fb_n * fb_n2; idx += NT) {
            const int i = idx / fb_n2, k = idx - i * fb_n2;
            fbK[size_t(k) * fb_n + i] = p.fb_gain[idx];
        }
        for (int idx = t; idx < (fb_n2p - fb_n2) * fb_n; idx += NT) fbK[size_t(fb_n2) * fb_n + idx] = T(0);
        for (int idx = t; idx < fb_G * (fb_n2p - fb_n2); idx += NT)
            fbx[size_t(idx / (fb_n2p - fb_n2)) * fb_n2p + fb_n2 + idx % (fb_n2p - fb_n2)] = T(0);
        __syncthreads();
        if (fb_mfma) fbm_gain_fragments<T>(fb_af, fbK, fb_n, fb_n2p, lane);
    }
    const bool corrected = (p.flags & 4u) != 0;
    const T dt = T(p.dt), hdt = T(0.5 * p.dt), dt6 = T(p.dt / 6.0);
    const size_t plane = size_t(p.n_node) * 4;
    const int n_groups = PACK ? (p.B + p.G - 1) / p.G : p.B;

    // Beam switch without a dependent global load (plans with one table set, one beam per workgroup at a time): while the current
    // beam steps, the NEXT beam's state records and impulse amplitude are already in flight, and the boundary-condition masks
    // are three bits of one register instead of three loads per beam -- in-kernel stamps put those loads at 1.5 of the 2.2 us a
    // beam switch takes (kernarg re-read 0.2, first exchange 0.15, epilogue 0.35).
    constexpr bool PREFETCH = !PACK && !FB;
    T nq[3] = {T(0), T(0), T(0)}, nv[3] = {T(0), T(0), T(0)}, namp = T(0);
    bool have_next = false;
    int mask_bits = 7;
    if (PREFETCH && shared_tables && has_slot) {
        const SlotConst<T>& sc0 = p.slot[j];
        mask_bits = (sc0.mask[0] != T(0) ? 1 : 0) | (sc0.mask[1] != T(0) ? 2 : 0) | (sc0.mask[2] != T(0) ? 4 : 0);
    }
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    CRB_FRESH(kp);
    p = CRB_PARAMS(kp);
    const int beam = PACK ? grp * p.G + pg : grp;
    const bool valid = has_slot && (!PACK || beam < p.B);
    const bool has_left = valid && j >= 1, has_right = valid && j + 1 < S;
    if (!shared_tables) load_tables(valid ? beam : 0);
    T phiR = T(0);
    T gx = p.gx, gy = p.gy;
    if (GRAV && p.gvec && valid) { gx = p.gvec[2 * size_t(beam)]; gy = p.gvec[2 * size_t(beam) + 1]; }   // per-beam ForceParams

    // ---- state
    const size_t node = size_t(valid ? j + p.off : 0);
    const size_t xoff = size_t(valid ? beam : 0) * 2 * plane + node * 4;
    T xq[3] = {T(0), T(0), T(0)}, xv[3] = {T(0), T(0), T(0)};
    T amp = T(0);
    if (PREFETCH && have_next) {                  // (wave-uniform: a real branch, the loads below are not issued)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const bool on = (mask_bits >> c) & 1;
            xq[c] = on ? nq[c] : T(0);
            xv[c] = on ? nv[c] : T(0);
        }
        amp = namp;
    } else if (valid) {
        const SlotConst<T>& sc = p.slot[size_t(beam) * p.slot_stride + j];   // (per-beam masks are not kept in registers)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xq[c] = p.x[xoff + c] * sc.mask[c];
            xv[c] = p.x[xoff + plane + c] * sc.mask[c];
        }
        if (p.amp && j == (p.imp_node_b ? p.imp_node_b[beam] - p.off : p.imp_slot)) amp = p.amp[beam];
    }
    have_next = false;
    if (PREFETCH && shared_tables && grp + int(gridDim.x) < n_groups) {   // (wave-uniform)
        have_next = true;
        if (has_slot) {
            const int nb = grp + int(gridDim.x);
            const size_t noff = size_t(nb) * 2 * plane + size_t(j + p.off) * 4;
#pragma unroll
            for (int c = 0; c < 3; ++c) { nq[c] = p.x[noff + c]; nv[c] = p.x[noff + plane + c]; }
            namp = T(0);
            if (p.amp && j == (p.imp_node_b ? p.imp_node_b[nb] - p.off : p.imp_slot)) namp = p.amp[nb];
        }
    }
    T uh[3] = {T(0), T(0), T(0)};
    if (HELD && valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) uh[c] = p.u_held[size_t(beam) * plane + node * 4 + c];
    }
    int red[3] = {-1, -1, -1};            // FB: reduced indices and reference of this node
    T rq[3] = {T(0), T(0), T(0)}, rv[3] = {T(0), T(0), T(0)};
    if (FB && valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            red[c] = p.red_map[3 * node + c];
            if (red[c] >= 0 && p.fb_ref) {
                rq[c] = p.fb_ref[size_t(beam) * fb_n2 + red[c]];
                rv[c] = p.fb_ref[size_t(beam) * fb_n2 + fb_n + red[c]];
            }
        }
    }

    // ---- left neighbour's q for the very first stage
    T qL[3];
    if (LOGNW == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            qL[c] = lane_lower<T, 1>(xq[c], lane);  // lane 0 reads 0 = clamped / absent root
            if (PACK) qL[c] = has_left ? qL[c] : T(0);   // (a select: the neighbouring beam may hold Inf/NaN)
        }
        if (GRAV) phiR = lane_higher<T, 1>(xq[2], lane);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) recA(ldsA, t, c) = xq[c];
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) qL[c] = recA(ldsA, t_l1, c);
        if (GRAV) phiR = recA(ldsA, t_r1, 2);
        __syncthreads();
    }

    double tc = p.t0;
    T accq[3], accv[3], sq[3], sv[3];  // RK4 accumulators and stage state
    // HELD, control schedule (crb_input_schedule): a run-time test in the HELD instantiations -- steps until the next
    // interval's force takes uh's place (never 0 without a schedule), and that interval's index.  Only these two scalars
    // stay live across the stages: what the reload needs of the launch parameters is re-read through a laundered kernarg
    // pointer inside the branch, and the loads are waited for there, not at uh's first use in every step.
    int sched_left = (HELD && p.sched_stride) ? p.sched_first : -1, sched_k = 0;
    for (int step = 0; step < p.n_steps; ++step) {
        if constexpr (HELD) {
            if (sched_left == 0) {   // (wave-uniform)
                auto kq = kp;
                CRB_FRESH(kq);
                const KParams<T>& q = CRB_PARAMS(kq);
                sched_left = q.sched_hold;
                ++sched_k;
                if (valid) {
                    const T* const u = q.u_held + size_t(sched_k) * q.sched_stride + (size_t(beam) * size_t(q.n_node) + node) * 4;
#pragma unroll
                    for (int c = 0; c < 3; ++c) uh[c] = u[c];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
                    for (int c = 0; c < 3; ++c) asm volatile("" : "+v"(uh[c]));
#endif
                }
            }
            --sched_left;
        }
        const double t_half = __dadd_rn(tc, 0.5 * p.dt), t_full = __dadd_rn(tc, p.dt);
#pragma unroll
        for (int c = 0; c < 3; ++c) { accq[c] = T(0); accv[c] = T(0); sq[c] = xq[c]; sv[c] = xv[c]; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double ts = (s == 0) ? tc : ((s == 3) ? t_full : t_half);
            const bool imp_on = ts < p.duration;  // wave-uniform: the impulse selector stays on the scalar unit
            const T w = (s == 0 || s == 3) ? T(1) : T(2);
            const T cs = (s == 2) ? dt : hdt;

            // -- positions of the next stage (or of the next step after stage 3)
            T qn[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                accq[c] += w * sv[c];
                qn[c] = (s == 3) ? (xq[c] + dt6 * accq[c]) : (xq[c] + cs * sv[c]);
            }
            // -- element force of the element left of this node
            T fl[3], fr[3];
            CRB_SETPRIO(P_FORCE);
            if (EM == EM_NONLINEAR) elem_force_nonlinear<T>(ec.c, qL, sq, false, fl, fr);
            else if (EM == EM_LINEAR) elem_force_linear<T>(ec.c, qL, sq, fl, fr);
            else elem_force<T>(ec, qL, sq, corrected, fl, fr);
            CRB_SETPRIO(P_XCHG);
            T pp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pp[c] = ((imp_on && c == p.imp_dof) ? T(1) : T(0)) * amp - fr[c];
                if (HELD) pp[c] += uh[c];
            }
            if (FB) {   // u = K (r - x) of the stage state (lqr_control.py:95-111)
                T* const e = fbx + size_t(valid ? pg : 0) * fb_n2p;
                if (valid) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (red[c] >= 0) { e[red[c]] = rq[c] - sq[c]; e[fb_n + red[c]] = rv[c] - sv[c]; }
                }
                T ufb[3];
                fb_feedback<T>(fb_mfma, fb_af, fbx, fbK, fbu, fb_G, valid ? pg : 0, fb_n, fb_n2p, lane, valid, red, ufb);
#pragma unroll
                for (int c = 0; c < 3; ++c) pp[c] += ufb[c];
            }
            pp[1] += drag_force<T>(dragc, sv[1]);
            if (GRAV) {
                T g_own[2], g_left[2];
                gravity_segment<T>(has_right ? T(0.5) * (sq[2] + phiR) : sq[2], gx, gy, hm_own, g_own);
                if (LOGNW == 0) {  // segment j-1 IS the left lane's own segment: take its result (bit-identical), one sincos less
                    g_left[0] = lane_lower<T, 1>(g_own[0], lane);
                    g_left[1] = lane_lower<T, 1>(g_own[1], lane);
                    if (PACK) { g_left[0] = has_left ? g_left[0] : T(0); g_left[1] = has_left ? g_left[1] : T(0); }
                } else {
                    gravity_segment<T>(T(0.5) * (qL[2] + sq[2]), gx, gy, hm_left, g_left);
                }
                pp[0] += g_own[0] + g_left[0];
                pp[1] += g_own[1] + g_left[1];
            }

            // -- round A: publish {qn, p, fl}; rebuild r of this node and of both stride-1 neighbours.
            // Outside the beam a neighbour reads as zeros (DPP edge / all-zero LDS record).
            T r[3], rlo[3], rhi[3];
            if (LOGNW == 0) {
                // one wave: no barrier to save by merging, so r is formed first and ITS neighbours are shifted in
                // (4 lane shifts per component instead of the merged round's 6, and 3 subtractions instead of 9;
                //  r of a neighbour is the same subtraction of the same operands, evaluated in the neighbour's lane)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    // (shuffles stay outside any condition: every lane must take part.  Lanes past
                    //  the last slot are padding threads whose p and fl are 0, wave edges shift in 0.)
                    if (GRAV && c == 2) phiR = lane_higher<T, 1>(qn[2], lane);
                    qL[c] = lane_lower<T, 1>(qn[c], lane);
                    const T fl_r1 = lane_higher<T, 1>(fl[c], lane);
                    if (PACK) {   // selects, not 0/1 factors: a neighbouring beam's Inf/NaN must not leak (0 * NaN = NaN)
                        qL[c] = has_left ? qL[c] : T(0);
                        r[c] = pp[c] - (has_right ? fl_r1 : T(0));
                    } else {
                        r[c] = pp[c] - fl_r1;
                    }
                    rlo[c] = lane_lower<T, 1>(r[c], lane);
                    rhi[c] = lane_higher<T, 1>(r[c], lane);
                    if (PACK) { rlo[c] = has_left ? rlo[c] : T(0); rhi[c] = has_right ? rhi[c] : T(0); }
                }
            } else {
                T* bufA = ldsA + ((LOGNW == 1 && (s & 1)) ? size_t(NT + 1) * RN : 0);
                if (SOA) {
                    // r first (one exchange of {qn, fl}), then ITS stride-1 neighbours (a second one): the same 9 stores +
                    // 12 loads as the merged round {qn, p, fl}, 6 subtractions less, one barrier more -- the fp64 stepper is
                    // bound by vector-ALU issue, not by its barriers: 27.72 -> 27.18 us per step at 4096 x 256
                    recA(bufA, t, 0) = qn[0]; recA(bufA, t, 1) = qn[1]; recA(bufA, t, 2) = qn[2];
                    recA(bufA, t, 6) = fl[0]; recA(bufA, t, 7) = fl[1]; recA(bufA, t, 8) = fl[2];
                    __syncthreads();
#pragma unroll
                    for (int c = 0; c < 3; ++c) r[c] = pp[c] - recA(bufA, t_r1, 6 + c);
                    if (GRAV) phiR = recA(bufA, t_r1, 2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) qL[c] = recA(bufA, t_l1, c);
                    recA(bufA, t, 3) = r[0]; recA(bufA, t, 4) = r[1]; recA(bufA, t, 5) = r[2];
                    __syncthreads();
#pragma unroll
                    for (int c = 0; c < 3; ++c) { rlo[c] = recA(bufA, t_l1, 3 + c); rhi[c] = recA(bufA, t_r1, 3 + c); }
                } else {
                    // fp32 records, r first: [qn0 qn1 qn2 - | fl0 fl1 fl2 -] out, the left neighbour's word 0 and the right
                    // one's word 1 (and its phi) in; then [r0 r1 r2 -] (word 2) out and both neighbours' in: 3 stores + 4 loads
                    typedef T rec4 __attribute__((ext_vector_type(4)));
                    rec4* recs = reinterpret_cast<rec4*>(bufA);
                    constexpr int W = RN / 4;   // 16-byte words per record
                    recs[size_t(t) * W + 0] = rec4{qn[0], qn[1], qn[2], T(0)};
                    recs[size_t(t) * W + 1] = rec4{fl[0], fl[1], fl[2], T(0)};
                    __syncthreads();
                    const rec4 lq = recs[size_t(t_l1) * W + 0], rf = recs[size_t(t_r1) * W + 1];
                    if (GRAV) phiR = recs[size_t(t_r1) * W + 0][2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { qL[c] = lq[c]; r[c] = pp[c] - rf[c]; }
                    recs[size_t(t) * W + 2] = rec4{r[0], r[1], r[2], T(0)};
                    __syncthreads();
                    const rec4 rl = recs[size_t(t_l1) * W + 2], rr = recs[size_t(t_r1) * W + 2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { rlo[c] = rl[c]; rhi[c] = rr[c]; }
                }
            }
            pcr_apply_level<T>(cf.lv[0], rlo, rhi, r);

            // -- remaining reduction levels and the final block inverse
            T a[3];
            lean_reduce_tail<T, LV, LOGNW, PACK, RECB>(cf, ldsB, t, lane, j, S, valid, r, a);

            // -- RK4 bookkeeping
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                accv[c] += w * a[c];
                sq[c] = qn[c];
                sv[c] = (s == 3) ? (xv[c] + dt6 * accv[c]) : (xv[c] + cs * a[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { xq[c] = sq[c]; xv[c] = sv[c]; }
        tc = t_full;
        if (p.rec_out && valid && (step + 1) % p.rec_every == 0) {
            const size_t k = size_t((step + 1) / p.rec_every - 1);
            if (p.rec_slot == REC_ALL_SLOTS) {   // whole-state snapshot k: every thread stores its node's two records
                typedef T rec4 __attribute__((ext_vector_type(4)));
                T* snap = p.rec_out + k * size_t(p.B) * 2 * plane + xoff;
                *reinterpret_cast<rec4*>(snap) = rec4{xq[0], xq[1], xq[2], T(0)};
                *reinterpret_cast<rec4*>(snap + plane) = rec4{xv[0], xv[1], xv[2], T(0)};
            } else if (j == p.rec_slot) {
                T val = xq[0];
#pragma unroll
                for (int c = 1; c < 6; ++c) val = (c == p.rec_comp) ? (c < 3 ? xq[c] : xv[c - 3]) : val;
                p.rec_out[size_t(beam) * p.rec_n + k] = val;
            }
        }
    }
    CRB_FRESH(kp);
    p = CRB_PARAMS(kp);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p.x[xoff + c] = xq[c];
            p.x[xoff + plane + c] = xv[c];
        }
        mark_nonfinite<T>(p, beam, xq, xv);
    }
    // (the next beam's first LDS writes come after barriers that follow this beam's last LDS reads: LOGNW >= 2 the
    //  level-1 exchange, LOGNW == 1 the alternating round-A buffers + the two barriers of the first-stage q exchange)
    }
#undef CRB_FRESH
#undef CRB_PARAMS
}

// The register-blocked stepper (crb_step_lean_kernel<double, LS, 2, false, EM, ..., NPL = 4>) with every lane's interior solved
// about its centre node (lean_blocked_body<..., TW = true>; CRB_BLK_TWIST): the instance that blocked plans of nonlinear elements run when their node
// blocks have the mirror structure of equal elements bitwise (crb_blocked.h: blocked_mirrored); the others run the block-Thomas
// instance above.  Four independent one-wave beams per workgroup, two waves per SIMD.
template <typename T, int LS, int EM>
__global__ void __launch_bounds__(256, 2) crb_step_lean_twist_kernel(const KParams<T> p_formal) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) KParams<T>* KP;
    KP kp = (KP)__builtin_amdgcn_kernarg_segment_ptr();   // (as crb_step_lean_kernel reads its parameters)
    (void)p_formal;
#else
    const KParams<T>* kp = &p_formal;
#endif
    lean_blocked_body<T, LS, EM, true>(kp);
}

// ------------------------------------------------------------------ lean stage kernel
// crb_stage_lean_kernel: ONE RK4 stage of the stage-split stepper (crb_rk4_stage: the input force changes per
// stage, e.g. LQR feedback u = K(r - x) evaluated by crb_feedback_force) with the lean stepper's machinery:
// register-resident multipliers, one merged exchange round {p, f_left} + level 0, in-wave levels by DPP.
// A launch is one RHS per beam, so what the generic stage kernel pays most for is re-reading the solve
// tables (440 B per node) for every beam: here a workgroup keeps them in registers and walks over several
// beams (shared-table plans; per-beam tables reload).  The left neighbour's q (and the right neighbour's
// rotation for gravity) are plain global loads of the stage state: no exchange round for them.
//   k = f(t_stage, xs, u_stage + impulse);  acc = (stage ? acc : 0) + w k;
//   stage < 3: out = x + c k;   stage 3: x += dt/6 acc           (same contract as MODE_STAGE)
// Beams of two / four waves move their node records through LDS in memory order (see the kernel); loading the NEXT beam's
// records one beam ahead was measured and is not taken (21.6 against 21.4 us at 2048 x 128, with 56 more registers).
constexpr int STAGE_IO_STREAMS = 7;   // xs q / v, x q / v, acc q / v, u
template <typename T>
__host__ __device__ constexpr size_t stage_lean_lds_bytes(int NT, int lognw) {
    // exchange columns (16-byte multiple) + the record staging of the transposed I/O (beams of more than one wave)
    const size_t cols = sizeof(T) * (size_t(NT + 1) * 6 * (lognw == 1 ? 2 : 1) + 3 * size_t(NT + 1) * size_t(lognw > 1 ? lognw - 1 : 0));
    const size_t io = (lognw > 0 && lognw <= 2) ? size_t(STAGE_IO_STREAMS) * size_t(NT + 1) * 4 * sizeof(T) : 0;   // (eight waves: no room)
    return ((cols + 31) / 32) * 32 + io;
}
template <typename T, int LV, int LOGNW, bool GRAV, int EM>
__global__ void __launch_bounds__(64 << LOGNW, (sizeof(T) == 4 && LOGNW <= 2) ? 3 : lean_minw_f64(LV, LOGNW, GRAV)) crb_stage_lean_kernel(const KParams<T> p) {
    static_assert(LV >= 1, "lean stage kernel needs at least one reduction level");
    constexpr int NW = 1 << LOGNW, NT = 64 << LOGNW, NULLT = NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char crb_smem[];
    T* const ldsA = reinterpret_cast<T*>(crb_smem);                         // [1 or 2][6][NT+1]: p0..2, fl0..2
    T* const ldsB = ldsA + size_t(NT + 1) * 6 * (LOGNW == 1 ? 2 : 1);       // [level-1][3][NT+1]
    // Transposed record I/O (beams of more than one wave).  A wave's slots are every NW-th node, so a thread that loads /
    // stores ITS OWN slot's 32-byte records makes every 16-byte half a memory request of its own (measured at equal
    // node count: 18 us per launch with one wave per beam, 24 with two, 31 with four).  Instead thread t moves the records
    // of node t -- consecutive lanes, consecutive records -- and the records change hands in LDS: staged at the position
    // of the OWNER thread (so that the owner and its stride-1 neighbours read consecutive positions), which also hands
    // the left neighbour's q and the right neighbour's rotation over without loads of their own.
    constexpr bool IO = LOGNW > 0 && LOGNW <= 2;
    typedef T rec4 __attribute__((ext_vector_type(4)));
    constexpr size_t COLS_BYTES = ((sizeof(T) * (size_t(NT + 1) * 6 * (LOGNW == 1 ? 2 : 1) + 3 * size_t(NT + 1) * size_t(LOGNW > 1 ? LOGNW - 1 : 0)) + 31) / 32) * 32;
    rec4* const io = reinterpret_cast<rec4*>(crb_smem + COLS_BYTES);        // [7][NT+1] records, position NT = zeros
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S;
    const int j = (lane << LOGNW) | wave;
    const bool valid = j < S;
    auto thread_of = [](int jj) { return ((jj & (NW - 1)) << 6) | (jj >> LOGNW); };
    const int t_l1 = (valid && j >= 1) ? thread_of(j - 1) : NULLT;
    const int t_r1 = (valid && j + 1 < S) ? thread_of(j + 1) : NULLT;
    const int t_r2 = (valid && j + 2 < S) ? thread_of(j + 2) : NULLT;
    if (LOGNW > 0 && t == 0) {
#pragma unroll
        for (int k = 0; k < 6 * (LOGNW == 1 ? 2 : 1); ++k) ldsA[size_t(k) * (NT + 1) + NULLT] = T(0);
#pragma unroll
        for (int l = 1; l < LOGNW; ++l)
#pragma unroll
            for (int c = 0; c < 3; ++c) ldsB[(size_t(l - 1) * 3 + c) * (NT + 1) + NULLT] = T(0);
    }
    if (IO && t < STAGE_IO_STREAMS) io[size_t(t) * (NT + 1) + NULLT] = rec4{T(0), T(0), T(0), T(0)};
    const bool shared_tables = p.slot_stride == 0 && p.lv_stride == 0 && p.fin_stride == 0;
    const bool corrected = (p.flags & 4u) != 0;
    const bool has_right = valid && j + 1 < S, has_left = valid && j >= 1;
    const size_t node = size_t(valid ? j + p.off : 0);
    // memory side of the transposed I/O: this thread moves the records of slot t (node t + off), whose owner is thread_of(t)
    const bool mvalid = t < S;
    const size_t mnode = size_t(mvalid ? t + p.off : 0);
    const int mpos = mvalid ? thread_of(t) : NULLT;
    const size_t plane = size_t(p.n_node) * 4;
    const T w = (p.stage == 0 || p.stage == 3) ? T(1) : T(2);
    const T cs = (p.stage == 2) ? T(p.dt) : T(0.5 * p.dt);
    const T dt6 = T(p.dt / 6.0);
    const bool imp_on = p.t0 < p.duration;

    ElemCoef<T> ec;
    T dragc = T(0), hm_own = T(0), hm_left = T(0);
    T mask[3] = {T(0), T(0), T(0)}, maskL[3] = {T(0), T(0), T(0)};
    SolveCoef<T, LV> cf;
    auto load_tables = [&](int beam) {
        if (valid) {
            const SlotConst<T>* st = p.slot + size_t(beam) * p.slot_stride;
            const SlotConst<T>& sc = st[j];
            ec = sc.elem;
            dragc = (p.flags & 1u) ? sc.drag : T(0);
#pragma unroll
            for (int c = 0; c < 3; ++c) { mask[c] = sc.mask[c]; maskL[c] = has_left ? st[j - 1].mask[c] : T(0); }
            if (GRAV) { hm_own = sc.half_mass; hm_left = has_left ? st[j - 1].half_mass : T(0); }
#pragma unroll
            for (int l = 0; l < LV; ++l) {
                const T* src = p.pcr_levels + size_t(beam) * p.lv_stride + (size_t(l) * size_t(S) + size_t(j)) * PCR_LEVEL_VALS;
#pragma unroll
                for (int k = 0; k < PCR_LEVEL_VALS; ++k) cf.lv[l][k] = src[k];
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) cf.fin[k] = p.pcr_final[size_t(beam) * p.fin_stride + size_t(j) * PCR_FINAL_VALS + k];
        } else {
            ec = padding_slot<T>().elem;
#pragma unroll
            for (int l = 0; l < LV; ++l)
#pragma unroll
                for (int k = 0; k < PCR_LEVEL_VALS; ++k) cf.lv[l][k] = T(0);
#pragma unroll
            for (int k = 0; k < 5; ++k) cf.fin[k] = T(0);
        }
    };
    if (shared_tables) load_tables(0);

    rec4 pre[STAGE_IO_STREAMS];   // (IO) the records of node t of the beam about to be staged
    auto fetch_io = [&](int beam) {
        const rec4 z = rec4{T(0), T(0), T(0), T(0)};
#pragma unroll
        for (int k = 0; k < STAGE_IO_STREAMS; ++k) pre[k] = z;
        if (mvalid && beam < p.B) {
            auto ldrec = [](const T* ptr) { return *reinterpret_cast<const rec4*>(ptr); };
            const size_t moff = size_t(beam) * 2 * plane + mnode * 4;
            pre[0] = ldrec(p.xs + moff); pre[1] = ldrec(p.xs + moff + plane);
            pre[2] = ldrec(p.x + moff); pre[3] = ldrec(p.x + moff + plane);
            if (p.stage > 0) { pre[4] = ldrec(p.acc + moff); pre[5] = ldrec(p.acc + moff + plane); }
            if (p.u_held) pre[6] = ldrec(p.u_held + size_t(beam) * plane + mnode * 4);
        }
    };
    int it = 0;
    for (int beam = blockIdx.x; beam < p.B; beam += gridDim.x, ++it) {
        if (!shared_tables) load_tables(beam);
        if (IO) fetch_io(beam);
        // ---- this stage's state, the neighbours' pieces of it, the input force
        const size_t xoff = size_t(beam) * 2 * plane + node * 4;
        T sq[3] = {T(0), T(0), T(0)}, sv[3] = {T(0), T(0), T(0)}, qL[3] = {T(0), T(0), T(0)}, uin[3] = {T(0), T(0), T(0)};
        T x0q[3] = {T(0), T(0), T(0)}, x0v[3] = {T(0), T(0), T(0)}, aq[3] = {T(0), T(0), T(0)}, av[3] = {T(0), T(0), T(0)};
        T phiR = T(0), amp = T(0);
        if (IO) {
            auto at = [&](int k, int pos) -> rec4& { return io[size_t(k) * (NT + 1) + pos]; };
            if (mvalid) {
#pragma unroll
                for (int k = 0; k < STAGE_IO_STREAMS; ++k) at(k, mpos) = pre[k];
            }
            __syncthreads();
            const int own = valid ? t : NULLT;
            const rec4 rq = at(0, own), rv = at(1, own), bq = at(2, own), bv = at(3, own), cq = at(4, own), cv = at(5, own), ru = at(6, own);
            const rec4 rl = at(0, t_l1);
            if (GRAV) phiR = at(0, t_r1)[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sq[c] = rq[c] * mask[c];
                sv[c] = rv[c] * mask[c];
                qL[c] = rl[c] * maskL[c];
                x0q[c] = bq[c] * mask[c];
                x0v[c] = bv[c] * mask[c];
                aq[c] = cq[c];
                av[c] = cv[c];
                uin[c] = ru[c];
            }
            if (valid && p.amp && j == (p.imp_node_b ? p.imp_node_b[beam] - p.off : p.imp_slot)) amp = p.amp[beam];
        } else if (valid) {
            // a node record is 4 values = one aligned 32-byte (fp64) / 16-byte (fp32) vector: whole-record
            // loads instead of three scalar ones (the slots of a wave are every NW-th node, so scalar loads
            // would pull each 128-byte line through L1 once per component: measured 31.7 -> 24 us)
            auto ldrec = [](const T* ptr) { return *reinterpret_cast<const rec4*>(ptr); };
            const rec4 rq = ldrec(p.xs + xoff), rv = ldrec(p.xs + xoff + plane);
            const rec4 bq = ldrec(p.x + xoff), bv = ldrec(p.x + xoff + plane);
            rec4 rl = rec4{T(0), T(0), T(0), T(0)}, cq = rl, cv = rl, ru = rl;
            if (has_left) rl = ldrec(p.xs + xoff - 4);
            if (p.stage > 0) { cq = ldrec(p.acc + xoff); cv = ldrec(p.acc + xoff + plane); }
            if (p.u_held) ru = ldrec(p.u_held + size_t(beam) * plane + node * 4);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sq[c] = rq[c] * mask[c];
                sv[c] = rv[c] * mask[c];
                qL[c] = rl[c] * maskL[c];
                x0q[c] = bq[c] * mask[c];
                x0v[c] = bv[c] * mask[c];
                aq[c] = cq[c];
                av[c] = cv[c];
                uin[c] = ru[c];
            }
            if (GRAV && has_right) phiR = p.xs[xoff + 4 + 2];
            if (p.amp && j == (p.imp_node_b ? p.imp_node_b[beam] - p.off : p.imp_slot)) amp = p.amp[beam];
        }
        // ---- forces on this node from its own element, drag, gravity, inputs
        T fl[3], fr[3];
        CRB_SETPRIO(P_FORCE);
        if (EM == EM_NONLINEAR) elem_force_nonlinear<T>(ec.c, qL, sq, false, fl, fr);
        else if (EM == EM_LINEAR) elem_force_linear<T>(ec.c, qL, sq, fl, fr);
        else elem_force<T>(ec, qL, sq, corrected, fl, fr);
        CRB_SETPRIO(P_XCHG);
        T pp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) pp[c] = uin[c] + ((imp_on && c == p.imp_dof) ? T(1) : T(0)) * amp - fr[c];
        pp[1] += drag_force<T>(dragc, sv[1]);
        if (GRAV) {
            T g_own[2], g_left[2];
            T gx = p.gx, gy = p.gy;
            if (p.gvec) { gx = p.gvec[2 * size_t(beam)]; gy = p.gvec[2 * size_t(beam) + 1]; }   // per-beam ForceParams
            gravity_segment<T>(has_right ? T(0.5) * (sq[2] + phiR) : sq[2], gx, gy, hm_own, g_own);
            if (LOGNW == 0) {  // (as in the stepper: the left lane's own segment)
                g_left[0] = lane_lower<T, 1>(g_own[0], lane);
                g_left[1] = lane_lower<T, 1>(g_own[1], lane);
            } else {
                gravity_segment<T>(T(0.5) * (qL[2] + sq[2]), gx, gy, hm_left, g_left);
            }
            pp[0] += g_own[0] + g_left[0];
            pp[1] += g_own[1] + g_left[1];
        }
        // ---- round A: publish {p, fl}, rebuild r of this node and of both stride-1 neighbours, level 0
        T r[3], rlo[3], rhi[3];
        if (LOGNW == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                r[c] = pp[c] - lane_higher<T, 1>(fl[c], lane);   // (one wave: r first, then ITS neighbours -- see the stepper)
                rlo[c] = lane_lower<T, 1>(r[c], lane);
                rhi[c] = lane_higher<T, 1>(r[c], lane);
            }
        } else {
            T* bufA = ldsA + ((LOGNW == 1 && (it & 1)) ? size_t(NT + 1) * 6 : 0);
            auto col = [&](int k, int th) -> T& { return bufA[size_t(k) * (NT + 1) + th]; };
#pragma unroll
            for (int c = 0; c < 3; ++c) { col(c, t) = pp[c]; col(3 + c, t) = fl[c]; }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                rlo[c] = col(c, t_l1) - fl[c];
                r[c] = pp[c] - col(3 + c, t_r1);
                rhi[c] = col(c, t_r1) - col(3 + c, t_r2);
            }
        }
        pcr_apply_level<T>(cf.lv[0], rlo, rhi, r);
        T a[3];
        lean_reduce_tail<T, LV, LOGNW>(cf, ldsB, t, lane, j, S, valid, r, a);
        // ---- RK4 bookkeeping of this stage
        if (IO) {
            auto at = [&](int k, int pos) -> rec4& { return io[size_t(k) * (NT + 1) + pos]; };
            T nq[3], nv[3], oq[3], ov[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                nq[c] = (p.stage ? aq[c] : T(0)) + w * sv[c];
                nv[c] = (p.stage ? av[c] : T(0)) + w * a[c];
                oq[c] = (p.stage < 3) ? x0q[c] + cs * sv[c] : x0q[c] + dt6 * nq[c];
                ov[c] = (p.stage < 3) ? x0v[c] + cs * a[c] : x0v[c] + dt6 * nv[c];
            }
            if (valid && p.stage == 3) mark_nonfinite<T>(p, beam, oq, ov);
            // (the staging is free again: every thread read its inputs before the barrier of round A)
            if (valid) {
                at(0, t) = rec4{oq[0], oq[1], oq[2], T(0)}; at(1, t) = rec4{ov[0], ov[1], ov[2], T(0)};
                if (p.stage < 3) { at(2, t) = rec4{nq[0], nq[1], nq[2], T(0)}; at(3, t) = rec4{nv[0], nv[1], nv[2], T(0)}; }
            }
            __syncthreads();
            if (mvalid) {
                const size_t moff = size_t(beam) * 2 * plane + mnode * 4;
                auto strec = [](T* ptr, const rec4 v) { *reinterpret_cast<rec4*>(ptr) = v; };
                if (p.stage < 3) {   // (whole records: the pad value is written as 0)
                    strec(p.out + moff, at(0, mpos)); strec(p.out + moff + plane, at(1, mpos));
                    strec(p.acc + moff, at(2, mpos)); strec(p.acc + moff + plane, at(3, mpos));
                } else {
                    strec(p.x + moff, at(0, mpos)); strec(p.x + moff + plane, at(1, mpos));
                }
            }
            __syncthreads();   // the next beam's records may be staged only after these reads
        } else if (valid) {
            auto strec = [](T* ptr, const T v[3]) { *reinterpret_cast<rec4*>(ptr) = rec4{v[0], v[1], v[2], T(0)}; };
            T nq[3], nv[3], oq[3], ov[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                nq[c] = (p.stage ? aq[c] : T(0)) + w * sv[c];
                nv[c] = (p.stage ? av[c] : T(0)) + w * a[c];
                oq[c] = (p.stage < 3) ? x0q[c] + cs * sv[c] : x0q[c] + dt6 * nq[c];
                ov[c] = (p.stage < 3) ? x0v[c] + cs * a[c] : x0v[c] + dt6 * nv[c];
            }
            if (p.stage < 3) {   // (whole records: the pad value is written as 0)
                strec(p.out + xoff, oq); strec(p.out + xoff + plane, ov);
                strec(p.acc + xoff, nq); strec(p.acc + xoff + plane, nv);
            } else {
                strec(p.x + xoff, oq); strec(p.x + xoff + plane, ov);
                mark_nonfinite<T>(p, beam, oq, ov);
            }
        }
        // LOGNW >= 2: the level-1 barrier above orders this beam's round-A reads before the next beam's
        // round-A writes; LOGNW == 1 alternates two round-A buffers; LOGNW == 0 uses no LDS
    }
}

}  // namespace crb
