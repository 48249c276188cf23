// crb_lean_launch.h -- host entry of the lean stepper's translation units (crb_lean.hip is compiled once
// per dtype so that the kernel instantiations build in parallel with the rest of the library).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_kernels.h"

namespace crb {
// ---- The shapes every lean family is built for.  crb_lean.hip instantiates a kernel exactly where its function holds, and
// the eligibility predicates of crbeam.hip ask the same function: adding or dropping an instance is an edit here alone.
// (f64: the plan's dtype; levels: the reduction levels the kernel runs; lognw: log2 of the waves per beam.)
// One-wave beams run 3 .. 6 levels.  Beams of more than 64 slots run the TRUNCATED reduction (their full one has >= 7
// levels): the level count is where the multipliers fall below the unit roundoff -- 5 (6 for slowly decaying mass
// matrices) in fp64, 4 (5) in fp32.
constexpr bool lean_levels_built(bool f64, int levels, int lognw) {
    const int lv_long = f64 ? 5 : 4;
    return lognw == 0 ? (levels >= 3 && levels <= 6) : (levels == lv_long || levels == lv_long + 1);
}
// the stepper and the stage kernel: up to 8 waves per beam
constexpr bool lean_step_built(bool f64, int levels, int lognw) { return lognw >= 0 && lognw <= 3 && lean_levels_built(f64, levels, lognw); }
constexpr bool lean_stage_built(bool f64, int levels, int lognw) { return lean_step_built(f64, levels, lognw); }
// the register-blocked stepper: fp64, `levels` separator levels, one element kind
constexpr bool lean_blocked_built(bool f64, int levels, int elem_mode) {
    return f64 && levels == 3 && (elem_mode == EM_LINEAR || elem_mode == EM_NONLINEAR);
}
// the packed stepper with the feedback inside its stages (one wave)
constexpr bool lean_feedback_built(int levels) { return levels >= 3 && levels <= 5; }
// RK45 with the lean RHS: up to 4 waves per beam
constexpr bool lean_rk45_built(bool f64, int levels, int lognw) { return lognw >= 0 && lognw <= 2 && lean_levels_built(f64, levels, lognw); }
// the implicit kernel, fp64 (crb_step_implicit refuses fp32): one beam per workgroup of 1 / 2 / 4 waves at 5 levels of A
// .. the full count of that width (33 .. 64 / 65 .. 128 / 129 .. 256 slots); several beams per wave at 3 .. 5 levels
constexpr bool lean_implicit_built(bool f64, int levels, int lognw) { return f64 && lognw >= 0 && lognw <= 2 && levels >= 5 && levels <= 6 + lognw; }
constexpr bool lean_implicit_pack_built(bool f64, int levels) { return f64 && levels >= 3 && levels <= 5; }
// ... and with a control schedule (KParams sched_*): the SCHED instantiation of every shape the family builds and of no
// other -- a scheduled call must run the arithmetic of the chain of held-force calls it stands for, so it runs the lean
// kernel exactly where they do.  (Shapes whose SCHED instance would spill at two waves per SIMD are built at one:
// implicit_lean_sched_minw in crb_stiff.h.)
constexpr bool lean_implicit_sched_built(bool f64, int levels, int lognw) { return lean_implicit_built(f64, levels, lognw); }
constexpr bool lean_implicit_pack_sched_built(bool f64, int levels) { return lean_implicit_pack_built(f64, levels); }

// ---- The launchers: hipErrorInvalidValue for a shape that is not built.
// launches crb_step_lean_kernel<T, levels, lognw, grav, elem_mode> on `n_beams` workgroups (lean_step_built)
hipError_t launch_lean(const KParams<double>& k, int n_beams, int levels, int lognw, bool grav, int elem_mode, hipStream_t st);
hipError_t launch_lean(const KParams<float>& k, int n_beams, int levels, int lognw, bool grav, int elem_mode, hipStream_t st);
// launches the register-blocked stepper crb_step_lean_kernel<double, levels, 2, false, elem_mode, ..., NPL = 4> (one wave per
// 256-slot beam, four beams per workgroup; k.blocked = the plan's blocked tables; lean_blocked_built); twist: its form with the
// interiors solved about their centre nodes, crb_step_lean_twist_kernel<double, levels, elem_mode>, whose table the plan then holds
hipError_t launch_lean_blocked(const KParams<double>& k, int n_beams, int levels, int elem_mode, bool twist, hipStream_t st);
// launches the packed one-wave stepper with the LQR feedback inside its stages (crb_step_lean_kernel<..., FB>): k.G >= 2 beams
// per wave, gain / reference / reduced map in k (lean_feedback_built)
hipError_t launch_lean_feedback(const KParams<double>& k, int n_beams, int levels, bool grav, hipStream_t st);
hipError_t launch_lean_feedback(const KParams<float>& k, int n_beams, int levels, bool grav, hipStream_t st);
// launches crb_stage_lean_kernel<T, levels, lognw, grav, elem_mode> on `n_groups` workgroups (each walks
// over beams blockIdx.x, blockIdx.x + n_groups, ...; lean_stage_built)
hipError_t launch_stage_lean(const KParams<double>& k, int n_groups, int levels, int lognw, bool grav, int elem_mode, hipStream_t st);
hipError_t launch_stage_lean(const KParams<float>& k, int n_groups, int levels, int lognw, bool grav, int elem_mode, hipStream_t st);
// launches crb_rk45_kernel with the lean RHS (plans without gravity, one beam per workgroup; lean_rk45_built)
hipError_t launch_rk45_lean(const KParams<double>& k, const Rk45Params& q, int n_beams, int levels, int lognw, int elem_mode, hipStream_t st);
hipError_t launch_rk45_lean(const KParams<float>& k, const Rk45Params& q, int n_beams, int levels, int lognw, int elem_mode, hipStream_t st);
// launches crb_implicit_lean_kernel (crb_stiff.h) on `groups` workgroups, each walking over beams, at `levels` levels of A:
// where its reduction stops for the step size at hand (crbeam.hip: stiff_tables).  k.G > 1: several beams per wave
// (lean_implicit_pack_built), else one beam per workgroup (lean_implicit_built)
hipError_t launch_implicit_lean(const KParams<double>& k, const StiffParams<double>& q, int groups, int levels, int lognw,
                                bool grav, int elem_mode, hipStream_t st);
hipError_t launch_implicit_lean(const KParams<float>& k, const StiffParams<float>& q, int groups, int levels, int lognw,
                                bool grav, int elem_mode, hipStream_t st);
}  // namespace crb
