// crb_host.h -- host-side helpers shared by the launch translation units (crbeam.hip, crb_lean.hip, crb_loop.hip,
// crb_ctrl.hip, crb_static.hip): the runtime switches and the mechanics of a launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "crb_generic.h"

namespace crb {

// Runtime switches.  Each is read when the call it steers is made (the tests flip them between calls on one ensemble),
// CRB_HOST_SPIN_MS alone at plan creation.  (switch: effect -- test of tests/test_gpu_parity.py that sets it)
//   CRB_DISABLE_LEAN: the general kernels on every path -- test_held_force_on_lean_size_beams,
//       test_adaptive_rk45_lean_rhs_equals_general_rhs, test_gravity_rotation_kernels_over_small_and_large_angles
//   CRB_DISABLE_BLOCKED: crb_step_rk4 of plans the register-blocked stepper takes (fp64 uniform 256-slot beams) runs the
//       one-node-per-lane lean stepper instead -- tests/test_blocked_stepper.py
//   CRB_DISABLE_LEAN_STAGE: the general kernel for crb_rk4_stage -- test_lean_stage_kernel_feedback_rollout_matches_oracle
//   CRB_DISABLE_LEAN_IMPLICIT: the general kernels for the implicit and the controlled implicit steppers --
//       test_implicit_lean_kernel_equals_the_general_one, test_controlled_implicit_kernel_takes_the_oracles_steps,
//       test_implicit_reduction_levels_follow_the_step_size
//   CRB_DISABLE_LEAN_FEEDBACK: the general kernels for the fused and the controlled closed loops --
//       test_fused_feedback_stepper_matches_the_stage_split_one_and_the_oracle,
//       test_controlled_closed_loop_kernel_takes_the_oracles_steps
//   CRB_FUSED_FEEDBACK=0|1: crb_step_rk4_feedback never / whenever the gain fits LDS in its fused form (unset: chosen by
//       size) -- test_fused_feedback_stepper_matches_the_stage_split_one_and_the_oracle,
//       test_fused_feedback_stepper_walks_over_groups_of_beams
//   CRB_IMPLICIT_FEEDBACK=0|1: crb_step_implicit_feedback as a chain of one GEMM and one implicit launch per sample / in its
//       in-kernel form wherever the gain fits LDS (unset: there, for ensembles whose workgroups are all resident) --
//       tests/test_implicit_feedback.py
//   CRB_CTRL_STREAM_GAIN=1: crb_solve_controlled's closed loop reads the gain from global memory even where it fits LDS --
//       test_controlled_closed_loop_large.py::test_streamed_gain_on_small_gains_takes_the_same_steps
//   CRB_LOOP=0|1: crb_step_rk4_feedback never / whenever eligible in its persistent form (unset: 512 beams and more) --
//       test_persistent_closed_loop_stepper_matches_the_oracle_and_the_stage_split_path,
//       test_per_beam_status_reports_the_launch_in_which_a_beam_went_non_finite
//   CRB_LOOP_FENCES=1: release / acquire fences around the persistent stepper's hand-offs --
//       test_persistent_closed_loop_stepper_with_release_acquire_fences
//   CRB_LOOP_MAX_GROUPS: groups of workgroups of the persistent stepper (several row blocks per group) --
//       test_persistent_closed_loop_stepper_matches_the_oracle_and_the_stage_split_path
//   CRB_LEAN_MAX_GROUPS: workgroups of the lean kernels that walk over beams -- test_workgroups_walking_over_beams_match_one_workgroup_per_beam,
//       test_implicit_lean_kernel_equals_the_general_one, test_fused_feedback_stepper_walks_over_groups_of_beams
//   CRB_LEAN_NO_WALK: one workgroup per beam for the lean stepper -- test_workgroups_walking_over_beams_match_one_workgroup_per_beam
//   CRB_STAGE_GROUPS: workgroups of the lean stage kernel -- test_lean_stage_kernel_feedback_rollout_matches_oracle
//   CRB_FEEDBACK_TILE=48|32: tile of the feedback GEMM -- test_fused_mfma_feedback_force_matches_matmul,
//       test_fp32_feedback_force_and_rollout
//   CRB_STIFF_ALL_LEVELS: the implicit stepper keeps every reduction level of A -- test_implicit_reduction_levels_follow_the_step_size
//   CRB_LOOP_TIMEOUT_MS: how long a hand-off of the persistent stepper waits before it gives up (default 2000) -- none
//   CRB_HOST_SPIN_MS: how long a host-vector call spins on its completion flag (default 200) -- none
inline const char* env(const char* name) { return std::getenv(name); }
inline bool env_set(const char* name) { return env(name) != nullptr; }
inline long env_int(const char* name, long unset) {
    const char* v = env(name);
    return v ? std::atol(v) : unset;
}

// Grid of a launch whose workgroups walk over `groups` groups of beams: at most `cap` workgroups (cap <= 0: no limit),
// the groups split evenly over them (4096 beams on 512 workgroups = 8 each).
inline int walk_grid(int groups, int cap) {
    if (cap <= 0 || groups <= cap) return groups;
    const int rounds = (groups + cap - 1) / cap;
    return (groups + rounds - 1) / rounds;
}

// Dynamic LDS above 64 KiB must be opted into per kernel (the CU has 160 KiB).
template <typename K>
hipError_t lds_opt_in(K kernel, size_t bytes) {
    if (bytes <= size_t(64) * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
}

// Workgroups a launch of `Kernel` keeps resident on the device: CUs x workgroups per CU by the occupancy query, asked once
// per kernel (every device of a node is the same part).  A failed query returns its error and leaves *groups = 0, which
// walk_grid reads as "no cap".
template <auto Kernel>
hipError_t resident_groups(int threads, size_t smem, int* groups) {
    static int resident = -1;
    if (resident < 0) {
        int dev = 0, cus = 0, per_cu = 0;
        *groups = 0;
        hipError_t e;
        if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
        if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, threads, smem)) != hipSuccess) return e;
        resident = cus * per_cu;
    }
    *groups = resident;
    return hipSuccess;
}

// One table set for the whole ensemble (k: a plan or a kernel parameter block): a workgroup may keep its rows of the
// tables and walk over several beams.
template <typename K>
bool shared_tables(const K& k) { return k.slot_stride == 0 && k.lv_stride == 0 && k.fin_stride == 0; }

// Run-time value -> template argument: calls f(std::integral_constant<int, V>()) for the V in LO .. HI that equals v (one
// instantiation of f's body per V) and returns its result; none() -- hipErrorInvalidValue when not given -- for any other v.
// A launcher builds an instance exactly where its family's ..._built(...) holds (crb_*_launch.h) with `if constexpr` inside f.
template <int LO, int HI, typename F, typename N>
auto with_int(int v, F&& f, N&& none) -> decltype(none()) {
    if (v == LO) return f(std::integral_constant<int, LO>());
    if constexpr (LO < HI) return with_int<LO + 1, HI>(v, f, none);
    else return none();
}
template <int LO, int HI, typename F>
hipError_t with_int(int v, F&& f) {
    return with_int<LO, HI>(v, f, [] { return hipErrorInvalidValue; });
}
template <typename F>
auto with_bool(bool b, F&& f) { return b ? f(std::true_type()) : f(std::false_type()); }
// the element kinds of a plan: anything but all-linear / all-nonlinear runs the per-lane branch
template <typename F>
auto with_elem_mode(int em, F&& f) {
    switch (em) {
        case EM_LINEAR: return f(std::integral_constant<int, EM_LINEAR>());
        case EM_NONLINEAR: return f(std::integral_constant<int, EM_NONLINEAR>());
        default: return f(std::integral_constant<int, EM_MIXED>());
    }
}

}  // namespace crb
