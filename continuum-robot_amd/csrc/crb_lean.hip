// crb_lean.hip -- instantiations and launch of the lean kernels for ONE dtype (-DCRB_LEAN_T=double|float).  Which shapes
// are built is stated in crb_lean_launch.h (lean_*_built); the launchers below instantiate exactly those.
#include "crb_host.h"
#include "crb_lean_launch.h"

#ifndef CRB_LEAN_T
#error "compile with -DCRB_LEAN_T=double or -DCRB_LEAN_T=float"
#endif

namespace crb {
namespace {
typedef CRB_LEAN_T T;
constexpr bool F64 = sizeof(T) == 8;

// Grid of workgroups that walk over `groups` groups of beams: what the device keeps resident, split evenly (4096 beams =
// 8 beams for each of 512 workgroups); no cap where the occupancy query fails
template <auto Kernel>
int walking_grid(int groups, int threads, size_t smem) {
    int resident = 0;
    (void)resident_groups<Kernel>(threads, smem, &resident);
    return walk_grid(groups, int(env_int("CRB_LEAN_MAX_GROUPS", resident)));
}

template <int LV, int LOGNW, bool GRAV, int EM, bool HELD, bool PACK = false>
hipError_t one_held(const KParams<T>& k, int n_beams, hipStream_t st) {
    const int groups = PACK ? (n_beams + k.G - 1) / k.G : n_beams;
    const size_t smem = lean_lds_bytes<T>(64 << LOGNW, LOGNW);
    constexpr auto kernel = crb_step_lean_kernel<T, LV, LOGNW, GRAV, EM, HELD, PACK>;
    if (hipError_t e = lds_opt_in(kernel, smem)) return e;
    // Shared-table plans: a workgroup loads its rows of the solve tables once and walks over several beams.
    // Per-beam tables are reloaded per beam anyway: one workgroup per beam, dispatched by the hardware.
    const bool walk = shared_tables(k) && !env_set("CRB_LEAN_NO_WALK");
    const int grid = walk ? walking_grid<kernel>(groups, 64 << LOGNW, smem) : groups;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 << LOGNW), smem, st, k);
    return hipGetLastError();
}
template <int LV, int LOGNW, bool GRAV, int EM>
hipError_t one(const KParams<T>& k, int n_beams, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return one_held<LV, LOGNW, GRAV, EM, false>(k, n_beams, st);
#else
    if (LOGNW == 0 && k.G > 1)   // several beams per wave
        return k.u_held ? one_held<LV, 0, GRAV, EM, true, true>(k, n_beams, st) : one_held<LV, 0, GRAV, EM, false, true>(k, n_beams, st);
    return k.u_held ? one_held<LV, LOGNW, GRAV, EM, true>(k, n_beams, st) : one_held<LV, LOGNW, GRAV, EM, false>(k, n_beams, st);
#endif
}
template <int LV, int LOGNW, bool GRAV, int EM>
hipError_t one_stage(const KParams<T>& k, int n_groups, hipStream_t st) {
    constexpr auto kernel = crb_stage_lean_kernel<T, LV, LOGNW, GRAV, EM>;
    const size_t smem = stage_lean_lds_bytes<T>(64 << LOGNW, LOGNW);
    if (hipError_t e = lds_opt_in(kernel, smem)) return e;
    hipLaunchKernelGGL(kernel, dim3(n_groups), dim3(64 << LOGNW), smem, st, k);
    return hipGetLastError();
}
// STAGE selects the kernel family: the fused multi-step stepper or the one-stage kernel.  It is tested at run time on
// purpose: a unit that launches one family holds the other one too, as the units always have.  The compiler optimises a
// unit as a whole, and with one family left out it generates other code for the eight-wave fp64 kernels that remain.
template <bool GRAV, bool STAGE>
hipError_t by_shape(const KParams<T>& k, int n, int levels, int lognw, int em, hipStream_t st) {
    return with_int<0, MAX_LV>(levels, [&](auto lv) { return with_int<0, 3>(lognw, [&](auto nw) { return with_elem_mode(em, [&](auto e) {
        static_assert(lean_stage_built(F64, lv, nw) == lean_step_built(F64, lv, nw), "the two families share their shapes");
        if constexpr (lean_step_built(F64, lv, nw))
            return STAGE ? one_stage<lv, nw, GRAV, e>(k, n, st) : one<lv, nw, GRAV, e>(k, n, st);
        else return hipErrorInvalidValue;
    }); }); });
}
template <int LV, int LNW, int EM>
hipError_t one_rk45(const KParams<T>& k, const Rk45Params& q, int n_beams, hipStream_t st) {
    constexpr int NT = 64 << LNW;
    // waves per SIMD the register allocation aims at: two, with 60 .. 160 spilled VGPRs -- measured against a spill-free
    // build at one wave per SIMD on single-wave beams: 4096 x 64 integrates in 1.26 ms against 1.76 ms (1024 x 64: 0.60 against 0.54)
    constexpr int MINW = 2;
    constexpr auto kernel = crb_rk45_kernel<T, LV, 256, MINW, LNW, EM>;
    const size_t smem = rk45_lds_bytes<T>(NT, true);
    if (hipError_t e = lds_opt_in(kernel, smem)) return e;
    hipLaunchKernelGGL(kernel, dim3(n_beams), dim3(NT), smem, st, k, q);
    return hipGetLastError();
}
}  // namespace

// The instantiations are spread over translation units that build in parallel (Makefile: -DCRB_LEAN_PART=1|2|3 per
// dtype; undefined = everything in one unit, the `make fast` tuning build): 1 = stepper without gravity (+ the
// dispatcher), 2 = stepper with nearest-neighbour gravity, 3 = one-stage kernel, RK45 with the lean RHS, implicit kernel.
#ifndef CRB_LEAN_PART
#define CRB_LEAN_PART 0
#endif
hipError_t launch_lean_grav(const KParams<T>& k, int n_beams, int levels, int lognw, int elem_mode, hipStream_t st);

#if CRB_LEAN_PART == 0 || CRB_LEAN_PART == 3
hipError_t launch_rk45_lean(const KParams<T>& k, const Rk45Params& q, int n_beams, int levels, int lognw, int elem_mode, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return hipErrorInvalidValue;
#else
    return with_int<0, MAX_LV>(levels, [&](auto lv) { return with_int<0, 3>(lognw, [&](auto nw) {
        if constexpr (lean_rk45_built(F64, lv, nw))
            return with_elem_mode(elem_mode, [&](auto e) { return one_rk45<lv, nw, e>(k, q, n_beams, st); });
        else return hipErrorInvalidValue;
    }); });
#endif
}
#endif

#if CRB_LEAN_PART == 0 || CRB_LEAN_PART == 2
hipError_t launch_lean_grav(const KParams<T>& k, int n_beams, int levels, int lognw, int elem_mode, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return hipErrorInvalidValue;
#else
    return by_shape<true, false>(k, n_beams, levels, lognw, elem_mode, st);
#endif
}
#endif

#if CRB_LEAN_PART == 0 || CRB_LEAN_PART == 1
namespace {
template <int LS, int EM, bool TW>
hipError_t one_blocked(const KParams<T>& k, int n_beams, hipStream_t st) {
    // NPL = 4: a wave is a beam, a workgroup four of them; shared-table plans only, so the workgroups walk over groups of beams
    // (TW: the instance with the twisted interior solve)
    constexpr auto kernel = [] {
        if constexpr (TW) return crb_step_lean_twist_kernel<T, LS, EM>;
        else return crb_step_lean_kernel<T, LS, 2, false, EM, false, false, false, BLK_NPL>;
    }();
    const size_t smem = blk_lds_bytes(LS);   // the separator tables and the waves' strips
    const int groups = (n_beams + 3) / 4;
    const int grid = env_set("CRB_LEAN_NO_WALK") ? groups : walking_grid<kernel>(groups, 256, smem);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), smem, st, k);
    return hipGetLastError();
}
}  // namespace
hipError_t launch_lean_blocked(const KParams<T>& k, int n_beams, int levels, int elem_mode, bool twist, hipStream_t st) {
    if (!k.blocked || (twist && !CRB_BLK_TWIST)) return hipErrorInvalidValue;
#ifdef CRB_FAST_BUILD   // (make fast: the config-3 instance, in both forms of the interior solve)
    if constexpr (F64)
        if (levels == 3 && elem_mode == EM_NONLINEAR) {
            if constexpr (CRB_BLK_TWIST)
                if (twist) return one_blocked<3, EM_NONLINEAR, true>(k, n_beams, st);
            return one_blocked<3, EM_NONLINEAR, false>(k, n_beams, st);
        }
    return hipErrorInvalidValue;
#else
    return with_int<0, MAX_LV>(levels, [&](auto ls) { return with_elem_mode(elem_mode, [&](auto e) {
        if constexpr (lean_blocked_built(F64, ls, e)) {
            if constexpr (CRB_BLK_TWIST && e == EM_NONLINEAR)
                if (twist) return one_blocked<ls, e, true>(k, n_beams, st);
            if (twist) return hipErrorInvalidValue;
            return one_blocked<ls, e, false>(k, n_beams, st);
        } else return hipErrorInvalidValue;
    }); });
#endif
}
#endif

#if (CRB_LEAN_PART == 0 || CRB_LEAN_PART == 1) && !defined(CRB_FAST_BUILD)
// the packed one-wave stepper with the state feedback inside its stages (crb_step_lean_kernel<..., FB>): k.G >= 2 beams per wave,
// gain / reference / reduced map in k; mixed element kinds are evaluated per lane
namespace {
template <int LV, bool GRAV>
hipError_t one_fb(const KParams<T>& k, int n_beams, hipStream_t st) {
    constexpr auto kernel = crb_step_lean_kernel<T, LV, 0, GRAV, EM_MIXED, false, true, true>;
    const size_t smem = fb_lean_lds_bytes<T>(k.G, k.n_red);
    if (hipError_t e = lds_opt_in(kernel, smem)) return e;
    const int groups = (n_beams + k.G - 1) / k.G;
    // (shared tables: a workgroup loads its tables and the gain once and walks over several groups of beams)
    const int grid = shared_tables(k) ? walking_grid<kernel>(groups, 64, smem) : groups;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), smem, st, k);
    return hipGetLastError();
}
}  // namespace
hipError_t launch_lean_feedback(const KParams<T>& k, int n_beams, int levels, bool grav, hipStream_t st) {
    if (k.G < 2 || !k.fb_gain || !k.red_map) return hipErrorInvalidValue;
    return with_int<0, MAX_LV>(levels, [&](auto lv) { return with_bool(grav, [&](auto g) {
        if constexpr (lean_feedback_built(lv)) return one_fb<lv, g>(k, n_beams, st);
        else return hipErrorInvalidValue;
    }); });
}
#endif

#if CRB_LEAN_PART == 0 || CRB_LEAN_PART == 1
hipError_t launch_lean(const KParams<T>& k, int n_beams, int levels, int lognw, bool grav, int elem_mode, hipStream_t st) {
#ifdef CRB_FAST_BUILD  // kernel-tuning build (make fast): only the config-3 instance
    if (sizeof(T) == 8 && levels == 5 && lognw == 2 && !grav && elem_mode == EM_NONLINEAR)
        return one<5, 2, false, EM_NONLINEAR>(k, n_beams, st);
    if (sizeof(T) == 4 && levels == 4 && lognw == 2 && !grav && elem_mode == EM_NONLINEAR)   // (make fast32)
        return one<4, 2, false, EM_NONLINEAR>(k, n_beams, st);
    return hipErrorInvalidValue;
#else
    return grav ? launch_lean_grav(k, n_beams, levels, lognw, elem_mode, st)
                : by_shape<false, false>(k, n_beams, levels, lognw, elem_mode, st);
#endif
}
#endif

#if (CRB_LEAN_PART == 0 || CRB_LEAN_PART == 3) && !defined(CRB_FAST_BUILD)
namespace {
template <int LV, int LOGNW, bool GRAV, int EM, bool PACK, bool SCHED>
hipError_t one_implicit(const KParams<T>& k, const StiffParams<T>& q, int groups, hipStream_t st) {
    constexpr auto kernel = crb_implicit_lean_kernel<T, LV, LOGNW, GRAV, EM, PACK, SCHED>;
    const size_t smem = implicit_lean_lds_bytes<T>(64 << LOGNW, LOGNW);
    if (hipError_t e = lds_opt_in(kernel, smem)) return e;
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(64 << LOGNW), smem, st, k, q);
    return hipGetLastError();
}
}  // namespace
hipError_t launch_implicit_lean(const KParams<T>& k, const StiffParams<T>& q, int groups, int levels, int lognw, bool grav,
                                int elem_mode, hipStream_t st) {
    return with_int<0, MAX_LV>(levels, [&](auto lv) { return with_int<0, 3>(lognw, [&](auto nw) { return with_bool(k.G > 1, [&](auto pack) {
        if constexpr (pack ? nw == 0 && lean_implicit_pack_built(F64, lv) : lean_implicit_built(F64, lv, nw))
            return with_bool(grav, [&](auto g) { return with_elem_mode(elem_mode, [&](auto e) {
                if (!k.sched_stride) return one_implicit<lv, nw, g, e, pack, false>(k, q, groups, st);
                // a control schedule (k.sched_*): its own instantiation, for the shapes lean_implicit_sched_built names
                if constexpr (pack ? lean_implicit_pack_sched_built(F64, lv) : lean_implicit_sched_built(F64, lv, nw))
                    return one_implicit<lv, nw, g, e, pack, true>(k, q, groups, st);
                else return hipErrorInvalidValue; }); });
        else return hipErrorInvalidValue;
    }); }); });
}
#endif

#if CRB_LEAN_PART == 0 || CRB_LEAN_PART == 3
hipError_t launch_stage_lean(const KParams<T>& k, int n_groups, int levels, int lognw, bool grav, int elem_mode, hipStream_t st) {
#ifdef CRB_FAST_BUILD  // kernel-tuning build: the config-5 instance (128 linear elements + gravity, fp64)
    if (sizeof(T) == 8 && levels == 5 && lognw == 1 && grav && elem_mode == EM_LINEAR)
        return one_stage<5, 1, true, EM_LINEAR>(k, n_groups, st);
    return hipErrorInvalidValue;
#else
    return grav ? by_shape<true, true>(k, n_groups, levels, lognw, elem_mode, st)
                : by_shape<false, true>(k, n_groups, levels, lognw, elem_mode, st);
#endif
}
#endif
}  // namespace crb
