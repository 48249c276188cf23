// crb_loop.hip -- instantiations and launch of crb_loop_kernel (the persistent closed-loop stepper, crb_loop.h).
#include "crb_host.h"
#include "crb_loop_launch.h"

namespace crb {
namespace {
typedef double T;

template <int LV, int LOGNW, int NB, bool GRAV, int EM, bool HAS_REF>
hipError_t one_loop(LoopParams<T> P, const T* gain, hipStream_t st) {
    constexpr auto kernel = crb_loop_kernel<T, LV, LOGNW, NB, GRAV, EM, HAS_REF>;
    const size_t smem = loop_lds_bytes<T, LV, LOGNW, NB>();
    hipError_t e = lds_opt_in(kernel, smem);
    if (e != hipSuccess) return e;
    // the grid is what the device keeps resident, in whole groups: a workgroup that is not running cannot arrive
    int resident = 0;
    if ((e = resident_groups<kernel>(256, smem, &resident)) != hipSuccess) return e;
    int groups = int(env_int("CRB_LOOP_MAX_GROUPS", resident / NB));   // (tests: several row blocks per group)
    if (groups > LOOP_MAX_GROUPS) groups = LOOP_MAX_GROUPS;
    if (groups > P.n_rb) groups = P.n_rb;
    if (groups < 1) return hipErrorInvalidConfiguration;
    P.n_groups = groups;
    constexpr int frag_vals = NB * 4 * 3 * 6 * NB * 64;
    hipLaunchKernelGGL((crb_loop_gain_kernel<T, NB>), dim3((frag_vals + 255) / 256), dim3(256), 0, st, gain, P.red_map, P.n_red, P.k.S, P.k.off,
                       const_cast<T*>(P.kfrag));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(groups * NB), dim3(256), smem, st, P);
    return hipGetLastError();
}
template <int LOGNW>
hipError_t by_shape(const LoopParams<T>& P, const T* gain, int levels, bool grav, int em, hipStream_t st) {
    // (a gain is designed on the linear model: all-linear topologies get the straight-line force, anything else the per-lane branch)
    return with_int<0, MAX_LV>(levels, [&](auto lv) { return with_bool(em == EM_LINEAR, [&](auto linear) {
        if constexpr (loop_built(lv, LOGNW))
            return with_bool(grav, [&](auto g) { return with_bool(P.ref != nullptr, [&](auto ref) {
                return one_loop<lv, LOGNW, loop_nb(LOGNW), g, linear ? EM_LINEAR : EM_MIXED, ref>(P, gain, st); }); });
        else return hipErrorInvalidValue;
    }); });
}
}  // namespace

#ifndef CRB_LOOP_PART   // 0 = everything in one unit; 1 / 2 = beams of 65 .. 128 / 33 .. 64 slots (Makefile: built in parallel)
#define CRB_LOOP_PART 0
#endif
#if CRB_LOOP_PART == 0 || CRB_LOOP_PART == 1
hipError_t launch_loop_long(const LoopParams<double>& P, const double* gain, int levels, bool grav, int elem_mode, hipStream_t st) {
#ifdef CRB_FAST_BUILD   // kernel-tuning build: the config-5 instance (128 linear elements + gravity, regulation to 0)
    if (levels == 5 && grav && elem_mode == EM_LINEAR && !P.ref) return one_loop<5, 1, 8, true, EM_LINEAR, false>(P, gain, st);
    return hipErrorInvalidValue;
#else
    return by_shape<1>(P, gain, levels, grav, elem_mode, st);
#endif
}
#endif
#if (CRB_LOOP_PART == 0 || CRB_LOOP_PART == 2) && defined(CRB_FAST_BUILD)
hipError_t launch_loop_short(const LoopParams<double>&, const double*, int, bool, int, hipStream_t) { return hipErrorInvalidValue; }
#endif
#if (CRB_LOOP_PART == 0 || CRB_LOOP_PART == 2) && !defined(CRB_FAST_BUILD)
hipError_t launch_loop_short(const LoopParams<double>& P, const double* gain, int levels, bool grav, int elem_mode, hipStream_t st) {
    return by_shape<0>(P, gain, levels, grav, elem_mode, st);
}
#endif
}  // namespace crb
