// crb_loop_launch.h -- host entry of the persistent closed-loop stepper's translation units (crb_loop.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_loop.h"

namespace crb {
// The instances of crb_loop_kernel<double, levels, lognw, NB, grav, elem_mode, has_ref> that are built (crb_loop.hip
// instantiates exactly these; crbeam.hip: loop_shape_ok asks the same function): beams of 33 .. 64 thread-carried nodes
// (one wave per beam, lognw = 0, groups of NB = 4 workgroups) and 65 .. 128 (two waves, lognw = 1, NB = 8) at the levels the
// truncated reduction of an fp64 mass matrix lands on.
constexpr int loop_nb(int lognw) { return lognw == 1 ? 8 : 4; }
constexpr bool loop_built(int levels, int lognw) { return (lognw == 0 || lognw == 1) && (levels == 5 || levels == 6); }
// launch_loop_long: lognw = 1; launch_loop_short: lognw = 0 (a translation unit each).  P.n_groups is chosen here (what the
// device keeps resident).  hipErrorInvalidValue when no instance covers the plan.
// `gain` [n][2n] is re-laid into P.kfrag by a small kernel of the same launch sequence (crb_loop_gain_kernel).
hipError_t launch_loop_long(const LoopParams<double>& P, const double* gain, int levels, bool grav, int elem_mode, hipStream_t st);
hipError_t launch_loop_short(const LoopParams<double>& P, const double* gain, int levels, bool grav, int elem_mode, hipStream_t st);

// Layout of the work buffer (bytes from its start): [sync words][gain fragments][E][U][own], every part sized for
// `groups` groups of NB workgroups (NB = 8 for beams of more than 64 thread-carried nodes, else 4)
struct LoopWork {
    size_t kfrag, ebuf, ubuf, ownbuf, total;
};
inline LoopWork loop_work_layout(int nb, int groups) {
    LoopWork w;
    const size_t e = size_t(8 * nb) * 64 * 12 * sizeof(double), u = size_t(64) * 48 * nb * sizeof(double), own = size_t(64) * 16 * nb * 12 * sizeof(double);
    w.kfrag = size_t(LOOP_SYNC_WORDS) * sizeof(unsigned);
    w.ebuf = w.kfrag + size_t(nb) * 4 * 3 * 6 * nb * 64 * sizeof(double);
    w.ubuf = w.ebuf + e * groups;
    w.ownbuf = w.ubuf + u * groups;
    w.total = w.ownbuf + own * groups;
    return w;
}
}  // namespace crb
