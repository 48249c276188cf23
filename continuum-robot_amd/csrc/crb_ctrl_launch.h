// crb_ctrl_launch.h -- host entry of the controlled steppers' translation unit (crb_ctrl.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_ctrl.h"

namespace crb {
// The instances of crb_controlled_kernel<double, levels, feedback, lean_lognw, grav, pack, stream_gain> that are built:
// crb_ctrl.hip instantiates exactly these, and crbeam.hip's eligibility predicates ask the same function.
//   the general RHS (lean_lognw = -1, gravity through its tables): 0 .. 8 levels of A for the implicit scheme, 0 .. 6 of M
//       for the closed loop.  Truncation at the unit roundoff (pick_levels) depends on the element's mass coefficients, not
//       on the rod's length: uniform Nitinol rods of 40 .. 255 elements, linear or nonlinear, with or without drag and
//       gravity, keep 5 of their 6 .. 8 levels, so no closed-loop instance beyond 6 is needed for them;
//   the lean closed loop: one wave, 1 .. 6 levels of M, the gain in LDS or streamed (stream_gain, closed loops only);
//   the lean implicit iteration: ALL ceil(log2 S) levels of a beam of 2 .. 64 / 65 .. 128 / 129 .. 256 slots;
//   pack: the lean implicit iteration on several beams of fewer than 33 slots per wave.
constexpr bool controlled_built(int levels, bool feedback, int lean_lognw, bool grav, bool pack, bool stream_gain) {
    if (stream_gain && !feedback) return false;
    if (lean_lognw < 0) return !grav && !pack && levels >= 0 && levels <= (feedback ? 6 : 8);
    if (feedback || pack) return !(feedback && pack) && lean_lognw == 0 && levels >= 1 && levels <= (pack ? 5 : 6);
    return lean_lognw == 0 ? (levels >= 1 && levels <= 6) : (lean_lognw <= 2 && levels == 6 + lean_lognw);
}

// launches crb_controlled_kernel on a grid of k.B workgroups of `threads` threads (one beam per workgroup);
// hipErrorInvalidValue when no instance covers the plan (controlled_built).  levels: the reduction levels of the tables the
// kernel solves with -- ALL levels of the beam for the implicit scheme (A = M + h^2/4 K0 is not as diagonally dominant as
// M, and one instance must serve every rung), the plan's truncated count for the closed-loop RK4 (the mass matrix's tables).
// lean_lognw >= 0: the lean RHS with 2^lean_lognw waves per beam (threads = 64 << lean_lognw), gravity absent or canonical
// (`grav`); -1: the general RHS.
// pack (k.G >= 2): a grid of ceil(k.B / k.G) one-wave workgroups, every wave with ONE step sequence for its beams.
// stream_gain: the instance that reads the gain from q.gain_t (built by launch_gain_transpose) instead of holding it in
// LDS -- lds_bytes from ctrl_lds_bytes(..., stream_gain = true).
hipError_t launch_controlled(const KParams<double>& k, const CtrlParams<double>& q, int levels, bool feedback, bool stream_gain, int lean_lognw,
                             bool grav, bool pack, int threads, size_t lds_bytes, hipStream_t st);
// Kt [rows][n] = the transpose of the gain K [n][2n], rows 2n .. rows-1 zero (rows >= 2n)
hipError_t launch_gain_transpose(const double* K, double* Kt, int n, int rows, hipStream_t st);
}  // namespace crb
