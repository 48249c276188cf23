// crb_ctrl_launch.h -- host entry of the controlled steppers' translation unit (crb_ctrl.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "crb_ctrl.h"

namespace crb {
// launches crb_controlled_kernel<double, levels, feedback> on a grid of k.B workgroups of `threads` threads (one beam per
// workgroup).  levels: the reduction levels of the tables the kernel solves with -- ALL levels of the beam for the
// implicit scheme (A = M + h^2/4 K0 is not as diagonally dominant as M, and one instance must serve every rung), the
// plan's truncated count for the closed-loop RK4 (the mass matrix's tables).  hipErrorInvalidValue when no instance
// covers the plan (more than 8 / 6 levels).
// lean_lognw >= 0 (implicit scheme): the lean iteration with 2^lean_lognw waves per beam (threads = 64 << lean_lognw, levels =
// ceil(log2 S) >= 1), gravity absent or canonical (`grav`); -1: the general RHS.
// pack (lean form with lean_lognw == 0, k.G >= 2 beams of fewer than 33 slots per wave): a grid of ceil(k.B / k.G) one-wave
// workgroups, every wave with ONE step sequence for its beams.
// stream_gain (feedback only): the instance that reads the gain from q.gain_t (built by launch_gain_transpose) instead of
// holding it in LDS -- lds_bytes from ctrl_lds_bytes(..., stream_gain = true).
// Levels: the closed loop's instances cover 0 .. 6 levels of M.  Truncation at the unit roundoff (pick_levels) depends on
// the element's mass coefficients, not on the rod's length: uniform Nitinol rods of 40 .. 255 elements, linear or nonlinear,
// with or without drag and gravity, keep 5 of their 6 .. 8 levels, so no instance beyond 6 is needed for them.
hipError_t launch_controlled(const KParams<double>& k, const CtrlParams<double>& q, int levels, bool feedback, bool stream_gain, int lean_lognw,
                             bool grav, bool pack, int threads, size_t lds_bytes, hipStream_t st);
// Kt [rows][n] = the transpose of the gain K [n][2n], rows 2n .. rows-1 zero (rows >= 2n)
hipError_t launch_gain_transpose(const double* K, double* Kt, int n, int rows, hipStream_t st);
}  // namespace crb
