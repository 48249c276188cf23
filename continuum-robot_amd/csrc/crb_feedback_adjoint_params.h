// crb_feedback_adjoint_params.h -- what the parameter blocks of the two closed-loop adjoints' matrix kernels share
// (crb_feedback_adjoint_launch.h: the RK4 loop; crb_implicit_feedback_adjoint_launch.h: the sampled-data implicit loop), and
// the launchers' test of it.  The tile loops that read it: crb_feedback_adjoint_tile.h.
#pragma once
#include <cstddef>
#include <cstdint>

namespace crb {
struct FbaParams {
    const double* ubar;        // (df/du)^T of the cotangents, force layout [n_node][4] per row; how a row's record is found is the loop's
    const int32_t* col_off;    // [2n] offset of reduced state index j inside a beam's state record
    const int32_t* row_off;    // [n]  offset of reduced position index i inside a beam's force record
    int rows, B, n, n2;        // rows = n_cot * B, n2 = 2n
    size_t x_stride, u_stride; // doubles per beam of a state / force record
    // the transposed product P = ubar_red . K
    const double* gain;        // [n][2n] row-major
    double* lam;               // [rows][2][n_node][4]  the cotangent the product is taken off
    double* ref_bar;           // [rows][2n] reduced, accumulated, or nullptr
    // the gain gradient
    const double* xs;          // [B][2][n_node][4] the state(s) the feedback force was formed at
    const double* ref;         // [B][2n] reduced, or nullptr (= 0)
    double* gain_bar;          // [n_cot][n][2n], accumulated
    double* partial;           // [n_cot][slices][n][2n] the slices' tiles (feedback_gain_grad_slices(B, n) > 1), else unused
    int slices;                // set by the gain gradient's launcher: feedback_gain_grad_slices(B, n)
};

inline bool fba_shape_ok(const FbaParams& p) {
    return p.rows >= 1 && p.B >= 1 && p.n >= 1 && p.n2 == 2 * p.n && p.rows % p.B == 0 && p.rows / p.B <= 65535;
}

// Slices the beam reduction of the gain gradient is split into: enough for 1536 workgroups (six per CU) per cotangent where
// the n x 2n output tiles alone give fewer, never more than the reduction has K steps of 32 beams.  A function of B and n
// only, so that the summation order -- and the result, bitwise -- does not depend on the number of cotangents.
inline int feedback_gain_grad_slices(int B, int n) {
    const int tiles = ((n + 31) / 32) * ((2 * n + 31) / 32), ksteps = (B + 31) / 32;
    const int want = (1536 + tiles - 1) / tiles;
    return want < ksteps ? want : ksteps;
}
}  // namespace crb
