// crb_implicit_feedback_tangent_launch.h -- host entry of the translation unit that holds the sample-boundary kernel of the
// tangent of the sampled-data implicit loop (crb_implicit_feedback_tangent.hip): its parameter block and launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace crb {
// One sample boundary: the held input u [B] force records and its tangent du, record (d, b) at du + d * du_dir_stride +
// b * u_stride, from the state x [B] and its tangents dx [n_dir][B] (state records).  Every tangent input may be nullptr (= 0).
struct ImpFbTanParams {
    const int32_t* col_off;    // [2n] offset of reduced state index j inside a beam's state record
    const int32_t* row_off;    // [n]  offset of reduced position index i inside a beam's force record
    int B, n, n2, n_dir;       // n2 = 2n
    size_t x_stride, u_stride; // doubles per beam of a state / force record
    const double* gain;        // [n][2n] row-major
    const double* d_gain;      // [n_dir][n][2n], or nullptr: its product is skipped
    const double* ref;         // [B][2n] reduced, or nullptr
    const double* d_ref;       // [n_dir][B][2n] reduced, or nullptr
    const double* x;           // [B][2][n_node][4]
    const double* dx;          // [n_dir][B][2][n_node][4]
    const double* f_held;      // [B][n_node][4], or nullptr
    const double* df_held;     // [n_dir][B][n_node][4], or nullptr
    double* u;                 // [B][n_node][4]: free-DOF entries written, the others left as they are
    double* du;                // the same per direction
    size_t du_dir_stride;
};

// crb_imp_fb_tangent_boundary_kernel on a grid of (n_dir + 1) * ceil(B / 32) x ceil(n / 32) workgroups
hipError_t launch_imp_fb_tangent_boundary(const ImpFbTanParams& p, hipStream_t st);
}  // namespace crb
