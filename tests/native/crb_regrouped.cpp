// crb_regrouped.cpp -- TEST HARNESS ONLY: the nonlinear element's two symmetric forms of crb_math.h on the host, assembled
// on a three-node patch the way the steppers assemble a node's right-hand side (tests/test_axial_regrouped_cpu.py).
// Built without contraction, so that both forms round once per operation whatever the compiler.
#include "../../continuum-robot_amd/csrc/crb_math.h"

using namespace crb;

extern "C" {
// c: the nonlinear ElemCoef pack {L, EA/L^2, 0.1 EA/L^3, 2 EI/L^3, EA/(2L^2), EI/L^2}; q: n patches [node0 node1 node2] x [u w phi];
// elements A (node0 -> node1) and B (node1 -> node2).  Per patch and form: r_u, r_w, r_phi of node1 (minus the internal
// force), then f1 and f2 of element B.  out_new: elem_force_nonlinear_regrouped, assembled as lean_blocked_body does;
// out_sym: elem_force_nonlinear_sym (corrected as given), r = -f_right(A) - f_left(B).
void regrouped_patch(int n, const double* c, const double* q, int corrected, double* out_new, double* out_sym) {
    for (int i = 0; i < n; ++i) {
        const double *q0 = q + 9 * i, *q1 = q0 + 3, *q2 = q0 + 6;
        double flA[3], frA[3], flB[3], frB[3];
        elem_force_nonlinear_sym<double>(c, q0, q1, corrected != 0, flA, frA);
        elem_force_nonlinear_sym<double>(c, q1, q2, corrected != 0, flB, frB);
        double* s = out_sym + 5 * i;
        for (int k = 0; k < 3; ++k) s[k] = -frA[k] - flB[k];
        s[3] = flB[0];
        s[4] = frB[0];
        const ElemForceRegrouped<double> A = elem_force_nonlinear_regrouped<double>(c, q0, q1);
        const ElemForceRegrouped<double> B = elem_force_nonlinear_regrouped<double>(c, q1, q2);
        double* o = out_new + 5 * i;
        const double m = A.f2 - B.f2;
        o[0] = -m - c[1] * B.W;
        o[1] = A.f3 - B.f3;          // -(-f3(A)) - f3(B)
        o[2] = -A.m_right - B.m_left;
        o[3] = c[1] * B.W - B.f2;
        o[4] = B.f2;
    }
}
}
