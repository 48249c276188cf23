// crb_shared.cpp -- TEST HARNESS ONLY: the nonlinear element's shared-membrane form (crb_math.h: elem_share_build,
// elem_force_nonlinear_shared) next to the folded and the symmetric forms on the host, element by element and assembled on
// a three-node patch the way lean_blocked_body assembles a node's right-hand side (tests/test_shared_forces_cpu.py).
// Built without contraction, so that every form rounds once per operation whatever the compiler.
#include "../../continuum-robot_amd/csrc/crb_math.h"

using namespace crb;

namespace {
ElemCoef<double> pack_of(const double* c) {
    ElemCoef<double> e;
    for (int i = 0; i < 6; ++i) e.c[i] = c[i];
    e.kind = KIND_NONLINEAR;
    e.pad = 0;
    return e;
}

// f2, cA1 W, f3, m_left, m_right of element B, then r_u, r_w, r_phi of node 1 between elements A and B
void regrouped_rows(const ElemForceRegrouped<double>& A, const ElemForceRegrouped<double>& B, double* o) {
    o[0] = B.f2;
    o[1] = B.W;                          // (carries cA1)
    o[2] = B.f3;
    o[3] = B.m_left;
    o[4] = B.m_right;
    const double fr = A.f2 - B.f2;       // lean_blocked_body: fr[k][0] = f2[k] - f2[k + 1]; r = -fr - cW[k + 1]
    o[5] = -fr - o[1];
    o[6] = A.f3 - B.f3;                  // h = -fr[k][1] = f3(A); r = h - fl[k + 1][1]
    o[7] = -A.m_right - B.m_left;
}
}  // namespace

extern "C" {
int share_count() { return SK_N; }

// c: the nonlinear ElemCoef pack; k: its SK_N constants
void share_constants(const double* c, double* k) { elem_share_build(pack_of(c), k); }

// q: n patches [node0 node1 node2] x [u w phi]; elements A (node0 -> node1), B (node1 -> node2)
void shared_patch(int n, const double* c, const double* q, double* out_shared, double* out_folded, double* out_sym) {
    double ks[SK_N], kf[FK_N];
    elem_share_build(pack_of(c), ks);
    elem_fold_build(pack_of(c), kf);
    for (int i = 0; i < n; ++i) {
        const double *q0 = q + 9 * i, *q1 = q0 + 3, *q2 = q0 + 6;
        regrouped_rows(elem_force_nonlinear_shared<double>(ks, q0, q1), elem_force_nonlinear_shared<double>(ks, q1, q2), out_shared + 8 * i);
        regrouped_rows(elem_force_nonlinear_folded<double>(kf, q0, q1), elem_force_nonlinear_folded<double>(kf, q1, q2), out_folded + 8 * i);
        double flA[3], frA[3], flB[3], frB[3];
        elem_force_nonlinear_sym<double>(c, q0, q1, false, flA, frA);
        elem_force_nonlinear_sym<double>(c, q1, q2, false, flB, frB);
        double* s = out_sym + 8 * i;
        s[0] = frB[0];
        s[1] = flB[0] + frB[0];              // f1 + f2 = cA1 W
        s[2] = flB[1];
        s[3] = flB[2];
        s[4] = frB[2];
        for (int j = 0; j < 3; ++j) s[5 + j] = -frA[j] - flB[j];
    }
}
}
