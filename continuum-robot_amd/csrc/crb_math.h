// crb_math.h -- per-node / per-element arithmetic of the beam hot path.
//
// Everything here is a small inline function of VALUES (no memory, no thread ids), so the
// same source is compiled into the gfx950 kernels (crb_kernels.h) and, for CPU-only
// debugging of the kernel arithmetic, into tests/native/crb_emul.cpp (test harness; it is
// not a product path).  Reference citations are file:line under
// /root/reference/src/continuum_robot/models/.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CRB_HD __host__ __device__ __forceinline__
#else
#define CRB_HD inline
#endif

namespace crb {

enum : int { KIND_NONE = 0, KIND_LINEAR = 1, KIND_NONLINEAR = 2 };

// Per-element coefficient pack (a1/a3 of SURVEY §8).  One element = the element to the
// LEFT of a slot's node.
//   linear    : c = { EA/L, 12EI/L^3, 6EI/L^2, 4EI/L, 2EI/L, 0 }        (segments.py:32-62)
//   nonlinear : c = { L, EA/L^2, 0.1 EA/L^3, 2 EI/L^3, EA/(2L^2), EI/L^2 } (segments.py:128-130; the
//               products of EA, EI and the 1/L^2, 0.1/L^3 prefactors the six forces use)
template <typename T>
struct ElemCoef {
    T c[6];
    int32_t kind;
    int32_t pad;
};

template <typename T>
CRB_HD void elem_coef_build(ElemCoef<T>& e, int kind, double L, double E, double I, double A) {
    const double EA = E * A, EI = E * I;
    e.kind = kind;
    e.pad = 0;
    if (kind == KIND_LINEAR) {
        e.c[0] = T(EA / L);
        e.c[1] = T(12 * EI / (L * L * L));
        e.c[2] = T(6 * EI / (L * L));
        e.c[3] = T(4 * EI / L);
        e.c[4] = T(2 * EI / L);
        e.c[5] = T(0);
    } else if (kind == KIND_NONLINEAR) {
        const double iL2 = 1.0 / (L * L), tenth_iL3 = 0.1 / (L * L * L);
        e.c[0] = T(L);
        e.c[1] = T(EA * iL2);
        e.c[2] = T(EA * tenth_iL3);
        e.c[3] = T(20.0 * EI * tenth_iL3);
        e.c[4] = T(0.5 * EA * iL2);
        e.c[5] = T(EI * iL2);
    } else {
        for (int i = 0; i < 6; ++i) e.c[i] = T(0);
    }
}

// Linear element internal force K_e x_e (segments.py:39-62), split into the halves that go
// to the left node (fl) and the right node (fr).  ql/qr = [u, w, phi] of the two nodes.
template <typename T>
CRB_HD void elem_force_linear(const T* c, const T ql[3], const T qr[3], T fl[3], T fr[3]) {
    const T du = ql[0] - qr[0];
    const T dw = ql[1] - qr[1];
    const T fa = c[0] * du;
    const T fw = c[1] * dw - c[2] * (ql[2] + qr[2]);
    const T m0 = -c[2] * dw;
    fl[0] = fa;
    fl[1] = fw;
    fl[2] = m0 + c[3] * ql[2] + c[4] * qr[2];
    fr[0] = -fa;
    fr[1] = -fw;
    fr[2] = m0 + c[4] * ql[2] + c[3] * qr[2];
}

// Nonlinear (von Karman) element internal force, segments.py:159-472, returned in the
// reference's order [f1,f3,f4 | f2,f5,f6] = forces on [u1,w1,th1 | u2,w2,th2]
// (segments.py:146-155).  The 30-term sums are regrouped in a = th1*L, b = th2*L,
// du = u1-u2, dw = w1-w2; every literal is the reference's.  Where the reference's expanded
// literals are not exactly 2x / 3x each other (sympy float artefacts such as
// 7.71428571428601 vs 2*3.857142857143) the remainder is kept as an explicit w1*w2 term, so
// the regrouped polynomial equals the shipped one identically.  f5 = -f3 term by term in the
// reference.  corrected == false keeps the shipped f1 (it lacks the
// -EA/L*u2 coupling); corrected == true uses f1 = -f2.
// base + c * ww, dropped at compile time when the literal remainder c is exactly 0
template <typename T>
CRB_HD T plus_remainder(T base, double c, T ww) {
    return c == 0.0 ? base : base + T(c) * ww;
}

// (literal form: c = { L, EA, EI, 1/L^2, 0.1/L^3 }, not the ElemCoef pack)
template <typename T>
CRB_HD void elem_force_nonlinear_literal(const T* c, const T ql[3], const T qr[3], bool corrected, T fl[3], T fr[3]) {
    const T L = c[0], A = c[1], D = c[2], iL2 = c[3], tenth_iL3 = c[4];
    const T u1 = ql[0], w1 = ql[1], u2 = qr[0], w2 = qr[1];
    const T a = ql[2] * L, b = qr[2] * L;
    const T du = u1 - u2, dw = w1 - w2;
    const T ww = w1 * w2, dw2 = dw * dw;
    const T a2 = a * a, b2 = b * b, ab = a * b;
    const T Ldu = L * du;

    // ---- f1, f2 (segments.py:178-208, 227-258)
    const T T0 = T(0.6) * dw - T(0.05) * (a + b);
    const T P = a * (T(0.0666666666666665) * a - T(0.0166666666666667) * b - T(0.05) * dw) -
                b * (T(0.0166666666666667) * a - T(0.0666666666666667) * b + T(0.05) * dw);
    const T f2 = A * iL2 * (P - Ldu + dw * T0);
    const T f1 = corrected ? -f2 : A * iL2 * (L * u1 - P - (u2 + dw) * T0);

    // ---- f3 = -f5 (segments.py:279-314, 386-421)
    const T Qa = plus_remainder<T>(T(3.8571428571413) * dw2, 2.0 * 3.8571428571413 - 7.7142857142826, ww);
    const T Qb = plus_remainder<T>(T(3.857142857143) * dw2, 2.0 * 3.857142857143 - 7.71428571428601, ww);
    const T Cw = dw * plus_remainder<T>(T(10.2857142857147) * dw2, 3.0 * 10.2857142857147 - 30.857142857144, ww);
    const T P3 = T(0.0357142857143344) * (a2 * a + b2 * b) - T(0.107142857143003) * ab * (a + b) +
                 T(1.28571428571433) * (a2 + b2) * dw + Ldu * (a + b) - a * Qa - b * Qb - T(12.0) * Ldu * dw + Cw;
    const T f3 = tenth_iL3 * (A * P3 + D * (T(120.0) * dw - T(60.0) * (a + b)));

    // ---- f4 (segments.py:335-365)
    const T Q4 = plus_remainder<T>(T(0.128571428571433) * dw2, 2.0 * 0.128571428571433 - 0.257142857142867, ww);
    const T C4 = dw * plus_remainder<T>(T(0.128571428571377) * dw2, 3.0 * 0.128571428571377 - 0.38571428571413, ww);
    const T P4 = T(0.0285714285714391) * a2 * a - T(0.0107142857142861) * a2 * b + T(0.0107142857142719) * a2 * dw +
                 T(0.00714285714286444) * a * b2 - T(0.0214285714286007) * ab * dw - T(0.133333333333333) * a * Ldu +
                 a * Q4 - T(0.00357142857143344) * b2 * b - T(0.0107142857142719) * b2 * dw +
                 T(0.0333333333333333) * b * Ldu + T(0.1) * Ldu * dw - C4;
    const T f4 = iL2 * (A * P4 + D * (T(4.0) * a + T(2.0) * b - T(6.0) * dw));

    // ---- f6 (segments.py:442-472)
    const T Q6 = plus_remainder<T>(T(0.128571428571428) * dw2, 2.0 * 0.128571428571428 - 0.257142857142856, ww);
    const T C6 = dw * plus_remainder<T>(T(0.128571428571433) * dw2, 3.0 * 0.128571428571433 - 0.3857142857143, ww);
    const T P6 = -T(0.00357142857143344) * a2 * a + T(0.00714285714286356) * a2 * b - T(0.0107142857143003) * a2 * dw -
                 T(0.0107142857142932) * a * b2 - T(0.021428571428558) * ab * dw + T(0.0333333333333333) * a * Ldu +
                 T(0.0285714285714271) * b2 * b + T(0.0107142857142932) * b2 * dw - T(0.133333333333333) * b * Ldu +
                 b * Q6 + T(0.1) * Ldu * dw - C6;
    const T f6 = iL2 * (A * P6 + D * (T(2.0) * a + T(4.0) * b - T(6.0) * dw));

    fl[0] = f1;
    fl[1] = f3;
    fl[2] = f4;
    fr[0] = f2;
    fr[1] = -f3;
    fr[2] = f6;
}

// The same forces in symmetric variables: s = a+b, d = a-b, p = a*b.  Up to the sympy float
// artefacts above, the shipped polynomials are those of the von Karman element with rational
// coefficients (1/15, 1/60, 27/7, 72/7, 1/28, 3/28, 9/7, 1/35, 3/280, 1/140, 3/140, 2/15,
// 1/30, 9/70), f6 is f4 with the two nodes exchanged, and P3 is symmetric in (a, b):
//   P   = s*(s/15 - dw/20) - p/6
//   P3  = s*((s^2 - 6p)/28 + L*du - 27/7 dw^2) + dw*(9/7 (s^2 - 2p) - 12 L*du + 72/7 dw^2)
//   P4+P6 = s*(s^2/40 - 11/140 p - L*du/10 + 9/70 dw^2) + dw*(-3/70 p + L*du/5 - 9/35 dw^2)
//   P4-P6 = d*(9/280 s^2 - p/20 + 3/140 s*dw - L*du/6 + 9/70 dw^2)
// which is 57 flops (with the prefactor products of the ElemCoef pack) against 135 for the literal form.  Every literal of the reference differs
// from its rational by <= 1.5e-12 relative (largest: 0.0214285714286007 vs 3/140), i.e. six
// orders below the 1e-6 parity tolerance; tests/native bounds the difference between the two
// forms.  -DCRB_LITERAL_POLY=1 builds the kernels with the literal form instead.
template <typename T>
CRB_HD void elem_force_nonlinear_sym(const T* c, const T ql[3], const T qr[3], bool corrected, T fl[3], T fr[3]) {
    const T L = c[0], cA1 = c[1], cA3 = c[2], cD3 = c[3], cA4 = c[4], cD4 = c[5];
    const T u1 = ql[0], u2 = qr[0];
    const T a = ql[2] * L, b = qr[2] * L;
    const T du = u1 - u2, dw = ql[1] - qr[1];
    const T s = a + b, d = a - b, p = a * b;
    const T s2 = s * s, dw2 = dw * dw, Ldu = L * du;

    // ---- f1, f2 (segments.py:178-208, 227-258): EA/L^2 * (...)
    const T T0 = T(0.6) * dw - T(0.05) * s;
    const T P = s * (T(1.0 / 15.0) * s - T(0.05) * dw) - T(1.0 / 6.0) * p;
    const T f2 = cA1 * (P - Ldu + dw * T0);
    const T f1 = corrected ? -f2 : cA1 * (L * u1 - P - (u2 + dw) * T0);

    // ---- f3 = -f5 (segments.py:279-314, 386-421): 0.1/L^3 * (EA*P3 + EI*(120 dw - 60 s))
    const T P3 = s * (T(1.0 / 28.0) * (s2 - T(6.0) * p) + Ldu - T(27.0 / 7.0) * dw2) +
                 dw * (T(9.0 / 7.0) * (s2 - T(2.0) * p) - T(12.0) * Ldu + T(72.0 / 7.0) * dw2);
    const T g = T(3.0) * s - T(6.0) * dw;   // 4a+2b-6dw = g + d,  2a+4b-6dw = g - d,  120dw-60s = -20 g
    const T f3 = cA3 * P3 - cD3 * g;

    // ---- f4, f6 (segments.py:335-365, 442-472): 1/L^2 * (EA*P4|6 + EI*(g +- d))
    const T S = s * (T(1.0 / 40.0) * s2 - T(11.0 / 140.0) * p - T(0.1) * Ldu + T(9.0 / 70.0) * dw2) +
                dw * (T(0.2) * Ldu - T(3.0 / 70.0) * p - T(9.0 / 35.0) * dw2);
    const T R = T(9.0 / 280.0) * s2 - T(0.05) * p + T(3.0 / 140.0) * (s * dw) - T(1.0 / 6.0) * Ldu +
                T(9.0 / 70.0) * dw2;
    const T X = cA4 * S + cD4 * g;
    const T Y = d * (cA4 * R + cD4);

    fl[0] = f1;
    fl[1] = f3;
    fl[2] = X + Y;
    fr[0] = f2;
    fr[1] = -f3;
    fr[2] = X - Y;
}

// The symmetric form again, for a caller that assembles the node right-hand sides of a CHAIN of elements itself (the
// blocked stepper, crb_lean.h), with the axial pair regrouped.  For the shipped f1 (corrected == false) two identities hold
// exactly in real arithmetic:
//   P + dw T0 = s^2/15 - (s dw)/10 - p/6 + 0.6 dw^2        (s dw is there already: R uses it)
//   f1 + f2   = cA1 u2 (L - T0) = cA1 u2 (L + 0.05 s - 0.6 dw)
// so an element hands out  f2 = cA1 E,  E = s^2/15 - L du - (s dw)/10 - p/6 + 0.6 dw^2   (5 flops)  and
// W = u2 (L + 0.05 s - 0.6 dw)   (3 flops),  and the axial right-hand side of the node between elements k and k+1 is
//   -f2(k) - f1(k+1) = (f2(k+1) - f2(k)) - cA1 W(k+1)      (2 flops)
// 10 flops per element and node against 14 (T0 2, P 4, f2 3, f1 4, the sum 1).  Where f1 itself is wanted it is
// cA1 W - f2.  The roundings differ from elem_force_nonlinear_sym's in order, not in number or size: both carry errors of
// eps cA1 L |u|, the size of the node's own axial force (tests/test_axial_regrouped_cpu.py bounds both against exact
// rational arithmetic).  f3 and the rotation pair fl[2] / fr[2] are elem_force_nonlinear_sym's, operation by operation.
// There is no corrected form: with f1 = -f2 nothing is shared and elem_force_nonlinear_sym is the cheaper one.
template <typename T>
struct ElemForceRegrouped {
    T f2, W, f3, m_left, m_right;   // f2, W as above; f3 (on w1; -f3 on w2); the moments on th1 and th2
};
template <typename T>
CRB_HD ElemForceRegrouped<T> elem_force_nonlinear_regrouped(const T* c, const T ql[3], const T qr[3]) {
    const T L = c[0], cA1 = c[1], cA3 = c[2], cD3 = c[3], cA4 = c[4], cD4 = c[5];
    const T u1 = ql[0], u2 = qr[0];
    const T a = ql[2] * L, b = qr[2] * L;
    const T du = u1 - u2, dw = ql[1] - qr[1];
    const T s = a + b, d = a - b, p = a * b;
    const T s2 = s * s, dw2 = dw * dw, Ldu = L * du, sdw = s * dw;

    T E = T(1.0 / 15.0) * s2 - Ldu;
    E = E - T(0.1) * sdw;
    E = E - T(1.0 / 6.0) * p;
    E = E + T(0.6) * dw2;
    T LT = L + T(0.05) * s;
    LT = LT - T(0.6) * dw;

    const T P3 = s * (T(1.0 / 28.0) * (s2 - T(6.0) * p) + Ldu - T(27.0 / 7.0) * dw2) +
                 dw * (T(9.0 / 7.0) * (s2 - T(2.0) * p) - T(12.0) * Ldu + T(72.0 / 7.0) * dw2);
    const T g = T(3.0) * s - T(6.0) * dw;
    const T S = s * (T(1.0 / 40.0) * s2 - T(11.0 / 140.0) * p - T(0.1) * Ldu + T(9.0 / 70.0) * dw2) +
                dw * (T(0.2) * Ldu - T(3.0 / 70.0) * p - T(9.0 / 35.0) * dw2);
    const T R = T(9.0 / 280.0) * s2 - T(0.05) * p + T(3.0 / 140.0) * sdw - T(1.0 / 6.0) * Ldu + T(9.0 / 70.0) * dw2;
    const T X = cA4 * S + cD4 * g;
    const T Y = d * (cA4 * R + cD4);

    ElemForceRegrouped<T> o;
    o.f2 = cA1 * E;
    o.W = u2 * LT;
    o.f3 = cA3 * P3 - cD3 * g;
    o.m_left = X + Y;
    o.m_right = X - Y;
    return o;
}

// The regrouped form once more, in chord-relative variables: e = s - 2 dw is L times the sum of the two end rotations
// measured from the element's chord (3 e is the g above), d = a - b as before, U = L du.  With s = e + 2 dw and
// p = (s^2 - d^2) / 4 every polynomial loses monomials, and neither p nor s dw is formed:
//   E  = dw^2/2 - U + d^2/24 + e^2/40                                      (f2 = cA1 E)
//   LT = L + e/20 - dw/2                                                    (W = u2 LT)
//   P3 = e (U + 3/56 d^2 - 3/2 dw^2 - e^2/56) + dw (3/4 d^2 - 10 U + 5 dw^2 + 15/28 e^2)
//   S  = e (11/560 d^2 - U/10 + 3/20 dw^2 + 3/560 e^2) + dw (d^2/20 + 3/140 e^2)
//   R  = d^2/80 - U/6 + 11/560 e^2 + dw (dw/4 + e/10)
// identically equal to the polynomials of elem_force_nonlinear_regrouped in rational arithmetic (tests/test_chord_forces_cpu.py
// checks the identities and bounds the rounding of both forms against exact values).  48 fp64 instructions per element
// against 52; the roundings differ from the other forms' in order and are fewer.  Every sum is an explicit chain, so that host
// and device round alike up to contraction.  The blocked stepper (crb_lean.h) is the caller; the same five values come back.
template <typename T>
CRB_HD ElemForceRegrouped<T> elem_force_nonlinear_chord(const T* c, const T ql[3], const T qr[3]) {
    const T L = c[0], cA1 = c[1], cA3 = c[2], cD3 = c[3], cA4 = c[4], cD4 = c[5];
    const T u2 = qr[0];
    const T a = ql[2] * L, b = qr[2] * L;
    const T du = ql[0] - u2, dw = ql[1] - qr[1];
    const T s = a + b, d = a - b;
    const T e = s - T(2.0) * dw;
    const T e2 = e * e, d2 = d * d, dw2 = dw * dw, U = L * du;

    T E = T(0.5) * dw2 - U;
    E = E + T(1.0 / 24.0) * d2;
    E = E + T(1.0 / 40.0) * e2;
    T LT = L + T(0.05) * e;
    LT = LT - T(0.5) * dw;

    T P3e = U + T(3.0 / 56.0) * d2;
    P3e = P3e - T(1.5) * dw2;
    P3e = P3e - T(1.0 / 56.0) * e2;
    T P3w = T(0.75) * d2 - T(10.0) * U;
    P3w = P3w + T(5.0) * dw2;
    P3w = P3w + T(15.0 / 28.0) * e2;
    const T P3 = e * P3e + dw * P3w;
    const T g = T(3.0) * e;
    T Se = T(11.0 / 560.0) * d2 - T(0.1) * U;
    Se = Se + T(0.15) * dw2;
    Se = Se + T(3.0 / 560.0) * e2;
    const T Sw = T(0.05) * d2 + T(3.0 / 140.0) * e2;
    const T S = e * Se + dw * Sw;
    T R = T(1.0 / 80.0) * d2 - T(1.0 / 6.0) * U;
    R = R + T(11.0 / 560.0) * e2;
    R = R + dw * (T(0.25) * dw + T(0.1) * e);
    const T X = cA4 * S + cD4 * g;
    const T Y = d * (cA4 * R + cD4);

    ElemForceRegrouped<T> o;
    o.f2 = cA1 * E;
    o.W = u2 * LT;
    o.f3 = cA3 * P3 - cD3 * g;
    o.m_left = X + Y;
    o.m_right = X - Y;
    return o;
}

// The chord form with every prefactor multiplied into the polynomial coefficients, for a caller whose elements all share
// ONE pack (the blocked stepper: 256 equal elements), so that a = phi L, U = L du, g = 3 e and the products with cA1, cA3,
// cD3, cA4, cD4 are one number per plan.  In du, dw, sigma = phi1 + phi2, delta = phi1 - phi2 and
// eps = sigma - (2/L) dw  (e = L eps, d = L delta):
//   f2      = k dw^2 + k du + k delta^2 + k eps^2
//   cA1 LT  = k0 + k eps + k dw                                        (W = u2 times that: it carries cA1)
//   f3      = eps (k0 + k du + k delta^2 + k dw^2 + k eps^2) + dw (k delta^2 + k du + k dw^2 + k eps^2)
//   X       = eps (k0 + k delta^2 + k du + k dw^2 + k eps^2) + dw (k delta^2 + k eps^2)
//   Rf      = k0 + k delta^2 + k du + k eps^2 + dw (k dw + k eps)
//   m_left  = X + delta Rf,   m_right = X - delta Rf
// identically equal to elem_force_nonlinear_chord's in rational arithmetic (tests/test_folded_forces_cpu.py checks the
// identities, the constants, and bounds the rounding against exact values next to the symmetric form's).  41 fp64
// instructions per element with contraction against 48 + 1 (cA1 W) + 1.25 (phi L per node).
enum : int {
    FK_EPS = 0,                                                   // eps = sigma - k dw
    FK_F2_DW2, FK_F2_DU, FK_F2_D2, FK_F2_E2,                      // f2
    FK_LT_0, FK_LT_E, FK_LT_DW,                                   // cA1 LT
    FK_F3E_0, FK_F3E_DU, FK_F3E_D2, FK_F3E_DW2, FK_F3E_E2,        // f3, the factor of eps
    FK_F3W_D2, FK_F3W_DU, FK_F3W_DW2, FK_F3W_E2,                  // f3, the factor of dw
    FK_XE_0, FK_XE_D2, FK_XE_DU, FK_XE_DW2, FK_XE_E2,             // X, the factor of eps
    FK_XW_D2, FK_XW_E2,                                           // X, the factor of dw
    FK_R_0, FK_R_D2, FK_R_DU, FK_R_E2, FK_R_DW, FK_R_E,           // Rf
    FK_N                                                          // 30
};
// The constants of a nonlinear pack, each formed in long double from the pack's values and rounded once.
#if defined(__HIPCC__)
__host__
#endif
inline void elem_fold_build(const ElemCoef<double>& e, double k[FK_N]) {
    const long double L = e.c[0], cA1 = e.c[1], cA3 = e.c[2], cD3 = e.c[3], cA4 = e.c[4], cD4 = e.c[5];
    const long double L2 = L * L, L3 = L2 * L;
    k[FK_EPS] = double(2.0L / L);                          // 2 / L
    k[FK_F2_DW2] = double(cA1 / 2.0L);                     // cA1 / 2
    k[FK_F2_DU] = double(-(cA1 * L));                      // -cA1 L
    k[FK_F2_D2] = double(cA1 * L2 / 24.0L);                // cA1 L^2 / 24
    k[FK_F2_E2] = double(cA1 * L2 / 40.0L);                // cA1 L^2 / 40
    k[FK_LT_0] = double(cA1 * L);                          // cA1 L
    k[FK_LT_E] = double(cA1 * L / 20.0L);                  // cA1 L / 20
    k[FK_LT_DW] = double(-(cA1 / 2.0L));                   // -cA1 / 2
    k[FK_F3E_0] = double(-(3.0L * cD3 * L));               // -3 cD3 L
    k[FK_F3E_DU] = double(cA3 * L2);                       // cA3 L^2
    k[FK_F3E_D2] = double(3.0L * cA3 * L3 / 56.0L);        // 3/56 cA3 L^3
    k[FK_F3E_DW2] = double(-(3.0L * cA3 * L / 2.0L));      // -3/2 cA3 L
    k[FK_F3E_E2] = double(-(cA3 * L3 / 56.0L));            // -cA3 L^3 / 56
    k[FK_F3W_D2] = double(3.0L * cA3 * L2 / 4.0L);         // 3/4 cA3 L^2
    k[FK_F3W_DU] = double(-(10.0L * cA3 * L));             // -10 cA3 L
    k[FK_F3W_DW2] = double(5.0L * cA3);                    // 5 cA3
    k[FK_F3W_E2] = double(15.0L * cA3 * L2 / 28.0L);       // 15/28 cA3 L^2
    k[FK_XE_0] = double(3.0L * cD4 * L);                   // 3 cD4 L
    k[FK_XE_D2] = double(11.0L * cA4 * L3 / 560.0L);       // 11/560 cA4 L^3
    k[FK_XE_DU] = double(-(cA4 * L2 / 10.0L));             // -cA4 L^2 / 10
    k[FK_XE_DW2] = double(3.0L * cA4 * L / 20.0L);         // 3/20 cA4 L
    k[FK_XE_E2] = double(3.0L * cA4 * L3 / 560.0L);        // 3/560 cA4 L^3
    k[FK_XW_D2] = double(cA4 * L2 / 20.0L);                // cA4 L^2 / 20
    k[FK_XW_E2] = double(3.0L * cA4 * L2 / 140.0L);        // 3/140 cA4 L^2
    k[FK_R_0] = double(cD4 * L);                           // cD4 L
    k[FK_R_D2] = double(cA4 * L3 / 80.0L);                 // cA4 L^3 / 80
    k[FK_R_DU] = double(-(cA4 * L2 / 6.0L));               // -cA4 L^2 / 6
    k[FK_R_E2] = double(11.0L * cA4 * L3 / 560.0L);        // 11/560 cA4 L^3
    k[FK_R_DW] = double(cA4 * L / 4.0L);                   // cA4 L / 4
    k[FK_R_E] = double(cA4 * L2 / 10.0L);                  // cA4 L^2 / 10
}
// (K: a plain or a constant-address-space pointer to the FK_N constants, or an array of them)
template <typename T, typename K = const T*>
CRB_HD ElemForceRegrouped<T> elem_force_nonlinear_folded(K k, const T ql[3], const T qr[3]) {
    const T u2 = qr[0];
    const T du = ql[0] - u2, dw = ql[1] - qr[1];
    const T sg = ql[2] + qr[2], dl = ql[2] - qr[2];
    const T eps = sg - k[FK_EPS] * dw;
    const T e2 = eps * eps, d2 = dl * dl, dw2 = dw * dw;

    T f2 = k[FK_F2_DW2] * dw2;
    f2 = f2 + k[FK_F2_DU] * du;
    f2 = f2 + k[FK_F2_D2] * d2;
    f2 = f2 + k[FK_F2_E2] * e2;
    T LT = k[FK_LT_0] + k[FK_LT_E] * eps;
    LT = LT + k[FK_LT_DW] * dw;

    T F3e = k[FK_F3E_0] + k[FK_F3E_DU] * du;
    F3e = F3e + k[FK_F3E_D2] * d2;
    F3e = F3e + k[FK_F3E_DW2] * dw2;
    F3e = F3e + k[FK_F3E_E2] * e2;
    T F3w = k[FK_F3W_D2] * d2;
    F3w = F3w + k[FK_F3W_DU] * du;
    F3w = F3w + k[FK_F3W_DW2] * dw2;
    F3w = F3w + k[FK_F3W_E2] * e2;
    T Xe = k[FK_XE_0] + k[FK_XE_D2] * d2;
    Xe = Xe + k[FK_XE_DU] * du;
    Xe = Xe + k[FK_XE_DW2] * dw2;
    Xe = Xe + k[FK_XE_E2] * e2;
    const T Xw = k[FK_XW_D2] * d2 + k[FK_XW_E2] * e2;
    const T X = eps * Xe + dw * Xw;
    T Rf = k[FK_R_0] + k[FK_R_D2] * d2;
    Rf = Rf + k[FK_R_DU] * du;
    Rf = Rf + k[FK_R_E2] * e2;
    Rf = Rf + dw * (k[FK_R_DW] * dw + k[FK_R_E] * eps);
    const T Y = dl * Rf;

    ElemForceRegrouped<T> o;
    o.f2 = f2;
    o.W = u2 * LT;
    o.f3 = eps * F3e + dw * F3w;
    o.m_left = X + Y;
    o.m_right = X - Y;
    return o;
}

// The folded form with the membrane strain's two combinations formed once.  In the folded constants the du and dw^2
// coefficients of five sub-forms are pairwise proportional: with
//   A1 = dw^2 - 2 L du          A2 = dw^2 - (2 L / 3) du
// f2 and the dw factor of f3 take du and dw^2 only through A1, the eps factors of f3 and X and Rf only through A2:
//   f2      = k A1 + k delta^2 + k eps^2
//   cA1 LT  = k0 + k eps + k dw                                        (as folded)
//   f3      = eps (k0 + k A2 + k delta^2 + k eps^2) + dw (k A1 + k delta^2 + k eps^2)
//   X       = eps (k0 + k A2 + k delta^2 + k eps^2) + dw (k delta^2 + k eps^2)
//   Rf      = k0 + k A2 + k delta^2 + k eps^2 + k (dw eps)
// identically the folded form's polynomials in rational arithmetic (tests/test_shared_forces_cpu.py checks the identities,
// the constants, and bounds the rounding against exact values next to the symmetric form's).  A1 and A2 cost one
// multiply-add each, the four sums lose one each and Rf one: 38 fp64 instructions per element against 41, 27 constants
// against 30.  A1 is rounded where it cancels (du ~ dw^2 / (2 L), the inextensible bend: the membrane strain itself), which
// the folded form's f2 was not: an error of 2^-53 dw^2 times the factor, the size of f2's own dw^2 monomial's rounding.
// The five sums of TWO products (the heads of f2 and of f3's dw factor, X's dw factor, X and f3) are written as one product
// and an explicit fused multiply-add: left to contraction the compiler fuses either product, and which one it picks changes
// with the code around the call (seen between two builds of the blocked stepper that differ only in where the constants
// are loaded), so the roundings would not be a property of this function.
template <typename T>
CRB_HD T fused_madd(T a, T b, T c);   // a b + c, rounded once
template <>
CRB_HD double fused_madd<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <>
CRB_HD float fused_madd<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
enum : int {
    SK_EPS = 0, SK_A1, SK_A2,                                     // eps = sigma - k dw, A1 = dw^2 + k du, A2 = dw^2 + k du
    SK_F2_A, SK_F2_D2, SK_F2_E2,                                  // f2
    SK_LT_0, SK_LT_E, SK_LT_DW,                                   // cA1 LT
    SK_F3E_0, SK_F3E_A, SK_F3E_D2, SK_F3E_E2,                     // f3, the factor of eps
    SK_F3W_A, SK_F3W_D2, SK_F3W_E2,                               // f3, the factor of dw
    SK_XE_0, SK_XE_A, SK_XE_D2, SK_XE_E2,                         // X, the factor of eps
    SK_XW_D2, SK_XW_E2,                                           // X, the factor of dw
    SK_R_0, SK_R_A, SK_R_D2, SK_R_E2, SK_R_DWE,                   // Rf
    SK_N                                                          // 27
};
// The constants of a nonlinear pack, each formed in long double from the pack's values and rounded once.
#if defined(__HIPCC__)
__host__
#endif
inline void elem_share_build(const ElemCoef<double>& e, double k[SK_N]) {
    const long double L = e.c[0], cA1 = e.c[1], cA3 = e.c[2], cD3 = e.c[3], cA4 = e.c[4], cD4 = e.c[5];
    const long double L2 = L * L, L3 = L2 * L;
    k[SK_EPS] = double(2.0L / L);                          // 2 / L
    k[SK_A1] = double(-(2.0L * L));                        // -2 L
    k[SK_A2] = double(-(2.0L * L / 3.0L));                 // -2 L / 3
    k[SK_F2_A] = double(cA1 / 2.0L);                       // cA1 / 2
    k[SK_F2_D2] = double(cA1 * L2 / 24.0L);                // cA1 L^2 / 24
    k[SK_F2_E2] = double(cA1 * L2 / 40.0L);                // cA1 L^2 / 40
    k[SK_LT_0] = double(cA1 * L);                          // cA1 L
    k[SK_LT_E] = double(cA1 * L / 20.0L);                  // cA1 L / 20
    k[SK_LT_DW] = double(-(cA1 / 2.0L));                   // -cA1 / 2
    k[SK_F3E_0] = double(-(3.0L * cD3 * L));               // -3 cD3 L
    k[SK_F3E_A] = double(-(3.0L * cA3 * L / 2.0L));        // -3/2 cA3 L
    k[SK_F3E_D2] = double(3.0L * cA3 * L3 / 56.0L);        // 3/56 cA3 L^3
    k[SK_F3E_E2] = double(-(cA3 * L3 / 56.0L));            // -cA3 L^3 / 56
    k[SK_F3W_A] = double(5.0L * cA3);                      // 5 cA3
    k[SK_F3W_D2] = double(3.0L * cA3 * L2 / 4.0L);         // 3/4 cA3 L^2
    k[SK_F3W_E2] = double(15.0L * cA3 * L2 / 28.0L);       // 15/28 cA3 L^2
    k[SK_XE_0] = double(3.0L * cD4 * L);                   // 3 cD4 L
    k[SK_XE_A] = double(3.0L * cA4 * L / 20.0L);           // 3/20 cA4 L
    k[SK_XE_D2] = double(11.0L * cA4 * L3 / 560.0L);       // 11/560 cA4 L^3
    k[SK_XE_E2] = double(3.0L * cA4 * L3 / 560.0L);        // 3/560 cA4 L^3
    k[SK_XW_D2] = double(cA4 * L2 / 20.0L);                // cA4 L^2 / 20
    k[SK_XW_E2] = double(3.0L * cA4 * L2 / 140.0L);        // 3/140 cA4 L^2
    k[SK_R_0] = double(cD4 * L);                           // cD4 L
    k[SK_R_A] = double(cA4 * L / 4.0L);                    // cA4 L / 4
    k[SK_R_D2] = double(cA4 * L3 / 80.0L);                 // cA4 L^3 / 80
    k[SK_R_E2] = double(11.0L * cA4 * L3 / 560.0L);        // 11/560 cA4 L^3
    k[SK_R_DWE] = double(cA4 * L2 / 10.0L);                // cA4 L^2 / 10
}
// (K: a plain or a constant-address-space pointer to the SK_N constants, or an array of them)
template <typename T, typename K = const T*>
CRB_HD ElemForceRegrouped<T> elem_force_nonlinear_shared(K k, const T ql[3], const T qr[3]) {
    const T u2 = qr[0];
    const T du = ql[0] - u2, dw = ql[1] - qr[1];
    const T sg = ql[2] + qr[2], dl = ql[2] - qr[2];
    const T eps = sg - k[SK_EPS] * dw;
    const T e2 = eps * eps, d2 = dl * dl, dw2 = dw * dw;
    const T A1 = dw2 + k[SK_A1] * du, A2 = dw2 + k[SK_A2] * du;

    T f2 = fused_madd<T>(k[SK_F2_D2], d2, k[SK_F2_A] * A1);
    f2 = f2 + k[SK_F2_E2] * e2;
    T LT = k[SK_LT_0] + k[SK_LT_E] * eps;
    LT = LT + k[SK_LT_DW] * dw;

    T F3e = k[SK_F3E_0] + k[SK_F3E_A] * A2;
    F3e = F3e + k[SK_F3E_D2] * d2;
    F3e = F3e + k[SK_F3E_E2] * e2;
    T F3w = fused_madd<T>(k[SK_F3W_D2], d2, k[SK_F3W_A] * A1);
    F3w = F3w + k[SK_F3W_E2] * e2;
    T Xe = k[SK_XE_0] + k[SK_XE_A] * A2;
    Xe = Xe + k[SK_XE_D2] * d2;
    Xe = Xe + k[SK_XE_E2] * e2;
    const T Xw = fused_madd<T>(k[SK_XW_E2], e2, k[SK_XW_D2] * d2);
    const T X = fused_madd<T>(dw, Xw, eps * Xe);
    T Rf = k[SK_R_0] + k[SK_R_A] * A2;
    Rf = Rf + k[SK_R_D2] * d2;
    Rf = Rf + k[SK_R_E2] * e2;
    Rf = Rf + k[SK_R_DWE] * (dw * eps);
    const T Y = dl * Rf;

    ElemForceRegrouped<T> o;
    o.f2 = f2;
    o.W = u2 * LT;
    o.f3 = fused_madd<T>(dw, F3w, eps * F3e);
    o.m_left = X + Y;
    o.m_right = X - Y;
    return o;
}

// Classical RK4 of a second-order system q' = v, v' = a(q, v), per component, with the position side carried on the
// accelerations alone: with a_i the acceleration of stage i (evaluated at q_i and the stage velocity v_i),
//   q_2 = q + dt/2 v     q_3 = q_2 + dt^2/4 a_1     q_4 = (q + dt v) + dt^2/2 a_2
//   q'  = (q + dt v) + dt^2/6 (a_1 + a_2 + a_3)     v' = v + dt/6 (a_1 + 2 a_2 + 2 a_3 + a_4)
// which is what the velocity sums of the textbook bookkeeping (sv = v + cs a, accq += w sv) expand to.  A caller whose force
// reads the stage velocity of some components only (the drag: w) forms v_i = v + cs a_{i-1} (rk4_stage_velocity) for those
// alone.  Rk4Pos is one component's registers over a step; the four stage ends take the stage's acceleration.  The next
// stage's position is `next` from the top of each stage on, and the state after the step is (next, v) after rk4_end3.
//   c6, c4, c2 = dt^2/6, dt^2/4, dt^2/2; hdt, dt6 = dt/2, dt/6.
template <typename T>
struct Rk4Pos {
    T next;   // the next stage's position: q_2, q_3, q_4, q'
    T full;   // q + dt v, then q_4 in its place
    T sum;    // q + dt v + dt^2/6 (a_1 [+ a_2]), the running q'
    T accv;   // a_1 + 2 a_2 + 2 a_3
};
template <typename T>
CRB_HD void rk4_begin(Rk4Pos<T>& r, T q, T v, T hdt, T dt) {
    r.next = q + hdt * v;
    r.full = q + dt * v;
}
template <typename T>
CRB_HD void rk4_end0(Rk4Pos<T>& r, T a, T c6, T c4) {
    r.accv = a;
    r.sum = r.full + c6 * a;
    r.next = r.next + c4 * a;
}
template <typename T>
CRB_HD void rk4_end1(Rk4Pos<T>& r, T a, T c6, T c2) {
    r.accv = r.accv + T(2) * a;
    r.sum = r.sum + c6 * a;
    r.full = r.full + c2 * a;
    r.next = r.full;
}
template <typename T>
CRB_HD void rk4_end2(Rk4Pos<T>& r, T a, T c6) {
    r.accv = r.accv + T(2) * a;
    r.next = r.sum + c6 * a;
}
template <typename T>
CRB_HD T rk4_end3(const Rk4Pos<T>& r, T v, T a, T dt6) {   // v'
    return v + dt6 * (r.accv + a);
}
template <typename T>
CRB_HD T rk4_stage_velocity(T v, T cs, T a) {
    return v + cs * a;
}

#ifndef CRB_LITERAL_POLY
#define CRB_LITERAL_POLY 0
#endif
template <typename T>
CRB_HD void elem_force_nonlinear(const T* c, const T ql[3], const T qr[3], bool corrected, T fl[3], T fr[3]) {
#if CRB_LITERAL_POLY
    const T iL2 = T(1) / (c[0] * c[0]);
    const T lit[5] = {c[0], c[1] / iL2, c[5] / iL2, iL2, T(0.1) * iL2 / c[0]};
    elem_force_nonlinear_literal<T>(lit, ql, qr, corrected, fl, fr);
#else
    elem_force_nonlinear_sym<T>(c, ql, qr, corrected, fl, fr);
#endif
}

template <typename T>
CRB_HD void elem_force(const ElemCoef<T>& e, const T ql[3], const T qr[3], bool corrected, T fl[3], T fr[3]) {
    if (e.kind == KIND_NONLINEAR) {
        elem_force_nonlinear<T>(e.c, ql, qr, corrected, fl, fr);
    } else if (e.kind == KIND_LINEAR) {
        elem_force_linear<T>(e.c, ql, qr, fl, fr);
    } else {
        fl[0] = fl[1] = fl[2] = fr[0] = fr[1] = fr[2] = T(0);
    }
}

// Gravity of one segment (gravity_forces.py:117-128): half the segment weight, rotated by the
// segment's mean rotation into [axial, transverse].  half_mass = 0.5*rho*A*L.
CRB_HD void crb_sincos(double x, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
    ::sincos(x, s, c);
#else
    *s = sin(x);
    *c = cos(x);
#endif
}
CRB_HD void crb_sincos(float x, float* s, float* c) {
#if defined(__HIP_DEVICE_COMPILE__)
    ::sincosf(x, s, c);
#else
    *s = sinf(x);
    *c = cosf(x);
#endif
}

template <typename T>
CRB_HD void gravity_segment(T phi, T gx, T gy, T half_mass, T out[2]) {
    T s, c;
    crb_sincos(phi, &s, &c);
    out[0] = (c * gx + s * gy) * half_mass;
    out[1] = (c * gy - s * gx) * half_mass;
}

// Fluid drag on a transverse DOF (fluid_forces.py:138): -c * v * |v|
CRB_HD double crb_abs(double v) { return __builtin_fabs(v); }
CRB_HD float crb_abs(float v) { return __builtin_fabsf(v); }
template <typename T>
CRB_HD T drag_force(T coef, T v) {
    return -coef * v * crb_abs(v);
}

// ------------------------------------------------------------------ mass blocks / PCR
// Node-block form of the consistent mass matrix (segments.py:64-78 assembled as in
// euler_bernoulli_beam.py:139-161).  The axial DOF (u) decouples from bending (w, phi), so a
// node row carries one scalar triple (a_ax, b_ax, c_ax) and one 2x2 triple (A, B, C), with
//   A = coupling to the node on the left, B = diagonal block, C = coupling to the right.
// 2x2 blocks are stored row-major [ww, wp, pw, pp].
struct NodeBlocks {
    double a_ax, b_ax, c_ax;
    double A[4], B[4], C[4];
};

// contributions of one element (length L, rhoA = rho*A) to its LEFT node's C/B and its RIGHT
// node's A/B
CRB_HD void mass_add_as_right_elem(NodeBlocks& n, double L, double rhoA) {
    // this node is the element's first node: block [0:3,0:3] on the diagonal, [0:3,3:6] to the right
    const double m = rhoA * L / 420.0;
    n.b_ax += 140.0 * m;
    n.c_ax += 70.0 * m;
    n.B[0] += 156.0 * m;
    n.B[1] += -22.0 * L * m;
    n.B[2] += -22.0 * L * m;
    n.B[3] += 4.0 * L * L * m;
    n.C[0] += 54.0 * m;
    n.C[1] += 13.0 * L * m;
    n.C[2] += -13.0 * L * m;
    n.C[3] += -3.0 * L * L * m;
}
CRB_HD void mass_add_as_left_elem(NodeBlocks& n, double L, double rhoA, bool has_left_node) {
    // this node is the element's second node: block [3:6,3:6] on the diagonal, [3:6,0:3] to the left
    const double m = rhoA * L / 420.0;
    n.b_ax += 140.0 * m;
    n.B[0] += 156.0 * m;
    n.B[1] += 22.0 * L * m;
    n.B[2] += 22.0 * L * m;
    n.B[3] += 4.0 * L * L * m;
    if (has_left_node) {
        n.a_ax += 70.0 * m;
        n.A[0] += 54.0 * m;
        n.A[1] += -13.0 * L * m;
        n.A[2] += 13.0 * L * m;
        n.A[3] += -3.0 * L * L * m;
    }
}

// alpha * K0 of one element added to the node blocks, K0 = the element's tangent stiffness AT q = 0 -- the
// iteration matrix A = M + alpha K0 of the implicit stepper (crb_stiff.h) has M's block structure.  For a linear
// element K0 is its stiffness (segments.py:39-62); from elem_force_linear, on [w, phi] the four 2x2 blocks are
//   K11 = [[c1,-c2],[-c2,c3]]  K12 = [[-c1,-c2],[c2,c4]]  K21 = [[-c1,c2],[-c2,c4]]  K22 = [[c1,c2],[c2,c3]]
// with c1 = 12EI/L^3, c2 = 6EI/L^2, c3 = 4EI/L, c4 = 2EI/L, and [[c0,-c0],[-c0,c0]], c0 = EA/L, on the axial DOFs.
// A nonlinear element has the same tangent at q = 0, EXCEPT that the shipped f1 (segments.py:178-208, SURVEY
// App. B-1) lacks the -EA/L u2 coupling: d f1 / d u2 = 0, i.e. the axial block is [[c0, 0],[-c0, c0]] (`axial_12`
// false) and A is not symmetric; the cyclic reduction carries the sub- and super-diagonal separately anyway.
CRB_HD void stiff_add_as_right_elem(NodeBlocks& n, double L, double EA, double EI, double alpha, bool axial_12) {
    // this node is the element's first node: K11 on the diagonal, K12 to the right
    const double c0 = alpha * EA / L, c1 = alpha * 12 * EI / (L * L * L), c2 = alpha * 6 * EI / (L * L), c3 = alpha * 4 * EI / L,
                 c4 = alpha * 2 * EI / L;
    n.b_ax += c0;
    if (axial_12) n.c_ax += -c0;
    n.B[0] += c1; n.B[1] += -c2; n.B[2] += -c2; n.B[3] += c3;
    n.C[0] += -c1; n.C[1] += -c2; n.C[2] += c2; n.C[3] += c4;
}
CRB_HD void stiff_add_as_left_elem(NodeBlocks& n, double L, double EA, double EI, double alpha, bool has_left_node) {
    // this node is the element's second node: K22 on the diagonal, K21 to the left
    const double c0 = alpha * EA / L, c1 = alpha * 12 * EI / (L * L * L), c2 = alpha * 6 * EI / (L * L), c3 = alpha * 4 * EI / L,
                 c4 = alpha * 2 * EI / L;
    n.b_ax += c0;
    n.B[0] += c1; n.B[1] += c2; n.B[2] += c2; n.B[3] += c3;
    if (has_left_node) {
        n.a_ax += -c0;
        n.A[0] += -c1; n.A[1] += c2; n.A[2] += -c2; n.A[3] += c4;
    }
}

// linear coefficient pack {EA/L, 12EI/L^3, 6EI/L^2, 4EI/L, 2EI/L} of an element from EITHER pack of ElemCoef
// (the nonlinear pack holds {L, EA/L^2, 0.1EA/L^3, 2EI/L^3, EA/(2L^2), EI/L^2})
template <typename T>
CRB_HD void elem_linear_coefs(const T* c, int kind, T out[5]) {
    if (kind == KIND_NONLINEAR) {
        const T L = c[0];
        out[0] = c[1] * L;
        out[1] = T(6) * c[3];
        out[2] = T(6) * c[5];
        out[3] = T(4) * c[5] * L;
        out[4] = T(2) * c[5] * L;
    } else {   // KIND_LINEAR (KIND_NONE: all zero already)
        for (int i = 0; i < 5; ++i) out[i] = c[i];
    }
}

// Boundary conditions (euler_bernoulli_beam.py:240-265) in place of physically removing
// rows/columns: a constrained DOF keeps its slot, its row/column become the identity.
// free_* are this node's masks, l_* / r_* the neighbours' (a missing neighbour = not free).
CRB_HD void mass_apply_masks(NodeBlocks& n, bool fu, bool fw, bool fp, bool lu, bool lw, bool lp, bool ru, bool rw,
                             bool rp) {
    if (!fu) { n.a_ax = 0; n.c_ax = 0; n.b_ax = 1; }
    if (!lu) n.a_ax = 0;
    if (!ru) n.c_ax = 0;
    const bool fr[2] = {fw, fp}, lf[2] = {lw, lp}, rf[2] = {rw, rp};
    for (int r = 0; r < 2; ++r)
        for (int cc = 0; cc < 2; ++cc) {
            if (!fr[r] || !lf[cc]) n.A[2 * r + cc] = 0;
            if (!fr[r] || !rf[cc]) n.C[2 * r + cc] = 0;
            if (!fr[r] || !fr[cc]) n.B[2 * r + cc] = (r == cc && !fr[r]) ? 1.0 : 0.0;
        }
}

CRB_HD void inv2(const double M[4], double R[4]) {
    const double det = M[0] * M[3] - M[1] * M[2];
    const double id = 1.0 / det;
    R[0] = M[3] * id;
    R[1] = -M[1] * id;
    R[2] = -M[2] * id;
    R[3] = M[0] * id;
}
CRB_HD void mul2(const double X[4], const double Y[4], double R[4]) {
    R[0] = X[0] * Y[0] + X[1] * Y[2];
    R[1] = X[0] * Y[1] + X[1] * Y[3];
    R[2] = X[2] * Y[0] + X[3] * Y[2];
    R[3] = X[2] * Y[1] + X[3] * Y[3];
}

// One level of parallel cyclic reduction on the (constant) mass matrix, factor phase.
// me = this row, lo = row i-s, hi = row i+s (has_lo / has_hi false outside the beam).
// Outputs the level's elimination multipliers
//     al = -A_i * inv(B_lo),  ga = -C_i * inv(B_hi)     (scalar for axial, 2x2 for bending)
// and the row after the level.  The solve phase only ever needs al/ga:
//     r_i <- r_i + al * r_{i-s} + ga * r_{i+s}.
struct PcrLevel {
    double al_ax, ga_ax;
    double al[4], ga[4];
};
CRB_HD void pcr_factor_level(const NodeBlocks& me, const NodeBlocks& lo, bool has_lo, const NodeBlocks& hi, bool has_hi,
                             PcrLevel& lv, NodeBlocks& out) {
    out = me;
    lv.al_ax = lv.ga_ax = 0.0;
    for (int k = 0; k < 4; ++k) lv.al[k] = lv.ga[k] = 0.0;
    out.a_ax = out.c_ax = 0.0;
    for (int k = 0; k < 4; ++k) out.A[k] = out.C[k] = 0.0;
    if (has_lo) {
        lv.al_ax = -me.a_ax / lo.b_ax;
        out.b_ax += lv.al_ax * lo.c_ax;
        out.a_ax = lv.al_ax * lo.a_ax;
        double Bi[4], t[4];
        inv2(lo.B, Bi);
        mul2(me.A, Bi, t);
        for (int k = 0; k < 4; ++k) lv.al[k] = -t[k];
        mul2(lv.al, lo.C, t);
        for (int k = 0; k < 4; ++k) out.B[k] += t[k];
        mul2(lv.al, lo.A, out.A);
    }
    if (has_hi) {
        lv.ga_ax = -me.c_ax / hi.b_ax;
        out.b_ax += lv.ga_ax * hi.a_ax;
        out.c_ax = lv.ga_ax * hi.c_ax;
        double Bi[4], t[4];
        inv2(hi.B, Bi);
        mul2(me.C, Bi, t);
        for (int k = 0; k < 4; ++k) lv.ga[k] = -t[k];
        mul2(lv.ga, hi.A, t);
        for (int k = 0; k < 4; ++k) out.B[k] += t[k];
        mul2(lv.ga, hi.C, out.C);
    }
}

// Size of a level's multipliers relative to 1, with the rotation DOF scaled by a
// characteristic length Lc so that force/moment units compare (used to decide how many
// levels the solve needs: below the unit roundoff 2^-53 a level no longer changes an fp64 result).
CRB_HD double pcr_level_norm(const PcrLevel& lv, double Lc) {
    double m = fabs(lv.al_ax);
    const double v[9] = {fabs(lv.ga_ax),       fabs(lv.al[0]),      fabs(lv.al[1]) * Lc, fabs(lv.al[2]) / Lc, fabs(lv.al[3]),
                         fabs(lv.ga[0]),       fabs(lv.ga[1]) * Lc, fabs(lv.ga[2]) / Lc, fabs(lv.ga[3])};
    for (int k = 0; k < 9; ++k) m = v[k] > m ? v[k] : m;
    return m;
}

// Solve-phase tables as the kernels read them (T = plan dtype).
//   level record : [al_ax, ga_ax, al[4], ga[4]]  -> 10 values per slot per level
//   final record : [1/b_ax, inv(B)[4]]           -> 5 values per slot (padded to 6)
constexpr int PCR_LEVEL_VALS = 10;
constexpr int PCR_FINAL_VALS = 6;

template <typename T>
CRB_HD void pcr_apply_level(const T* cf, const T rlo[3], const T rhi[3], T r[3]) {
    const T r0 = r[0] + cf[0] * rlo[0] + cf[1] * rhi[0];
    const T r1 = r[1] + cf[2] * rlo[1] + cf[3] * rlo[2] + cf[6] * rhi[1] + cf[7] * rhi[2];
    const T r2 = r[2] + cf[4] * rlo[1] + cf[5] * rlo[2] + cf[8] * rhi[1] + cf[9] * rhi[2];
    r[0] = r0;
    r[1] = r1;
    r[2] = r2;
}
template <typename T>
CRB_HD void pcr_apply_final(const T* cf, const T r[3], T x[3]) {
    x[0] = cf[0] * r[0];
    x[1] = cf[1] * r[1] + cf[2] * r[2];
    x[2] = cf[3] * r[1] + cf[4] * r[2];
}

// ------------------------------------------------------------------ tangent stiffness / static equilibrium (crb_static.h)
// Forward-mode dual number: v + d eps, eps^2 = 0.  elem_force<Dual<T>> with one input seeded (d = 1) returns in the d parts
// the column of the element tangent for that input, exactly (no hand-derived polynomials: every form of elem_force --
// linear, nonlinear symmetric / literal, the corrected flag -- is differentiated as written).
template <typename T>
struct Dual {
    T v, d;
    CRB_HD Dual() : v(T(0)), d(T(0)) {}
    CRB_HD Dual(double x) : v(T(x)), d(T(0)) {}
    CRB_HD Dual(T x, T dx) : v(x), d(dx) {}
};
template <typename T> CRB_HD Dual<T> operator+(Dual<T> a, Dual<T> b) { return Dual<T>(a.v + b.v, a.d + b.d); }
template <typename T> CRB_HD Dual<T> operator-(Dual<T> a, Dual<T> b) { return Dual<T>(a.v - b.v, a.d - b.d); }
template <typename T> CRB_HD Dual<T> operator-(Dual<T> a) { return Dual<T>(-a.v, -a.d); }
template <typename T> CRB_HD Dual<T> operator*(Dual<T> a, Dual<T> b) { return Dual<T>(a.v * b.v, a.d * b.v + a.v * b.d); }
template <typename T> CRB_HD Dual<T> operator/(Dual<T> a, Dual<T> b) {
    const T q = a.v / b.v;
    return Dual<T>(q, (a.d - q * b.d) / b.v);
}
// |x| and sin / cos on dual numbers (drag_force and gravity_segment on dual velocities and rotations, crb_tangent.h).  At
// x = 0 the derivative of |x| is taken as +1: drag_force multiplies it by v = 0, so -c v|v| has the exact derivative 0 there.
template <typename T> CRB_HD Dual<T> crb_abs(Dual<T> x) { return x.v < T(0) ? -x : x; }
template <typename T>
CRB_HD void crb_sincos(Dual<T> x, Dual<T>* s, Dual<T>* c) {
    T sv, cv;
    crb_sincos(x.v, &sv, &cv);
    *s = Dual<T>(sv, cv * x.d);
    *c = Dual<T>(cv, -sv * x.d);
}

// Element tangent d[fl; fr] / d[ql; qr] (6 x 6, row = force component, column = input) of elem_force at (ql, qr): six
// dual passes, one seed each.  The element forces fl / fr of the point come out of the first pass.
template <typename T>
CRB_HD void elem_tangent(const ElemCoef<T>& e, const T ql[3], const T qr[3], bool corrected, T K[6][6], T fl[3], T fr[3]) {
    typedef Dual<T> D;
    ElemCoef<D> ed;
    ed.kind = e.kind;
    ed.pad = 0;
    for (int k = 0; k < 6; ++k) ed.c[k] = D(e.c[k], T(0));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 6; ++s) {
        D dl[3], dr[3], gl[3], gr[3];
        for (int c = 0; c < 3; ++c) {
            dl[c] = D(ql[c], s == c ? T(1) : T(0));
            dr[c] = D(qr[c], s == 3 + c ? T(1) : T(0));
        }
        elem_force<D>(ed, dl, dr, corrected, gl, gr);
        for (int c = 0; c < 3; ++c) {
            K[c][s] = gl[c].d;
            K[3 + c][s] = gr[c].d;
            if (s == 0) { fl[c] = gl[c].v; fr[c] = gr[c].v; }
        }
    }
}

// d/dphi of gravity_segment: the segment force rotated by a further 90 degrees, [g1, -g0]
template <typename T>
CRB_HD void gravity_segment_dphi(const T g[2], T dg[2]) {
    dg[0] = g[1];
    dg[1] = -g[0];
}

// 3 x 3 blocks, row-major.  inv3: Gauss-Jordan elimination with partial pivoting (the raw adjugate loses the small
// pivots of blocks that mix EA/L and 4EI/L).  A singular block gives non-finite entries.  The pivot search is a chain of
// conditional row swaps with compile-time indices (a data-dependent row index would put the array in scratch memory).
template <typename T>
CRB_HD void inv3(const T M[9], T R[9]) {
    T a[3][6];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { a[r][c] = M[3 * r + c]; a[r][3 + c] = (r == c) ? T(1) : T(0); }
    for (int k = 0; k < 3; ++k) {
        for (int r = k + 1; r < 3; ++r) {
            const bool sw = __builtin_fabs(double(a[r][k])) > __builtin_fabs(double(a[k][k]));
            for (int c = 0; c < 6; ++c) {
                const T x = a[k][c], y = a[r][c];
                a[k][c] = sw ? y : x;
                a[r][c] = sw ? x : y;
            }
        }
        const T ip = T(1) / a[k][k];
        for (int c = 0; c < 6; ++c) a[k][c] *= ip;
        for (int r = 0; r < 3; ++r) {
            if (r == k) continue;
            const T f = a[r][k];
            for (int c = 0; c < 6; ++c) a[r][c] -= f * a[k][c];
        }
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = a[r][3 + c];
}
template <typename T>
CRB_HD void mul3(const T X[9], const T Y[9], T R[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = X[3 * r] * Y[c] + X[3 * r + 1] * Y[3 + c] + X[3 * r + 2] * Y[6 + c];
}
template <typename T>
CRB_HD void mulv3(const T X[9], const T y[3], T r[3]) {
    for (int i = 0; i < 3; ++i) r[i] = X[3 * i] * y[0] + X[3 * i + 1] * y[1] + X[3 * i + 2] * y[2];
}

// One node row of the block-tridiagonal system  A_i x_{i-s} + B_i x_i + C_i x_{i+s} = r_i  in 3 x 3 blocks on [u, w, phi].
struct Row3 {
    double A[9], B[9], C[9], r[3];
};
// Block-Jacobi normalisation of a row: B_i -> I (A, C, r multiplied by inv(B_i)).  What a level of the reduction reads
// from the rows i - s and i + s is their normalised A, C and r.  In two parts, so that one matrix pass can serve several
// right-hand sides (crb_static_sens_kernel): the matrix part returns inv(B_i) for the right-hand sides.
CRB_HD void row3_normalise_matrix(double A[9], double B[9], double C[9], double Bi[9]) {
    double t[9];
    inv3<double>(B, Bi);
    mul3<double>(Bi, A, t);
    for (int k = 0; k < 9; ++k) A[k] = t[k];
    mul3<double>(Bi, C, t);
    for (int k = 0; k < 9; ++k) C[k] = t[k];
    for (int k = 0; k < 3; ++k) { B[k * 3 + 0] = k == 0; B[k * 3 + 1] = k == 1; B[k * 3 + 2] = k == 2; }
}
CRB_HD void row3_normalise_rhs(const double Bi[9], double r[3]) {
    double v[3];
    mulv3<double>(Bi, r, v);
    for (int k = 0; k < 3; ++k) r[k] = v[k];
}
CRB_HD void row3_normalise(Row3& w) {
    double Bi[9];
    row3_normalise_matrix(w.A, w.B, w.C, Bi);
    row3_normalise_rhs(Bi, w.r);
}
// One level of block cyclic reduction, factorisation and right-hand side together: with the normalised rows `me`, `lo` = row
// i - s, `hi` = row i + s (zero blocks outside the beam) the couplings to i -+ s are eliminated:
//   B' = I - A lo.C - C hi.A,   A' = -A lo.A,   C' = -C hi.C,   r' = r - A lo.r - C hi.r
// The right-hand-side part reads the row's A and C from BEFORE the level.
CRB_HD void row3_level_matrix(const double meA[9], const double meC[9], const double loA[9], const double loC[9],
                              const double hiA[9], const double hiC[9], double outA[9], double outB[9], double outC[9]) {
    double t[9], u[9];
    mul3<double>(meA, loC, t);
    mul3<double>(meC, hiA, u);
    for (int k = 0; k < 9; ++k) outB[k] = ((k % 4) == 0 ? 1.0 : 0.0) - t[k] - u[k];
    mul3<double>(meA, loA, t);
    mul3<double>(meC, hiC, u);
    for (int k = 0; k < 9; ++k) { outA[k] = -t[k]; outC[k] = -u[k]; }
}
CRB_HD void row3_level_rhs(const double meA[9], const double meC[9], const double mer[3], const double lor[3],
                           const double hir[3], double outr[3]) {
    double v[3], w[3];
    mulv3<double>(meA, lor, v);
    mulv3<double>(meC, hir, w);
    for (int k = 0; k < 3; ++k) outr[k] = mer[k] - v[k] - w[k];
}
CRB_HD void row3_level(const Row3& me, const double loA[9], const double loC[9], const double lor[3], const double hiA[9],
                       const double hiC[9], const double hir[3], Row3& out) {
    row3_level_matrix(me.A, me.C, loA, loC, hiA, hiC, out.A, out.B, out.C);
    row3_level_rhs(me.A, me.C, me.r, lor, hir, out.r);
}

}  // namespace crb
