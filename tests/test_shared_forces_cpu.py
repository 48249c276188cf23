"""CPU checks of the blocked fp64 stepper's shared-membrane element polynomials (crb_math.h: elem_share_build,
elem_force_nonlinear_shared) through a host harness (tests/native/crb_shared.cpp, g++, no contraction: the shared form's
five explicit fused multiply-adds are its only fused operations here).

Constants.  The 27 constants of a pack equal their exact rational values (products of the pack's floats, powers of L and the
chord form's rationals) rounded once.

Identities.  With those rationals unrounded, f2, cA1 W, f3, m_left and m_right of the shared form are the symmetric form's
polynomials identically (nothing sampled): A1 = dw^2 - 2 L du and A2 = dw^2 - (2 L / 3) du carry every du and dw^2 term of
f2, of both factors of f3, of the eps factor of X and of Rf.

Forces.  f2, cA1 W, f3, m_left, m_right of an element and r_u, r_w, r_phi of the middle node of a three-node patch, from the
shared form and from elem_force_nonlinear_sym, each against the rational polynomials evaluated exactly on the float inputs,
with tests/test_chord_forces_cpu.py's scales, at element lengths 0.25 (the shipped pack: the products with L are exact), 0.3
and 0.0731 (they round), the radius scaled with L.  The sample is seeded: 2400 patches of tests/test_chord_forces_cpu.py's
six kinds and 600 inextensible bends, where du lies within four ulp of dw^2 / (2 L) in both elements, so that A1 cancels to
rounding (the shared form rounds A1 there; the folded form added the two monomials to f2 one by one).  Bound, the project's
own: the shared form's worst error may be at most TWICE the symmetric form's on the same sample, output by output.
Measured (3000 patches), shared / symmetric in units of 2^-53 and their ratio, in the order f2, cA1 W, f3, m_left, m_right,
r_u, r_w, r_phi:
  L = 0.25:   2.86 / 5.99 (0.48), 2.17 / 1.1e5 (2e-5), 3.40 / 3.25 (1.05), 4.79 / 6.56 (0.73), 4.12 / 6.70 (0.61),
              3.19 / 4.53 (0.70), 2.74 / 2.87 (0.95), 3.39 / 4.58 (0.74)
  L = 0.3:    2.89 / 6.73 (0.43), 1.91 / 8.2e5 (2e-6), 3.49 / 3.47 (1.01), 4.92 / 6.11 (0.81), 3.95 / 5.78 (0.68),
              2.92 / 3.58 (0.82), 2.75 / 2.89 (0.95), 4.24 / 4.84 (0.88)
  L = 0.0731: 3.54 / 5.58 (0.64), 2.28 / 2.2e5 (1e-5), 3.78 / 4.67 (0.81), 5.11 / 5.72 (0.89), 5.42 / 5.47 (0.99),
              3.06 / 3.69 (0.83), 3.48 / 4.88 (0.71), 4.85 / 5.66 (0.86)
(the symmetric form's f1 + f2 cancels cA1 L u1, hence its cA1 W).  On the 600 inextensible bends alone the shared form's f2
errs by 2.22 / 2.81 / 2.29 units at the three lengths, the folded form's by the same, the symmetric form's by 3.83 / 4.04 /
3.34: the rounding of A1 where it cancels does not show."""
import ctypes as C
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from tests.test_chord_forces_cpu import (A_, B_, DW, EPS, OUTPUTS, U2, U_, _p, element_outputs, exact_patch, inner_symmetric,
                                         sample_states)
from tests.test_folded_forces_cpu import LENGTHS, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_GENERIC_EACH, N_BENDS = 400, 600


def _lib():
    src = os.path.join(ROOT, "tests", "native", "crb_shared.cpp")
    so = os.path.join(ROOT, "tests", "native", "_build_libcrb_shared.so")
    hdr = os.path.join(ROOT, "continuum-robot_amd", "csrc", "crb_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.share_constants.argtypes = [dp, dp]
    lib.shared_patch.argtypes = [C.c_int, dp, dp, dp, dp, dp]
    return lib


def exact_constants(c):
    """The shared form's constants as exact rationals of the pack's floats, in the order of crb_math.h's SK_* enum."""
    L, cA1, cA3, cD3, cA4, cD4 = (F(float(v)) for v in c)
    L2, L3 = L * L, L * L * L
    return [
        2 / L, -2 * L, -2 * L / 3,                                                               # eps, A1, A2
        cA1 / 2, cA1 * L2 / 24, cA1 * L2 / 40,                                                   # f2: A1, delta^2, eps^2
        cA1 * L, cA1 * L / 20, -cA1 / 2,                                                         # cA1 LT: 1, eps, dw
        -3 * cD3 * L, -F(3, 2) * cA3 * L, F(3, 56) * cA3 * L3, -cA3 * L3 / 56,                   # f3 | eps: 1, A2, delta^2, eps^2
        5 * cA3, F(3, 4) * cA3 * L2, F(15, 28) * cA3 * L2,                                       # f3 | dw: A1, delta^2, eps^2
        3 * cD4 * L, F(3, 20) * cA4 * L, F(11, 560) * cA4 * L3, F(3, 560) * cA4 * L3,            # X | eps: 1, A2, delta^2, eps^2
        cA4 * L2 / 20, F(3, 140) * cA4 * L2,                                                     # X | dw: delta^2, eps^2
        cD4 * L, cA4 * L / 4, cA4 * L3 / 80, F(11, 560) * cA4 * L3, cA4 * L2 / 10,               # Rf: 1, A2, delta^2, eps^2, dw eps
    ]


def shared_outputs(c, k):
    """f2, cA1 W, f3, m_left, m_right of the shared form with the constants k, as polynomials in (a, b, dw, U, u2)."""
    L = F(float(c[0]))
    du, sg, dl = U_ * (1 / L), (A_ + B_) * (1 / L), (A_ - B_) * (1 / L)
    eps = sg - k[0] * DW
    e2, d2, dw2 = eps * eps, dl * dl, DW * DW
    A1, A2 = dw2 + k[1] * du, dw2 + k[2] * du
    f2 = k[3] * A1 + k[4] * d2 + k[5] * e2
    LT = k[6] + k[7] * eps + k[8] * DW
    f3 = eps * (k[9] + k[10] * A2 + k[11] * d2 + k[12] * e2) + DW * (k[13] * A1 + k[14] * d2 + k[15] * e2)
    X = eps * (k[16] + k[17] * A2 + k[18] * d2 + k[19] * e2) + DW * (k[20] * d2 + k[21] * e2)
    Rf = k[22] + k[23] * A2 + k[24] * d2 + k[25] * e2 + k[26] * (DW * eps)
    return [f2, U2 * LT, f3, X + dl * Rf, X - dl * Rf]


@pytest.mark.parametrize("L", LENGTHS)
def test_the_constants_are_the_exact_rationals_rounded_once(L):
    c = np.ascontiguousarray(pack(L))
    lib = _lib()
    n = lib.share_count()
    exact = exact_constants(c)
    assert n == len(exact) == 27
    k = np.empty(n)
    lib.share_constants(_p(c), _p(k))
    want = np.array([float(v) for v in exact])     # (Fraction -> float rounds the exact value once, to nearest)
    assert (want != 0).all()
    assert np.array_equal(k, want), np.nonzero(k != want)


@pytest.mark.parametrize("L", LENGTHS)
def test_the_shared_polynomials_are_the_symmetric_ones_identically(L):
    """Polynomial identities in (a, b, dw, U, u2) with rational coefficients: nothing sampled."""
    c = pack(L)
    for name, sym, shared in zip(OUTPUTS, element_outputs(c, inner_symmetric()), shared_outputs(c, exact_constants(c))):
        assert sym == shared and len(sym.t) > 0, name


# ------------------------------------------------------------------ forces against exact values
def inextensible_bends(L, n=N_BENDS, seed=4242):
    """Three-node patches whose two elements bend without stretching to second order: du = dw^2 / (2 L) up to four ulp, so
    that A1 = dw^2 - 2 L du cancels to rounding.  The middle node's u is 0, which makes both du exact differences."""
    rng = np.random.default_rng(seed)
    q = rng.normal(0.0, 1.0, (n, 9)) * np.array([0.0, 1e-2, 1e-1] * 3) * 10.0 ** rng.uniform(-2, 0, (n, 1))
    ulps = rng.integers(-4, 5, (n, 2))
    dw_a, dw_b = q[:, 1] - q[:, 4], q[:, 4] - q[:, 7]
    q[:, 3] = 0.0
    q[:, 0] = dw_a * dw_a / (2.0 * L) * (1.0 + ulps[:, 0] * 2.0 ** -52)        # du_A = u0 - 0
    q[:, 6] = -(dw_b * dw_b / (2.0 * L)) * (1.0 + ulps[:, 1] * 2.0 ** -52)     # du_B = 0 - u2
    return q


def sample(L):
    return np.ascontiguousarray(np.vstack([sample_states(N_GENERIC_EACH), inextensible_bends(L)]))


@pytest.mark.parametrize("L", LENGTHS)
def test_the_sample_holds_the_inextensible_bends(L):
    q = sample(L)
    assert len(q) >= 3000
    bends = q[-N_BENDS:]
    for du, dw in ((bends[:, 0] - bends[:, 3], bends[:, 1] - bends[:, 4]), (bends[:, 3] - bends[:, 6], bends[:, 4] - bends[:, 7])):
        dw2 = dw * dw
        a1 = np.array([abs(F(float(w)) - 2 * F(float(L)) * F(float(u))) for w, u in zip(dw2, du)], dtype=float)
        # (four ulp of du, the rounding of dw^2 and the two of forming dw^2 / (2 L): below eight ulp of dw^2)
        assert (dw2 > 0).all() and (a1 <= 8 * 2.0 ** -52 * dw2).all()
    # (and the generic kinds do not: A1 keeps its size there)
    g = q[:-N_BENDS]
    du, dw = g[:, 3] - g[:, 6], g[:, 4] - g[:, 7]
    assert (np.abs(dw * dw - 2 * L * du) > 1e-6 * (dw * dw + np.abs(2 * L * du))).mean() > 0.99


@pytest.mark.parametrize("L", LENGTHS)
def test_shared_form_is_as_accurate_as_the_symmetric_form(L):
    c = np.ascontiguousarray(pack(L))
    q = sample(L)
    shared, folded, sym = (np.empty((len(q), 8)) for _ in range(3))
    _lib().shared_patch(len(q), _p(c), _p(q), _p(shared), _p(folded), _p(sym))
    polys = element_outputs(c, inner_symmetric())
    forms = (("shared", shared), ("folded", folded), ("symmetric", sym))
    worst = {name: np.zeros(8) for name, _ in forms}
    bends = {name: np.zeros(8) for name, _ in forms}
    for i, row in enumerate(q):
        val, sc = exact_patch(c, polys, row)
        for name, got in forms:
            for j in range(8):
                assert sc[j] > 0
                err = float(abs(F(float(got[i][j])) - val[j]) / sc[j])
                worst[name][j] = max(worst[name][j], err)
                if i >= len(q) - N_BENDS:
                    bends[name][j] = max(bends[name][j], err)
    for name in worst:
        print(f"L = {L}: worst error / scale in units of 2^-53, {name}:", dict(zip(OUTPUTS, np.round(worst[name] / EPS, 2))))
        print(f"L = {L}:   on the inextensible bends alone, {name}:", dict(zip(OUTPUTS, np.round(bends[name] / EPS, 2))))
    ratio = worst["shared"] / worst["symmetric"]
    print(f"L = {L}: shared / symmetric:", dict(zip(OUTPUTS, np.round(ratio, 4))))
    assert np.isfinite(shared).all() and (worst["symmetric"] > 0).all()
    assert (worst["shared"] <= 2.0 * worst["symmetric"]).all(), ratio
    assert not np.array_equal(shared, sym)      # (another order of roundings: equal outputs would mean the same function ran twice)
    assert not np.array_equal(shared, folded)   # (nor is it the folded form again)
