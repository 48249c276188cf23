"""CPU checks of the blocked fp64 stepper's folded element polynomials (crb_math.h: elem_fold_build,
elem_force_nonlinear_folded) through a host harness (tests/native/crb_folded.cpp, g++, no contraction).

Constants.  The 30 folded constants of a pack equal their exact rational values (products of the pack's floats, powers of L
and the chord form's rationals) rounded once.

Identities.  With those rationals unrounded, f2, cA1 W, f3, m_left and m_right of the folded form are the symmetric form's
polynomials identically (nothing sampled).

Forces.  f2, cA1 W, f3, m_left, m_right of an element and r_u, r_w, r_phi of the middle node of a three-node patch, from the
folded form and from elem_force_nonlinear_sym, each against the rational polynomials evaluated exactly on the float inputs,
on tests/test_chord_forces_cpu.py's sample and with its scales, at element lengths 0.25 (the shipped pack: the products
with L are exact), 0.3 and 0.0731 (they round), the radius scaled with L.  Bound, the project's own: the folded form's worst
error may be at most TWICE the symmetric form's on the same sample, output by output.  Measured (3000 patches), folded /
symmetric in units of 2^-53 and their ratio, in the order f2, cA1 W, f3, m_left, m_right, r_u, r_w, r_phi:
  L = 0.25:   3.35 / 6.01 (0.56), 2.16 / 2e4 (1e-4), 3.89 / 3.95 (0.98), 4.76 / 6.34 (0.75), 4.67 / 8.07 (0.58),
              2.39 / 4.53 (0.53), 3.09 / 4.05 (0.76), 4.13 / 5.09 (0.81)
  L = 0.3:    3.65 / 7.04 (0.52), 1.93 / 1.4e4 (1e-4), 3.92 / 3.72 (1.05), 3.79 / 7.10 (0.53), 4.25 / 6.92 (0.61),
              2.45 / 5.61 (0.44), 3.01 / 3.34 (0.90), 3.57 / 5.29 (0.68)
  L = 0.0731: 3.37 / 6.79 (0.50), 2.22 / 2e4 (1e-4), 5.08 / 5.36 (0.95), 5.13 / 5.75 (0.89), 4.89 / 6.06 (0.81),
              2.80 / 5.08 (0.55), 5.31 / 5.62 (0.94), 6.16 / 5.14 (1.20)
(the symmetric form's f1 + f2 cancels cA1 L u1, hence its cA1 W)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from tests.test_chord_forces_cpu import (A_, B_, DW, EPS, OUTPUTS, U2, U_, _p, element_outputs, exact_patch, inner_symmetric,
                                         sample_states)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0.25, 0.3, 0.0731)


def pack(L):
    """The nonlinear ElemCoef pack of the benchmark's rod at element length L, the radius scaled with L (elem_coef_build)."""
    r, E = 0.005 * (L / 0.25), 75e9
    EA, EI = E * (np.pi * r**2), E * (np.pi * r**4 / 4)
    iL2, tenth_iL3 = 1.0 / (L * L), 0.1 / (L * L * L)
    return np.array([L, EA * iL2, EA * tenth_iL3, 20.0 * EI * tenth_iL3, 0.5 * EA * iL2, EI * iL2])


def _lib():
    src = os.path.join(ROOT, "tests", "native", "crb_folded.cpp")
    so = os.path.join(ROOT, "tests", "native", "_build_libcrb_folded.so")
    hdr = os.path.join(ROOT, "continuum-robot_amd", "csrc", "crb_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.fold_constants.argtypes = [dp, dp]
    lib.folded_patch.argtypes = [C.c_int, dp, dp, dp, dp]
    return lib


def exact_constants(c):
    """The folded constants as exact rationals of the pack's floats, in the order of crb_math.h's FK_* enum."""
    L, cA1, cA3, cD3, cA4, cD4 = (F(float(v)) for v in c)
    L2, L3 = L * L, L * L * L
    return [
        2 / L,                                                                                   # eps = sigma - k dw
        cA1 / 2, -cA1 * L, cA1 * L2 / 24, cA1 * L2 / 40,                                         # f2: dw^2, du, delta^2, eps^2
        cA1 * L, cA1 * L / 20, -cA1 / 2,                                                         # cA1 LT: 1, eps, dw
        -3 * cD3 * L, cA3 * L2, F(3, 56) * cA3 * L3, -F(3, 2) * cA3 * L, -cA3 * L3 / 56,         # f3 | eps: 1, du, delta^2, dw^2, eps^2
        F(3, 4) * cA3 * L2, -10 * cA3 * L, 5 * cA3, F(15, 28) * cA3 * L2,                        # f3 | dw: delta^2, du, dw^2, eps^2
        3 * cD4 * L, F(11, 560) * cA4 * L3, -cA4 * L2 / 10, F(3, 20) * cA4 * L, F(3, 560) * cA4 * L3,   # X | eps: 1, delta^2, du, dw^2, eps^2
        cA4 * L2 / 20, F(3, 140) * cA4 * L2,                                                     # X | dw: delta^2, eps^2
        cD4 * L, cA4 * L3 / 80, -cA4 * L2 / 6, F(11, 560) * cA4 * L3, cA4 * L / 4, cA4 * L2 / 10,  # Rf: 1, delta^2, du, eps^2, dw dw, dw eps
    ]


def folded_outputs(c, k):
    """f2, cA1 W, f3, m_left, m_right of the folded form with the constants k, as polynomials in (a, b, dw, U, u2)."""
    L = F(float(c[0]))
    du, sg, dl = U_ * (1 / L), (A_ + B_) * (1 / L), (A_ - B_) * (1 / L)
    eps = sg - k[0] * DW
    e2, d2, dw2 = eps * eps, dl * dl, DW * DW
    f2 = k[1] * dw2 + k[2] * du + k[3] * d2 + k[4] * e2
    LT = k[5] + k[6] * eps + k[7] * DW
    f3 = eps * (k[8] + k[9] * du + k[10] * d2 + k[11] * dw2 + k[12] * e2) + DW * (k[13] * d2 + k[14] * du + k[15] * dw2 + k[16] * e2)
    X = eps * (k[17] + k[18] * d2 + k[19] * du + k[20] * dw2 + k[21] * e2) + DW * (k[22] * d2 + k[23] * e2)
    Rf = k[24] + k[25] * d2 + k[26] * du + k[27] * e2 + DW * (k[28] * DW + k[29] * eps)
    return [f2, U2 * LT, f3, X + dl * Rf, X - dl * Rf]


@pytest.mark.parametrize("L", LENGTHS)
def test_the_constants_are_the_exact_rationals_rounded_once(L):
    c = np.ascontiguousarray(pack(L))
    lib = _lib()
    n = lib.fold_count()
    exact = exact_constants(c)
    assert n == len(exact) == 30
    k = np.empty(n)
    lib.fold_constants(_p(c), _p(k))
    want = np.array([float(v) for v in exact])     # (Fraction -> float rounds the exact value once, to nearest)
    assert (want != 0).all()
    assert np.array_equal(k, want), np.nonzero(k != want)


@pytest.mark.parametrize("L", LENGTHS)
def test_the_folded_polynomials_are_the_symmetric_ones_identically(L):
    """Polynomial identities in (a, b, dw, U, u2) with rational coefficients: nothing sampled."""
    c = pack(L)
    for name, sym, fold in zip(OUTPUTS, element_outputs(c, inner_symmetric()), folded_outputs(c, exact_constants(c))):
        assert sym == fold and len(sym.t) > 0, name


# ------------------------------------------------------------------ forces against exact values
@pytest.fixture(scope="module")
def sample():
    return np.ascontiguousarray(sample_states())


@pytest.mark.parametrize("L", LENGTHS)
def test_folded_form_is_as_accurate_as_the_symmetric_form(sample, L):
    c = np.ascontiguousarray(pack(L))
    q = sample
    assert len(q) >= 3000
    folded, sym = np.empty((len(q), 8)), np.empty((len(q), 8))
    _lib().folded_patch(len(q), _p(c), _p(q), _p(folded), _p(sym))
    polys = element_outputs(c, inner_symmetric())
    worst = {"folded": np.zeros(8), "symmetric": np.zeros(8)}
    for i, row in enumerate(q):
        val, sc = exact_patch(c, polys, row)
        for name, got in (("folded", folded[i]), ("symmetric", sym[i])):
            for j in range(8):
                assert sc[j] > 0
                worst[name][j] = max(worst[name][j], float(abs(F(float(got[j])) - val[j]) / sc[j]))
    for name in worst:
        print(f"L = {L}: worst error / scale in units of 2^-53, {name}:", dict(zip(OUTPUTS, np.round(worst[name] / EPS, 2))))
    ratio = worst["folded"] / worst["symmetric"]
    print(f"L = {L}: folded / symmetric:", dict(zip(OUTPUTS, np.round(ratio, 4))))
    assert np.isfinite(folded).all() and (worst["symmetric"] > 0).all()
    assert (worst["folded"] <= 2.0 * worst["symmetric"]).all(), ratio
    assert not np.array_equal(folded, sym)    # (another order of roundings: equal outputs would mean the same function ran twice)
