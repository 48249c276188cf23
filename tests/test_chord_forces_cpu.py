"""CPU checks of the blocked fp64 stepper's chord-relative element polynomials (crb_math.h: elem_force_nonlinear_chord) and of
its RK4 stage ends (crb_math.h: Rk4Pos), through a host harness (tests/native/crb_chord.cpp, g++, no contraction).

Forces.  f2, cA1 W, f3, m_left, m_right of an element and r_u, r_w, r_phi of the middle node of a three-node patch, from the
chord form and from elem_force_nonlinear_sym (cA1 W of the symmetric form is its f1 + f2), each against the rational
polynomials evaluated exactly on the float inputs.  Scale of an output: the sum of the absolute values of its literal
monomials in a = phi1 L, b = phi2 L, dw, U = L du, u2, prefactors included (for a node, of both elements' contributions); it
depends on neither form.  Bound: the chord form is a different order of no more roundings, so its worst error may be at most
TWICE the symmetric form's on the same sample, output by output.  Measured (3000 patches), chord / symmetric, in units of
2^-53: f2 3.4 / 6.0, cA1 W 3.1 / 2e4 (the symmetric form's f1 + f2 cancels cA1 L u1), f3 5.1 / 4.0, m_left 5.4 / 6.3,
m_right 4.7 / 8.1, r_u 2.5 / 4.5, r_w 3.2 / 4.1, r_phi 4.5 / 5.1: the largest ratio is 1.28 (f3), every other one below 0.9.

RK4.  The stage ends carry the positions on the accelerations alone (q' = v); on q'' = -k q - k3 q^3 - c v |v| they follow the
stage-velocity bookkeeping they replace, and a long-double classical RK4, to rounding.  Bound: the two bookkeepings differ by
about a dozen roundings per step, each at most 2^-53 of the state's scale and of either sign, so their difference walks as
2^-52 sqrt(steps) (a dozen roundings of variance (2^-53)^2 / 3 each); 8 x 2^-52 sqrt(steps) is eight standard deviations
of that walk (the oscillator is damped: nothing amplifies it).  Measured over 400 steps, four step sizes (dt omega from 4e-4
to 0.5) and two initial states: 4.1e-15 of the state's scale against the old bookkeeping and 3.2e-15 against long double, for
a bound of 3.6e-14."""
import ctypes as C
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from tests.test_axial_regrouped_cpu import coef_pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
OUTPUTS = ("f2", "cA1 W", "f3", "m_left", "m_right", "r_u", "r_w", "r_phi")


def _lib():
    src = os.path.join(ROOT, "tests", "native", "crb_chord.cpp")
    so = os.path.join(ROOT, "tests", "native", "_build_libcrb_chord.so")
    hdr = os.path.join(ROOT, "continuum-robot_amd", "csrc", "crb_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.chord_patch.argtypes = [C.c_int, dp, dp, dp, dp, dp]
    L.rk4_scalar.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp, dp]
    L.rk4_scalar_long.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, dp, dp]
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ------------------------------------------------------------------ polynomials with rational coefficients
class Poly:
    """Polynomial in (a, b, dw, U, u2): {exponents: Fraction}."""
    NV = 5

    def __init__(self, terms=None):
        self.t = {k: v for k, v in (terms or {}).items() if v != 0}

    @staticmethod
    def var(i):
        return Poly({tuple(1 if j == i else 0 for j in range(Poly.NV)): F(1)})

    @staticmethod
    def const(c):
        return Poly({(0,) * Poly.NV: F(c)})

    def _lift(o):
        return o if isinstance(o, Poly) else Poly.const(o)

    def __add__(self, o):
        o = Poly._lift(o)
        t = dict(self.t)
        for k, v in o.t.items():
            t[k] = t.get(k, F(0)) + v
        return Poly(t)

    __radd__ = __add__

    def __neg__(self):
        return Poly({k: -v for k, v in self.t.items()})

    def __sub__(self, o):
        return self + (-Poly._lift(o))

    def __rsub__(self, o):
        return Poly._lift(o) - self

    def __mul__(self, o):
        o = Poly._lift(o)
        t = {}
        for k1, v1 in self.t.items():
            for k2, v2 in o.t.items():
                k = tuple(x + y for x, y in zip(k1, k2))
                t[k] = t.get(k, F(0)) + v1 * v2
        return Poly(t)

    __rmul__ = __mul__

    def __eq__(self, o):
        return self.t == Poly._lift(o).t

    def value_and_scale(self, vals):
        """The exact value at the Fractions `vals` and the sum of the absolute values of the monomials."""
        tot, sc = F(0), F(0)
        for k, cf in self.t.items():
            m = cf
            for x, n in zip(vals, k):
                if n:
                    m *= x ** n
            tot += m
            sc += abs(m)
        return tot, sc


A_, B_, DW, U_, U2 = (Poly.var(i) for i in range(5))
R = F


def inner_symmetric():
    """E, LT, P3, g, S, R of elem_force_nonlinear_sym / _regrouped, as the comments of crb_math.h state them."""
    s, d, p = A_ + B_, A_ - B_, A_ * B_
    s2, dw2 = s * s, DW * DW
    E = R(1, 15) * s2 - U_ - R(1, 10) * s * DW - R(1, 6) * p + R(3, 5) * dw2
    P3 = s * (R(1, 28) * (s2 - 6 * p) + U_ - R(27, 7) * dw2) + DW * (R(9, 7) * (s2 - 2 * p) - 12 * U_ + R(72, 7) * dw2)
    g = 3 * s - 6 * DW
    S = s * (R(1, 40) * s2 - R(11, 140) * p - R(1, 10) * U_ + R(9, 70) * dw2) + DW * (R(1, 5) * U_ - R(3, 70) * p - R(9, 35) * dw2)
    Rr = R(9, 280) * s2 - R(1, 20) * p + R(3, 140) * s * DW - R(1, 6) * U_ + R(9, 70) * dw2
    LTs = R(1, 20) * s - R(3, 5) * DW            # LT - L
    return E, LTs, P3, g, S, Rr, d


def inner_chord():
    """The same six in e = s - 2 dw, d, dw, U: the forms elem_force_nonlinear_chord evaluates."""
    s, d = A_ + B_, A_ - B_
    e = s - 2 * DW
    e2, d2, dw2 = e * e, d * d, DW * DW
    E = R(1, 2) * dw2 - U_ + R(1, 24) * d2 + R(1, 40) * e2
    LTs = R(1, 20) * e - R(1, 2) * DW
    P3 = e * (U_ + R(3, 56) * d2 - R(3, 2) * dw2 - R(1, 56) * e2) + DW * (R(3, 4) * d2 - 10 * U_ + 5 * dw2 + R(15, 28) * e2)
    S = e * (R(11, 560) * d2 - R(1, 10) * U_ + R(3, 20) * dw2 + R(3, 560) * e2) + DW * (R(1, 20) * d2 + R(3, 140) * e2)
    Rr = R(1, 80) * d2 - R(1, 6) * U_ + R(11, 560) * e2 + DW * (R(1, 4) * DW + R(1, 10) * e)
    return E, LTs, P3, 3 * e, S, Rr, d


def element_outputs(c, inner):
    """f2, cA1 W, f3, m_left, m_right as polynomials in (a, b, dw, U, u2) with the pack's floats as exact prefactors."""
    L, cA1, cA3, cD3, cA4, cD4 = (F(float(v)) for v in c)
    E, LTs, P3, g, S, Rr, d = inner
    X, Y = cA4 * S + cD4 * g, d * (cA4 * Rr + cD4)
    return [cA1 * E, cA1 * (U2 * (L + LTs)), cA3 * P3 - cD3 * g, X + Y, X - Y]


def test_the_chord_polynomials_are_the_symmetric_ones_identically():
    """Polynomial identities in (a, b, dw, U) with rational coefficients: nothing sampled."""
    for name, sym, chord in zip(("E", "LT", "P3", "g", "S", "R"), inner_symmetric(), inner_chord()):
        assert sym == chord, name
    c = coef_pack()
    for sym, chord in zip(element_outputs(c, inner_symmetric()), element_outputs(c, inner_chord())):
        assert sym == chord and len(sym.t) > 0


# ------------------------------------------------------------------ forces against exact values
def sample_states(n_each=500):
    """Three-node patches [u w phi] x 3: generic states over three decades, a ~ b to 1e-3 relative, s ~ 2 dw to 1e-3 relative
    (e cancels), both at once (a near-rigid rotation), states of the benchmark's size (after 1000 steps of its tip impulse:
    u 1e-7, w 1e-4, phi 1e-3 and smooth: neighbouring nodes differ by a few per cent) and large_state-sized ones
    (tests/test_blocked_axial_regrouped.py: u 1e-4, w 1e-3, phi 1e-1)."""
    rng = np.random.default_rng(2025)
    L = coef_pack()[0]
    scale = np.array([1e-4, 1e-2, 1e-1] * 3)
    gen = rng.normal(0.0, 1.0, (n_each, 9)) * scale * 10.0 ** rng.uniform(-3, 0, (n_each, 1))

    def near(rel):
        return 1.0 + rng.uniform(-rel, rel, n_each)

    ab = rng.normal(0.0, 1.0, (n_each, 9)) * scale
    ab[:, 5] = ab[:, 2] * near(1e-3)
    ab[:, 8] = ab[:, 5] * near(1e-3)
    ecan = rng.normal(0.0, 1.0, (n_each, 9)) * scale
    for k in (0, 1):   # dw = w_k - w_{k+1} = (a + b) / 2 up to 1e-3
        ecan[:, 3 * k + 4] = ecan[:, 3 * k + 1] - 0.5 * L * (ecan[:, 3 * k + 2] + ecan[:, 3 * k + 5]) * near(1e-3)
    rigid = rng.normal(0.0, 1.0, (n_each, 9)) * scale
    rigid[:, 5] = rigid[:, 2] * near(1e-3)
    rigid[:, 8] = rigid[:, 5] * near(1e-3)
    for k in (0, 1):
        rigid[:, 3 * k + 4] = rigid[:, 3 * k + 1] - 0.5 * L * (rigid[:, 3 * k + 2] + rigid[:, 3 * k + 5]) * near(1e-3)

    def smooth(size):
        base = rng.normal(0.0, 1.0, (n_each, 3)) * size
        return np.hstack([base * (1.0 + rng.normal(0.0, 0.03, (n_each, 3))) for _ in range(3)])

    return np.vstack([gen, ab, ecan, rigid, smooth(np.array([1e-7, 1e-4, 1e-3])), smooth(np.array([1e-4, 1e-3, 1e-1]))])


def exact_patch(c, polys, row):
    """Exact values and scales of the eight outputs for one patch."""
    L = F(float(c[0]))
    n = [[F(float(v)) for v in row[3 * k:3 * k + 3]] for k in range(3)]

    def elem(ql, qr):
        vals = (ql[2] * L, qr[2] * L, ql[1] - qr[1], L * (ql[0] - qr[0]), qr[0])
        return [p.value_and_scale(vals) for p in polys]

    A, B = elem(n[0], n[1]), elem(n[1], n[2])
    (f2A, sf2A), (f2B, sf2B), (cWB, scWB) = A[0], B[0], B[1]
    (f3A, sf3A), (f3B, sf3B), (mrA, smrA), (mlB, smlB) = A[2], B[2], A[4], B[3]
    val = [B[i][0] for i in range(5)] + [-f2A - (cWB - f2B), f3A - f3B, -mrA - mlB]
    sc = [B[i][1] for i in range(5)] + [sf2A + scWB + sf2B, sf3A + sf3B, smrA + smlB]
    return val, sc


@pytest.fixture(scope="module")
def forces():
    c = coef_pack()
    q = np.ascontiguousarray(sample_states())
    chord, regrouped, sym = (np.empty((len(q), 8)) for _ in range(3))
    _lib().chord_patch(len(q), _p(np.ascontiguousarray(c)), _p(q), _p(chord), _p(regrouped), _p(sym))
    polys = element_outputs(c, inner_symmetric())
    worst = {name: np.zeros(8) for name in ("chord", "regrouped", "symmetric")}
    for i, row in enumerate(q):
        val, sc = exact_patch(c, polys, row)
        for name, got in (("chord", chord[i]), ("regrouped", regrouped[i]), ("symmetric", sym[i])):
            for j in range(8):
                assert sc[j] > 0
                worst[name][j] = max(worst[name][j], float(abs(F(float(got[j])) - val[j]) / sc[j]))
    return q, chord, sym, worst


def test_the_sample_holds_the_cancelling_cases(forces):
    q = forces[0]
    L = coef_pack()[0]
    a, b, dw = L * q[:, 5], L * q[:, 8], q[:, 4] - q[:, 7]
    s = a + b
    assert len(q) >= 3000
    assert (np.abs(a - b) <= 1.1e-3 * np.abs(a)).sum() >= 1000
    assert (np.abs(s - 2 * dw) <= 1.1e-3 * np.abs(s)).sum() >= 1000
    assert ((np.abs(a - b) <= 1.1e-3 * np.abs(a)) & (np.abs(s - 2 * dw) <= 1.1e-3 * np.abs(s))).sum() >= 500


def test_chord_form_is_as_accurate_as_the_symmetric_form(forces):
    _, chord, sym, worst = forces
    for name in worst:
        print(f"worst error / scale in units of 2^-53, {name}:", dict(zip(OUTPUTS, np.round(worst[name] / EPS, 2))))
    ratio = worst["chord"] / worst["symmetric"]
    print("chord / symmetric:", dict(zip(OUTPUTS, np.round(ratio, 3))))
    assert (worst["symmetric"] > 0).all()
    assert (worst["chord"] <= 2.0 * worst["symmetric"]).all(), ratio
    assert not np.array_equal(chord, sym)    # (another order of roundings: equal outputs would mean the same function ran twice)


# ------------------------------------------------------------------ RK4 stage ends
RK_STEPS = 400
RK_CASES = [(dt, q0, v0) for dt in (2e-5, 1e-3, 7.3e-3, 2.5e-2) for q0, v0 in ((1.0, 0.0), (0.3, -25.0))]
RK_K = np.array([400.0, 900.0, 0.35])     # omega = 20 (dt omega up to 0.5), a cubic term of the linear one's size, drag


def _rk(form, dt, q0, v0):
    out = np.empty(4)
    _lib().rk4_scalar(form, RK_STEPS, dt, q0, v0, _p(RK_K), _p(out))
    return out


def test_stage_ends_follow_the_stage_velocity_bookkeeping_and_long_double_rk4():
    bound = 8 * 2 * EPS * np.sqrt(RK_STEPS)
    worst_old = worst_ld = 0.0
    for dt, q0, v0 in RK_CASES:
        new, old = _rk(0, dt, q0, v0), _rk(1, dt, q0, v0)
        ld = np.empty(2)
        _lib().rk4_scalar_long(RK_STEPS, dt, q0, v0, _p(RK_K), _p(ld))
        scale = np.array([max(new[2], old[2]), max(new[3], old[3])])
        assert np.isfinite(new).all() and (scale > 0).all()
        assert abs(new[0] - q0) > 1e-3 * scale[0] or dt < 1e-4      # (the state moved: the comparison is not of two copies of x0)
        worst_old = max(worst_old, (np.abs(new[:2] - old[:2]) / scale).max())
        worst_ld = max(worst_ld, (np.abs(new[:2] - ld) / scale).max())
    print(f"stage ends against the stage-velocity bookkeeping {worst_old:.2e}, against long double {worst_ld:.2e}, bound {bound:.2e}")
    assert worst_old <= bound and worst_ld <= bound
