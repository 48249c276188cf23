"""CPU side of the implicit stepper's tangent (crb_step_implicit_tangent[_sched], BeamEnsemble.step_implicit_tangent /
linearize_implicit; tests/test_implicit_tangent.py holds the GPU side and imports the inputs from here).

  * the two entry points are declared in include/crbeam.h, exported and bound; CRB_VERSION is unchanged; the two methods have the
    documented signatures;
  * every refusal shows on a host-only plan, in the documented order -- CRB_EINVAL (the call's own cases, then the
    schedule's), CRB_EUNSUPPORTED, CRB_ENODEV -- names the entry point and the argument and leaves *t_end alone; the order is
    checked with two faults in one call;
  * the inputs of the GPU file's finite-difference test are proved on the oracle alone: fd_check's rule is capped at 1e-6, so on
    every DOF block of every case the oracle's own two central differences (steps e and e / 4) agree within SELF_BAR;
  * the dense Cayley recursion that the GPU file holds linearize_implicit to is what the oracle's implicit(n_iter=1) computes on
    the linear rods, per n x n block.

The difference steps (FD_EPS): 1e-3 relative on the amplitude, 1e-3 along the held-force direction, 1e-4 along the state
direction -- except the state direction of n64_drag_three_iterations, whose self-difference at 1e-4 is 1.3e-6 on w, phi and
dw/dt and falls linearly with the step (the kink of the drag's |v|): 4e-6 there."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests.helpers import BLOCKS, block_errs, nitinol_columns, oracle_beam
from tests.test_implicit_adjoint import FD_CASES, FD_STEPS, blockwise, fd_inputs
from tests.test_tangent_linear import oracle_kw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_step_implicit_tangent", "crb_step_implicit_tangent_sched")
TAG = "[implicit-tangent]"
P = C.c_void_p
X_, DX, F, DSCHED, HELD, DHELD, AMP, DAMP = (P(64 * k) for k in range(1, 9))   # distinct fake device addresses (never read)
H, STEPS, K, HOLD = 1e-4, 33, 5, 7
SELF_BAR = 2.5e-7
FD_EPS = {name: dict(amp=1e-3, held=1e-3, x0=1e-4) for name in FD_CASES}
FD_EPS["n64_drag_three_iterations"]["x0"] = 4e-6


# ------------------------------------------------------------------ 1. symbols and signatures
def header():
    return open(os.path.join(ROOT, "include", "crbeam.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from continuum_robot import _native as nat

    hdr, lib = header(), nat.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.crb_version() == 106 == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))
    doc = hdr[hdr.index("Tangent of the implicit stepper"):hdr.index("int crb_step_implicit_tangent(")]
    assert "example_utilities.py:153-159" in doc and "linear_quadratic_regulator.py" in doc


def test_python_methods_have_the_documented_signatures():
    from continuum_robot.batched import BeamEnsemble

    sig = inspect.signature(BeamEnsemble.step_implicit_tangent)
    assert list(sig.parameters) == ["self", "n_steps", "h", "dx0_red", "n_iter", "impulse_amp", "impulse_duration", "impulse_index",
                                    "held_force", "d_impulse_amp", "d_held_force", "t0"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(n_iter=2, impulse_amp=None, impulse_duration=0.01, impulse_index=-2, held_force=None, d_impulse_amp=None,
                            d_held_force=None, t0=None)
    sig = inspect.signature(BeamEnsemble.linearize_implicit)
    assert list(sig.parameters) == ["self", "h", "n_steps", "n_iter", "x_red", "held_force"]
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == dict(
        n_steps=1, n_iter=2, x_red=None, held_force=None)


# ------------------------------------------------------------------ 2. refusals, before the device is touched
class Calls:
    """the two entry points on one host-only plan, with valid fake arguments unless overridden"""

    def __init__(self, dtype, n=4):
        from continuum_robot import _native as nat

        self.nat, self.lib = nat, nat.load()
        self.plan = nat.Plan(nitinol_columns(n, "nonlinear" if n < 100 else "linear"), n_beams=2, device=-1, dtype=dtype)
        self.t_end = C.c_double(-1.0)

    def sched(self, f=F.value, k=K, hold=HOLD):
        return self.nat.InputSchedule(f, k, hold)

    def plain(self, x=X_, dx=DX, n_dir=2, h=H, n=STEPS, n_iter=2, desc=None, din=None, plan=True):
        return self.lib.crb_step_implicit_tangent(self.plan.h if plan else None, x, dx, n_dir, 0.0, h, n, n_iter, desc, din,
                                                  C.byref(self.t_end), None)

    def scheduled(self, s, d_sched=DSCHED, x=X_, dx=DX, n_dir=2, h=H, n=STEPS, n_iter=2, desc=None, din=None, plan=True):
        return self.lib.crb_step_implicit_tangent_sched(self.plan.h if plan else None, x, dx, n_dir, 0.0, h, n, n_iter, desc, din, s,
                                                        d_sched, C.byref(self.t_end), None)

    def error(self):
        return self.lib.crb_last_error().decode()

    def refused(self, rc, code, *words):
        msg = self.error()
        assert rc == code, (rc, code, msg)
        for w in words:
            assert w in msg, (w, msg)
        assert self.t_end.value == -1.0          # (*t_end is written only by a call that is not refused)


def bad_input(nat):
    d = nat.InputDesc()
    d.kind = 77
    return C.byref(d)


def held_input(nat):
    d = nat.InputDesc()
    d.kind, d.f_held = nat.CRB_INPUT_NONE, HELD.value
    return C.byref(d)


def impulse_input(nat):
    d = nat.InputDesc()
    d.kind, d.node, d.dof, d.duration, d.amp = nat.CRB_INPUT_IMPULSE, 4, 1, 0.01, AMP.value
    return C.byref(d)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_in_order_before_the_device(dtype):
    c = Calls(dtype)
    nat, inval = c.nat, c.nat.CRB_EINVAL
    last = nat.CRB_ENODEV if dtype == "f64" else nat.CRB_EUNSUPPORTED
    last_word = "host-only" if dtype == "f64" else "fp64"
    ok = C.byref(c.sched())
    worst = C.byref(c.sched(f=None, k=0, hold=0))
    d_amp = C.byref(nat.InputTangent(DAMP.value, None))
    df_held = C.byref(nat.InputTangent(None, DHELD.value))
    calls = ((c.plain, NAMES[0]), (lambda **kw: c.scheduled(ok, **kw), NAMES[1]), (lambda **kw: c.scheduled(worst, **kw), NAMES[1]))
    for call, who in calls:
        # the call's own CRB_EINVAL cases, each alone (and, in the third form, next to a schedule bad in every field)
        c.refused(call(plan=False), inval, who, "null plan")
        c.refused(call(x=None), inval, who, "null state or tangent")
        c.refused(call(dx=None), inval, who, "null state or tangent")
        for n_dir in (0, -1, 65536):
            c.refused(call(n_dir=n_dir), inval, who, "n_dir")
        c.refused(call(n=-1), inval, who, "n_steps must")
        for n_iter in (0, 17):
            c.refused(call(n_iter=n_iter), inval, who, "n_iter")
        for h in (0.0, -1e-4, float("nan")):
            c.refused(call(h=h), inval, who, "h must")
        c.refused(call(desc=bad_input(nat)), inval, who, "input kind")
        c.refused(call(din=d_amp), inval, who, "d_amp")                              # no impulse input
        c.refused(call(desc=held_input(nat), din=d_amp), inval, who, "d_amp")
        # two faults in one call: the earlier one of the documented order is the one reported
        c.refused(call(plan=False, x=None), inval, who, "null plan")
        c.refused(call(x=None, n_dir=0), inval, who, "null state or tangent")
        c.refused(call(n_dir=0, n=-1), inval, who, "n_dir")
        c.refused(call(n=-1, n_iter=0), inval, who, "n_steps must")
        c.refused(call(n_iter=0, h=0.0), inval, who, "n_iter")
        c.refused(call(h=0.0, desc=bad_input(nat)), inval, who, "h must")
        c.refused(call(desc=bad_input(nat), din=d_amp), inval, who, "input kind")
    # the schedule's cases, after the call's own
    who = NAMES[1]
    c.refused(c.scheduled(None, d_sched=DSCHED), inval, who, "d_sched")
    c.refused(c.scheduled(None, d_sched=DSCHED, din=d_amp), inval, who, "d_amp")                     # (the earlier case)
    for bad, word in ((c.sched(f=None), "f_sched"), (c.sched(k=0), "n_intervals"), (c.sched(k=-3), "n_intervals"),
                      (c.sched(hold=0), "hold"), (c.sched(hold=-1), "hold")):
        c.refused(c.scheduled(C.byref(bad)), inval, who, word)
    c.refused(c.scheduled(worst), inval, who, "f_sched")
    c.refused(c.scheduled(C.byref(c.sched(k=0, hold=0))), inval, who, "n_intervals")
    c.refused(c.scheduled(ok, n=K * HOLD + 1), inval, who, "n_steps exceeds")
    c.refused(c.scheduled(ok, desc=held_input(nat)), inval, who, "input->f_held")
    c.refused(c.scheduled(ok, din=df_held), inval, who, "df_held")
    c.refused(c.scheduled(ok, desc=held_input(nat), din=df_held), inval, who, "input->f_held")        # (f_held comes first)
    c.refused(c.scheduled(ok, n=K * HOLD + 1, din=df_held), inval, who, "n_steps exceeds")
    # valid arguments: CRB_EUNSUPPORTED for fp32, CRB_ENODEV for the host-only fp64 plan -- only now
    for rc, who in ((c.plain(), NAMES[0]), (c.plain(n_dir=1, n_iter=16, n=1), NAMES[0]), (c.plain(n_dir=65535), NAMES[0]),
                    (c.plain(desc=impulse_input(nat), din=d_amp), NAMES[0]), (c.plain(desc=held_input(nat), din=df_held), NAMES[0]),
                    (c.plain(n=0), NAMES[0]), (c.scheduled(ok), NAMES[1]), (c.scheduled(ok, d_sched=None), NAMES[1]),
                    (c.scheduled(ok, n=K * HOLD), NAMES[1]), (c.scheduled(ok, desc=impulse_input(nat), din=d_amp), NAMES[1])):
        c.refused(rc, last, who, last_word)
    # without a schedule the scheduled entry point is the plain one: the same code and message
    for kw in (dict(), dict(n=-1), dict(n_iter=0), dict(din=d_amp), dict(x=None)):
        want = (c.plain(**kw), c.error())
        assert (c.scheduled(None, d_sched=None, **kw), c.error()) == want, kw


def test_more_than_256_thread_carried_nodes_are_unsupported_before_the_device():
    c = Calls("f64", n=300)
    ok = C.byref(c.sched())
    c.refused(c.plain(n_iter=0), c.nat.CRB_EINVAL, NAMES[0], "n_iter")                 # (CRB_EINVAL still comes first)
    c.refused(c.scheduled(C.byref(c.sched(hold=0))), c.nat.CRB_EINVAL, NAMES[1], "hold")
    c.refused(c.plain(), c.nat.CRB_EUNSUPPORTED, NAMES[0], "256")
    c.refused(c.scheduled(ok), c.nat.CRB_EUNSUPPORTED, NAMES[1], "256")
    assert Calls("f64", n=256).plain() == c.nat.CRB_ENODEV


# ------------------------------------------------------------------ 3. the inputs of the GPU file's FD test, on the oracle alone
class FdCase:
    """One FD case: fd_inputs' start state (the oracle's after 30 steps under the impulse), amplitude, held force and directions,
    and the oracle's rollouts F(e) of FD_STEPS steps along each of the three inputs (memoised: fd_check asks for the same four)"""

    def __init__(self, name):
        self.name, self.c = name, FD_CASES[name]
        self.i = i = fd_inputs(self.c)
        self.ob, self.fi, self.n = i["ob"], i["fi"], i["n"]
        self.eps = FD_EPS[name]
        self._memo = {}

    def run(self, x0=None, amp=0.0, u=None):
        i, c = self.i, self.c
        return self.ob.implicit(i["X"] if x0 is None else x0, c["h"], FD_STEPS, n_iter=c["n_iter"], amp=amp, duration=i["dur"], u_held=u)

    def F(self, kind):
        i = self.i

        def f(e):
            if (kind, e) not in self._memo:
                self._memo[(kind, e)] = {"amp": lambda: self.run(amp=i["amp"] * (1.0 + e)),
                                         "held": lambda: self.run(u=i["U"] + e * i["dU"]),
                                         "x0": lambda: self.run(x0=i["X"] + e * i["dX"], amp=i["amp"])}[kind]()
            return self._memo[(kind, e)]
        return f

    def differences(self, kind):
        F, e = self.F(kind), self.eps[kind]
        return (F(e) - F(-e)) / (2 * e), (F(e / 4) - F(-e / 4)) / (e / 2)


@functools.lru_cache(maxsize=None)
def fd_case(name):
    return FdCase(name)


@pytest.mark.parametrize("kind", ["amp", "held", "x0"])
@pytest.mark.parametrize("name", list(FD_CASES))
def test_oracle_differences_agree_on_every_block(name, kind):
    k = fd_case(name)
    fd1, fd4 = k.differences(kind)
    assert np.all(np.isfinite(fd4)) and np.max(np.abs(fd4)) > 0.0
    errs = block_errs(fd1, fd4, k.fi)
    print(f"{TAG} {name} | oracle differences along {kind} (e = {k.eps[kind]:g}) | " + " ".join(f"{b} {e:.1e}" for b, e in errs.items()))
    assert set(errs) == set(BLOCKS)                                 # no block is left out
    for blk, e in errs.items():
        assert e <= SELF_BAR, (name, kind, blk, e)


# ------------------------------------------------------------------ 4. the dense Cayley recursion is the oracle's implicit(n_iter=1)
LINEAR_RODS = {"n6_h1e-4": (6, 1e-4), "n10_h1e-3": (10, 1e-3), "n64_h1e-3": (64, 1e-3)}


def cayley(A, Bu, h, n_steps):
    """(A_d, B_d) of n_steps steps of the implicit midpoint rule on xdot = A x + Bu u with u held: one step is
    A_1 = (I - h/2 A)^-1 (I + h/2 A), B_1 = (I - h/2 A)^-1 h Bu; then x_{k+1} = A_1 x_k + B_1 u"""
    I = np.eye(A.shape[0])
    A1 = np.linalg.solve(I - 0.5 * h * A, I + 0.5 * h * A)
    B1 = np.linalg.solve(I - 0.5 * h * A, h * Bu)
    Ad, Bd = I.copy(), np.zeros_like(B1)
    for _ in range(n_steps):
        Ad, Bd = A1 @ Ad, A1 @ Bd + B1
    return Ad, Bd


@pytest.mark.parametrize("rod", list(LINEAR_RODS))
def test_cayley_recursion_is_the_oracles_implicit_step_on_linear_rods(rod):
    n_elem, h = LINEAR_RODS[rod]
    ob = oracle_beam(nitinol_columns(n_elem, "linear"), **oracle_kw(False, False))
    n = ob.n
    A = np.stack([ob.rhs(e) for e in np.eye(2 * n)], axis=1)
    Bu = np.stack([ob.rhs(np.zeros(2 * n), u) for u in np.eye(n)], axis=1)
    for n_steps in (1, 3):
        Ad, Bd = cayley(A, Bu, h, n_steps)
        got_A = np.stack([ob.implicit(e, h, n_steps, n_iter=1) for e in np.eye(2 * n)], axis=1)
        got_B = np.stack([ob.implicit(np.zeros(2 * n), h, n_steps, n_iter=1, u_held=u) for u in np.eye(n)], axis=1)
        e_a, e_b = blockwise(got_A, Ad, n), blockwise(got_B, Bd, n)
        print(f"{TAG} {rod} | {n_steps} step(s) | oracle against Cayley | A_d {e_a:.1e} | B_d {e_b:.1e}")
        assert e_a <= 1e-10 and e_b <= 1e-10, (rod, n_steps, e_a, e_b)
