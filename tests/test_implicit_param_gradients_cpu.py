"""CPU side of the implicit adjoint's parameter gradients (crb_implicit_adjoint_params_work_bytes,
crb_step_implicit_adjoint_params, crb_step_implicit_adjoint_params_sched; tests/test_implicit_param_gradients.py holds the GPU
side and imports the case tables, the losses and the oracle's differences from here).

  * the entry points are declared in include/crbeam.h, exported and bound; the version is the header's;
  * every refusal shows on a host-only plan, in the documented order, and names the entry point and the argument;
  * the work-bytes formula;
  * the inputs of the GPU file are proved on the oracle alone: for every case and direction it asserts, the oracle's own two
    central differences agree to SELF_BAR = 2.5e-7.

The loss.  w_tip after 40 steps plus four weighted tip samples (steps 10, 20, 30, 40), from rest under the tip impulse whose
window closes after 10 steps.  Every sample is a full oracle run from step 0, as tests/test_implicit_adjoint.py takes them:
OracleBeam.implicit restarts its iterate per call, so a run continued from sample to sample is NOT the map one call computes.
The scheduled loss is the opposite on purpose: one call per interval with that interval's force, which IS the scheduled map.

Step sizes of the differences (relative; g_x in units of 9.81): 1e-4 for elastic_modulus and moment_inertia -- at 1e-3 their two
differences are 2.4e-6 apart -- and 1e-3 for drag_coef, fluid_density, g_y and g_x.  The figures the oracle gave at these steps
are in the docstrings of the tests below."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests.helpers import nitinol_columns
from tests.test_param_gradients import AMPS, C_REC, interior_pin, perturbed_oracle, pinned_root

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_step_implicit_adjoint_params", "crb_step_implicit_adjoint_params_sched")
WORK_BYTES = "crb_implicit_adjoint_params_work_bytes"
TAG = "[implicit-param-grad]"
SELF_BAR = 2.5e-7

STEPS, EVERY, WINDOW = 40, 10, 10.0       # steps, steps per sample, impulse window in steps
EPS = {"elastic_modulus": 1e-4, "moment_inertia": 1e-4, "drag_coef": 1e-3, "fluid_density": 1e-3, "g_y": 1e-3, "g_x": 1e-3}
ALL_DIRECTIONS = tuple(EPS)
MAPPING_DIRECTIONS = ("elastic_modulus", "fluid_density", "g_y")


def case(n, kind, h, n_iter, drag=True, grav=True, bcs=None):
    return dict(n=n, kind=kind, h=h, n_iter=n_iter, drag=drag, grav=grav, bcs=bcs)


# every direction (drag and gravity on)
ORACLE_CASES = {
    "nonlinear_8_packed": case(8, "nonlinear", 1e-4, 2),
    "nonlinear_32_one_iteration": case(32, "nonlinear", 2e-4, 1),
    "nonlinear_32_two_iterations": case(32, "nonlinear", 2e-4, 2),
    "linear_32_one_iteration": case(32, "linear", 2e-4, 1),
    "nonlinear_64_drag_three_iterations": case(64, "nonlinear", 5e-4, 3),
    "linear_6_h_1e-3_one_iteration": case(6, "linear", 1e-3, 1),
}
# moment_inertia on drag-free, gravity-free linear rods: with one iteration the iteration-matrix term is 8.8e-2 (6 elements) and
# 2.4e-2 (32 elements) of the derivative; with two it is zero to rounding (one iteration is exact on a linear, drag-free rod)
MATRIX_CASES = {
    "linear_6_one_iteration": case(6, "linear", 1e-4, 1, False, False),
    "linear_32_one_iteration": case(32, "linear", 2e-4, 1, False, False),
    "linear_6_two_iterations": case(6, "linear", 1e-4, 2, False, False),
    "linear_32_two_iterations": case(32, "linear", 2e-4, 2, False, False),
}
# every thread mapping: h = 2e-4, two iterations
MAPPING_CASES = {
    "linear_1": case(1, "linear", 2e-4, 2), "linear_6": case(6, "linear", 2e-4, 2), "linear_33": case(33, "linear", 2e-4, 2),
    "linear_64": case(64, "linear", 2e-4, 2), "linear_65": case(65, "linear", 2e-4, 2),
    "linear_129": case(129, "linear", 2e-4, 2), "linear_256": case(256, "linear", 2e-4, 2),
    "pinned_root_32_slots": case(31, "linear", 2e-4, 2, bcs=pinned_root),
    "interior_pin_32_slots": case(32, "linear", 2e-4, 2, bcs=interior_pin),
    "nonlinear_64": case(64, "nonlinear", 2e-4, 2),
}
# a control schedule of 4 intervals x 10 steps on the 8-element rod
SCHED_CASE = case(8, "nonlinear", 1e-4, 2)
SCHED_K, SCHED_HOLD = 4, 10
SCHED_DIRECTIONS = ("elastic_modulus", "fluid_density")
# per-case step sizes, where the oracle's two differences at EPS miss SELF_BAR (none dropped: the step moves, not the bar)
EPS_OF_CASE = {}
TABLES = {"oracle": ORACLE_CASES, "matrix": MATRIX_CASES, "mapping": MAPPING_CASES, "schedule": {"nonlinear_8": SCHED_CASE}}
DIRECTIONS = {"oracle": ALL_DIRECTIONS, "matrix": ("moment_inertia",), "mapping": MAPPING_DIRECTIONS, "schedule": SCHED_DIRECTIONS}


def columns(c):
    return nitinol_columns(c["n"], c["kind"], bcs=c["bcs"](c["n"]) if c["bcs"] else None)


def schedule(n):
    """the control of the scheduled case, [K, n] reduced: transverse entries only (the shipped f1 lets axial modes run away)"""
    rng = np.random.default_rng(515)
    w = np.arange(n) % 3 == 1
    return np.where(w[None], rng.normal(0.0, 0.05, (SCHED_K, n)), 0.0)


def oracle_loss(ob, c, amp):
    """w_tip(T) + sum_k C_REC[k] w_tip(t_k): every term one run of the oracle's implicit() from rest at step 0"""
    tip, dur = ob.n - 2, WINDOW * c["h"]
    run = lambda k: ob.implicit(np.zeros(2 * ob.n), c["h"], k, n_iter=c["n_iter"], amp=amp, duration=dur)[tip]   # noqa: E731
    return run(STEPS) + sum(C_REC[k] * run(EVERY * (k + 1)) for k in range(4))


def oracle_sched_loss(ob, c, amp):
    """the same loss of the scheduled map: one implicit() call per interval, the state and the clock carried over"""
    tip, dur, U = ob.n - 2, WINDOW * c["h"], schedule(ob.n)
    x, t, loss = np.zeros(2 * ob.n), 0.0, 0.0
    for k in range(SCHED_K):
        x = ob.implicit(x, c["h"], SCHED_HOLD, n_iter=c["n_iter"], amp=amp, duration=dur, t0=t, u_held=U[k])
        for _ in range(SCHED_HOLD):
            t = t + c["h"]
        loss += C_REC[k] * x[tip]
    return loss + x[tip]


def step_size(table, name, direction):
    return EPS_OF_CASE.get((table, name), {}).get(direction, EPS[direction])


@functools.lru_cache(maxsize=None)
def oracle_differences(table, name, direction):
    """[(FD(eps), FD(eps / 4)) for each amplitude of AMPS] of the case's loss along ``direction``"""
    c = TABLES[table][name]
    cols, eps = columns(c), step_size(table, name, direction)
    loss = oracle_sched_loss if table == "schedule" else oracle_loss

    def L(e):
        ob = perturbed_oracle(cols, direction, e, c["drag"], c["grav"])
        return np.array([loss(ob, c, a) for a in AMPS])

    fd1, fd4 = (L(eps) - L(-eps)) / (2 * eps), (L(eps / 4) - L(-eps / 4)) / (eps / 2)
    return list(zip(fd1, fd4))


def every_asserted_input():
    return [(t, n, d) for t in TABLES for n in TABLES[t] for d in DIRECTIONS[t]]


# ------------------------------------------------------------------ 1. symbols
def header():
    return open(os.path.join(ROOT, "include", "crbeam.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from continuum_robot import _native as nat
    from continuum_robot.batched import BeamEnsemble

    hdr, lib = header(), nat.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert re.search(rf"\bsize_t {WORK_BYTES}\s*\(", hdr) and lib.crb_implicit_adjoint_params_work_bytes.restype is C.c_size_t
    assert lib.crb_version() == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))
    assert hasattr(BeamEnsemble, "step_implicit_adjoint_params")
    assert "not the linear sum" not in hdr and "dK0/dtheta" in hdr


# ------------------------------------------------------------------ 2. refusals, before the device is touched
P = C.c_void_p
CK, LAM, WORK, PBAR, F, FBAR, HELD, REC = (P(64 * k) for k in range(1, 9))   # distinct fake device addresses (never read)
H = 1e-4


class Calls:
    """the two entry points on one host-only plan, with valid fake arguments unless overridden"""

    def __init__(self, dtype, n=4):
        from continuum_robot import _native as nat

        self.nat, self.lib = nat, nat.load()
        self.plan = nat.Plan(nitinol_columns(n, "nonlinear" if n < 100 else "linear"), n_beams=2, device=-1, dtype=dtype)

    def pgrad(self, bar=PBAR):
        g = self.nat.ParamCotangent()
        g.param_bar = bar.value if bar is not None else None
        return C.byref(g)

    PG = object()

    def plain(self, ck=CK, lam=LAM, n_cot=2, h=H, n=STEPS, n_iter=2, every=4, desc=None, rec=None, grad=None, pg=PG, work=WORK):
        pg = self.pgrad() if pg is Calls.PG else pg
        return self.lib.crb_step_implicit_adjoint_params(self.plan.h, ck, lam, n_cot, 0.0, h, n, n_iter, every, desc, rec, grad,
                                                         pg, work, None)

    def sched(self, ck=CK, lam=LAM, n_cot=2, h=H, n=STEPS, n_iter=2, every=4, desc=None, rec=None, grad=None, pg=PG, s=None,
              sched_bar=None, work=WORK):
        pg = self.pgrad() if pg is Calls.PG else pg
        return self.lib.crb_step_implicit_adjoint_params_sched(self.plan.h, ck, lam, n_cot, 0.0, h, n, n_iter, every, desc, rec,
                                                               grad, pg, s, sched_bar, work, None)

    def refused(self, rc, code, *words):
        msg = self.lib.crb_last_error().decode()
        assert rc == code, (rc, code, msg)
        for w in words:
            assert w in msg, (w, msg)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_in_order_before_the_device(dtype):
    c = Calls(dtype)
    nat, inval = c.nat, c.nat.CRB_EINVAL
    last = nat.CRB_ENODEV if dtype == "f64" else nat.CRB_EUNSUPPORTED
    last_word = "host-only" if dtype == "f64" else "fp64"
    for call, who in ((c.plain, NAMES[0]), (c.sched, NAMES[0])):   # (without a schedule the *_sched call is the plain one)
        # the parameter cotangent, then the work buffer, then aliasing, then the counts -- each next to every later fault
        c.refused(call(pg=None, work=None, n_cot=0), inval, who, "parameter cotangent")
        c.refused(call(pg=c.pgrad(None), work=None, n_cot=0), inval, who, "param_bar")
        c.refused(call(work=None, n_cot=0, every=0), inval, who, "null work buffer", WORK_BYTES)
        c.refused(call(pg=c.pgrad(LAM), n_cot=0), inval, who, "param_bar must not alias")
        c.refused(call(pg=c.pgrad(WORK), every=0), inval, who, "param_bar must not alias")
        c.refused(call(pg=c.pgrad(CK), n_iter=0), inval, who, "param_bar must not alias")
        c.refused(call(n_cot=0, every=0, n_iter=0), inval, who, "n_cot")
        c.refused(call(n_cot=65536), inval, who, "n_cot")
        c.refused(call(n=-1, every=0), inval, who, "n_steps")
        c.refused(call(every=0, n_iter=0), inval, who, "every")
        c.refused(call(n_iter=0, h=0.0), inval, who, "n_iter")
        c.refused(call(n_iter=17), inval, who, "n_iter")
        c.refused(call(h=0.0), inval, who, "h must")
        # what comes before them: the plain call's own pointers
        c.refused(call(ck=None, pg=None), inval, who, "null checkpoint")
        c.refused(call(lam=None, pg=None), inval, who, "null checkpoint")
        # then the checks of crb_step_implicit_adjoint, with its codes
        rec = nat.RecordDesc(0, 1, 1, 0, REC.value)    # every = 0
        c.refused(call(rec=C.byref(rec)), inval, who, "record")
        amp_only = nat.InputCotangent(HELD.value, None)
        c.refused(call(grad=C.byref(amp_only)), inval, who, "amp_bar")
        both = nat.InputCotangent(None, PBAR.value)
        c.refused(call(grad=C.byref(both)), inval, who, "alias")
        c.refused(call(), last, who, last_word)
        c.refused(call(n=0), last, who, last_word)
    # with a schedule: named by the *_sched entry point; param_bar against the schedule's buffers
    ok = C.byref(nat.InputSchedule(F.value, SCHED_K, SCHED_HOLD))
    c.refused(c.sched(s=ok, pg=None), inval, NAMES[1], "parameter cotangent")
    c.refused(c.sched(s=ok, work=None), inval, NAMES[1], WORK_BYTES)
    c.refused(c.sched(s=C.byref(nat.InputSchedule(F.value, 0, SCHED_HOLD))), inval, NAMES[1], "n_intervals")
    c.refused(c.sched(s=ok, sched_bar=FBAR, pg=c.pgrad(FBAR)), inval, NAMES[1], "param_bar must not alias")
    c.refused(c.sched(s=ok, pg=c.pgrad(F)), inval, NAMES[1], "param_bar must not alias")
    c.refused(c.sched(s=ok, sched_bar=FBAR), last, NAMES[1], last_word)
    c.refused(c.sched(sched_bar=FBAR), inval, NAMES[0], "sched_bar")
    # a NULL plan
    assert c.lib.crb_step_implicit_adjoint_params(None, CK, LAM, 1, 0.0, H, 3, 2, 4, None, None, None, c.pgrad(), WORK, None) == inval


def test_more_than_256_thread_carried_nodes_are_unsupported():
    c = Calls("f64", n=300)
    c.refused(c.plain(pg=None), c.nat.CRB_EINVAL, NAMES[0], "parameter cotangent")
    c.refused(c.plain(), c.nat.CRB_EUNSUPPORTED, NAMES[0], "256")


# ------------------------------------------------------------------ 3. the work buffer
@pytest.mark.parametrize("n,B", [(4, 1), (6, 3), (200, 5)])
def test_work_bytes_formula(n, B):
    from continuum_robot import _native as nat

    lib = nat.load()
    plan = nat.Plan(nitinol_columns(n, "linear"), n_beams=B, device=-1, dtype="f64")
    n_node = n + 1
    for every, n_iter, n_cot in ((1, 1, 1), (7, 2, 1), (7, 2, 3), (40, 3, 8), (3, 16, 2)):
        plain = lib.crb_implicit_adjoint_work_bytes(plan.h, every, n_iter, n_cot)
        assert plain == (every * ((2 + n_iter) * B * n_node * 4 + 1) + n_cot * B * n_node * 4) * 8
        assert lib.crb_implicit_adjoint_params_work_bytes(plan.h, every, n_iter, n_cot) == \
            plain + (every * n_iter * n_cot + 1) * B * n_node * 4 * 8
    for bad in ((0, 2, 1), (4, 0, 1), (4, 2, 0), (-1, 2, 1), (4, -1, 1), (4, 2, -1)):
        assert lib.crb_implicit_adjoint_params_work_bytes(plan.h, *bad) == 0
    assert lib.crb_implicit_adjoint_params_work_bytes(None, 4, 2, 1) == 0


# ------------------------------------------------------------------ 4. the inputs of the GPU file, on the oracle alone
@pytest.mark.parametrize("table,name,direction", every_asserted_input(), ids=lambda v: str(v))
def test_oracle_differences_agree_with_themselves(table, name, direction):
    """|FD(eps) - FD(eps / 4)| / |FD(eps / 4)| of the oracle alone, both amplitudes, at the step sizes of EPS, against
    SELF_BAR = 2.5e-7.  Measured, the worst per table and direction: every direction -- elastic_modulus 2.5e-8, moment_inertia
    2.5e-8, drag_coef 3.3e-8, fluid_density 4.2e-8, g_y 1.9e-8, g_x 9.8e-9; the iteration matrix -- moment_inertia 2.4e-8;
    mappings -- elastic_modulus 1.7e-7 (129 slots; 1.2e-7 on 33 and 256), fluid_density 8.2e-10, g_y 1.6e-9; schedule --
    elastic_modulus 2.2e-8, fluid_density 2.0e-10.  No case needed a step of its own (EPS_OF_CASE is empty) and none was
    dropped."""
    for b, (fd1, fd4) in enumerate(oracle_differences(table, name, direction)):
        assert np.isfinite(fd4) and fd4 != 0.0
        self_err = abs(fd1 - fd4) / abs(fd4)
        print(f"{TAG} {table} {name} amp {AMPS[b]} {direction}: FD(eps/4) {fd4:.12e} self {self_err:.2e}")
        assert self_err <= SELF_BAR, (table, name, direction, b, fd1, fd4, self_err)
