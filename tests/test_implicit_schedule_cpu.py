"""CPU side of the control schedule in the implicit stepper (crb_step_implicit_sched, crb_step_implicit_checkpoint_sched,
crb_step_implicit_adjoint_sched; tests/test_implicit_schedule.py holds the GPU side and imports the case table, the inputs
and the oracle's chained rollouts from here).

  * the three entry points are declared in include/crbeam.h, exported and bound;
  * every refusal shows on a host-only plan, in the documented order -- the counterpart's own CRB_EINVAL cases, the schedule's
    CRB_EINVAL cases, CRB_EUNSUPPORTED, CRB_ENODEV -- and names the entry point and the argument; with sched == NULL each
    call returns what its counterpart returns;
  * the inputs of the GPU file are proved on the oracle alone.  The CPU statement of a scheduled call is OracleBeam.implicit
    chained per interval with u_held = control[k] and the clock carried over (every call of it starts its first step's
    iteration from 0, which is the reset the kernels make at an interval's first step).  For every case the chained rollout is
    finite and the impulse window closes inside interval 1; for the gradient cases the oracle's two central differences
    agree to SELF_BAR per asserted DOF block along each asserted direction and the smaller step moves each block by at least
    RESOLVED ulps (the two conditions of tests/test_implicit_adjoint_mappings_cpu.py).

What was chosen on the oracle alone so that the conditions hold is written next to FD_CASES."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests.helpers import nitinol_columns, oracle_beam
from tests.test_control_schedule import ADJOINT_MAPPINGS
from tests.test_derivative_mappings import block_normalised, clock
from tests.test_tangent_linear import oracle_kw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_step_implicit_sched", "crb_step_implicit_checkpoint_sched", "crb_step_implicit_adjoint_sched")
TAG = "[implicit-schedule]"
P = C.c_void_p
X_, CK, LAM, WORK, F, FBAR, HELD, REC = (P(64 * k) for k in range(1, 9))   # distinct fake device addresses (never read)

B = 3
STEPS, K, HOLD = 33, 5, 7           # the last interval is cut to 5 steps
H = 1e-4
WINDOW = 12.3                       # the impulse window closes inside step 12: interval 1 holds steps 7 .. 13
WARM = 30                           # steps of the oracle's rollout from rest that gives the start state (5 at h = 1e-3)
SELF_BAR = 2.5e-7
RESOLVED = 4e7
BLOCKS = ("u", "w", "phi", "du_dt", "dw_dt", "dphi_dt")

# (mapping of tests/test_control_schedule.py, h, n_iter): every mapping at h = 1e-4 with n_iter 1 and 2 -- with one iteration
# the carried iterate is all that links two steps, so the reset is what is tested -- and the 256-slot rod also at h = 1e-3,
# the step that keeps all 8 levels of A
RUNS = [(name, H, n_iter) for name in ADJOINT_MAPPINGS for n_iter in (1, 2)] + [("four_waves_256", 1e-3, 1), ("four_waves_256", 1e-3, 2)]


def run_id(r):
    return f"{r[0]}-h{r[1]:g}-it{r[2]}"


# ------------------------------------------------------------------ the inputs, on the oracle alone
def beam_columns(name):
    cols, fps, _ = ADJOINT_MAPPINGS[name]
    many = isinstance(cols, list)
    return [(cols[b] if many else cols, fps[b] if many else fps) for b in range(B)]


@functools.lru_cache(maxsize=None)
def _oracle(name, b):
    cols, fp = beam_columns(name)[b]
    return oracle_beam(cols, **oracle_kw(bool(fp.enable_fluid_effects), bool(fp.enable_gravity_effects)))


def oracle(name, b):
    return _oracle(name, b if isinstance(ADJOINT_MAPPINGS[name][0], list) else 0)


class Inputs:
    """One mapping on the oracle alone, every beam: start states (the oracle's after a warm start from rest under the tip
    impulse: non-zero velocities), tip-impulse amplitudes, a random schedule that differs per beam -- transverse entries only on
    rods with nonlinear elements (the shipped f1 lets axial modes run away), nothing past a beam's own DOF count -- all padded
    to the longest beam's n as BeamEnsemble pads them.  ``load`` scales amplitudes and schedule."""

    def __init__(self, name, h, n_iter, load=1.0, n_intervals=K, seed=0):
        self.name, self.h, self.n_iter = name, h, n_iter
        self.obs = [oracle(name, b) for b in range(B)]
        self.nb = [ob.n for ob in self.obs]
        self.n = n = max(self.nb)
        self.fi = [ob.red2full() for ob in self.obs]
        self.rng = rng = np.random.default_rng(3000 + sum(map(ord, name)) + 7 * n_iter + seed)
        self.amps = load * np.linspace(0.1, 0.2, B)
        self.duration = WINDOW * h
        self.loaded = np.zeros((B, n), bool)
        for b in range(B):
            linear = all(str(t) == "linear" for t in beam_columns(name)[b][0]["type"])
            self.loaded[b, :self.nb[b]] = True if linear else (self.fi[b] % 3 == 1)
        self.sigma = 0.05 * load
        self.U = self.schedule(n_intervals)
        warm = 5 if h > 5e-4 else WARM
        self.X = self.pad([ob.implicit(np.zeros(2 * ob.n), h, warm, n_iter=n_iter, amp=self.amps[b], duration=10.0 * h)
                           for b, ob in enumerate(self.obs)])

    def schedule(self, n_intervals):
        return np.where(self.loaded[None], self.rng.normal(0.0, self.sigma, (n_intervals, B, self.n)), 0.0)

    def pad_row(self, b, x):
        """beam b's own reduced state [2 n_b] -> its padded row [2n]"""
        out, nb = np.zeros(2 * self.n), self.nb[b]
        out[:nb], out[self.n:self.n + nb] = x[:nb], x[nb:]
        return out

    def pad(self, states):
        """per-beam reduced states [2 n_b] -> [B, 2n]"""
        return np.stack([self.pad_row(b, x) for b, x in enumerate(states)])

    def own(self, b, x):
        """row b of a padded [B, 2n] state -> the beam's own [2 n_b]"""
        nb = self.nb[b]
        return np.concatenate([x[:nb], x[self.n:self.n + nb]])

    def chained(self, b, x0=None, U=None, amp=None, n_steps=STEPS, hold=HOLD, samples=False):
        """OracleBeam.implicit chained per interval on beam b from the padded start state: one call per interval with u_held =
        that interval's vector, the clock carried over by the stepper's additions.  Returns the beam's own final state [2 n_b];
        ``samples``: and the state after every step, [n_steps, 2 n_b] -- each interval re-run to every length (one-step calls
        cannot be chained inside an interval: every call resets the iterate)."""
        ob, nb = self.obs[b], self.nb[b]
        x = self.own(b, self.X[b] if x0 is None else x0)
        U = self.U if U is None else U
        amp = self.amps[b] if amp is None else amp
        t, left, k, rec = 0.0, n_steps, 0, []
        while left > 0:
            m = min(hold, left)
            kw = dict(n_iter=self.n_iter, amp=amp, duration=self.duration, t0=t, u_held=U[k, b, :nb])
            if samples:
                rec += [ob.implicit(x, self.h, j + 1, **kw) for j in range(m)]
            x = ob.implicit(x, self.h, m, **kw)
            t, left, k = clock(t, self.h, m), left - m, k + 1
        return (x, np.stack(rec)) if samples else x


@functools.lru_cache(maxsize=None)
def inputs(name, h, n_iter):
    return Inputs(name, h, n_iter)


# ------------------------------------------------------------------ 1. symbols
def header():
    return open(os.path.join(ROOT, "include", "crbeam.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from continuum_robot import _native as nat
    from continuum_robot.batched import BeamEnsemble

    hdr, lib = header(), nat.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.crb_version() == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))
    for method in (BeamEnsemble.step_implicit, BeamEnsemble.rollout_implicit):
        assert list(inspect.signature(method).parameters)[-2:] == ["control", "control_hold"], method.__name__
    # the header no longer lists schedules as uncovered, and states the reset
    tail = hdr[hdr.index("Adjoint of the implicit stepper"):]
    uncovered = tail[tail.index("Not covered:"):tail.index("size_t crb_implicit_adjoint_work_bytes")]
    assert "the damped variant" in uncovered and not re.search(r"rho_inf < 1\), control schedules", uncovered)
    assert "first step of EVERY interval" in tail


# ------------------------------------------------------------------ 2. refusals, before the device is touched
class Calls:
    """the three entry points and their counterparts on one host-only plan, with valid fake arguments unless overridden"""

    def __init__(self, dtype, n=4):
        from continuum_robot import _native as nat

        self.nat, self.lib = nat, nat.load()
        self.plan = nat.Plan(nitinol_columns(n, "nonlinear" if n < 100 else "linear"), n_beams=2, device=-1, dtype=dtype)
        self.t_end = C.c_double(-1.0)

    def sched(self, f=F.value, k=K, hold=HOLD):
        return self.nat.InputSchedule(f, k, hold)

    def step(self, s, x=X_, h=H, n=STEPS, n_iter=2, desc=None, rec=None):
        return self.lib.crb_step_implicit_sched(self.plan.h, x, 0.0, h, n, n_iter, desc, s, rec, C.byref(self.t_end), None)

    def step0(self, x=X_, h=H, n=STEPS, n_iter=2, desc=None, rec=None):
        return self.lib.crb_step_implicit(self.plan.h, x, 0.0, h, n, n_iter, desc, rec, C.byref(self.t_end), None)

    def ckpt(self, s, x=X_, ck=CK, h=H, n=STEPS, n_iter=2, every=4, desc=None, rec=None):
        return self.lib.crb_step_implicit_checkpoint_sched(self.plan.h, x, 0.0, h, n, n_iter, every, desc, s, rec, ck,
                                                           C.byref(self.t_end), None)

    def ckpt0(self, x=X_, ck=CK, h=H, n=STEPS, n_iter=2, every=4, desc=None, rec=None):
        return self.lib.crb_step_implicit_checkpoint(self.plan.h, x, 0.0, h, n, n_iter, every, desc, rec, ck,
                                                     C.byref(self.t_end), None)

    def adj(self, s, ck=CK, lam=LAM, n_cot=2, h=H, n=STEPS, n_iter=2, every=4, desc=None, rec=None, grad=None, sched_bar=FBAR,
            work=WORK):
        return self.lib.crb_step_implicit_adjoint_sched(self.plan.h, ck, lam, n_cot, 0.0, h, n, n_iter, every, desc, rec, grad,
                                                        s, sched_bar, work, None)

    def adj0(self, ck=CK, lam=LAM, n_cot=2, h=H, n=STEPS, n_iter=2, every=4, desc=None, rec=None, grad=None, work=WORK):
        return self.lib.crb_step_implicit_adjoint(self.plan.h, ck, lam, n_cot, 0.0, h, n, n_iter, every, desc, rec, grad, work,
                                                  None)

    def error(self):
        return self.lib.crb_last_error().decode()

    def refused(self, rc, code, *words):
        msg = self.error()
        assert rc == code, (rc, code, msg)
        for w in words:
            assert w in msg, (w, msg)
        assert self.t_end.value == -1.0          # (*t_end is written only by a call that is not refused)


def bad_record(nat):
    r = nat.RecordDesc(0, 1, 1, 0, REC.value)    # every = 0
    return C.byref(r)


def bad_input(nat):
    d = nat.InputDesc()
    d.kind = 77
    return C.byref(d)


def held_input(nat):
    d = nat.InputDesc()
    d.kind, d.f_held = nat.CRB_INPUT_NONE, HELD.value
    return C.byref(d)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_in_order_before_the_device(dtype):
    c = Calls(dtype)
    nat, inval = c.nat, c.nat.CRB_EINVAL
    ok = C.byref(c.sched())
    last = nat.CRB_ENODEV if dtype == "f64" else nat.CRB_EUNSUPPORTED
    last_word = "host-only" if dtype == "f64" else "fp64"
    bad_scheds = ((c.sched(f=None), "f_sched"), (c.sched(k=0), "n_intervals"), (c.sched(k=-3), "n_intervals"),
                  (c.sched(hold=0), "hold"), (c.sched(hold=-1), "hold"))
    for call, who in ((c.step, NAMES[0]), (c.ckpt, NAMES[1]), (c.adj, NAMES[2])):
        # 1. the counterpart's own CRB_EINVAL cases come first, also next to a bad schedule
        worst = C.byref(c.sched(f=None, k=0, hold=0))
        c.refused(call(worst, n=-1), inval, who, "n_steps")
        c.refused(call(worst, h=0.0), inval, who, "h must")
        c.refused(call(worst, n_iter=0), inval, who, "n_iter")
        c.refused(call(worst, rec=bad_record(nat)), inval, who, "record")
        c.refused(call(worst, desc=bad_input(nat)), inval, who, "input kind")
        # 2. the schedule's, in their order
        for bad, word in bad_scheds:
            c.refused(call(C.byref(bad)), inval, who, word)
        c.refused(call(worst), inval, who, "f_sched")
        c.refused(call(C.byref(c.sched(k=0, hold=0))), inval, who, "n_intervals")
        c.refused(call(ok, n=K * HOLD + 1), inval, who, "n_steps exceeds")
        c.refused(call(C.byref(c.sched(hold=0)), n=K * HOLD + 1), inval, who, "hold")
        c.refused(call(ok, desc=held_input(nat)), inval, who, "f_held")
        # 3. / 4. valid arguments: the last interval cut short, every interval in full, one interval
        c.refused(call(ok), last, who, last_word)
        c.refused(call(ok, n=K * HOLD), last, who, last_word)
        c.refused(call(C.byref(c.sched(k=1, hold=STEPS))), last, who, last_word)
    # the checkpoint pass and the adjoint: their own pointer and aliasing cases before the schedule's
    worst = C.byref(c.sched(f=None))
    c.refused(c.step(worst, x=None), inval, NAMES[0], "null")
    c.refused(c.ckpt(worst, x=None), inval, NAMES[1], "null")
    c.refused(c.ckpt(worst, ck=X_), inval, NAMES[1], "alias")
    c.refused(c.ckpt(worst, every=0), inval, NAMES[1], "every")
    c.refused(c.adj(worst, lam=None), inval, NAMES[2], "null")
    c.refused(c.adj(worst, work=None), inval, NAMES[2], "work")
    c.refused(c.adj(worst, work=LAM), inval, NAMES[2], "alias")
    c.refused(c.adj(worst, n_cot=0), inval, NAMES[2], "n_cot")
    c.refused(c.adj(worst, every=0), inval, NAMES[2], "every")
    amp_only = nat.InputCotangent(HELD.value, None)
    c.refused(c.adj(worst, grad=C.byref(amp_only)), inval, NAMES[2], "amp_bar")            # no impulse input
    # the adjoint's schedule cases: f_held_bar next to a schedule, sched_bar without one, sched_bar aliasing
    f_bar = nat.InputCotangent(None, HELD.value)
    c.refused(c.adj(ok, grad=C.byref(f_bar)), inval, NAMES[2], "f_held_bar")
    c.refused(c.adj(ok, desc=held_input(nat), grad=C.byref(f_bar)), inval, NAMES[2], "input->f_held")   # (f_held comes first)
    c.refused(c.adj(None, sched_bar=FBAR), inval, "crb_step_implicit_adjoint", "sched_bar")
    for alias in (LAM, WORK, CK, F):
        c.refused(c.adj(ok, sched_bar=alias), inval, NAMES[2], "sched_bar")
    c.refused(c.adj(ok, grad=C.byref(f_bar), sched_bar=LAM), inval, NAMES[2], "f_held_bar")              # (the earlier case)
    c.refused(c.adj(ok, sched_bar=None), last, NAMES[2], last_word)                                      # (not wanted)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_without_a_schedule_each_call_is_its_counterpart(dtype):
    """sched == NULL (and sched_bar == NULL): the same code and the same message as the existing entry point, refusal by
    refusal"""
    c = Calls(dtype)
    nat = c.nat
    amp_only = nat.InputCotangent(HELD.value, None)
    f_bar = nat.InputCotangent(None, WORK.value)
    cases = {
        "step": (lambda **kw: c.step(None, **kw), c.step0,
                 [dict(), dict(x=None), dict(n=-1), dict(h=0.0), dict(h=float("nan")), dict(n_iter=0), dict(rec=bad_record(nat)),
                  dict(desc=bad_input(nat)), dict(desc=held_input(nat)), dict(n=0)]),
        "checkpoint": (lambda **kw: c.ckpt(None, **kw), c.ckpt0,
                       [dict(), dict(x=None), dict(ck=None), dict(ck=X_), dict(n=-1), dict(every=0), dict(n_iter=0), dict(n_iter=17),
                        dict(h=0.0), dict(rec=bad_record(nat)), dict(desc=bad_input(nat)), dict(desc=held_input(nat)), dict(n=0)]),
        "adjoint": (lambda **kw: c.adj(None, sched_bar=None, **kw), c.adj0,
                    [dict(), dict(ck=None), dict(lam=None), dict(work=None), dict(work=LAM), dict(ck=LAM), dict(work=CK),
                     dict(grad=C.byref(f_bar)), dict(n_cot=0), dict(n_cot=65536), dict(n=-1), dict(every=0), dict(n_iter=0),
                     dict(n_iter=17), dict(h=0.0), dict(rec=bad_record(nat)), dict(desc=bad_input(nat)),
                     dict(grad=C.byref(amp_only)), dict(desc=held_input(nat)), dict(n=0)]),
    }
    for what, (new, old, kws) in cases.items():
        for kw in kws:
            c.t_end.value = -1.0
            want = (old(**kw), c.error(), c.t_end.value)
            c.t_end.value = -1.0
            got = (new(**kw), c.error(), c.t_end.value)
            assert got == want, (what, kw, got, want)
            assert want[0] != nat.CRB_OK, (what, kw)        # (a host-only plan: even a valid call is refused)
    # a NULL plan
    for name in NAMES:
        old = getattr(c.lib, name[:-len("_sched")])
        args_new = {NAMES[0]: (None, X_, 0.0, H, 3, 2, None, None, None, None, None),
                    NAMES[1]: (None, X_, 0.0, H, 3, 2, 4, None, None, None, CK, None, None),
                    NAMES[2]: (None, CK, LAM, 1, 0.0, H, 3, 2, 4, None, None, None, None, None, WORK, None)}[name]
        args_old = {NAMES[0]: (None, X_, 0.0, H, 3, 2, None, None, None, None),
                    NAMES[1]: (None, X_, 0.0, H, 3, 2, 4, None, None, CK, None, None),
                    NAMES[2]: (None, CK, LAM, 1, 0.0, H, 3, 2, 4, None, None, None, WORK, None)}[name]
        want = (old(*args_old), c.error())
        assert (getattr(c.lib, name)(*args_new), c.error()) == want and want[0] == nat.CRB_EINVAL, name
    ok = C.byref(c.sched())
    assert c.lib.crb_step_implicit_sched(None, X_, 0.0, H, 3, 2, None, ok, None, None, None) == nat.CRB_EINVAL
    assert NAMES[0] in c.error() and "null plan" in c.error()


def test_more_than_256_thread_carried_nodes_are_unsupported_before_the_device():
    c = Calls("f64", n=300)
    ok = C.byref(c.sched())
    for call, who in ((c.step, NAMES[0]), (c.ckpt, NAMES[1]), (c.adj, NAMES[2])):
        c.refused(call(C.byref(c.sched(hold=0))), c.nat.CRB_EINVAL, who, "hold")      # (CRB_EINVAL still comes first)
        c.refused(call(ok), c.nat.CRB_EUNSUPPORTED, who, "256")


# ------------------------------------------------------------------ 3. the inputs of the GPU file, on the oracle alone
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_chained_oracle_rollouts_are_finite_and_the_window_closes_inside_interval_1(run):
    i = inputs(*run)
    h = i.h
    assert STEPS <= K * HOLD and STEPS > (K - 1) * HOLD and STEPS % HOLD != 0            # the last interval is reached and cut
    on = [clock(0.0, h, s) + 0.5 * h < i.duration for s in range(STEPS)]
    assert on == [s < 12 for s in range(STEPS)] and HOLD <= 12 < 2 * HOLD                 # the last forced midpoint: step 11
    for b in range(B):
        assert np.all(np.isfinite(i.X[b])) and np.max(np.abs(i.X[b, i.n:])) > 0.0        # non-zero velocities
        x = i.chained(b)
        assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0.0, (run, b)
        assert np.all(i.U[:, b, i.nb[b]:] == 0.0) and np.max(np.abs(i.U[:, b])) > 0.0
        # the schedule drives the result, and each beam has its own
        assert not np.array_equal(x, i.chained(b, U=np.broadcast_to(i.U[:1], i.U.shape)))
    assert not np.array_equal(i.U[:, 0, :i.nb[0]], i.U[:, 1, :i.nb[0]])


# ---- the gradient cases: control_bar against the chained oracle's central differences, per DOF block of the final state.
# Chosen on the oracle alone, before any kernel was compared:
#   * loads x ``load`` (x 50: impulses of 5 .. 10 N, a schedule of 0.5 N per node, as tests/test_implicit_adjoint_mappings_cpu.py):
#     the axial blocks answer a transverse force only through the deflection, and at the 0.05 N of the bitwise cases their
#     response sits at the differences' rounding.  x 10 on the 256-slot rod at h = 1e-3: at x 50 its third beam is not finite
#     after the 33 steps, at x 20 self reaches 1.8e-7;
#   * the cotangent of block k is the block-normalised oracle tangent along the direction, restricted to that block: the
#     scalar <lam_k, dx(T)/de> sums squares, without cancellation;
#   * e: the difference step along the (0.5 N) directions, per case.
FD_CASES = {
    "packed_6": dict(h=1e-4, n_iter=2, e=1e-3, load=50.0),
    "two_waves_65": dict(h=1e-4, n_iter=1, e=1e-3, load=50.0),
    "four_waves_256": dict(h=1e-3, n_iter=2, e=3e-4, load=10.0),      # all 8 levels of A
}
FD_INTERVAL = 2                     # the interval that carries the one-interval direction (fully inside the run, after the window)


class FdInputs(Inputs):
    """A gradient case: the inputs at the case's load, two directions of the schedule per beam (dense; on FD_INTERVAL alone), and per
    direction and DOF block the cotangent and the chained oracle's two central differences of <cotangent, x(T)>"""

    def __init__(self, name):
        c = FD_CASES[name]
        super().__init__(name, c["h"], c["n_iter"], load=c["load"])
        self.e = c["e"]
        dense = self.schedule(K)
        single = np.zeros_like(dense)
        single[FD_INTERVAL] = self.schedule(1)[0]
        self.dirs = [("dense", dense), (f"interval {FD_INTERVAL} only", single)]
        self._memo = {}

    def moved(self, b, k, e):
        key = (b, k, e)
        if key not in self._memo:
            self._memo[key] = self.chained(b, U=self.U + e * self.dirs[k][1])
        return self._memo[key]

    def differences(self, b, k):
        """(FD(e), FD(e / 4)) of beam b's final state along direction k"""
        return tuple((self.moved(b, k, s) - self.moved(b, k, -s)) / (2 * s) for s in (self.e, self.e / 4))

    def block_sel(self, b, blk):
        dof = np.concatenate([self.fi[b] % 3, 3 + self.fi[b] % 3])
        return np.flatnonzero(dof == blk)

    def cotangents(self, b, k):
        """[6, 2 n_b]: row blk = the block-normalised tangent FD(e / 4) on block blk, zero elsewhere"""
        t = block_normalised(self.differences(b, k)[1], self.fi[b])
        out = np.zeros((6, t.size))
        for blk in range(6):
            sel = self.block_sel(b, blk)
            out[blk, sel] = t[sel]
        return out

    def figures(self, b, k, blk, g=None):
        """fd_scalar's figures for block blk: (err of the gradient figure g or None, allowed, self, fd4)"""
        lam = self.cotangents(b, k)[blk]
        fd1, fd4 = (float(lam @ d) for d in self.differences(b, k))
        self_err = abs(fd1 - fd4) / abs(fd4)
        return (None if g is None else abs(g - fd4) / abs(fd4)), min(max(1e-7, 4 * self_err), 1e-6), self_err, fd4

    def loss(self, b, k, blk):
        """L(e) for tests.test_adjoint.fd_scalar"""
        lam = self.cotangents(b, k)[blk]
        return lambda e: float(lam @ self.moved(b, k, e))


@functools.lru_cache(maxsize=None)
def fd_inputs(name):
    return FdInputs(name)


@pytest.mark.parametrize("name", list(FD_CASES))
def test_oracle_differences_agree_along_the_schedule_directions(name):
    i = fd_inputs(name)
    assert 0 < FD_INTERVAL < K - 1 and FD_INTERVAL * HOLD > 12
    worst, least = 0.0, np.inf
    for b in range(B):
        assert np.all(np.isfinite(i.chained(b)))
        for k, (label, v) in enumerate(i.dirs):
            assert np.max(np.abs(v[:, b])) > 0.0
            hi, lo = i.moved(b, k, i.e / 4), i.moved(b, k, -i.e / 4)
            for blk in range(6):
                sel = i.block_sel(b, blk)
                if sel.size == 0:
                    continue
                _, _, s, fd4 = i.figures(b, k, blk)
                assert fd4 > 0.0, (name, b, label, BLOCKS[blk])
                assert s <= SELF_BAR, (name, b, label, BLOCKS[blk], s)
                moved, size = np.max(np.abs(hi[sel] - lo[sel])), np.max(np.abs(hi[sel]))
                assert moved >= RESOLVED * np.finfo(np.float64).eps * size, (name, b, label, BLOCKS[blk], moved / size)
                worst, least = max(worst, s), min(least, moved / size)
    print(f"{TAG} {name} | oracle differences | worst self {worst:.2e} | least moved {least:.1e} of its block")


# ------------------------------------------------------------------ 4. Python argument checks that need no device
@pytest.mark.parametrize("kw, word", [
    (dict(control=[[[0.0] * 12] * 2] * 5, control_hold=7, held_force=[[0.0] * 12] * 2), "held_force"),
    (dict(control=[[[0.0] * 12] * 2] * 5), "implicit steps per interval"),
    (dict(control_hold=7), "control_hold needs control"),
    (dict(control=[[0.0] * 12] * 2, control_hold=7), "control must be"),
    (dict(control=[[[0.0] * 12] * 2] * 4, control_hold=7), "n_steps"),
])
def test_python_argument_checks_need_no_device(kw, word):
    import torch

    from continuum_robot.batched import BeamEnsemble

    ens = BeamEnsemble.__new__(BeamEnsemble)
    ens.dtype, ens.device, ens.n_beams, ens.n = torch.float64, torch.device("cpu"), 2, 12
    with pytest.raises(ValueError, match=word):
        ens._control(kw.get("held_force"), kw.get("control"), kw.get("control_hold"), 33, "step_implicit", "implicit steps")
