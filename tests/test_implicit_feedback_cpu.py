"""CPU side of the sampled-data state feedback inside the implicit stepper (crb_step_implicit_feedback; the GPU side is
tests/test_implicit_feedback.py, which imports the case table, the inputs and the oracle's chain from here).

  * the three entry points are declared in include/crbeam.h, exported and bound, and CRB_VERSION stays 106;
  * every refusal shows on a host-only plan in the documented order and names the entry point;
  * the Python argument errors need no device;
  * the reference of the GPU file is proved on the oracle alone.  The CPU statement of the call is OracleBeam.implicit chained
    per sample with u_held = f_held + K (r - x_k), x_k the state as it stands at the sample, the clock carried over (every call
    of it starts its first step's iteration from 0: the reset the kernel makes at a sample's first step).  For every case the
    chain stays finite, differs from the open loop (K = 0) by far more than the GPU bound, and perturbing every u_k by its
    rounding bound -- (2n + 2) 2^-53 (|f_held| + |K| |r - x_k|), the any-order summation bound of the 2n-term product plus the
    subtraction and the addition around it -- moves no DOF block of the final state by a tenth of the 1e-7 the GPU file
    allows: that bound has margin whatever order the device sums in.

The gain: a dense seeded normal [n, 2n] matrix plus a velocity-damping diagonal, both scaled from the sampled plant's own
compliance (gain_scales) so that the zero-order-hold loop contracts.  The scale is computed, and what it was computed for is
asserted."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests.helpers import block_errs, nitinol_columns, oracle_beam
from tests.test_control_schedule import MAPPINGS
from tests.test_tangent_linear import force_params, oracle_kw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_step_implicit_feedback", "crb_implicit_feedback_work_bytes", "crb_implicit_feedback_path")
WHO = NAMES[0]
P = C.c_void_p
X_, GAIN, REF, WORK, UOUT, HELD, REC = (P(64 * k) for k in range(1, 8))   # distinct fake device addresses (never read)

B = 3
H, N_ITER, HOLD, STEPS = 1e-4, 2, 4, 22      # six samples, the last one cut to 2 steps
N_SAMPLES = -(-STEPS // HOLD)
WINDOW = 9.3                                 # the impulse window closes inside step 9: sample 2 holds steps 8 .. 11
WARM = 30                                    # steps of the oracle's rollout from rest that gives the start state
FORCE = 0.05                                 # N: the held forces of the suite (tests/test_control_schedule.py: sigma)
GPU_BOUND = 1e-7                             # per DOF block, the suite's forward bound (tests/test_implicit_adjoint_mappings.py)
EPS = 2.0 ** -53

# name -> (columns, ForceParams, (n_slots, threads, packed) of the plan), in_kernel: the smallest shapes at which each path of
# the call can go wrong
CASES = {
    "general_3": (MAPPINGS["general_3"], True),                  # fewer than 5 slots
    "packed_6": (MAPPINGS["packed_6"], True),                    # several beams per wave, a ragged last group, LDS product
    "packed_10": ((nitinol_columns(10, "nonlinear"), force_params(True, False), (10, 64, True)), True),   # n = 30: matrix cores
    "pinned_gravity_16": (MAPPINGS["pinned_gravity_16"], True),  # a root DOF without a reduced index, 17 slots, gravity
    "packed_30": ((nitinol_columns(30, "linear"), force_params(True, False), (30, 64, True)), True),      # largest gain in LDS
    "one_wave_33": (MAPPINGS["one_wave_33"], False),             # first gain that leaves LDS
    "two_waves_65": (MAPPINGS["two_waves_65"], False),
    "four_waves_256": (MAPPINGS["four_waves_256"], False),
}
IN_KERNEL = [name for name, (_, fused) in CASES.items() if fused]


def clock(t, h, k):
    for _ in range(k):
        t = t + h
    return t


@functools.lru_cache(maxsize=None)
def oracle(name):
    cols, fp, _ = CASES[name][0]
    return oracle_beam(cols, **oracle_kw(bool(fp.enable_fluid_effects), bool(fp.enable_gravity_effects)))


LOOP = 0.2                                   # loop gain per sample of each part of the gain on the plant's most compliant DOF


def sample_response(ob, h, hold, n_iter):
    """s / kg: the largest rate change of a tip DOF (u, w, phi of the free end: the least inertia of the rod) one sample after
    a unit force on that DOF is switched on at rest -- the largest diagonal entry of the rate rows of the sampled plant's B_d"""
    n, rest = ob.n, np.zeros(2 * ob.n)
    base = ob.implicit(rest, h, hold, n_iter=n_iter, amp=0.0)               # (gravity alone)
    out = []
    for i in (n - 3, n - 2, n - 1):
        e = np.zeros(n)
        e[i] = 1.0
        out.append(abs(ob.implicit(rest, h, hold, n_iter=n_iter, amp=0.0, u_held=e)[n + i] - base[n + i]))
    return max(out)


def gain_scales(resp, n):
    """(scale of the dense normal [n, 2n] part, velocity-damping coefficient).  A zero-order-hold rate feedback d on a DOF whose
    rate answers a unit force with `resp` per sample multiplies that rate by 1 - d resp per sample: d = LOOP / resp keeps the
    factor at 1 - LOOP on the most compliant DOF and nearer 1 on every other.  The dense part is held to the same loop gain
    through its 2-norm, sqrt(n) + sqrt(2n) in expectation for normal entries.  (Scaling both to a fixed FORCE instead gives
    d resp = 7 on the tip rotation of the 0.25 m elements at hold = 4, h = 1e-4: the sampled loop is unstable whatever the
    stepper, the oracle's chain overflows within the 22 steps.)"""
    return LOOP / (resp * (np.sqrt(n) + np.sqrt(2 * n))), LOOP / resp


class Inputs:
    """One case on the oracle alone: start states (the oracle's after a warm start from rest under the tip impulse), impulse
    amplitudes, a held force (transverse entries only on rods with nonlinear elements: the shipped f1 lets axially loaded
    modes run away), a nonzero reference and the gain."""

    def __init__(self, name, h=H, n_iter=N_ITER):
        self.name, self.h, self.n_iter = name, h, n_iter
        self.ob = ob = oracle(name)
        self.n = n = ob.n
        self.fi = ob.red2full()
        rng = np.random.default_rng(5000 + sum(map(ord, name)))
        self.amps = np.linspace(0.1, 0.2, B)
        self.duration = WINDOW * h
        linear = all(str(t) == "linear" for t in CASES[name][0][0]["type"])
        loaded = np.ones(n, bool) if linear else (self.fi % 3 == 1)
        self.f_held = np.where(loaded[None], rng.normal(0.0, FORCE, (B, n)), 0.0)
        self.X = np.stack([ob.implicit(np.zeros(2 * n), h, WARM, n_iter=n_iter, amp=a, duration=10.0 * h) for a in self.amps])
        self.R = 0.3 * np.roll(self.X, 1, axis=0)                # another beam's state, scaled: nonzero, of the state's size
        # the gain: dense normal entries plus a velocity-damping diagonal (u_i += d (r_v - v)_i), both scaled from the sampled
        # plant's own compliance so that the zero-order-hold loop stays a contraction (see gain_scales)
        self.G = rng.normal(0.0, 1.0, (n, 2 * n))
        self.resp = sample_response(ob, h, HOLD, n_iter)
        self.scale, self.damp = gain_scales(self.resp, n)
        self.K = self.scale * self.G
        self.K[np.arange(n), n + np.arange(n)] += self.damp

    def control(self, b, x, K=None):
        return self.f_held[b] + (self.K if K is None else K) @ (self.R[b] - x)

    def bound(self, b, x):
        """the rounding bound of u_k, elementwise: any-order summation of the 2n products, the subtraction, the addition"""
        return (2 * self.n + 2) * EPS * (np.abs(self.f_held[b]) + np.abs(self.K) @ np.abs(self.R[b] - x))

    def chain(self, b, K=None, n_steps=STEPS, hold=HOLD, perturb=None, x0=None):
        """OracleBeam.implicit chained per sample on beam b: (final state [2n], controls [samples, n], the states x_k the
        samples were taken at [samples, 2n]).  ``perturb`` [samples, n]: signs (or any factors) of the rounding bound added to
        every u_k."""
        x = (self.X[b] if x0 is None else x0).copy()
        t, left, k, U, XK = 0.0, n_steps, 0, [], []
        while left > 0:
            m = min(hold, left)
            u = self.control(b, x, K)
            if perturb is not None:
                u = u + perturb[k] * self.bound(b, x)
            U.append(u)
            XK.append(x.copy())
            x = self.ob.implicit(x, self.h, m, n_iter=self.n_iter, amp=self.amps[b], duration=self.duration, t0=t, u_held=u)
            t, left, k = clock(t, self.h, m), left - m, k + 1
        return x, np.array(U).reshape(-1, self.n), np.array(XK).reshape(-1, 2 * self.n)


@functools.lru_cache(maxsize=None)
def inputs(name):
    return Inputs(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's chain of every beam of a case: (final states [B, 2n], controls [samples, B, n])"""
    inp = inputs(name)
    out = [inp.chain(b) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out], axis=1)


# ------------------------------------------------------------------ 1. symbols
def header():
    return open(os.path.join(ROOT, "include", "crbeam.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from continuum_robot import _native as nat
    from continuum_robot.batched import BeamEnsemble

    hdr, lib = header(), nat.load()
    for name, ret in zip(NAMES, ("int", "size_t", "int")):
        assert re.search(rf"\b{ret} {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.crb_implicit_feedback_work_bytes.restype is C.c_size_t
    assert lib.crb_version() == 106 == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))
    sig = inspect.signature(BeamEnsemble.step_implicit_feedback).parameters
    assert list(sig)[1:] == ["n_steps", "h", "gain", "reference", "hold", "n_iter", "impulse_amp", "impulse_duration",
                             "impulse_index", "held_force", "t0", "record", "record_every", "return_control"]
    assert (sig["hold"].default, sig["n_iter"].default, sig["return_control"].default) == (1, 2, False)
    assert callable(BeamEnsemble.implicit_feedback_path)


# ------------------------------------------------------------------ 2. refusals, before the device is touched
class Calls:
    def __init__(self, dtype, cols=None):
        from continuum_robot import _native as nat

        self.nat, self.lib = nat, nat.load()
        self.plan = nat.Plan(nitinol_columns(4, "nonlinear") if cols is None else cols, n_beams=2, device=-1, dtype=dtype)
        self.t_end = C.c_double(-1.0)

    def step(self, x=X_, h=H, n=STEPS, n_iter=2, hold=HOLD, gain=GAIN, ref=REF, desc=None, rec=None, u_out=UOUT, work=WORK, plan=True):
        return self.lib.crb_step_implicit_feedback(self.plan.h if plan else None, x, 0.0, h, n, n_iter, hold, gain, ref, desc, rec,
                                                   u_out, work, C.byref(self.t_end), None)

    def refused(self, rc, code, *words):
        msg = self.lib.crb_last_error().decode()
        assert rc == code, (rc, code, msg)
        for w in (WHO,) + words:
            assert w in msg, (w, msg)
        assert self.t_end.value == -1.0          # (*t_end is written only by a call that is not refused)


def record(nat, every):
    return C.byref(nat.RecordDesc(0, 1, 1, every, REC.value))


def bad_input(nat):
    d = nat.InputDesc()
    d.kind = 77
    return C.byref(d)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_in_order_before_the_device(dtype):
    c = Calls(dtype)
    nat, inval = c.nat, c.nat.CRB_EINVAL
    last = (nat.CRB_ENODEV, "host-only") if dtype == "f64" else (nat.CRB_EUNSUPPORTED, "fp64")
    # 1. CRB_EINVAL, each case next to every later one
    c.refused(c.step(plan=False, x=None, n=-1), inval, "null plan")
    worse = dict(n=-1, h=0.0, n_iter=0, hold=0, rec=record(nat, 0), desc=bad_input(nat))
    for kw in (dict(x=None), dict(gain=None), dict(work=None)):
        c.refused(c.step(**{**worse, **kw}), inval, "null pointer")
    order = [("n", -1, "n_steps"), ("h", 0.0, "h must"), ("n_iter", 0, "n_iter"), ("hold", 0, "hold must"),
             ("rec", record(nat, 0), "record"), ("desc", bad_input(nat), "input kind")]
    for i, (key, value, word) in enumerate(order):
        later = {k: v for k, v, _ in order[i + 1:]}
        c.refused(c.step(**{**later, key: value}), inval, word)
    c.refused(c.step(h=float("nan")), inval, "h must")
    c.refused(c.step(hold=-2), inval, "hold must")
    # the record stride: a divisor or a multiple of hold, nothing else -- before the input description is looked at
    for every in (3, 6, 5):
        c.refused(c.step(rec=record(nat, every), desc=bad_input(nat)), inval, "record stride")
    for every in (1, 2, 4, 8, 12):
        c.refused(c.step(rec=record(nat, every), desc=bad_input(nat)), inval, "input kind")
    # 2. / 3. valid arguments: CRB_EUNSUPPORTED for fp32, else CRB_ENODEV -- also without reference, record and u_out
    c.refused(c.step(), *last)
    c.refused(c.step(ref=None, u_out=None), *last)
    c.refused(c.step(rec=record(nat, 2), n=0), *last)
    c.refused(c.step(hold=STEPS + 1), *last)


def test_unsupported_plans_are_refused_before_the_device():
    from continuum_robot import _native as nat

    big = Calls("f64", nitinol_columns(300, "linear"))
    big.refused(big.step(), nat.CRB_EUNSUPPORTED, "256")
    big.refused(big.step(hold=0), nat.CRB_EINVAL, "hold must")              # (CRB_EINVAL comes first)
    # (a plan of mixed topology has no host-only form: its refusal is in the GPU file)
    big32 = Calls("f32", nitinol_columns(300, "linear"))
    big32.refused(big32.step(), nat.CRB_EUNSUPPORTED, "fp64")                # (the dtype is looked at first)
    lib = nat.load()
    assert lib.crb_implicit_feedback_path(None) == 0 and lib.crb_implicit_feedback_work_bytes(None) == 0
    small = Calls("f64")
    assert lib.crb_implicit_feedback_work_bytes(small.plan.h) == 2 * small.plan.n_node * 4 * 8
    assert lib.crb_implicit_feedback_path(big.plan.h) == 0


# ------------------------------------------------------------------ 3. Python argument errors
@pytest.mark.parametrize("kw, error, word", [
    (dict(gain=np.zeros((12, 24)), hold=0), ValueError, "hold must be"),
    (dict(gain=np.zeros((12, 24)), hold=1.5), ValueError, "hold must be"),
    (dict(gain=np.zeros((11, 24))), ValueError, "gain must be"),
    (dict(gain=np.zeros((24, 12))), ValueError, "gain must be"),
    (dict(gain=np.zeros((12, 24)), reference=[[0.0] * 24] * 3), ValueError, "reference must be"),
    (dict(gain=np.zeros((12, 24)), reference=[0.0] * 24), ValueError, "reference must be"),
])
def test_python_argument_checks_need_no_device(kw, error, word):
    import torch

    from continuum_robot.batched import BeamEnsemble

    ens = BeamEnsemble.__new__(BeamEnsemble)
    ens.dtype, ens.device, ens.n_beams, ens.n = torch.float64, torch.device("cpu"), 2, 12
    with pytest.raises(error, match=word):
        ens.step_implicit_feedback(STEPS, H, **kw)
    with pytest.raises(NotImplementedError, match="list of gains"):
        ens.step_implicit_feedback(STEPS, H, [np.zeros((12, 24))] * 2)
    with pytest.raises(NotImplementedError, match="list of gains"):
        ens.step_implicit_feedback(STEPS, H, (None, np.zeros((12, 24))), hold=0)


# ------------------------------------------------------------------ 4. / 5. the reference and the gain, on the oracle alone
@pytest.mark.parametrize("name", list(CASES))
def test_gain_scale_is_what_it_was_computed_for(name):
    inp = inputs(name)
    n, e0 = inp.n, inp.R - inp.X
    assert inp.K.shape == (n, 2 * n) and np.all(inp.K != 0.0)                               # dense
    assert inp.resp > 0.0 and inp.damp * inp.resp == pytest.approx(LOOP, rel=1e-12)
    assert inp.scale * inp.resp * (np.sqrt(n) + np.sqrt(2 * n)) == pytest.approx(LOOP, rel=1e-12)
    assert np.linalg.norm(inp.scale * inp.G, 2) * inp.resp <= 1.1 * LOOP                    # (the 2-norm is what was expected)
    assert np.array_equal(inp.K[np.arange(n), n + np.arange(n)], inp.scale * inp.G[np.arange(n), n + np.arange(n)] + inp.damp)
    assert np.max(np.abs(e0 @ inp.K.T)) > 0.0
    assert np.any(inp.R != 0.0) and np.any(inp.f_held != 0.0)
    # the impulse window closes inside a sample: the first step whose midpoint lies outside it is not a sample's first
    first_off = min(k for k in range(STEPS) if not clock(0.0, H, k) + 0.5 * H < inp.duration)
    assert 0 < first_off < STEPS and first_off % HOLD != 0


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_chain_is_finite_driven_by_the_gain_and_insensitive_to_the_products_rounding(name):
    inp = inputs(name)
    ref, U = reference(name)
    assert U.shape == (N_SAMPLES, B, inp.n) and np.all(np.isfinite(ref)) and np.all(np.isfinite(U))
    rng = np.random.default_rng(11)
    for b in range(B):
        open_loop, U0, _ = inp.chain(b, K=np.zeros_like(inp.K))
        assert np.array_equal(U0, np.broadcast_to(inp.f_held[b], U0.shape))
        moved = block_errs(ref[b], open_loop, inp.fi)
        assert max(moved.values()) > 1e3 * GPU_BOUND, (name, b, moved)          # the feedback is what drives the result
        assert np.all(np.any(U[:, b] != inp.f_held[b], axis=1))
        worst = {}
        for trial in range(2):   # random signs, then every entry pushed the same way
            signs = rng.choice([-1.0, 1.0], size=(N_SAMPLES, inp.n)) if trial == 0 else np.ones((N_SAMPLES, inp.n))
            got, _, _ = inp.chain(b, perturb=signs)
            for k, e in block_errs(got, ref[b], inp.fi).items():
                worst[k] = max(worst.get(k, 0.0), e)
        assert max(worst.values()) < 0.1 * GPU_BOUND, (name, b, worst)
