"""CPU side of the adjoint of the sampled-data implicit loop (crb_step_implicit_feedback_checkpoint / _adjoint,
BeamEnsemble.step_implicit_feedback_adjoint / rollout_implicit_feedback; the GPU side is
tests/test_implicit_feedback_adjoint.py, which imports the directions and the oracle's losses from here).

  * the three entry points are declared in include/crbeam.h, exported and bound, and CRB_VERSION stays 106;
  * every refusal shows on a host-only plan in the documented order and names the entry point;
  * the work-buffer size follows the header's formula;
  * the Python argument errors need no device;
  * the finite-difference reference of the GPU file is proved on the oracle alone: for every case of
    tests/test_implicit_feedback_cpu.py (B = 3, h = 1e-4, n_iter = 2, hold = 4, 22 steps: six samples, the last cut to 2
    steps; the impulse window closes inside step 9; a nonzero reference and a held force) and the loss L = x_T[tip w] of
    beam 0 over Inputs.chain, central differences at relative step 1e-3 along a gain, a reference, a start-state, a
    held-force and an amplitude direction agree with those at a quarter of the step so closely that fd_scalar's allowance,
    max(1e-7, 4 |fd1 - fd4| / |fd4|), sits at its floor -- and every derivative is nonzero.

The losses are evaluated once per (case, direction, step) and kept (loss_at): the GPU file reads the same table."""
import copy
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests.helpers import nitinol_columns
from tests.test_implicit_feedback_cpu import B, CASES, FORCE, H, HOLD, N_ITER, N_SAMPLES, STEPS, inputs
from tests.test_tangent_linear import directions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_implicit_feedback_adjoint_work_bytes", "crb_step_implicit_feedback_checkpoint", "crb_step_implicit_feedback_adjoint")
PASS, ADJ = NAMES[1], NAMES[2]
P = C.c_void_p
X_, GAIN, REF, WORK, CKPT, UCK, LAM, HELD, REC, GBAR, RBAR, ABAR, FBAR, AMP = (P(64 * k) for k in range(1, 15))   # never read

FD_STEP = 1e-3                               # relative step of the central differences (1e-2: packed_6 reaches 6.3e-7)
FD_FLOOR = 1e-7                              # the floor of fd_scalar's allowance
DIRECTIONS = ("gain", "reference", "x0", "held", "amp")
# a second start-state direction, of the size of each DOF block's maximum at EVERY node (tests.test_tangent_linear.directions):
# it weighs the root nodes as heavily as the tip.  Its differences do not reach the floor (pinned_gravity_16: 4.9e-7), so it is
# held to fd_scalar's rule with its 1e-6 cap, not to the floor (test_block_sized_start_state_direction_...).
X0_BLOCKS = "x0_blocks"
BEAM_WEIGHTS = np.array([1.0, -0.5, 0.75])                      # of x_T[tip w] in the GPU file's loss
SAMPLE_WEIGHTS = np.array([0.5, -1.0, 2.0, 0.25, -0.75])        # of the tip samples after steps 4, 8, ..., 20 (record_every = hold)


# ------------------------------------------------------------------ the oracle's losses and their differences
@functools.lru_cache(maxsize=None)
def direction(name, which):
    """the seeded direction of one input of a case, sized like the input itself"""
    inp = inputs(name)
    rng = np.random.default_rng(7000 + sum(map(ord, name)) + (DIRECTIONS + (X0_BLOCKS,)).index(which))
    if which == X0_BLOCKS:
        return directions(inp.X, rng, 1, inp.fi)[0]
    if which == "gain":
        return inp.scale * rng.normal(0.0, 1.0, (inp.n, 2 * inp.n))
    if which == "reference":
        return 0.3 * directions(inp.X, rng, 1, inp.fi)[0]
    if which == "x0":
        # every entry moved relative to ITSELF: a relative step, entry by entry.  (A white direction of the size of each DOF
        # block's maximum puts root nodes at the tip's amplitude -- a state far rougher than any the rod takes, along which
        # the differences of the pinned rod under gravity agree to 4.9e-7 only, 1.2e-6 with another seed: X0_BLOCKS.)
        return inp.X * rng.normal(0.0, 1.0, inp.X.shape)
    if which == "held":
        return np.where(inp.f_held != 0.0, rng.normal(0.0, FORCE, (B, inp.n)), 0.0)
    return inp.amps * rng.uniform(0.5, 1.5, B)


def perturbed(inp, which, d, e):
    """(a copy of the inputs with one of them moved by e d, the gain, the start states) -- the cached inputs stay as they are"""
    q, K, X = copy.copy(inp), inp.K, inp.X
    if which == "gain":
        K = inp.K + e * d
    elif which == "reference":
        q.R = inp.R + e * d
    elif which in ("x0", X0_BLOCKS):
        X = inp.X + e * d
    elif which == "held":
        q.f_held = inp.f_held + e * d
    else:
        q.amps = inp.amps + e * d
    return q, K, X


def losses(inp, K, X, n_steps=STEPS, hold=HOLD, beam_weights=BEAM_WEIGHTS, sample_weights=SAMPLE_WEIGHTS):
    """(x_T[tip w] of beam 0; sum_b a_b x_T,b[tip w] + sum_b sum_k c_k w_tip,b after sample k) over Inputs.chain"""
    tip = inp.n - 2
    first, total = None, 0.0
    for b in range(len(beam_weights)):
        xT, _, XK = inp.chain(b, K=K, x0=X[b], n_steps=n_steps, hold=hold)
        taken = np.append(XK[1:, tip], xT[tip])[:n_steps // hold]          # the samples a record every `hold` steps takes
        first = xT[tip] if b == 0 else first
        k = min(taken.size, len(sample_weights))
        total += beam_weights[b] * xT[tip] + float(sample_weights[:k] @ taken[:k])
    return float(first), float(total)


@functools.lru_cache(maxsize=None)
def loss_at(name, which, e):
    inp = inputs(name)
    return losses(*perturbed(inp, which, direction(name, which), e))


def differences(name, which, loss=0):
    """(fd1, fd4): central differences of loss 0 / 1 at FD_STEP and a quarter of it -- the evaluations fd_scalar makes"""
    L = lambda e: loss_at(name, which, e)[loss]
    h = FD_STEP
    return (L(h) - L(-h)) / (2 * h), (L(h / 4) - L(-h / 4)) / (h / 2)


@pytest.mark.parametrize("which", DIRECTIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_differences_sit_at_the_floor_of_the_allowance(name, which):
    fd1, fd4 = differences(name, which)
    assert np.isfinite(fd1) and np.isfinite(fd4) and fd4 != 0.0, (name, which, fd1, fd4)
    self_err = 4.0 * abs(fd1 - fd4) / abs(fd4)
    print(f"[implicit-feedback adjoint] {name} {which}: d loss {fd4:.6e}, 4 |fd1 - fd4| / |fd4| = {self_err:.2e}")
    assert self_err <= FD_FLOOR, (name, which, fd1, fd4, self_err)
    # the GPU file's loss (every beam, the recorded tip samples): finite and nonzero too
    g1, g4 = differences(name, which, loss=1)
    assert np.isfinite(g1) and np.isfinite(g4) and g4 != 0.0, (name, which, g1, g4)


@pytest.mark.parametrize("name", list(CASES))
def test_block_sized_start_state_direction_is_resolved_well_inside_the_cap(name):
    """Along X0_BLOCKS fd_scalar's allowance may sit at its 1e-6 cap.  The differences are second order, so the finer one is
    off by about |fd1 - fd4| / 15; that is asserted to be a tenth of the cap at most, for both losses: the cap then measures
    the adjoint, not the reference."""
    for loss in (0, 1):
        fd1, fd4 = differences(name, X0_BLOCKS, loss)
        assert np.isfinite(fd1) and np.isfinite(fd4) and fd4 != 0.0
        own = abs(fd1 - fd4) / (15.0 * abs(fd4))
        print(f"[implicit-feedback adjoint] {name} {X0_BLOCKS} loss {loss}: 4 |fd1 - fd4| / |fd4| = {60.0 * own:.2e}, "
              f"error of fd4 ~ {own:.2e}")
        assert own <= 1e-7, (name, loss, fd1, fd4, own)


def test_oracle_differences_at_hold_one():
    inp = inputs("packed_6")
    for which in ("gain", "reference"):
        d = direction("packed_6", which)
        L = lambda e: losses(*perturbed(inp, which, d, e), hold=1)[0]
        fd1 = (L(FD_STEP) - L(-FD_STEP)) / (2 * FD_STEP)
        fd4 = (L(FD_STEP / 4) - L(-FD_STEP / 4)) / (FD_STEP / 2)
        assert fd4 != 0.0 and 4.0 * abs(fd1 - fd4) / abs(fd4) <= FD_FLOOR, (which, fd1, fd4)


def test_the_cached_inputs_are_left_unchanged():
    inp = inputs("packed_6")
    before = [a.copy() for a in (inp.K, inp.R, inp.X, inp.f_held, inp.amps)]
    for which in DIRECTIONS:
        loss_at("packed_6", which, FD_STEP)
    for a, b in zip(before, (inp.K, inp.R, inp.X, inp.f_held, inp.amps)):
        assert np.array_equal(a, b)
    assert N_SAMPLES == 6 and STEPS // HOLD == SAMPLE_WEIGHTS.size and len(BEAM_WEIGHTS) == B


# ------------------------------------------------------------------ symbols
def header():
    return open(os.path.join(ROOT, "include", "crbeam.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from continuum_robot import _native as nat
    from continuum_robot.batched import BeamEnsemble

    hdr, lib = header(), nat.load()
    for name, ret in zip(NAMES, ("size_t", "int", "int")):
        assert re.search(rf"\b{ret} {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.crb_implicit_feedback_adjoint_work_bytes.restype is C.c_size_t
    assert lib.crb_version() == 106 == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))
    assert "the adjoint of this map." not in hdr and "Not covered: per-beam gain groups, the damped variant." in hdr
    sig = inspect.signature(BeamEnsemble.step_implicit_feedback_adjoint).parameters
    assert list(sig)[1:] == ["n_steps", "h", "lam_red", "gain", "reference", "hold", "n_iter", "x0_red", "impulse_amp",
                             "impulse_duration", "impulse_index", "held_force", "t0", "record", "record_every", "lam_record",
                             "checkpoint_every", "want_gain"]
    assert (sig["hold"].default, sig["n_iter"].default, sig["want_gain"].default, sig["reference"].default) == (1, 2, True, None)
    sig = inspect.signature(BeamEnsemble.rollout_implicit_feedback).parameters
    assert list(sig)[1:9] == ["x0_red", "n_steps", "h", "gain", "reference", "hold", "n_iter", "impulse_amp"]
    assert sig["return_control"].default is False and "checkpoint_every" in sig
    assert "implicit_feedback" in inspect.signature(BeamEnsemble.checkpoint_interval).parameters


# ------------------------------------------------------------------ the work buffer
def slices_of(B_, n):
    tiles = -(-n // 32) * -(-2 * n // 32)
    return min(-(-B_ // 32), -(-1536 // tiles))


def test_work_bytes_formula_on_host_only_plans():
    from continuum_robot import _native as nat

    lib = nat.load()
    wb = lib.crb_implicit_feedback_adjoint_work_bytes
    seen = set()
    for n_elem, nb in ((4, 1), (6, 3), (6, 70), (40, 200)):
        plan = nat.Plan(nitinol_columns(n_elem, "nonlinear"), n_beams=nb, device=-1)
        n, F = 3 * n_elem, nb * (n_elem + 1) * 4           # free DOFs (clamped root), doubles of one [B][n_node][4] record
        Z = slices_of(nb, n)
        seen.add(Z)
        for every, hold in ((1, 1), (8, 4), (12, 4), (32, 1), (30, 10)):
            for n_iter in (1, 2, 16):
                for n_cot in (1, 5, 65535):
                    want = (every * ((2 + n_iter) * F + 1) + n_cot * (1 + every // hold) * F
                            + (n_cot * Z * n * 2 * n if Z > 1 else 0)) * 8
                    assert wb(plan.h, every, n_iter, hold, n_cot) == want, (n_elem, nb, every, hold, n_iter, n_cot)
        # every, n_iter, hold, n_cot out of range: 0
        for bad in ((0, 2, 1, 1), (-4, 2, 4, 1), (4, 0, 4, 1), (4, 17, 4, 1), (4, 2, 0, 1), (4, 2, -1, 1), (6, 2, 4, 1), (2, 2, 4, 1),
                    (4, 2, 4, 0), (4, 2, 4, 65536)):
            assert wb(plan.h, *bad) == 0, bad
    assert wb(None, 4, 2, 4, 1) == 0
    assert 1 in seen and max(seen) > 1                     # with and without partial tiles


# ------------------------------------------------------------------ refusals, before the device is touched
class Calls:
    def __init__(self, dtype, cols=None):
        from continuum_robot import _native as nat

        self.nat, self.lib = nat, nat.load()
        self.plan = nat.Plan(nitinol_columns(4, "nonlinear") if cols is None else cols, n_beams=2, device=-1, dtype=dtype)
        self.t_end = C.c_double(-1.0)

    def ckp(self, x=X_, h=H, n=STEPS, n_iter=N_ITER, hold=HOLD, every=2 * HOLD, gain=GAIN, ref=REF, desc=None, rec=None, ckpt=CKPT,
            u_ckpt=UCK, work=WORK, plan=True):
        return self.lib.crb_step_implicit_feedback_checkpoint(self.plan.h if plan else None, x, 0.0, h, n, n_iter, hold, every, gain,
                                                              ref, desc, rec, ckpt, u_ckpt, work, C.byref(self.t_end), None)

    def adj(self, ckpt=CKPT, u_ckpt=UCK, lam=LAM, n_cot=1, h=H, n=STEPS, n_iter=N_ITER, hold=HOLD, every=2 * HOLD, gain=GAIN,
            ref=REF, desc=None, rec=None, gain_bar=GBAR, ref_bar=RBAR, amp_bar=None, f_bar=FBAR, grad=True, igrad=True, work=WORK,
            plan=True):
        g, ig = self.nat.FeedbackCotangent(), self.nat.InputCotangent()
        g.gain_bar, g.ref_bar = getattr(gain_bar, "value", None), getattr(ref_bar, "value", None)
        ig.amp_bar, ig.f_held_bar = getattr(amp_bar, "value", None), getattr(f_bar, "value", None)
        return self.lib.crb_step_implicit_feedback_adjoint(self.plan.h if plan else None, ckpt, u_ckpt, lam, n_cot, 0.0, h, n, n_iter,
                                                           hold, every, gain, ref, desc, rec, C.byref(g) if grad else None,
                                                           C.byref(ig) if igrad else None, work, None)

    def refused(self, rc, code, who, *words):
        msg = self.lib.crb_last_error().decode()
        assert rc == code, (rc, code, msg)
        for w in (who,) + words:
            assert w in msg, (w, msg)
        assert self.t_end.value == -1.0          # (*t_end is written only by a call that is not refused)


def record(nat, every, node=1):
    return C.byref(nat.RecordDesc(0, node, 1, every, REC.value))


def bad_input(nat):
    d = nat.InputDesc()
    d.kind = 77
    return C.byref(d)


def impulse(nat):
    d = nat.InputDesc()
    d.kind, d.node, d.dof, d.duration, d.amp = nat.CRB_INPUT_IMPULSE, 4, 1, 1e-3, AMP.value
    return C.byref(d)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_in_order_before_the_device(dtype):
    c = Calls(dtype)
    nat, inval = c.nat, c.nat.CRB_EINVAL
    last = (nat.CRB_ENODEV, "host-only") if dtype == "f64" else (nat.CRB_EUNSUPPORTED, "fp64")
    # every later fault of the documented order, next to which each earlier one must still be the one reported
    order = [("n", -1, "n_steps"), ("every", 0, "every must be >= 1"), ("hold", 0, "hold must"), ("every", 6, "multiple of hold"),
             ("n_iter", 17, "n_iter"), ("h", 0.0, "h must"), ("rec", record(nat, 0), "record"), ("rec", record(nat, 3), "record stride"),
             ("desc", bad_input(nat), "input kind")]

    def later(i):
        out = {}
        for k, v, _ in reversed(order[i + 1:]):
            out[k] = v               # (of two faults of one argument the earlier one stays)
        return out

    for call, who in ((c.ckp, PASS), (c.adj, ADJ)):
        worst = later(-1)
        # 1. CRB_EINVAL: NULL plan and buffers, then aliasing, before every size
        c.refused(call(plan=False, **worst), inval, who, "null plan")
        nulls = ("x", "gain", "ckpt", "u_ckpt", "work") if who == PASS else ("ckpt", "u_ckpt", "lam", "gain", "work")
        for key in nulls:
            c.refused(call(**{**worst, key: None}), inval, who, "null")
        if who == ADJ:
            c.refused(call(grad=False, **worst), inval, who, "grad is null")
            for kw, word in ((dict(lam=CKPT), "lam"), (dict(lam=UCK), "lam"), (dict(lam=WORK), "lam"), (dict(lam=GAIN), "lam"),
                             (dict(lam=REF), "lam"), (dict(gain_bar=GAIN), "gain_bar"), (dict(gain_bar=WORK), "gain_bar"),
                             (dict(ref_bar=REF), "ref_bar"), (dict(ref_bar=UCK), "ref_bar"), (dict(amp_bar=WORK), "amp_bar"),
                             (dict(amp_bar=CKPT), "amp_bar"), (dict(f_bar=UCK), "f_held_bar"), (dict(f_bar=GAIN), "f_held_bar"),
                             (dict(gain_bar=LAM), "lam"), (dict(ref_bar=GBAR), "gain_bar"), (dict(amp_bar=RBAR), "ref_bar"),
                             (dict(f_bar=ABAR, amp_bar=ABAR), "amp_bar"), (dict(work=CKPT), "work"), (dict(u_ckpt=CKPT), "work")):
                c.refused(call(**{**worst, **kw}), inval, who, "alias", word)
            for n_cot in (0, -1, 65536):
                c.refused(call(n_cot=n_cot, **worst), inval, who, "n_cot")
        else:
            for kw in (dict(ckpt=X_), dict(u_ckpt=X_), dict(work=X_), dict(u_ckpt=CKPT), dict(work=CKPT), dict(work=UCK),
                       dict(gain=X_), dict(ref=CKPT), dict(ref=UCK), dict(gain=WORK)):
                c.refused(call(**{**worst, **kw}), inval, who, "alias")
        # ... then the sizes, the record and the input, each next to every later one
        for i, (key, value, word) in enumerate(order):
            c.refused(call(**{**later(i), key: value}), inval, who, word)
        for kw, word in ((dict(every=-2), "every must"), (dict(hold=-1), "hold must"), (dict(every=HOLD + 1), "multiple of hold"),
                         (dict(every=HOLD // 2), "multiple of hold"), (dict(n_iter=0), "n_iter"), (dict(h=float("nan")), "h must"),
                         (dict(h=-1e-4), "h must")):
            c.refused(call(**kw), inval, who, word)
        for every in (3, 6, 5):
            c.refused(call(rec=record(nat, every), desc=bad_input(nat)), inval, who, "record stride")
        for every in (1, 2, 4, 8, 12):
            c.refused(call(rec=record(nat, every), desc=bad_input(nat)), inval, who, "input kind")
        if who == ADJ:
            c.refused(call(amp_bar=ABAR), inval, who, "amp_bar", "impulse")                      # no input at all
            c.refused(call(amp_bar=ABAR, desc=bad_input(nat)), inval, who, "input kind")          # (the input comes first)
        # 2. / 3. valid arguments: CRB_EUNSUPPORTED for fp32, else CRB_ENODEV -- also without what is optional
        c.refused(call(), last[0], who, last[1])
        c.refused(call(ref=None, rec=record(nat, 2)), last[0], who, last[1])
        c.refused(call(n=0), last[0], who, last[1])
        c.refused(call(hold=STEPS + 1, every=STEPS + 1), last[0], who, last[1])
        c.refused(call(every=HOLD), last[0], who, last[1])
        if who == ADJ:
            c.refused(call(amp_bar=ABAR, desc=impulse(nat)), last[0], who, last[1])
            c.refused(call(gain_bar=None, ref_bar=None, f_bar=None), last[0], who, last[1])
            c.refused(call(igrad=False), last[0], who, last[1])
        # whole-state snapshots: unsupported, after every CRB_EINVAL and after the dtype
        all_ = record(nat, HOLD, node=-1)
        c.refused(call(rec=all_, desc=bad_input(nat)), inval, who, "input kind")
        c.refused(call(rec=all_), nat.CRB_EUNSUPPORTED, who, "fp64" if dtype == "f32" else "CRB_RECORD_ALL")


def test_unsupported_plans_are_refused_before_the_device():
    from continuum_robot import _native as nat

    big = Calls("f64", nitinol_columns(300, "linear"))
    big32 = Calls("f32", nitinol_columns(300, "linear"))
    for who, call, call32 in ((PASS, big.ckp, big32.ckp), (ADJ, big.adj, big32.adj)):
        big.refused(call(), nat.CRB_EUNSUPPORTED, who, "256")
        big.refused(call(hold=0), nat.CRB_EINVAL, who, "hold must")             # (CRB_EINVAL comes first)
        big32.refused(call32(), nat.CRB_EUNSUPPORTED, who, "fp64")              # (the dtype is looked at first)
    # (a plan of mixed topology has no host-only form: its refusal is in the GPU file)


# ------------------------------------------------------------------ Python argument errors
def bare_ensemble():
    import torch

    from continuum_robot.batched import BeamEnsemble

    ens = BeamEnsemble.__new__(BeamEnsemble)
    ens.dtype, ens.device, ens.n_beams, ens.n = torch.float64, torch.device("cpu"), 2, 12
    return ens


@pytest.mark.parametrize("kw, error, word", [
    (dict(hold=0), ValueError, "hold must be"),
    (dict(hold=2.5), ValueError, "hold must be"),
    (dict(hold=4, checkpoint_every=6), ValueError, "multiple of hold"),
    (dict(hold=4, checkpoint_every=2), ValueError, "multiple of hold"),
    (dict(hold=4, checkpoint_every=0), ValueError, "multiple of hold"),
    (dict(hold=4, record="all"), NotImplementedError, "record='all'"),
])
def test_python_argument_checks_need_no_device(kw, error, word):
    ens = bare_ensemble()
    K, lam, x0 = np.zeros((12, 24)), np.zeros((2, 24)), np.zeros((2, 24))
    with pytest.raises(error, match=word):
        ens.step_implicit_feedback_adjoint(STEPS, H, lam, K, **kw)
    with pytest.raises(error, match=word):
        ens.rollout_implicit_feedback(x0, STEPS, H, K, **kw)
    if "checkpoint_every" in kw:
        with pytest.raises(error, match=word):
            ens.checkpoint_interval(STEPS, kw["checkpoint_every"], implicit_feedback=(2, kw["hold"], 1))


def test_a_list_of_gains_is_not_differentiable_and_a_given_interval_is_returned():
    ens = bare_ensemble()
    for gains in ([np.zeros((12, 24))] * 2, (None, np.zeros((12, 24)))):
        with pytest.raises(NotImplementedError, match="list of gains"):
            ens.step_implicit_feedback_adjoint(STEPS, H, np.zeros((2, 24)), gains, hold=0)
        with pytest.raises(NotImplementedError, match="list of gains"):
            ens.rollout_implicit_feedback(np.zeros((2, 24)), STEPS, H, gains)
    assert ens.checkpoint_interval(STEPS, 8, implicit_feedback=(2, 4, 1)) == 8
    assert ens.checkpoint_interval(STEPS, 24, implicit_feedback=(2, 4, 3)) == 24
    with pytest.raises(ValueError, match="given together"):
        ens.checkpoint_interval(STEPS, None, implicit=(2, 1), implicit_feedback=(2, 4, 1))


def test_automatic_interval_is_a_multiple_of_hold_within_the_budget():
    import torch

    from continuum_robot import _native as nat
    from continuum_robot.batched import BeamEnsemble

    ens = bare_ensemble()
    ens.plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=2, device=-1)
    ens._lib = nat.load()
    wb = lambda every, hold: ens._lib.crb_implicit_feedback_adjoint_work_bytes(ens.plan.h, every, 2, hold, 1)
    for n_steps, hold, want in ((22, 4, 8), (22, 1, 5), (100, 10, 10), (101, 10, 20), (6, 9, 9), (0, 4, 4), (400, 4, 20)):
        assert ens.checkpoint_interval(n_steps, implicit_feedback=(2, hold, 1)) == want, (n_steps, hold)
    # a budget between one and two samples per segment: lowered by hold; below one sample: an error that names the budget
    ens.ADJOINT_WORK_BUDGET = wb(8, 4) - 1
    assert ens.checkpoint_interval(400, implicit_feedback=(2, 4, 1)) == 4
    ens.ADJOINT_WORK_BUDGET = wb(4, 4) - 1
    with pytest.raises(ValueError, match="ADJOINT_WORK_BUDGET"):
        ens.checkpoint_interval(400, implicit_feedback=(2, 4, 1))
    assert BeamEnsemble.ADJOINT_WORK_BUDGET == 1 << 30 and torch.float64 == ens.dtype
