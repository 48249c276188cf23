"""Piecewise-constant control schedules in the RK4 rollout family (crb_input_schedule; step / step_tangent / step_adjoint /
step_adjoint_params / rollout), on every thread mapping: the smallest beams at which each mapping can go wrong.

What is asserted is derived, not measured.  A schedule only changes WHICH force vector a step adds, and a launch that starts
where another ended continues it bitwise: so one call with a schedule is bitwise the chain of one call per interval
with that interval's vector as the held force -- state, clock, samples, tangents, and in reverse the cotangents, which are the
same additions in the same order about the same stage points.  Only sums that the chain forms in another association (the
impulse amplitude's gradient, the parameter gradients: K partial results added up) are compared within K * 2^-53 of their
terms' scale, asserted at 1e-13.

``step_tangent`` and ``step_adjoint`` take the schedule as ``held_force=ControlSchedule(U, hold)`` (their signatures are
fixed); ``step``, ``step_adjoint_params`` and ``rollout`` also as ``control=U, control_hold=hold``."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble, ControlSchedule
from tests.helpers import assert_blocks, nitinol_columns, oracle_beam
from tests.test_adjoint import dot_check
from tests.test_tangent_linear import force_params, oracle_kw, rollout_state

pytestmark = pytest.mark.gpu

DT = 2e-5
STEPS, K, HOLD = 33, 5, 7          # the last interval is cut to 5 steps
DURATION = 12.5 * DT               # the impulse window closes inside interval 1
B = 3
CHUNKS = [(k, min(HOLD, STEPS - k * HOLD)) for k in range(K)]


def pinned_root(n):
    return ["PINNED"] + ["NONE"] * (n - 1)


def mixed_kinds(n):
    return (["linear", "nonlinear"] * n)[:n]


# name -> (column sets: one for all beams or one per beam, ForceParams likewise, (n_slots, threads, packed) of the plan)
MAPPINGS = {
    "general_3": (nitinol_columns(3, "nonlinear"), force_params(True, False), (3, 64, True)),          # fewer than 5 slots
    "packed_6": (nitinol_columns(6, "nonlinear"), force_params(True, False), (6, 64, True)),           # several beams per wave
    "one_wave_33": (nitinol_columns(33, "linear"), force_params(True, False), (33, 64, False)),
    "two_waves_65": (nitinol_columns(65, "nonlinear"), force_params(True, False), (65, 128, False)),
    "four_waves_129": (nitinol_columns(129, mixed_kinds(129)), force_params(False, False), (129, 256, False)),
    "four_waves_256": (nitinol_columns(256, "nonlinear"), force_params(True, False), (256, 256, False)),
    "pinned_gravity_16": (nitinol_columns(16, "nonlinear", bcs=pinned_root(16)), force_params(True, True), (17, 64, True)),
    "heterogeneous": ([nitinol_columns(6, "nonlinear"), nitinol_columns(65, "nonlinear"), nitinol_columns(129, "linear")],
                      [force_params(True, False), force_params(False, False), force_params(True, False)], (129, 256, False)),
}
ONE_SLOT = {"one_slot": (nitinol_columns(1, "linear"), force_params(True, False), (1, 64, True))}
ADJOINT_MAPPINGS = {**MAPPINGS, **ONE_SLOT}


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def clock(t0, k):
    """the clock after k steps: dt added k times in fp64, as the stepper does"""
    t = t0
    for _ in range(k):
        t = t + DT
    return t


class Case:
    """A mapping set up: the ensemble (its mapping asserted), a different random schedule per beam, the tip impulse"""

    def __init__(self, name, dtype=torch.float64, n_beams=B, n_intervals=K):
        cols, fp, (slots, threads, packed) = ADJOINT_MAPPINGS[name]
        self.name = name
        self.ens = ens = BeamEnsemble(cols, n_beams, force_params=fp, dtype=dtype)
        lay = ens.plan.layout
        assert (lay.n_slots, lay.threads, lay.beams_per_group > 1) == (slots, threads, packed), name
        assert ens.mixed_topology == isinstance(cols, list)
        self.n = ens.n
        self.rng = rng = np.random.default_rng(2000 + sum(map(ord, name)))
        # loads: every DOF of an all-linear beam, the transverse ones of the others (axial loads excite the runaway axial
        # modes of the shipped nonlinear element); entries past a beam's own DOF count stay 0
        self.load = np.zeros((n_beams, self.n), bool)
        for b in range(n_beams):
            c = cols[b] if isinstance(cols, list) else cols
            fi = ens.free_index_per_beam[b]
            self.load[b, :fi.size] = True if all(str(t) == "linear" for t in c["type"]) else (fi % 3 == 1)
        self.U = self.schedule(n_intervals)
        self.amps = np.linspace(0.1, 0.2, n_beams)
        self.impulse = dict(impulse_amp=self.amps, impulse_duration=DURATION)
        self.rec = (int(min(ens.n_elem_per_beam)), "w")      # the tip of the shortest beam: a node every beam has
        self.rec_i = [ens.reduced_index(*self.rec, beam=b) for b in range(n_beams)]

    def schedule(self, n_intervals, sigma=0.05):
        return np.where(self.load[None], self.rng.normal(0.0, sigma, (n_intervals,) + self.load.shape), 0.0)

    def start(self):
        """[B, 2n]: the state of a short rollout from rest (non-zero velocities: drag is exercised)"""
        return rollout_state(self.ens)

    def cotangents(self, D):
        lam = self.rng.normal(0.0, 1.0, (D, self.ens.n_beams, 2 * self.n))
        for b in range(self.ens.n_beams):          # (padding entries are ignored: keep them zero for the dot products)
            nb = int(self.ens.n_per_beam[b])
            lam[:, b, nb:self.n] = 0.0
            lam[:, b, self.n + nb:] = 0.0
        return lam


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(MAPPINGS))
def test_one_call_is_bitwise_the_chain_of_held_calls(name, dtype):
    c = Case(name, dtype)
    ens = c.ens
    ens.zero_state()
    t1, s1 = ens.step(STEPS, DT, control=c.U, control_hold=HOLD, record=c.rec, record_every=1, **c.impulse)
    x1 = ens.state.clone()
    ens.zero_state()
    parts = []
    for k, m in CHUNKS:
        t2, sk = ens.step(m, DT, held_force=c.U[k], record=c.rec, record_every=1, **c.impulse)
        parts.append(sk)
    assert torch.isfinite(x1).all() and float(x1.abs().max()) > 0.0
    assert torch.equal(x1, ens.state)
    assert t1 == t2 == clock(0.0, STEPS)
    assert torch.equal(s1, torch.cat(parts, dim=1))
    # ... and the schedule is what drives it: holding the first vector throughout gives another state
    ens.zero_state()
    ens.step(STEPS, DT, held_force=c.U[0], **c.impulse)
    assert not torch.equal(x1, ens.state)
    # the same schedule through held_force=ControlSchedule(...)
    ens.zero_state()
    ens.step(STEPS, DT, held_force=ControlSchedule(c.U, HOLD), **c.impulse)
    assert torch.equal(x1, ens.state)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(MAPPINGS))
def test_degenerate_shapes(name, dtype):
    c = Case(name, dtype, n_intervals=20)
    ens = c.ens
    # K = 1, hold = n_steps: the held force
    ens.zero_state()
    ta, sa = ens.step(STEPS, DT, control=c.U[:1], control_hold=STEPS, record=c.rec, record_every=1, **c.impulse)
    xa = ens.state.clone()
    ens.zero_state()
    tb, sb = ens.step(STEPS, DT, held_force=c.U[0], record=c.rec, record_every=1, **c.impulse)
    assert torch.equal(xa, ens.state) and ta == tb and torch.equal(sa, sb)
    # hold = 1, K = n_steps = 20: twenty chained one-step calls
    ens.zero_state()
    ta, sa = ens.step(20, DT, control=c.U, control_hold=1, record=c.rec, record_every=1, **c.impulse)
    xa = ens.state.clone()
    ens.zero_state()
    parts = []
    for k in range(20):
        tb, sk = ens.step(1, DT, held_force=c.U[k], record=c.rec, record_every=1, **c.impulse)
        parts.append(sk)
    assert torch.equal(xa, ens.state) and ta == tb and torch.equal(sa, torch.cat(parts, dim=1))


def test_oracle_chained_per_interval():
    """8 nonlinear elements + drag, no impulse, against OracleBeam.rk4_held chained per interval: 1e-9 per DOF block, the
    suite's bound for oracle-seeded ensembles"""
    cols = nitinol_columns(8, "nonlinear")
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    ob = oracle_beam(cols, **oracle_kw(True, False))
    rng = np.random.default_rng(7)
    X = rollout_state(ens)
    U = np.where((ens.free_index % 3 == 1)[None, None], rng.normal(0.0, 0.05, (K, B, ens.n)), 0.0)
    ens.set_state(X)
    ens.step(STEPS, DT, control=U, control_hold=HOLD)
    got = ens.unpack_state().cpu().numpy()
    ref = X.copy()
    for b in range(B):
        for k, m in CHUNKS:
            ref[b] = ob.rk4_held(ref[b], DT, m, U[k, b])
    assert_blocks(got, ref, ens.free_index, 1e-9, what="schedule vs chained oracle")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_a_nan_in_one_beams_schedule_stays_in_that_beam(dtype):
    c = Case("packed_6", dtype, n_beams=12)
    ens = c.ens
    _ = ens.status
    ens.zero_state()
    ens.step(STEPS, DT, control=c.U, control_hold=HOLD, **c.impulse)
    clean = ens.state.clone()
    assert int(ens.status.abs().sum()) == 0
    bad = c.U.copy()
    bad[2, 3, c.rec_i[3]] = np.nan          # interval 2, beam 3 (a wave-mate of beams 0 .. 9)
    ens.zero_state()
    ens.step(STEPS, DT, control=bad, control_hold=HOLD, **c.impulse)
    others = [b for b in range(12) if b != 3]
    assert torch.equal(ens.state[others], clean[others])
    assert not torch.isfinite(ens.state[3]).all()
    status = ens.status.cpu().numpy()
    assert status[3] == STEPS and np.all(status[others] == 0)


# ------------------------------------------------------------------ tangent
@pytest.mark.parametrize("name", list(MAPPINGS))
def test_tangent_is_bitwise_the_chain(name):
    c = Case(name)
    ens, D = c.ens, 3
    X = c.start()
    dX = c.cotangents(D) * 1e-3
    dU = np.stack([c.schedule(K) for _ in range(D)])          # [D, K, B, n]
    damp = c.rng.normal(0.0, 1.0, (D, B))
    ens.set_state(X, 0.0)
    got = ens.step_tangent(STEPS, DT, dX, held_force=ControlSchedule(c.U, HOLD), d_held_force=dU, d_impulse_amp=damp, **c.impulse)
    xa, ta = ens.state.clone(), ens.time
    ens.set_state(X, 0.0)
    d = dX
    for k, m in CHUNKS:
        d = ens.step_tangent(m, DT, d, held_force=c.U[k], d_held_force=dU[:, k], d_impulse_amp=damp, **c.impulse)
    assert torch.equal(got, d) and float(got.abs().max()) > 0.0
    assert torch.equal(xa, ens.state) and ta == ens.time == clock(0.0, STEPS)
    # one tangent [K, B, n] serves every direction
    ens.set_state(X, 0.0)
    one = ens.step_tangent(STEPS, DT, dX, held_force=ControlSchedule(c.U, HOLD), d_held_force=dU[0], **c.impulse)
    ens.set_state(X, 0.0)
    rep = ens.step_tangent(STEPS, DT, dX, held_force=ControlSchedule(c.U, HOLD), d_held_force=np.stack([dU[0]] * D), **c.impulse)
    assert torch.equal(one, rep)


# ------------------------------------------------------------------ adjoint
def chained_autograd(c, X, lam, n_steps=STEPS, hold=HOLD):
    """The reference: one differentiable rollout per interval with that interval's vector as its held force, chained from x0 on
    the stepper's clock, and <lam, x_K>.backward().  Returns (xbar0, [amp_bar of interval k], control_bar [K, B, n])."""
    ens = c.ens
    dev = dict(dtype=torch.float64, device=ens.device)
    x0 = torch.tensor(X, requires_grad=True, **dev)
    Us = [torch.tensor(c.U[k], requires_grad=True, **dev) for k in range(c.U.shape[0])]
    As = [torch.tensor(c.amps, requires_grad=True, **dev) for _ in Us]
    x, t, left = x0, 0.0, n_steps
    for k in range(len(Us)):
        m = min(hold, left)
        if m == 0:
            break
        x = ens.rollout(x, m, DT, impulse_amp=As[k], held_force=Us[k], impulse_duration=DURATION, t0=t)
        t, left = clock(t, m), left - m
    (torch.tensor(lam, **dev) * x).sum().backward()
    zero = torch.zeros((ens.n_beams, c.n), **dev)
    return (x0.grad, [a.grad if a.grad is not None else torch.zeros(ens.n_beams, **dev) for a in As],
            torch.stack([u.grad if u.grad is not None else zero for u in Us]))


@pytest.mark.parametrize("name", list(ADJOINT_MAPPINGS))
def test_adjoint_is_bitwise_the_chained_autograd_reference(name):
    c = Case(name)
    ens = c.ens
    X = c.start()
    lam = c.cotangents(1)[0]
    rx, ra, rc = chained_autograd(c, X, lam)
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    xb, ab, cb = ens.step_adjoint(STEPS, DT, lam, x0_red=X, held_force=ControlSchedule(c.U, HOLD), t0=0.0, **c.impulse)
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)
    assert tuple(cb.shape) == (K, B, c.n) and float(cb.abs().max()) > 0.0
    assert torch.equal(xb, rx)
    assert torch.equal(cb, rc)
    terms = torch.stack(ra)                                   # [K, B]: the chain adds K partial results in another association
    err, scale = (ab - terms.sum(dim=0)).abs(), terms.abs().sum(dim=0)
    print(f"[{name}] amp_bar association error / scale: {np_(err / scale.clamp_min(1e-300))}")
    assert float(scale.min()) > 0.0 and bool((err <= 1e-13 * scale).all())
    # a rollout that stops short: the intervals it does not reach have exactly zero gradient, and so has every entry past a
    # beam's own DOF count
    short = 20
    rx, ra, rc = chained_autograd(c, X, lam, short)
    xb, ab, cb = ens.step_adjoint(short, DT, lam, x0_red=X, held_force=ControlSchedule(c.U, HOLD), t0=0.0, **c.impulse)
    assert torch.equal(xb, rx) and torch.equal(cb, rc)
    assert float(cb[:3].abs().max()) > 0.0 and bool((cb[3:] == 0.0).all())
    for b in range(B):
        nb = int(ens.n_per_beam[b])
        assert bool((cb[:, b, nb:] == 0.0).all()) and bool((xb[b, nb:c.n] == 0.0).all()) and bool((xb[b, c.n + nb:] == 0.0).all())
    # a switch after EVERY swept step: hold = 1, K = n_steps, with segments of 4 steps
    c1 = Case(name, n_intervals=short)
    rx, ra, rc = chained_autograd(c1, X, lam, short, hold=1)
    xb, ab, cb = c1.ens.step_adjoint(short, DT, lam, x0_red=X, held_force=ControlSchedule(c1.U, 1), t0=0.0, checkpoint_every=4,
                                     **c1.impulse)
    assert torch.equal(xb, rx) and torch.equal(cb, rc)
    assert bool((cb.abs().amax(dim=(1, 2)) > 0.0).all())          # every interval got its gradient


@pytest.mark.parametrize("name", list(ADJOINT_MAPPINGS))
def test_adjoint_is_bitwise_independent_of_segments_and_batching(name):
    c = Case(name)
    ens, D = c.ens, 3
    X = c.start()
    lam = c.cotangents(D)
    lam_rec = c.rng.normal(0.0, 1.0, (D, B, STEPS // 7))

    def run(lm, lr, ce):
        return ens.step_adjoint(STEPS, DT, lm, x0_red=X, held_force=ControlSchedule(c.U, HOLD), t0=0.0, record=c.rec,
                                record_every=7, lam_record=lr, checkpoint_every=ce, **c.impulse)

    ref = run(lam, lam_rec, 1)
    for ce in (4, 7, STEPS, None):            # (4: segments straddle the interval boundaries)
        for r, g in zip(ref, run(lam, lam_rec, ce)):
            assert torch.equal(r, g), ce
    for d in range(D):
        for r, g in zip(ref, run(lam[d], lam_rec[d], 4)):
            assert torch.equal(r[d], g), d


@pytest.mark.parametrize("name", list(ADJOINT_MAPPINGS))
def test_dot_product_identity_with_the_tangent(name):
    """<lam, dx(T)> + <lam_rec, d samples> = <xbar0, dx0> + <amp_bar, d amp> + <control_bar, d control>, to 1e-10 of
    sum |lam_i (J v)_i| (DESIGN §10's tolerance for rollouts with drag and gravity).  Four samples, every 7 steps: each at an
    interval's last step."""
    c = Case(name)
    ens = c.ens
    X = c.start()
    lam = c.cotangents(1)[0]
    n_rec = STEPS // 7
    lam_rec = c.rng.normal(0.0, 1.0, (B, n_rec))
    dX = c.cotangents(1)[0] * 1e-3
    dU = c.schedule(K)
    damp = c.rng.normal(0.0, 1.0, B)
    sched = ControlSchedule(c.U, HOLD)

    def tangent(m):
        ens.set_state(X, 0.0)
        return np_(ens.step_tangent(m, DT, dX, held_force=sched, d_held_force=dU, d_impulse_amp=damp, **c.impulse))

    dT = tangent(STEPS)
    d_samples = np.zeros((B, n_rec))
    for j in range(n_rec):
        dj = tangent(7 * (j + 1))
        d_samples[:, j] = [dj[b, c.rec_i[b]] for b in range(B)]
    xb, ab, cb = ens.step_adjoint(STEPS, DT, lam, x0_red=X, held_force=sched, t0=0.0, record=c.rec, record_every=7,
                                  lam_record=lam_rec, **c.impulse)
    err = dot_check([(lam, dT), (lam_rec, d_samples)], [(xb, dX), (ab, damp), (cb, dU)], 1e-10, name)
    print(f"[{name}] dot-product identity: {err:.2e}")


@pytest.mark.parametrize("name", list(ADJOINT_MAPPINGS))
def test_parameter_gradients_with_a_schedule(name):
    c = Case(name)
    ens = c.ens
    X = c.start()
    lam = c.cotangents(1)[0]
    kw = dict(x0_red=X, t0=0.0, **c.impulse)
    ref = ens.step_adjoint(STEPS, DT, lam, held_force=ControlSchedule(c.U, HOLD), **kw)
    got = ens.step_adjoint_params(STEPS, DT, lam, control=c.U, control_hold=HOLD, checkpoint_every=4, **kw)
    for r, g in zip(ref, got[:3]):
        assert torch.equal(r, g)
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    other = ens.step_adjoint_params(STEPS, DT, lam, control=c.U, control_hold=HOLD, checkpoint_every=STEPS, **kw)
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)
    for key, v in got[3].items():
        assert torch.equal(v, other[3][key]), key
    # the chain: interval by interval from the last, the state cotangent carried down; every entry is the sum of the chain's K
    # entries, in another association
    starts, x, t = [], torch.tensor(X, dtype=torch.float64, device=ens.device), 0.0
    for k, m in CHUNKS:
        starts.append((x, t))
        x = ens.rollout(x, m, DT, held_force=c.U[k], impulse_amp=c.amps, impulse_duration=DURATION, t0=t).detach()
        t = clock(t, m)
    lm, parts = lam, []
    for k, m in reversed(CHUNKS):
        xk, tk = starts[k]
        lm, _, _, pd = ens.step_adjoint_params(m, DT, lm, x0_red=xk, held_force=c.U[k], t0=tk, **c.impulse)
        parts.append(pd)
    assert torch.equal(lm, ref[0])
    for key, v in got[3].items():
        terms = torch.stack([p[key] for p in parts])
        err, scale = (v - terms.sum(dim=0)).abs(), terms.abs().sum(dim=0)
        worst = float((err / scale.clamp_min(1e-300)).max())
        print(f"[{name}] {key}: association error / scale {worst:.2e}")
        assert bool((err <= 1e-13 * scale).all()), (key, worst)


def test_rollout_gradcheck_and_backward():
    cols = nitinol_columns(4, "nonlinear")
    nb, steps, k_int, hold = 2, 10, 3, 4
    ens = BeamEnsemble(cols, nb, force_params=force_params(True, False))
    X = rollout_state(ens, 40)
    dev = dict(dtype=torch.float64, device=ens.device)
    x0 = torch.tensor(X, requires_grad=True, **dev)
    amp = torch.tensor([0.1, 0.2], requires_grad=True, **dev)
    ctrl = torch.zeros((k_int, nb, ens.n), **dev)
    ctrl[:, :, 1::3] = torch.linspace(-0.02, 0.03, k_int * nb, **dev).reshape(k_int, nb, 1)
    ctrl.requires_grad_(True)
    f = lambda x, a, u: ens.rollout(x, steps, DT, impulse_amp=a, control=u, control_hold=hold)   # noqa: E731
    assert torch.autograd.gradcheck(f, (x0, amp, ctrl), eps=1e-6)
    # loss.backward() on a recorded-tip loss is bitwise step_adjoint
    weights = torch.linspace(0.5, 2.0, 5, **dev)
    xT, samples = ens.rollout(x0, steps, DT, impulse_amp=amp, control=ctrl, control_hold=hold, record=(ens.n_elem, "w"),
                              record_every=2)
    (xT[:, ens.n - 2].sum() + (samples * weights).sum()).backward()
    lam = np.zeros((nb, 2 * ens.n))
    lam[:, ens.n - 2] = 1.0
    xb, ab, cb = ens.step_adjoint(steps, DT, lam, x0_red=X, impulse_amp=[0.1, 0.2], held_force=ControlSchedule(np_(ctrl), hold),
                                  t0=0.0, record=(ens.n_elem, "w"), record_every=2, lam_record=np_(weights)[None].repeat(nb, 0))
    assert torch.equal(x0.grad, xb) and torch.equal(amp.grad, ab) and torch.equal(ctrl.grad, cb)
    assert float(ctrl.grad[:, :, 1::3].abs().min()) > 0.0


def test_argument_checks():
    ens = BeamEnsemble(nitinol_columns(4, "nonlinear"), 2)
    U = np.zeros((5, 2, ens.n))
    with pytest.raises(ValueError, match="held_force"):
        ens.step(STEPS, DT, control=U, control_hold=HOLD, held_force=U[0])
    with pytest.raises(ValueError, match="control must be"):
        ens.step(STEPS, DT, control=U[:, :1], control_hold=HOLD)
    with pytest.raises(ValueError, match="n_steps"):
        ens.step(STEPS + 3, DT, control=U, control_hold=HOLD)
    with pytest.raises(ValueError, match="tangent of a control schedule"):
        ens.step_tangent(STEPS, DT, np.zeros((2, 2 * ens.n)), held_force=ControlSchedule(U, HOLD), d_held_force=U[0])
    assert ens.time == 0.0 and float(ens.state.abs().max()) == 0.0


def test_full_size_4096_beams_of_256_elements():
    cols = nitinol_columns(256, "nonlinear")
    nb, steps, k_int, hold = 4096, 20, 4, 5
    fp = force_params(True, False)
    ens = BeamEnsemble(cols, nb, force_params=fp)
    rng = np.random.default_rng(10)
    X = rollout_state(ens)
    amps = np.linspace(0.1, 0.5, nb)
    U = np.where((ens.free_index % 3 == 1)[None, None], rng.normal(0.0, 0.05, (k_int, nb, ens.n)), 0.0)
    lam = rng.normal(0.0, 1.0, (nb, 2 * ens.n))
    xb, ab, cb = ens.step_adjoint(steps, DT, lam, x0_red=X, impulse_amp=amps, held_force=ControlSchedule(U, hold), t0=0.0)
    assert bool(torch.isfinite(xb).all()) and bool(torch.isfinite(ab).all()) and bool(torch.isfinite(cb).all())
    pick = [0, 2047, 4095]
    small = BeamEnsemble(cols, 3, force_params=fp)
    sx, sa, sc = small.step_adjoint(steps, DT, lam[pick], x0_red=X[pick], impulse_amp=amps[pick],
                                    held_force=ControlSchedule(U[:, pick], hold), t0=0.0)
    assert float(sc.abs().max()) > 0.0
    assert torch.equal(cb[:, pick], sc) and torch.equal(xb[pick], sx) and torch.equal(ab[pick], sa)
