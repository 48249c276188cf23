"""Control schedules in the implicit stepper and its adjoint (crb_step_implicit_sched, crb_step_implicit_checkpoint_sched,
crb_step_implicit_adjoint_sched; BeamEnsemble.step_implicit / step_implicit_adjoint / rollout_implicit) on every thread mapping
of tests/test_control_schedule.py: the smallest beams at which each mapping can go wrong.  The case table, the inputs and the
oracle's chained rollouts come from tests/test_implicit_schedule_cpu.py, which proves them on the oracle alone.

What is asserted is derived, not measured.  A scheduled call IS the chain of one call per interval with f_held = that
interval's vector: the kernels reload the force and reset the starting iterate to 0 at an interval's first step, which is
what the first step of a call does -- so state, clock, samples and status are bitwise the chain's, and in reverse the
cotangents are, the carried cotangent of the starting iterate being dropped where the chain's calls end.  Only the impulse
amplitude's gradient, which the chain forms as K partial sums in another association, is compared within K * 2^-53 of its
terms' scale, asserted at 1e-13 (as the RK4 family's test does).  Against the oracle the bounds are the suite's own: 1e-7 per
DOF block for the forward pass (tests/test_implicit_adjoint_mappings.py), fd_scalar's two-step-size rule for gradients.

``step_implicit_adjoint`` takes the schedule as ``held_force=ControlSchedule(U, hold)`` (its signature is fixed);
``step_implicit`` and ``rollout_implicit`` also as ``control=U, control_hold=hold``."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble, ControlSchedule
from tests.helpers import assert_blocks, block_errs, nitinol_columns
from tests.test_adjoint import fd_scalar, np_
from tests.test_control_schedule import ADJOINT_MAPPINGS
from tests.test_derivative_mappings import clock
from tests.test_implicit_schedule_cpu import (B, BLOCKS, FD_CASES, HOLD, K, RUNS, STEPS, TAG, fd_inputs, inputs, run_id)
from tests.test_tangent_linear import force_params

pytestmark = pytest.mark.gpu

CHUNKS = [(k, min(HOLD, STEPS - k * HOLD)) for k in range(K)]
SHORT = 20                          # a rollout that stops inside interval 2


class Setup:
    """A run of the table on the GPU: the ensemble with its plan layout asserted, and the CPU file's inputs"""

    def __init__(self, run, i=None):
        self.i = i = inputs(*run) if i is None else i
        cols, fp, (slots, threads, packed) = ADJOINT_MAPPINGS[i.name]
        self.ens = ens = BeamEnsemble(cols, B, force_params=fp)
        lay = ens.plan.layout
        assert (lay.n_slots, lay.threads, lay.beams_per_group > 1) == (slots, threads, packed), i.name
        assert ens.n == i.n and all(np.array_equal(ens.free_index_per_beam[b], i.fi[b]) for b in range(B))
        self.h, self.n = i.h, i.n
        self.kw = dict(n_iter=i.n_iter, impulse_amp=i.amps, impulse_duration=i.duration)
        self.rec = (int(min(ens.n_elem_per_beam)), "w")      # the tip of the shortest beam: a node every beam has
        self.rec_i = [ens.reduced_index(*self.rec, beam=b) for b in range(B)]

    def cotangents(self, D, rng):
        lam = rng.normal(0.0, 1.0, (D, B, 2 * self.n))
        for b in range(B):                 # (padding entries are ignored: keep them zero)
            nb = self.i.nb[b]
            lam[:, b, nb:self.n] = 0.0
            lam[:, b, self.n + nb:] = 0.0
        return lam

    def adjoint(self, lam, U=None, n_steps=STEPS, hold=HOLD, **over):
        kw = dict(self.kw, x0_red=self.i.X, t0=0.0, held_force=ControlSchedule(self.i.U if U is None else U, hold))
        kw.update(over)
        return self.ens.step_implicit_adjoint(n_steps, self.h, lam, **kw)


def set_kernel(monkeypatch, kernel):
    """default: the lean kernel where the plan has one; walk: its workgroups walk over beams (2 workgroups for 3 beams);
    general: crb_implicit_kernel"""
    monkeypatch.delenv("CRB_DISABLE_LEAN_IMPLICIT", raising=False)
    monkeypatch.delenv("CRB_LEAN_MAX_GROUPS", raising=False)
    if kernel == "general":
        monkeypatch.setenv("CRB_DISABLE_LEAN_IMPLICIT", "1")
    elif kernel == "walk":
        monkeypatch.setenv("CRB_LEAN_MAX_GROUPS", "2")


# ------------------------------------------------------------------ 1. forward: bitwise the chain
@pytest.mark.parametrize("kernel", ["default", "walk", "general"])
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_one_call_is_bitwise_the_chain_of_held_calls(run, kernel, monkeypatch):
    set_kernel(monkeypatch, kernel)
    s = Setup(run)
    ens, i, h = s.ens, s.i, s.h
    record = dict(record=s.rec, record_every=1)
    _ = ens.status
    ens.set_state(i.X, 0.0)
    t1, s1 = ens.step_implicit(STEPS, h, control=i.U, control_hold=HOLD, **record, **s.kw)
    x1, st1 = ens.state.clone(), ens.status.clone()
    ens.reset_status()
    ens.set_state(i.X, 0.0)
    parts = []
    for k, m in CHUNKS:
        t2, sk = ens.step_implicit(m, h, held_force=i.U[k], **record, **s.kw)
        parts.append(sk)
    assert torch.isfinite(x1).all() and float(x1.abs().max()) > 0.0
    assert torch.equal(x1, ens.state)
    assert t1 == t2 == clock(0.0, h, STEPS)
    assert torch.equal(s1, torch.cat(parts, dim=1))
    assert torch.equal(st1, ens.status) and int(st1.abs().sum()) == 0
    # ... and the schedule is what drives it: holding the first vector throughout gives another state
    ens.set_state(i.X, 0.0)
    ens.step_implicit(STEPS, h, held_force=i.U[0], **s.kw)
    assert not torch.equal(x1, ens.state)
    # the same schedule through held_force=ControlSchedule(...)
    ens.set_state(i.X, 0.0)
    ens.step_implicit(STEPS, h, held_force=ControlSchedule(i.U, HOLD), **s.kw)
    assert torch.equal(x1, ens.state)
    # whole-state snapshots, and a rollout that stops short of the last intervals
    ens.set_state(i.X, 0.0)
    _, snaps = ens.step_implicit(SHORT, h, control=i.U, control_hold=HOLD, record="all", record_every=HOLD, **s.kw)
    xs = ens.state.clone()
    ens.set_state(i.X, 0.0)
    for k, m in ((0, HOLD), (1, HOLD), (2, SHORT - 2 * HOLD)):
        ens.step_implicit(m, h, held_force=i.U[k], **s.kw)
        if m == HOLD:
            assert torch.equal(snaps[k], ens.state), k
    assert torch.equal(xs, ens.state)


# ------------------------------------------------------------------ 2. against the oracle chained per interval
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_scheduled_call_matches_the_chained_oracle(run):
    """step_implicit and rollout_implicit with a schedule against OracleBeam.implicit chained per interval, per DOF block at
    1e-7: the bound rollout_implicit against the oracle carries in tests/test_implicit_adjoint_mappings.py (3e-12 measured
    there)"""
    s = Setup(run)
    ens, i = s.ens, s.i
    ens.set_state(i.X, 0.0)
    ens.step_implicit(STEPS, s.h, control=i.U, control_hold=HOLD, **s.kw)
    got = ens.unpack_state().cpu().numpy()
    xT, samples = ens.rollout_implicit(i.X, STEPS, s.h, control=i.U, control_hold=HOLD, record=s.rec, record_every=1, **s.kw)
    worst = 0.0
    for b in range(B):
        ref, rec = i.chained(b, samples=True)
        for what, x in (("step_implicit", got[b]), ("rollout_implicit", np_(xT)[b])):
            errs = block_errs(i.own(b, x), ref, i.fi[b])
            worst = max(worst, max(errs.values()))
            print(f"{TAG} {run_id(run)} beam {b} | {what} vs chained oracle | " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
            assert_blocks(i.own(b, x), ref, i.fi[b], 1e-7, what=f"{run_id(run)} beam {b} {what}")
        want = rec[:, s.rec_i[b]]
        rec_err = float(np.max(np.abs(np_(samples)[b] - want)) / np.max(np.abs(want)))
        assert rec_err <= 1e-7, (run, b, rec_err)
    print(f"{TAG} {run_id(run)} | forward vs chained oracle | worst block {worst:.2e}")


# ------------------------------------------------------------------ 3. adjoint: bitwise the chained autograd reference
def chained_autograd(s, lam, U, n_steps=STEPS, hold=HOLD):
    """The reference: one differentiable implicit rollout per interval with that interval's vector as its held force, chained
    from x0 on the stepper's clock, and <lam, x_K>.backward().  Returns (xbar0, [amp_bar of interval k], control_bar)."""
    ens, i = s.ens, s.i
    dev = dict(dtype=torch.float64, device=ens.device)
    x0 = torch.tensor(i.X, requires_grad=True, **dev)
    Us = [torch.tensor(U[k], requires_grad=True, **dev) for k in range(U.shape[0])]
    As = [torch.tensor(i.amps, requires_grad=True, **dev) for _ in Us]
    x, t, left = x0, 0.0, n_steps
    for k in range(len(Us)):
        m = min(hold, left)
        if m == 0:
            break
        x = ens.rollout_implicit(x, m, s.h, n_iter=i.n_iter, impulse_amp=As[k], held_force=Us[k], impulse_duration=i.duration, t0=t)
        t, left = clock(t, s.h, m), left - m
    (torch.tensor(lam, **dev) * x).sum().backward()
    zero = torch.zeros((B, s.n), **dev)
    return (x0.grad, [a.grad if a.grad is not None else torch.zeros(B, **dev) for a in As],
            torch.stack([u.grad if u.grad is not None else zero for u in Us]))


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_adjoint_is_bitwise_the_chained_autograd_reference(run):
    s = Setup(run)
    ens, i = s.ens, s.i
    rng = np.random.default_rng(11 + sum(map(ord, i.name)))
    lam = s.cotangents(1, rng)[0]
    rx, ra, rc = chained_autograd(s, lam, i.U)
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    xb, ab, cb = s.adjoint(lam)
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)
    assert tuple(cb.shape) == (K, B, s.n) and float(cb.abs().max()) > 0.0
    assert torch.equal(xb, rx)
    assert torch.equal(cb, rc)
    terms = torch.stack(ra)                                   # [K, B]: the chain adds K partial results in another association
    err, scale = (ab - terms.sum(dim=0)).abs(), terms.abs().sum(dim=0)
    print(f"{TAG} {run_id(run)} | amp_bar association error / scale: {np_(err / scale.clamp_min(1e-300))}")
    assert float(scale.min()) > 0.0 and bool((err <= 1e-13 * scale).all())
    # a rollout that stops short: the intervals it does not reach have exactly zero gradient, and so has every entry past a
    # beam's own DOF count
    rx, ra, rc = chained_autograd(s, lam, i.U, SHORT)
    xb, ab, cb = s.adjoint(lam, n_steps=SHORT)
    assert torch.equal(xb, rx) and torch.equal(cb, rc)
    assert float(cb[:3].abs().max()) > 0.0 and bool((cb[3:] == 0.0).all())
    for b in range(B):
        nb = i.nb[b]
        assert bool((cb[:, b, nb:] == 0.0).all()) and bool((xb[b, nb:s.n] == 0.0).all()) and bool((xb[b, s.n + nb:] == 0.0).all())
    # a switch after EVERY swept step: hold = 1, K = n_steps, with segments of 4 steps that straddle the intervals
    U1 = i.schedule(SHORT)
    rx, ra, rc = chained_autograd(s, lam, U1, SHORT, hold=1)
    xb, ab, cb = s.adjoint(lam, U=U1, n_steps=SHORT, hold=1, checkpoint_every=4)
    assert torch.equal(xb, rx) and torch.equal(cb, rc)
    assert bool((cb.abs().amax(dim=(1, 2)) > 0.0).all())          # every interval got its gradient


# ------------------------------------------------------------------ 4. bitwise independence of segments and batching
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_adjoint_is_bitwise_independent_of_segments_and_batching(run):
    s = Setup(run)
    i, D = s.i, 3
    rng = np.random.default_rng(23 + sum(map(ord, i.name)))
    lam = s.cotangents(D, rng)
    lam_rec = rng.normal(0.0, 1.0, (D, B, STEPS // 5))

    def go(lm, lr, ce):
        return s.adjoint(lm, record=s.rec, record_every=5, lam_record=lr, checkpoint_every=ce)

    ref = go(lam, lam_rec, 1)
    assert all(bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0.0 for r in ref)
    for ce in (4, 7, STEPS, None):            # (4: segments straddle the interval boundaries; 7: they coincide with them)
        for r, g in zip(ref, go(lam, lam_rec, ce)):
            assert torch.equal(r, g), ce
    for d in range(D):
        for r, g in zip(ref, go(lam[d], lam_rec[d], 4)):
            assert torch.equal(r[d], g), d


# ------------------------------------------------------------------ 5. the gradient against the oracle's differences
@pytest.mark.parametrize("name", list(FD_CASES))
def test_control_gradient_matches_the_chained_oracles_differences(name):
    """control_bar dotted with a dense direction and with a direction on one interval only, per DOF block of the final state
    (the cotangent of a block: the block-normalised oracle tangent on it), against the chained oracle's central difference
    under fd_scalar's rule err <= min(max(1e-7, 4 self), 1e-6)"""
    i = fd_inputs(name)
    s = Setup(None, i)
    for k, (label, v) in enumerate(i.dirs):
        lam = np.zeros((6, B, 2 * s.n))
        for b in range(B):
            lam[:, b] = np.stack([i.pad_row(b, row) for row in i.cotangents(b, k)])
        _, _, cb = s.adjoint(lam, checkpoint_every=4)
        for b in range(B):
            for blk in range(6):
                if i.block_sel(b, blk).size == 0:
                    continue
                g = float(np.sum(np_(cb)[blk, :, b] * v[:, b]))
                err, allowed, self_err, _ = i.figures(b, k, blk, g)
                print(f"{TAG} {name} beam {b} | {label} | {BLOCKS[blk]} | err {err:.2e} | allowed {allowed:.2e} | self {self_err:.2e}")
                fd_scalar(g, i.loss(b, k, blk), i.e, f"{name} beam {b} {label} {BLOCKS[blk]}")


# ------------------------------------------------------------------ 6. the reset is real
@pytest.mark.parametrize("kernel", ["default", "general"])
def test_equal_vectors_are_the_chain_not_the_single_held_call(kernel, monkeypatch):
    """A nonlinear rod with drag, n_iter = 1: a schedule of K equal vectors restarts the iteration at every interval, so it
    differs from the one call that holds the vector (whose iterate carries through), and equals the chain bitwise.  n_iter = 2
    shrinks the difference to the iteration's convergence error: both are printed per DOF block."""
    set_kernel(monkeypatch, kernel)
    for name, h in (("two_waves_65", 1e-4), ("packed_6", 1e-4)):
        for n_iter in (1, 2):
            s = Setup((name, h, n_iter))
            ens, i = s.ens, s.i
            same = np.broadcast_to(i.U[:1], i.U.shape).copy()
            ens.set_state(i.X, 0.0)
            ens.step_implicit(STEPS, h, control=same, control_hold=HOLD, **s.kw)
            sched = ens.state.clone()
            got = ens.unpack_state().cpu().numpy()
            ens.set_state(i.X, 0.0)
            for k, m in CHUNKS:
                ens.step_implicit(m, h, held_force=same[k], **s.kw)
            assert torch.equal(sched, ens.state)
            ens.set_state(i.X, 0.0)
            ens.step_implicit(STEPS, h, held_force=same[0], **s.kw)
            assert not torch.equal(sched, ens.state), (name, n_iter)
            errs = block_errs(got, ens.unpack_state().cpu().numpy(), ens.free_index)
            print(f"{TAG} {name} n_iter {n_iter} {kernel} | K equal vectors vs one held call | " +
                  " ".join(f"{k} {e:.1e}" for k, e in errs.items()))


def test_ten_element_example_rod_reset_size():
    """The figure DESIGN.md section 10 quotes: the 10-element example rod (nonlinear, drag), h = 1e-4, n_iter = 2, 200 steps
    in 20 intervals of equal vectors against the one held call.  Printed, not asserted against a bound."""
    ens = BeamEnsemble(nitinol_columns(10, "nonlinear"), 1, force_params=force_params(True, False))
    u = np.zeros((1, ens.n))
    u[0, ens.n - 2] = 0.05
    kw = dict(n_iter=2, impulse_amp=[0.15])
    ens.zero_state()
    ens.step_implicit(200, 1e-4, control=np.broadcast_to(u, (20, 1, ens.n)).copy(), control_hold=10, **kw)
    a = ens.unpack_state().cpu().numpy()
    ens.zero_state()
    ens.step_implicit(200, 1e-4, held_force=u, **kw)
    b = ens.unpack_state().cpu().numpy()
    errs = block_errs(a, b, ens.free_index)
    print(f"{TAG} 10-element example rod, 20 x 10 steps, n_iter 2 | equal vectors vs one held call | " +
          " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert not np.array_equal(a, b) and np.all(np.isfinite(a))


# ------------------------------------------------------------------ 7. autograd
def test_rollout_implicit_gradcheck_and_backward():
    cols, fp, _ = ADJOINT_MAPPINGS["packed_6"]
    nb, steps, k_int, hold, h = 2, 8, 4, 2, 1e-4
    ens = BeamEnsemble(cols, nb, force_params=fp)
    ens.zero_state()
    ens.step_implicit(40, h, impulse_amp=[0.1, 0.2], t0=0.0)
    X = ens.unpack_state().cpu().numpy()
    dev = dict(dtype=torch.float64, device=ens.device)
    x0 = torch.tensor(X, requires_grad=True, **dev)
    amp = torch.tensor([0.1, 0.2], requires_grad=True, **dev)
    ctrl = torch.zeros((k_int, nb, ens.n), **dev)
    ctrl[:, :, 1::3] = torch.linspace(-0.02, 0.03, k_int * nb, **dev).reshape(k_int, nb, 1)
    ctrl.requires_grad_(True)
    f = lambda x, a, u: ens.rollout_implicit(x, steps, h, impulse_amp=a, control=u, control_hold=hold, checkpoint_every=3)   # noqa: E731
    assert torch.autograd.gradcheck(f, (x0, amp, ctrl), eps=1e-6)
    # loss.backward() on a recorded-tip loss reaches x0, impulse_amp and control together: bitwise step_implicit_adjoint
    weights = torch.linspace(0.5, 2.0, 4, **dev)
    xT, samples = ens.rollout_implicit(x0, steps, h, impulse_amp=amp, control=ctrl, control_hold=hold, record=(ens.n_elem, "w"),
                                       record_every=2)
    (xT[:, ens.n - 2].sum() + (samples * weights).sum()).backward()
    lam = np.zeros((nb, 2 * ens.n))
    lam[:, ens.n - 2] = 1.0
    xb, ab, cb = ens.step_implicit_adjoint(steps, h, lam, x0_red=X, impulse_amp=[0.1, 0.2],
                                           held_force=ControlSchedule(np_(ctrl), hold), t0=0.0, record=(ens.n_elem, "w"),
                                           record_every=2, lam_record=np_(weights)[None].repeat(nb, 0))
    assert torch.equal(x0.grad, xb) and torch.equal(amp.grad, ab) and torch.equal(ctrl.grad, cb)
    assert float(ctrl.grad[:, :, 1::3].abs().min()) > 0.0


# ------------------------------------------------------------------ 8. isolation
@pytest.mark.parametrize("name", ["packed_6", "two_waves_65"])
def test_a_nan_in_one_beams_schedule_stays_in_that_beam(name):
    s = Setup((name, 1e-4, 2))
    ens, i = s.ens, s.i
    rng = np.random.default_rng(5)
    lam = s.cotangents(1, rng)[0]
    _ = ens.status
    ens.set_state(i.X, 0.0)
    ens.step_implicit(STEPS, s.h, control=i.U, control_hold=HOLD, **s.kw)
    clean = ens.state.clone()
    assert int(ens.status.abs().sum()) == 0
    clean_bar = s.adjoint(lam)
    bad = i.U.copy()
    bad[2, 1, s.rec_i[1]] = np.nan          # interval 2, beam 1 (packed: a wave-mate of beams 0 and 2)
    ens.set_state(i.X, 0.0)
    ens.step_implicit(STEPS, s.h, control=bad, control_hold=HOLD, **s.kw)
    others = [0, 2]
    assert torch.equal(ens.state[others], clean[others])
    assert not torch.isfinite(ens.state[1]).all()
    status = ens.status.cpu().numpy()
    assert status[1] != 0 and np.all(status[others] == 0)
    ens.reset_status()
    xb, ab, cb = s.adjoint(lam, U=bad)
    assert torch.equal(xb[others], clean_bar[0][others]) and torch.equal(ab[others], clean_bar[1][others])
    assert torch.equal(cb[:, others], clean_bar[2][:, others])
    assert not torch.isfinite(cb[:, 1]).all()


# ------------------------------------------------------------------ 9. Python argument checks
def test_argument_checks():
    ens = BeamEnsemble(nitinol_columns(4, "nonlinear"), 2)
    U = np.zeros((5, 2, ens.n))
    lam = np.zeros((2, 2 * ens.n))
    with pytest.raises(ValueError, match="held_force"):
        ens.step_implicit(STEPS, 1e-4, control=U, control_hold=HOLD, held_force=U[0])
    with pytest.raises(ValueError, match="control_hold needs control"):
        ens.step_implicit(STEPS, 1e-4, control_hold=HOLD)
    with pytest.raises(ValueError, match="implicit steps per interval"):
        ens.step_implicit(STEPS, 1e-4, control=U)
    with pytest.raises(ValueError, match="control must be"):
        ens.step_implicit(STEPS, 1e-4, control=U[:, :1], control_hold=HOLD)
    with pytest.raises(ValueError, match="n_steps"):
        ens.step_implicit(STEPS + 3, 1e-4, control=U, control_hold=HOLD)
    with pytest.raises(ValueError, match="n_steps"):
        ens.step_implicit_adjoint(STEPS + 3, 1e-4, lam, held_force=ControlSchedule(U, HOLD))
    with pytest.raises(NotImplementedError, match="rho_inf"):
        ens.step_implicit(STEPS, 1e-4, control=U, control_hold=HOLD, rho_inf=0.5)
    with pytest.raises(NotImplementedError, match="rho_inf"):
        ens.step_implicit(STEPS, 1e-4, held_force=ControlSchedule(U, HOLD), rho_inf=0.5)
    with pytest.raises(ValueError, match="ControlSchedule"):
        ens.step_implicit(STEPS, 1e-4, held_force=ControlSchedule(U, HOLD), control=U, control_hold=HOLD)
    with pytest.raises(ValueError, match="ControlSchedule"):
        ens.rollout_implicit(np.zeros((2, 2 * ens.n)), STEPS, 1e-4, held_force=ControlSchedule(U, HOLD), control=U, control_hold=HOLD)
    with pytest.raises(ValueError, match="held_force"):
        ens.rollout_implicit(np.zeros((2, 2 * ens.n)), STEPS, 1e-4, control=U, control_hold=HOLD, held_force=U[0])
    assert ens.time == 0.0 and float(ens.state.abs().max()) == 0.0


# ------------------------------------------------------------------ 10. full size, once
def test_full_size_4096_beams_of_256_elements():
    cols = nitinol_columns(256, "nonlinear")
    nb, steps, k_int, hold, h = 4096, 8, 4, 2, 1e-4
    fp = force_params(True, False)
    ens = BeamEnsemble(cols, nb, force_params=fp)
    rng = np.random.default_rng(10)
    ens.zero_state()
    ens.step_implicit(10, h, impulse_amp=np.linspace(0.1, 0.5, nb), t0=0.0)
    X = ens.unpack_state().cpu().numpy()
    amps = np.linspace(0.1, 0.5, nb)
    U = np.where((ens.free_index % 3 == 1)[None, None], rng.normal(0.0, 0.05, (k_int, nb, ens.n)), 0.0)
    lam = rng.normal(0.0, 1.0, (nb, 2 * ens.n))
    kw = dict(n_iter=2, t0=0.0)
    ens.set_state(X, 0.0)
    ens.step_implicit(steps, h, control=U, control_hold=hold, impulse_amp=amps, n_iter=2)
    xT = ens.unpack_state()
    xb, ab, cb = ens.step_implicit_adjoint(steps, h, lam, x0_red=X, impulse_amp=amps, held_force=ControlSchedule(U, hold), **kw)
    assert all(bool(torch.isfinite(t).all()) for t in (xT, xb, ab, cb))
    pick = [0, 2047, 4095]
    small = BeamEnsemble(cols, 3, force_params=fp)
    small.set_state(X[pick], 0.0)
    small.step_implicit(steps, h, control=U[:, pick], control_hold=hold, impulse_amp=amps[pick], n_iter=2)
    sx, sa, sc = small.step_implicit_adjoint(steps, h, lam[pick], x0_red=X[pick], impulse_amp=amps[pick],
                                             held_force=ControlSchedule(U[:, pick], hold), **kw)
    assert float(sc.abs().max()) > 0.0
    assert torch.equal(xT[pick], small.unpack_state())
    assert torch.equal(cb[:, pick], sc) and torch.equal(xb[pick], sx) and torch.equal(ab[pick], sa)
