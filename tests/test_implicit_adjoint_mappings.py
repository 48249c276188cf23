"""The implicit stepper's adjoint (BeamEnsemble.step_implicit_adjoint / rollout_implicit, crb_implicit_adjoint.h) on every thread
mapping it accepts and on the input edges it owns.  The case table, the inputs and the oracle's differences come from
tests/test_implicit_adjoint_mappings_cpu.py, which proves them well conditioned before any kernel is compared.

  1. entry by entry: unit cotangents on every free DOF of the probe nodes (root, wave seams, last valid slot, pins, tip; every
     node of the two small rods), all in one call; row d dotted with a direction against entry r_d of the oracle's
     central-difference tangent, per DOF block of the probe entries under fd_check's rule; held force likewise; the amplitude
     by fd_scalar against the block-normalised oracle tangent.  Every comparison prints
     ``[implicit-adjoint-map] case beam | what | block | err | allowed | self`` (pytest -s).
  2. whole-state snapshot cotangents and a recorded rate component, against the oracle; junk off the free entries; autograd.
  3. the impulse window on and one ulp past a step's midpoint, on the first midpoint, beyond the end, with the step first and
     last in its checkpoint segment, from a clock that does not start at 0.
  4. heterogeneous ensembles across mappings (with a graded member), bitwise independence of checkpoints and batching.
  5. the forward pass against step_implicit (lean and general kernels) and the oracle on every mapping.
  6. the cache of A's tables across other step sizes; n_iter = 16, one step, record_every and checkpoint_every > n_steps.

Nonlinear rods get transverse impulses and held loads only (the note at the head of test_derivative_mappings.py)."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from tests.helpers import assert_blocks, block_errs, graded_columns, nitinol_columns
from tests.test_adjoint import fd_scalar, np_
from tests.test_derivative_mappings import clock, free_mask, to_device_layout
from tests.test_implicit_adjoint import FD_EVERY, FD_STEPS, FD_WEIGHTS, fd_inputs
from tests.test_implicit_adjoint_mappings_cpu import (AMP_STEP, CASES, CKPT, EDGES, K_EDGE, RATE_CASE, RATE_NODE, SNAP_EVERY,
                                                      SNAPSHOT_CASES, STATE_STEP, T0, TAG, WINDOW_CASES, WINDOW_CKPT, case_columns,
                                                      checked_beams, inputs, mixed, pinned_root, probe_blocks, scalar_figures,
                                                      snapshot_loss)
from tests.test_tangent_linear import directions, fd_check, force_params

pytestmark = pytest.mark.gpu


class Setup:
    """A case of the table on the GPU: the ensemble with its plan layout asserted, and the inputs of every beam"""

    def __init__(self, name):
        c = self.c = CASES[name]
        self.name = name
        self.ens = ens = BeamEnsemble(case_columns(c), c["B"], force_params=force_params(True, True), corrected_axial=c["corrected"])
        lay = ens.plan.layout
        assert (lay.n_slots, lay.beams_per_group, lay.threads) == c["layout"], name
        self.beams = [inputs(name, b) for b in range(c["B"])]
        i0 = self.beams[0]
        assert ens.n == i0.n and np.array_equal(ens.free_index, i0.fi)
        self.n, self.B, self.h, self.n_iter, self.steps = ens.n, c["B"], c["h"], c["n_iter"], c["steps"]
        self.X = np.stack([i.X for i in self.beams])
        self.U = np.stack([i.U for i in self.beams])
        self.amps = np.array([i.amp for i in self.beams])
        self.kw = dict(n_iter=self.n_iter, impulse_duration=i0.duration, impulse_index=i0.idx, t0=T0)

    def adjoint(self, lam, **over):
        kw = dict(self.kw, x0_red=self.X, impulse_amp=self.amps, held_force=self.U, checkpoint_every=CKPT)
        kw.update(over)
        return self.ens.step_implicit_adjoint(self.steps, self.h, lam, **kw)

    def rollout(self, x0, amp, held, **over):
        kw = dict(self.kw, impulse_amp=amp, held_force=held, checkpoint_every=CKPT)
        kw.update(over)
        return self.ens.rollout_implicit(x0, self.steps, self.h, **kw)

    def leaves(self):
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=self.ens.device, requires_grad=True)   # noqa: E731
        return t(self.X), t(self.amps), t(self.U)


def scalar_check(g, L, e, what):
    """fd_scalar with its figures printed first (L memoises: nothing is computed twice)"""
    err, allowed, self_err = scalar_figures(g, L, e)
    print(f"{TAG} {what} | scalar | err {err:.2e} | allowed {allowed:.2e} | self {self_err:.2e}")
    fd_scalar(g, L, e, what)


# ---- 1. entry by entry
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_entry_by_entry_at_the_probes(name):
    k = Setup(name)
    c, i0 = k.c, k.beams[0]
    probes = i0.probes
    D = probes.size
    lam = np.zeros((D + 1, k.B, 2 * k.n))
    lam[np.arange(D), :, probes] = 1.0               # e_r for every free reduced DOF r of the probe nodes, both planes
    for b in checked_beams(c):
        lam[D, b] = k.beams[b].amp_cotangent()       # and the block-normalised amplitude tangent of the oracle
    xb, ab, fb = (np_(t) for t in k.adjoint(lam))
    for b in checked_beams(c):
        i = k.beams[b]
        for kind, dirs, rows in (("state", i.state_dirs, xb[:D, b]), ("held", i.held_dirs, fb[:D, b])):
            for kd, (label, v) in enumerate(dirs):
                fd1, fd4 = i.differences(kind, kd)
                got = rows @ v                       # entry d: <row d, direction> = (J direction)[r_d]
                probe_blocks(i, got, fd1, fd4, f"{kind} {label}")
                if c["full"] and kind == "state":    # all 2n entries are probes: the whole column, under fd_check itself
                    fd_check(got, lambda e, kd=kd: i.perturbed("state", kd, e), i.step_of("state"), i.fi, f"{name} beam {b} {label}")
        scalar_check(float(ab[D, b]) * i.amp, lambda e: float(lam[D, b] @ i.perturbed("amp", 0, e)), AMP_STEP,
                     f"{name} beam {b} | amplitude")
    if c["full"]:
        assert D == 2 * k.n and len(i0.state_dirs) == 2 * k.n


# ---- 2. snapshot cotangents (record="all") and a recorded rate component
def snapshot_cotangents(k, rate_node):
    losses = [snapshot_loss(k.name, b, rate_node) for b in range(k.B)]
    lam = np.stack([s.lam for s in losses])
    C_red = np.stack([s.C for s in losses], axis=1)                                          # [n_s, B, 2n]
    return losses, lam, C_red


@pytest.mark.parametrize("name", SNAPSHOT_CASES)
def test_snapshot_cotangents(name):
    k = Setup(name)
    ens = k.ens
    losses, lam, C_red = snapshot_cotangents(k, None)
    n_s = C_red.shape[0]
    assert n_s == k.steps // SNAP_EVERY
    C = np.stack([to_device_layout(ens, C_red[j]) for j in range(n_s)])                      # [n_s, B, 2, n_node, 4]
    run = lambda cot: k.adjoint(lam, record="all", record_every=SNAP_EVERY, lam_record=cot)  # noqa: E731
    xb, ab, fb = run(C)
    for b in checked_beams(k.c):
        s = losses[b]
        for kind in ("state", "held", "amp"):
            g = s.gradient_along(kind, np_(xb)[b], np_(ab)[b], np_(fb)[b])
            scalar_check(g, lambda e, kind=kind: s.loss(kind, e), STATE_STEP if kind == "state" else s.i.step_of(kind),
                         f"{name} beam {b} | snapshots {kind}")
    # junk on the 4th component and on every constrained DOF: no effect
    mask = free_mask(ens)
    assert np.all(C[:, ~mask] == 0.0)
    rng = np.random.default_rng(3)
    junk = np.where(mask[None], 0.0, rng.normal(0.0, 1.0, C.shape) * np.max(np.abs(C)))
    assert np.count_nonzero(junk) > 0
    for r, g in zip((xb, ab, fb), run(C + junk)):
        assert torch.equal(r, g)
    # rollout_implicit(record="all") under loss.backward() is step_implicit_adjoint, bitwise
    x0, amp, held = k.leaves()
    xT, samples = k.rollout(x0, amp, held, record="all", record_every=SNAP_EVERY)
    assert tuple(samples.shape) == (n_s, k.B, 2, ens.n_node, 4)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device=ens.device)   # noqa: E731
    ((xT * dev(lam)).sum() + (samples * dev(C)).sum()).backward()
    assert torch.equal(x0.grad, xb) and torch.equal(amp.grad, ab) and torch.equal(held.grad, fb)
    assert float(xb.abs().max()) > 0 and float(ab.abs().max()) > 0 and float(fb.abs().max()) > 0


def test_recorded_rate_component_in_another_wave():
    k = Setup(RATE_CASE)
    losses, lam, _ = snapshot_cotangents(k, RATE_NODE)
    c_rec = np.stack([s.c for s in losses])                                                   # [B, n_s]
    record = dict(record=(RATE_NODE, "dw_dt"), record_every=SNAP_EVERY)
    xb, ab, fb = k.adjoint(lam, lam_record=c_rec, **record)
    for b in checked_beams(k.c):
        s = losses[b]
        assert s.rec_idx == k.n + k.ens.reduced_index(RATE_NODE, "w")
        for kind in ("state", "held", "amp"):
            g = s.gradient_along(kind, np_(xb)[b], np_(ab)[b], np_(fb)[b])
            scalar_check(g, lambda e, kind=kind: s.loss(kind, e), STATE_STEP if kind == "state" else s.i.step_of(kind),
                         f"{RATE_CASE} beam {b} | dw_dt of node {RATE_NODE} {kind}")
    x0, amp, held = k.leaves()
    xT, samples = k.rollout(x0, amp, held, **record)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device=k.ens.device)   # noqa: E731
    ((xT * dev(lam)).sum() + (samples * dev(c_rec)).sum()).backward()
    assert torch.equal(x0.grad, xb) and torch.equal(amp.grad, ab) and torch.equal(held.grad, fb)
    want = np.stack([[s.i.run(steps=t)[s.rec_idx] for t in s.times] for s in losses])
    assert np.max(np.abs(np_(samples) - want)) <= 1e-7 * np.max(np.abs(want))


# ---- 3. the impulse window against the midpoint clock
@pytest.mark.parametrize("segment", list(WINDOW_CKPT))
@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("name", WINDOW_CASES)
def test_impulse_window_edges(name, edge, segment):
    k = Setup(name)
    ens, ce = k.ens, WINDOW_CKPT[segment]
    dur = float(EDGES[edge](k.h, k.steps))
    closed = edge == "on_the_first_midpoint"
    if edge.endswith("the_midpoint"):     # the midpoint of step K as the kernel forms it: the clock after K additions, plus h / 2
        assert (clock(T0, k.h, K_EDGE) + 0.5 * k.h < dur) == (edge == "one_ulp_past_the_midpoint")
    rng = np.random.default_rng(6)
    lam = directions(k.X, rng, 1, ens.free_index)[0]
    if not closed:
        for b in checked_beams(k.c):
            lam[b] = k.beams[b].amp_cotangent(duration=dur)
    _, ab, _ = k.adjoint(lam, impulse_duration=dur, checkpoint_every=ce)
    if closed:
        assert float(ab.abs().max()) == 0.0
    else:
        for b in checked_beams(k.c):
            i = k.beams[b]
            scalar_check(float(np_(ab)[b]) * i.amp, lambda e: float(lam[b] @ i.perturbed("amp", 0, e, duration=dur)), AMP_STEP,
                         f"{name} beam {b} | window {edge} {segment}")
    x0, amp, held = k.leaves()
    xT = k.rollout(x0, amp, held, impulse_duration=dur, checkpoint_every=ce)
    (xT * torch.tensor(lam, dtype=torch.float64, device=ens.device)).sum().backward()
    assert torch.equal(amp.grad, ab)


# ---- 4. heterogeneous ensembles whose members run three mappings; with a graded member
HET_H, HET_STEPS, HET_CKPT = 2e-4, 25, 10


def hetero(graded):
    sets = [nitinol_columns(6, "nonlinear"), nitinol_columns(100, "nonlinear", bcs=pinned_root(100)), nitinol_columns(200, mixed(200))]
    fps = [force_params(True, True), force_params(False, True), force_params(True, False)]
    layouts = [(10, 64), (1, 128), (1, 256)]
    if graded:
        sets.append(graded_columns(100, "nonlinear", "allcols"))
        fps.append(force_params(True, True))
        layouts.append((1, 128))
    ens = BeamEnsemble.from_dataframes(sets, force_params=fps)
    assert ens.mixed_topology
    singles = [BeamEnsemble(s, 1, force_params=f) for s, f in zip(sets, fps)]
    assert [(int(s.plan.beams_per_group), int(s.plan.threads)) for s in singles] == layouts
    rng = np.random.default_rng(9 + graded)
    amps = np.array([0.1, 0.2, 0.3, 0.02])[:len(sets)]
    states = []
    for b, s in enumerate(singles):      # (the default impulse index: each beam's own tip w, a different node per beam)
        s.zero_state()
        s.step_implicit(20, HET_H, impulse_amp=amps[b:b + 1], t0=0.0)
        states.append(s.unpack_state().cpu().numpy()[0])
    lams = [directions(x[None], rng, 1, s.free_index)[0, 0] for x, s in zip(states, singles)]
    helds = [np.where(s.free_index % 3 == 1, rng.normal(0.0, 0.01, s.n), 0.0) for s in singles]
    H = np.zeros((len(sets), ens.n))
    for b, u in enumerate(helds):
        H[b, :u.size] = u
    return ens, singles, amps, states, lams, helds, H


@pytest.mark.parametrize("graded", [False, True])
def test_heterogeneous_ensemble_across_mappings(graded):
    ens, singles, amps, states, lams, helds, H = hetero(graded)
    kw = dict(n_iter=2, t0=T0, impulse_duration=T0 + 12.3 * HET_H, checkpoint_every=HET_CKPT)
    assert HET_STEPS % HET_CKPT != 0
    xb, ab, fb = ens.step_implicit_adjoint(HET_STEPS, HET_H, ens.pad_states(lams), x0_red=ens.pad_states(states), impulse_amp=amps,
                                           held_force=H, **kw)
    xb, ab, fb = np_(xb), np_(ab), np_(fb)
    for b, s in enumerate(singles):
        wx, wa, wf = s.step_implicit_adjoint(HET_STEPS, HET_H, lams[b][None], x0_red=states[b][None], impulse_amp=amps[b:b + 1],
                                             held_force=helds[b][None], **kw)
        wx, wa, wf = np_(wx)[0], np_(wa)[0], np_(wf)[0]
        nb = int(ens.n_per_beam[b])
        assert np.max(np.abs(wx)) > 0 and np.max(np.abs(wf)) > 0 and abs(wa) > 0
        np.testing.assert_allclose(ens.beam_state(b, xb), wx, rtol=0, atol=1e-13 * np.max(np.abs(wx)))
        np.testing.assert_allclose(fb[b, :nb], wf, rtol=0, atol=1e-13 * np.max(np.abs(wf)))
        np.testing.assert_allclose(ab[b], wa, rtol=1e-13)
        assert np.all(xb[b, nb:ens.n] == 0.0) and np.all(xb[b, ens.n + nb:] == 0.0) and np.all(fb[b, nb:] == 0.0)


def bitwise_independent(run, lam, c_rec, steps):
    """``run(lam, c_rec, checkpoint_every)``: the same bits for every checkpoint interval and for one cotangent at a time"""
    assert steps % 7 != 0
    ref = run(lam, c_rec, 1)
    for ce in (7, steps, None):
        for r, g in zip(ref, run(lam, c_rec, ce)):
            assert torch.equal(r, g), ce
    for d in range(lam.shape[0]):
        for r, g in zip(ref, run(lam[d], c_rec[d], 7)):
            assert torch.equal(r[d], g), d
    assert all(torch.isfinite(r).all() and float(r.abs().max()) > 0 for r in ref)


@pytest.mark.parametrize("n_iter", [1, 2])
def test_bitwise_independent_of_checkpoints_and_batching_on_four_waves(n_iter):
    k = Setup("four_waves_padded")
    rng = np.random.default_rng(41)
    D, every = 3, 9
    lam = directions(k.X, rng, D, k.ens.free_index)
    c_rec = rng.normal(0.0, 1.0, (D, k.B, k.steps // every))
    run = lambda lm, cr, ce: k.adjoint(lm, n_iter=n_iter, record=(70, "phi"), record_every=every, lam_record=cr,   # noqa: E731
                                       checkpoint_every=ce)
    bitwise_independent(run, lam, c_rec, k.steps)


def test_bitwise_independent_of_checkpoints_and_batching_on_a_heterogeneous_ensemble():
    ens, singles, amps, states, lams, helds, H = hetero(True)
    rng = np.random.default_rng(42)
    D, every, X = 3, 4, ens.pad_states(states)
    lam = np.stack([ens.pad_states([directions(x[None], rng, 1, s.free_index)[0, 0] for x, s in zip(states, singles)])
                    for _ in range(D)])
    c_rec = rng.normal(0.0, 1.0, (D, ens.n_beams, HET_STEPS // every))
    run = lambda lm, cr, ce: ens.step_implicit_adjoint(HET_STEPS, HET_H, lm, n_iter=2, x0_red=X, impulse_amp=amps, held_force=H,   # noqa: E731
                                                       t0=T0, impulse_duration=T0 + 12.3 * HET_H, record=(3, "w"),
                                                       record_every=every, lam_record=cr, checkpoint_every=ce)
    bitwise_independent(run, lam, c_rec, HET_STEPS)


# ---- 5. the forward pass on every mapping: against step_implicit (lean and general kernels) and against the oracle
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "general"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_step_implicit_and_the_oracle(name, lean, monkeypatch):
    if lean:
        monkeypatch.delenv("CRB_DISABLE_LEAN_IMPLICIT", raising=False)
    else:
        monkeypatch.setenv("CRB_DISABLE_LEAN_IMPLICIT", "1")
    k = Setup(name)
    ens, every = k.ens, 9
    record = dict(record=(k.c["n"], "w"), record_every=every)
    inp = dict(k.kw, impulse_amp=k.amps, held_force=k.U)
    xT, samples = ens.rollout_implicit(k.X, k.steps, k.h, **inp, **record)
    ens.set_state(k.X, T0)
    t_end, want_samples = ens.step_implicit(k.steps, k.h, **inp, **record)
    assert abs(t_end - clock(T0, k.h, k.steps)) < 1e-12
    want = ens.unpack_state().cpu().numpy()
    errs = block_errs(np_(xT), want, ens.free_index)
    rec_err = float(np.max(np.abs(np_(samples) - np_(want_samples))) / np.max(np.abs(np_(want_samples))))
    worst = 0.0
    for b in checked_beams(k.c):
        worst = max(worst, max(block_errs(np_(xT)[b], k.beams[b].run(), ens.free_index).values()))
    print(f"{TAG} {name} {'lean' if lean else 'general'} | forward | vs step_implicit {max(errs.values()):.2e} | samples {rec_err:.2e} "
          f"| vs oracle {worst:.2e} | allowed 1.00e-07")
    assert max(errs.values()) <= 1e-7, errs
    assert samples.shape == want_samples.shape == (k.B, k.steps // every) and rec_err <= 1e-7
    for b in checked_beams(k.c):     # (the bound of test_implicit_stepper_matches_oracle for this conditioning of A)
        assert_blocks(np_(xT)[b], k.beams[b].run(), ens.free_index, 1e-7, what=f"{name} beam {b} against the oracle")


# ---- 6. the cache of A's tables, and the ends of the ranges
def test_backward_after_other_step_sizes_evicted_the_tables():
    """stiff_tables keeps four sets keyed by alpha = h^2 / 4: four other step sizes between forward and backward evict the
    forward's set, and the adjoint call fetches its own again"""
    k = Setup("two_waves_padded")
    lam = torch.tensor(directions(k.X, np.random.default_rng(8), 1, k.ens.free_index)[0], dtype=torch.float64, device=k.ens.device)
    grads = []
    for interleave in (False, True):
        x0, amp, held = k.leaves()
        xT = k.rollout(x0, amp, held)
        if interleave:
            for h_other in (1e-4, 2e-4, 3e-4, 1e-3):
                assert h_other != k.h
                k.ens.zero_state()
                k.ens.step_implicit(2, h_other, n_iter=2, impulse_amp=k.amps, t0=0.0)
        (xT * lam).sum().backward()
        grads.append((x0.grad, amp.grad, held.grad))
    for r, g in zip(*grads):
        assert torch.equal(r, g) and float(r.abs().max()) > 0


def test_sixteen_iterations_match_oracle_differences():
    c = dict(n=8, kind="nonlinear", drag=True, grav=True, h=1e-4, n_iter=16)
    i = fd_inputs(c)
    ens = BeamEnsemble(i["cols"], 1, force_params=force_params(True, True))
    lam = np.zeros((1, 2 * ens.n))
    lam[0, i["tip"]] = 1.0
    kw = dict(n_iter=16, x0_red=i["X"][None], t0=0.0, record=(ens.n_elem, "w"), record_every=FD_EVERY, lam_record=FD_WEIGHTS[None],
              checkpoint_every=7)
    xb, ab, _ = ens.step_implicit_adjoint(FD_STEPS, c["h"], lam, impulse_amp=[i["amp"]], impulse_duration=i["dur"], **kw)
    _, _, fb = ens.step_implicit_adjoint(FD_STEPS, c["h"], lam, held_force=i["U"][None], **kw)
    fd_scalar(float(np_(ab)[0]) * i["amp"], i["L_amp"], 1e-3, "n_iter 16: amplitude")
    fd_scalar(float(np.sum(np_(fb)[0] * i["dU"])), i["L_held"], 1e-3, "n_iter 16: held force")
    fd_scalar(float(np.sum(np_(xb)[0] * i["dX"])), i["L_x0"], 1e-4, "n_iter 16: x0")


def test_one_step_and_intervals_beyond_the_run():
    k = Setup("packed_partial")
    rng = np.random.default_rng(15)
    lam = directions(k.X, rng, 1, k.ens.free_index)[0]
    # one step, against the oracle's differences along a dense direction
    dX = directions(k.X, rng, 1, k.ens.free_index)[0]
    xb, ab, fb = k.ens.step_implicit_adjoint(1, k.h, lam, x0_red=k.X, impulse_amp=k.amps, held_force=k.U, **k.kw)
    for b in checked_beams(k.c):
        i = k.beams[b]
        scalar_check(float(np_(xb)[b] @ dX[b]), lambda e: float(lam[b] @ i.run(x0=i.X + e * dX[b], steps=1)), STATE_STEP,
                     f"packed_partial beam {b} | one step state")
        scalar_check(float(np_(ab)[b]) * i.amp, lambda e: float(lam[b] @ i.run(amp=i.amp * (1 + e), steps=1)), AMP_STEP,
                     f"packed_partial beam {b} | one step amplitude")
    # record_every > n_steps: no sample, the gradients unchanged; checkpoint_every > n_steps: one segment
    ref = k.adjoint(lam)
    beyond = k.adjoint(lam, record=(3, "w"), record_every=k.steps + 1, lam_record=np.zeros((k.B, 0)))
    one_segment = k.adjoint(lam, checkpoint_every=k.steps + 5)
    for r, g, s in zip(ref, beyond, one_segment):
        assert torch.equal(r, g) and torch.equal(r, s) and float(r.abs().max()) > 0
    xT, samples = k.ens.rollout_implicit(k.X, k.steps, k.h, impulse_amp=k.amps, held_force=k.U, record=(3, "w"),
                                         record_every=k.steps + 1, **k.kw)
    assert tuple(samples.shape) == (k.B, 0)
    assert torch.equal(xT, k.ens.rollout_implicit(k.X, k.steps, k.h, impulse_amp=k.amps, held_force=k.U, **k.kw))
