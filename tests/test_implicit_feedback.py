"""Sampled-data state feedback inside the implicit stepper (BeamEnsemble.step_implicit_feedback / crb_step_implicit_feedback) on
the GPU, on the smallest shapes at which each path can go wrong (the case table, the inputs and the oracle's chain are those
of tests/test_implicit_feedback_cpu.py, which proves them on the oracle alone).

What is asserted is derived, not measured:
  1. the call is bitwise replayed by step_implicit with the returned control as a schedule (general implicit kernel on both
     sides: CRB_DISABLE_LEAN_IMPLICIT=1) -- state, clock, samples, status: the step arithmetic, the sample boundaries, the
     iterate reset and the layout of u_out;
  2. every u_k is f_held + K (r - x_k) of the recorded x_k within the any-order summation bound
     (2n + 2) 2^-53 (|f_held| + |K| |r - x_k|), whichever unit formed the product (LDS, matrix cores, GEMM);
  3. the final state is the oracle's chain within the suite's forward bound, 1e-7 per DOF block;
  4. the in-kernel form and the forced chain agree within what two controls inside bound 2 can differ by, propagated as the
     CPU file measures on the oracle (a tenth of 1e-7 per bound);
  5. the edges; 6. the digital LQR loop of tests/test_implicit_tangent.py in one call.
Every in-kernel case also runs as a chain (CRB_IMPLICIT_FEEDBACK=0)."""
import functools

import numpy as np
import pytest
import torch

from continuum_robot import _native as nat
from continuum_robot.batched import BeamEnsemble, ControlSchedule
from tests.helpers import assert_blocks, block_errs, nitinol_columns
from tests.test_implicit_feedback_cpu import (B, CASES, EPS, GPU_BOUND, H, HOLD, IN_KERNEL, N_ITER, N_SAMPLES, STEPS, clock, inputs,
                                              reference)
from tests.test_tangent_linear import force_params

pytestmark = pytest.mark.gpu

# (case, form): every case as the library chooses, every in-kernel case also as a forced chain
RUNS = [(name, "chosen") for name in CASES] + [(name, "chain") for name in IN_KERNEL]


def run_id(r):
    return f"{r[0]}-{r[1]}"


def np_(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def ensemble(name):
    cols, fp, (slots, threads, packed) = CASES[name][0]
    ens = BeamEnsemble(cols, B, force_params=fp)
    lay = ens.plan.layout
    assert (lay.n_slots, lay.threads, lay.beams_per_group > 1) == (slots, threads, packed), name
    assert not ens.mixed_topology and ens.n == inputs(name).n
    return ens


def select(monkeypatch, name, form):
    """the form of the call: as chosen (asserted against the case table) or the forced chain"""
    ens = ensemble(name)
    monkeypatch.delenv("CRB_IMPLICIT_FEEDBACK", raising=False)
    assert ens.implicit_feedback_path() == ("in-kernel" if CASES[name][1] else "chain"), name
    if form == "chain":
        monkeypatch.setenv("CRB_IMPLICIT_FEEDBACK", "0")
        assert ens.implicit_feedback_path() == "chain"
    return ens, inputs(name)


def feedback(ens, inp, n_steps=STEPS, hold=HOLD, gain=None, x0=None, **kw):
    """one call from the case's start state at t = 0: (time, samples or None, control, state, status)"""
    ens.set_state(inp.X if x0 is None else x0, 0.0)
    status = ens.status
    out = ens.step_implicit_feedback(n_steps, inp.h, inp.K if gain is None else gain, reference=inp.R, hold=hold,
                                     n_iter=inp.n_iter, impulse_amp=inp.amps, impulse_duration=inp.duration,
                                     held_force=inp.f_held, return_control=True, **kw)
    samples = out[1] if len(out) == 3 else None
    return out[0], samples, out[-1], ens.state.clone(), status.clone()


def open_loop(ens, inp, n_steps, **kw):
    return ens.step_implicit(n_steps, inp.h, n_iter=inp.n_iter, impulse_amp=inp.amps, impulse_duration=inp.duration, **kw)


def control_bound(inp, xk):
    """[B, n]: bound 2 for the states xk [B, 2n]"""
    return (2 * inp.n + 2) * EPS * (np.abs(inp.f_held) + np.abs(inp.R - xk) @ np.abs(inp.K).T)


# ------------------------------------------------------------------ 1. bitwise replay
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_replay_through_the_schedule_is_bitwise(run, monkeypatch):
    monkeypatch.setenv("CRB_DISABLE_LEAN_IMPLICIT", "1")
    ens, inp = select(monkeypatch, *run)
    rec = (ens.n_elem, "w")
    t1, s1, U, x1, st1 = feedback(ens, inp, record=rec, record_every=1)
    assert U.shape == (N_SAMPLES, B, inp.n) and s1.shape == (B, STEPS)
    assert torch.isfinite(x1).all() and torch.isfinite(U).all() and float(x1.abs().max()) > 0.0
    ens.set_state(inp.X, 0.0)
    t2, s2 = open_loop(ens, inp, STEPS, control=U, control_hold=HOLD, record=rec, record_every=1)
    assert torch.equal(x1, ens.state)
    assert t1 == t2 == clock(0.0, H, STEPS)
    assert torch.equal(s1, s2)
    assert torch.equal(st1, ens.status) and int(st1.abs().max()) == 0
    # ... as a ControlSchedule, and whole-state snapshots
    _, a1, _, _, _ = feedback(ens, inp, record="all", record_every=1)
    ens.set_state(inp.X, 0.0)
    _, a2 = open_loop(ens, inp, STEPS, held_force=ControlSchedule(U, HOLD), record="all", record_every=1)
    assert torch.equal(x1, ens.state) and torch.equal(a1, a2) and a1.shape[0] == STEPS


# ------------------------------------------------------------------ 2. / 3. the control is the product; the oracle's chain
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_control_is_the_product_and_the_state_is_the_oracles(run, monkeypatch):
    ens, inp = select(monkeypatch, *run)
    _, snaps, U, x1, _ = feedback(ens, inp, record="all", record_every=HOLD)
    xk = np.concatenate([inp.X[None], np_(ens.unpack_snapshots(snaps))])[:N_SAMPLES]        # x_0, then the state after every sample
    assert xk.shape == (N_SAMPLES, B, 2 * inp.n)
    U = np_(U)
    worst = 0.0
    for k in range(N_SAMPLES):
        want = inp.f_held + (inp.R - xk[k]) @ inp.K.T
        bound = control_bound(inp, xk[k])
        err = np.abs(U[k] - want)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (run, k, float(np.max(err / bound)))
        assert np.all(np.any(U[k] != inp.f_held, axis=1)), (run, k)
    print(f"[implicit-feedback] {run_id(run)} | worst control error / bound {worst:.3f}")
    ref, Uref = reference(run[0])
    errs = assert_blocks(np_(ens.unpack_state()), ref, ens.free_index, GPU_BOUND, what=run_id(run))
    print(f"[implicit-feedback] {run_id(run)} | worst block error against the oracle's chain {max(errs.values()):.2e}")


# ------------------------------------------------------------------ 4. the two forms agree
@pytest.mark.parametrize("name", IN_KERNEL)
def test_in_kernel_form_and_chain_agree(name, monkeypatch):
    ens, inp = select(monkeypatch, name, "chosen")
    _, _, Ua, _, _ = feedback(ens, inp)
    xa = np_(ens.unpack_state())
    select(monkeypatch, name, "chain")
    _, _, Ub, _, _ = feedback(ens, inp)
    xb = np_(ens.unpack_state())
    # the first sample is taken at the same state: each control is within bound 2 of the exact product
    assert np.all(np.abs(np_(Ua)[0] - np_(Ub)[0]) <= 2.0 * control_bound(inp, inp.X))
    # perturbing every u_k by its bound moves no block by a tenth of GPU_BOUND (the CPU file, on the oracle): two bounds apart
    errs = block_errs(xa, xb, ens.free_index)
    assert max(errs.values()) <= 2.0 * 0.1 * GPU_BOUND, (name, errs)


# ------------------------------------------------------------------ 5. edges
EDGE_RUNS = [("packed_6", "chosen"), ("packed_6", "chain"), ("packed_10", "chosen"), ("one_wave_33", "chosen")]


@pytest.mark.parametrize("run", EDGE_RUNS, ids=run_id)
def test_hold_of_one_step_and_hold_beyond_the_call(run, monkeypatch):
    monkeypatch.setenv("CRB_DISABLE_LEAN_IMPLICIT", "1")
    ens, inp = select(monkeypatch, *run)
    n_steps = 6
    # hold = 1: a sample at every step -- the schedule's replay, and the oracle's chain of one-step calls
    t1, _, U, x1, _ = feedback(ens, inp, n_steps=n_steps, hold=1)
    assert U.shape[0] == n_steps
    ens.set_state(inp.X, 0.0)
    open_loop(ens, inp, n_steps, control=U, control_hold=1)
    assert torch.equal(x1, ens.state) and t1 == clock(0.0, H, n_steps)
    ref = np.stack([inp.chain(b, n_steps=n_steps, hold=1)[0] for b in range(B)])
    assert_blocks(np_(ens.unpack_state()), ref, ens.free_index, GPU_BOUND, what=run_id(run) + " hold=1")
    # hold > n_steps: one sample, one held call
    t1, _, U, x1, _ = feedback(ens, inp, n_steps=n_steps, hold=n_steps + 3)
    assert U.shape[0] == 1
    ens.set_state(inp.X, 0.0)
    t2 = open_loop(ens, inp, n_steps, held_force=U[0])
    assert torch.equal(x1, ens.state) and t1 == t2
    want = inp.f_held + (inp.R - inp.X) @ inp.K.T
    assert np.all(np.abs(np_(U[0]) - want) <= control_bound(inp, inp.X))


@pytest.mark.parametrize("run", EDGE_RUNS, ids=run_id)
def test_zero_gain_is_the_held_call_split_at_the_samples_and_no_steps_change_nothing(run, monkeypatch):
    monkeypatch.setenv("CRB_DISABLE_LEAN_IMPLICIT", "1")
    ens, inp = select(monkeypatch, *run)
    rec = (ens.n_elem, "w")
    t1, s1, U, x1, _ = feedback(ens, inp, gain=np.zeros_like(inp.K), record=rec, record_every=1)
    assert torch.equal(U, torch.as_tensor(inp.f_held, device=U.device).expand_as(U))
    ens.set_state(inp.X, 0.0)
    parts = []
    for k in range(N_SAMPLES):
        t2, sk = open_loop(ens, inp, min(HOLD, STEPS - k * HOLD), held_force=inp.f_held, record=rec, record_every=1)
        parts.append(sk)
    assert torch.equal(x1, ens.state) and t1 == t2 and torch.equal(s1, torch.cat(parts, dim=1))
    # n_steps = 0
    ens.set_state(inp.X, 0.25)
    state0 = ens.state.clone()
    t, s, U = ens.step_implicit_feedback(0, H, inp.K, reference=inp.R, hold=HOLD, held_force=inp.f_held, record=rec,
                                         return_control=True)
    assert t == 0.25 == ens.time and torch.equal(ens.state, state0) and tuple(U.shape) == (0, B, inp.n) and s.shape == (B, 0)


@pytest.mark.parametrize("run", EDGE_RUNS, ids=run_id)
def test_record_strides_that_divide_hold_or_are_multiples_of_it(run, monkeypatch):
    ens, inp = select(monkeypatch, *run)
    rec = (ens.n_elem, "w")
    _, s1, U1, x1, _ = feedback(ens, inp, record=rec, record_every=1)
    _, a1, _, _, _ = feedback(ens, inp, record="all", record_every=1)
    for every in (HOLD, 2, 2 * HOLD, 3 * HOLD):
        _, s, U, x, _ = feedback(ens, inp, record=rec, record_every=every)
        assert torch.equal(x, x1) and torch.equal(U, U1)
        assert s.shape == (B, STEPS // every) and torch.equal(s, s1[:, every - 1::every])
        _, a, _, x, _ = feedback(ens, inp, record="all", record_every=every)
        assert torch.equal(x, x1) and a.shape[0] == STEPS // every and torch.equal(a, a1[every - 1::every])
    with pytest.raises(nat.NativeError, match="record stride") as e:
        feedback(ens, inp, record=rec, record_every=3)
    assert e.value.code == nat.CRB_EINVAL
    # a stride beyond the call records nothing
    _, s, _, x, _ = feedback(ens, inp, record=rec, record_every=8 * HOLD)
    assert torch.equal(x, x1) and s.shape == (B, 0)


@pytest.mark.parametrize("run", [("packed_6", "chosen"), ("packed_6", "chain"), ("packed_10", "chosen"), ("packed_10", "chain")],
                         ids=run_id)
def test_a_nan_in_one_beams_start_state_stays_in_that_beam(run, monkeypatch):
    ens, inp = select(monkeypatch, *run)
    _, _, U1, x1, st1 = feedback(ens, inp)
    bad = inp.X.copy()
    bad[1, inp.n + 1] = float("nan")
    _, _, U2, x2, st2 = feedback(ens, inp, x0=bad)
    keep = [0, 2]
    assert torch.equal(x1[keep], x2[keep]) and torch.equal(U1[:, keep], U2[:, keep])
    assert torch.isfinite(x2[keep]).all() and not torch.isfinite(x2[1]).all() and not torch.isfinite(U2[:, 1]).all()
    assert int(st1.abs().max()) == 0
    assert st2.tolist() == [0, STEPS, 0]           # marked with the ensemble's step count at the end of the call


def test_ensembles_of_mixed_topology_are_refused():
    ens = BeamEnsemble([nitinol_columns(6, "nonlinear"), nitinol_columns(9, "nonlinear")], 2, force_params=force_params(True, False))
    assert ens.mixed_topology and ens.implicit_feedback_path() == "chain"
    ens.zero_state()
    state0 = ens.state.clone()
    with pytest.raises(nat.NativeError, match="crb_step_implicit_feedback") as e:
        ens.step_implicit_feedback(4, H, np.zeros((ens.n, 2 * ens.n)))
    assert e.value.code == nat.CRB_EUNSUPPORTED and "one free-DOF set" in str(e.value)
    assert torch.equal(ens.state, state0) and ens.time == 0.0


# ------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("form", ["chosen", "chain"])
def test_digital_lqr_loop_in_one_call_follows_the_recursion(form, monkeypatch):
    """The loop of tests/test_implicit_tangent.py::test_digital_lqr_on_the_linearisation_closes_the_loop_the_recursion_predicts
    (6 linear elements, h = 1e-3, 50 samples, the gain of the discrete Riccati equation on the linearisation) in ONE call,
    against the recursion x <- (A_d - B_d K) x under that test's allowance: the one call differs from its host loop only by the
    rounding of K x."""
    scipy_linalg = pytest.importorskip("scipy.linalg")
    from tests.test_implicit_tangent import allowed

    monkeypatch.delenv("CRB_IMPLICIT_FEEDBACK", raising=False)
    if form == "chain":
        monkeypatch.setenv("CRB_IMPLICIT_FEEDBACK", "0")
    h, samples, nb = 1e-3, 50, 4
    ens = BeamEnsemble(nitinol_columns(6, "linear"), nb, force_params=force_params(False, False))
    assert ens.implicit_feedback_path() == ("in-kernel" if form == "chosen" else "chain")
    n = ens.n
    ens.zero_state()
    Ad, Bd = (np_(t)[0] for t in ens.linearize_implicit(h, n_iter=1))
    Q = np.eye(2 * n)
    Q[:n, :n] *= 100.0
    Q[n:, n:] *= 10.0
    R = np.eye(n)
    P = scipy_linalg.solve_discrete_are(Ad, Bd, Q, R)
    K = np.linalg.solve(R + Bd.T @ P @ Bd, Bd.T @ P @ Ad)
    Acl = Ad - Bd @ K
    assert np.max(np.abs(np.linalg.eigvals(Acl))) < 1.0
    x0 = 1e-3 * np.random.default_rng(8).normal(0.0, 1.0, (nb, 2 * n))
    ens.set_state(x0, 0.0)
    t, snaps, U = ens.step_implicit_feedback(samples, h, K, hold=1, n_iter=1, record="all", record_every=1, return_control=True)
    got = np_(ens.unpack_snapshots(snaps))
    assert t == clock(0.0, h, samples) and U.shape == (samples, nb, n)
    want, worst = x0.copy(), 0.0
    for k in range(samples):
        want = want @ Acl.T
        worst = max(worst, max(block_errs(got[k], want, ens.free_index).values()))
    assert worst <= allowed("closed loop 50 samples", worst), worst
    open_end = x0.copy()
    for _ in range(samples):
        open_end = open_end @ Ad.T
    tip = n - 2
    closed_tip, open_tip = np.abs(got[-1][:, tip]), np.abs(open_end[:, tip])
    assert np.all(np.isfinite(closed_tip)) and np.max(closed_tip) < np.max(open_tip)
    assert np.linalg.norm(got[-1]) < np.linalg.norm(open_end)
