"""Adjoint (reverse mode) on the GPU (BeamEnsemble.rhs_vjp / step_adjoint / rollout, crb_adjoint.h): dot-product identities
against the forward-mode kernels (rhs_jvp, linearize, step_tangent), the gradient of a recorded-trajectory loss against central
differences of the C oracle, autograd, bitwise determinism across checkpoint intervals and cotangent batching, side effects,
heterogeneous ensembles, the full-size ensemble and the isolation of non-finite cotangents."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from tests.helpers import nitinol_columns, oracle_beam
from tests.test_tangent_linear import RHS_CASES, directions, force_params, oracle_kw, rollout_state

pytestmark = pytest.mark.gpu

DT = 2e-5


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def dot_check(lhs_terms, rhs_terms, tol, what):
    """<lam, J v> (lhs_terms: pairs (lam, Jv)) against <J^T lam, v> (rhs_terms), relative to the cancellation-aware scale
    sum |lam_i (Jv)_i|"""
    lhs = sum(float(np.sum(np_(a) * np_(b))) for a, b in lhs_terms)
    rhs = sum(float(np.sum(np_(a) * np_(b))) for a, b in rhs_terms)
    scale = sum(float(np.sum(np.abs(np_(a) * np_(b)))) for a, b in lhs_terms)
    assert scale > 0.0, what
    err = abs(lhs - rhs) / scale
    assert err <= tol, (what, lhs, rhs, err)
    return err


def make(c, B=2):
    c = dict(c)
    corrected = c.pop("corrected", False)
    cols = nitinol_columns(c["n"], c["kind"], bcs=c.get("bcs"))
    return BeamEnsemble(cols, B, force_params=force_params(c["drag"], c["grav"]), corrected_axial=corrected), cols


# ---- 1. RHS: <lam, rhs_jvp(v)> = <rhs_vjp(lam), v>, state and input parts
@pytest.mark.parametrize("name", list(RHS_CASES))
def test_rhs_dot_product_identity(name):
    ens, _ = make(RHS_CASES[name])
    rng = np.random.default_rng(21)
    X = rollout_state(ens)
    U = rng.normal(0.0, 0.05, (2, ens.n))
    D = 3
    dX = directions(X, rng, D, ens.free_index)
    dU = rng.normal(0.0, 0.05, (D, 2, ens.n))
    _, Jv = ens.rhs_jvp(dX, X, U, dU)
    lam = directions(np_(Jv).sum(axis=0) + X, rng, D, ens.free_index)
    xb, ub = ens.rhs_vjp(lam, X, U)
    for d in range(D):
        for b in range(2):
            dot_check([(lam[d, b], np_(Jv)[d, b])], [(np_(xb)[d, b], dX[d, b]), (np_(ub)[d, b], dU[d, b])], 1e-12,
                      f"{name} cot {d} beam {b}")


# ---- 2. rhs_vjp of identity cotangents = linearize()'s A^T, Bu^T
@pytest.mark.parametrize("name", ["nonlinear_drag_grav", "pinned_root_grav", "interior_pinned_grav", "one_wave_50"])
@pytest.mark.parametrize("at", ["rest", "rollout"])
def test_rhs_vjp_is_the_transpose_of_linearize(name, at):
    ens, _ = make(RHS_CASES[name])
    X = np.zeros((2, 2 * ens.n)) if at == "rest" else rollout_state(ens)
    A, Bu = ens.linearize(X)
    n2 = 2 * ens.n
    eye = np.broadcast_to(np.eye(n2)[:, None, :], (n2, 2, n2)).copy()
    xb, ub = ens.rhs_vjp(eye, X)
    A, Bu, xb, ub = np_(A), np_(Bu), np_(xb), np_(ub)
    n = ens.n
    for b in range(2):
        got_A, got_B = xb[:, b, :], ub[:, b, :]      # row d: A[b, d, :], Bu[b, d, :]
        for r0 in (0, n):
            for c0 in (0, n):
                blk = A[b, r0:r0 + n, c0:c0 + n]
                err = np.max(np.abs(got_A[r0:r0 + n, c0:c0 + n] - blk))
                assert err <= 1e-12 * max(np.max(np.abs(blk)), 1e-300), (name, at, b, r0, c0, err)
            blk = Bu[b, r0:r0 + n]
            err = np.max(np.abs(got_B[r0:r0 + n] - blk))
            assert err <= 1e-12 * max(np.max(np.abs(blk)), 1e-300), (name, at, b, r0, err)


# ---- 3. rollout: <lam, step_tangent(v)> = <step_adjoint(lam), v>, state, amplitude and held force
@pytest.mark.parametrize("kind,drag,grav,tol", [("nonlinear", True, True, 1e-10), ("linear", False, False, 1e-12)])
def test_rollout_dot_product_identity(kind, drag, grav, tol):
    cols = nitinol_columns(32, kind)
    B, steps = 2, 200
    ens = BeamEnsemble(cols, B, force_params=force_params(drag, grav))
    rng = np.random.default_rng(31)
    X = np.zeros((B, 2 * ens.n))
    amps = np.array([0.15, 0.3])
    w = (ens.free_index % 3 == 1)[None]
    U = np.where(w, rng.normal(0.0, 0.02, (B, ens.n)), 0.0)
    ens.set_state(rollout_state(ens, 50))
    scaleX = ens.unpack_state().cpu().numpy()
    dX = directions(scaleX, rng, 1, ens.free_index)[0]
    damp = rng.normal(0.0, 1.0, B)
    dU = np.where(w, rng.normal(0.0, 0.02, (B, ens.n)), 0.0)
    ens.set_state(X)
    dT = np_(ens.step_tangent(steps, DT, dX, impulse_amp=amps, held_force=U, d_impulse_amp=damp, d_held_force=dU))
    lam = directions(dT, rng, 1, ens.free_index)[0]
    xb, ab, fb = ens.step_adjoint(steps, DT, lam, x0_red=X, impulse_amp=amps, held_force=U, t0=0.0)
    for b in range(B):
        dot_check([(lam[b], dT[b])], [(np_(xb)[b], dX[b]), (np_(ab)[b], damp[b]), (np_(fb)[b], dU[b])], tol,
                  f"{kind} beam {b}")


# ---- 4. the adjoint of 2n identity cotangents is the transposed state-transition matrix
def test_adjoint_state_transition_matrix_of_64_short_rods():
    cols = nitinol_columns(6, "nonlinear")
    B, steps = 64, 1000
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    X = rollout_state(ens)
    amps = np.linspace(0.05, 0.5, B)
    n2, n = 2 * ens.n, ens.n
    seeds = np.ascontiguousarray(np.broadcast_to(np.eye(n2)[:, None, :], (n2, B, n2)))
    ens.set_state(X)
    Phi = np_(ens.step_tangent(steps, DT, seeds, impulse_amp=amps))       # Phi[col, b, row]
    xb, _, _ = ens.step_adjoint(steps, DT, seeds, x0_red=X, impulse_amp=amps, t0=0.0)
    PhiT = np_(xb)                                                          # PhiT[row, b, col] = Phi[b][row, col]
    for b in range(B):
        want = Phi[:, b, :].T
        got = PhiT[:, b, :]
        for r0 in (0, n):
            for c0 in (0, n):
                blk = want[r0:r0 + n, c0:c0 + n]
                err = np.max(np.abs(got[r0:r0 + n, c0:c0 + n] - blk))
                assert err <= 1e-10 * max(np.max(np.abs(blk)), 1e-300), (b, r0, c0, err)


# ---- 5. the gradient of a recorded-trajectory loss against central differences of the oracle
def fd_scalar(g, L, h, what):
    fd1 = (L(h) - L(-h)) / (2 * h)
    fd4 = (L(h / 4) - L(-h / 4)) / (h / 2)
    allowed = min(max(1e-7, 4 * abs(fd1 - fd4) / abs(fd4)), 1e-6)
    err = abs(g - fd4) / abs(fd4)
    assert err <= allowed, (what, g, fd4, err, allowed)


def test_recorded_tip_loss_gradient_matches_oracle_differences():
    cols = nitinol_columns(32, "nonlinear")
    B, steps, every = 2, 200, 50
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    ob = oracle_beam(cols, **oracle_kw(True, True))
    n, tip = ens.n, ens.n - 2
    c = np.array([0.5, -1.0, 2.0, 0.25])                      # weights of the recorded tip samples (steps 50 .. 200)
    lam = np.zeros((B, 2 * n))
    lam[:, tip] = 1.0
    lam_rec = np.broadcast_to(c, (B, 4)).copy()
    X = np.zeros((B, 2 * n))
    amps = np.array([0.15, 0.3])
    rng = np.random.default_rng(5)
    w = (ens.free_index % 3 == 1)[None]
    U = np.where(w, rng.normal(0.0, 0.05, (B, n)), 0.0)
    dU = np.where(w, rng.normal(0.0, 0.05, (B, n)), 0.0)
    rec = (ens.n_elem, "w")
    _, ab, _ = ens.step_adjoint(steps, DT, lam, x0_red=X, impulse_amp=amps, t0=0.0, record=rec, record_every=every,
                                lam_record=lam_rec)
    _, _, fb = ens.step_adjoint(steps, DT, lam, x0_red=X, held_force=U, t0=0.0, record=rec, record_every=every,
                                lam_record=lam_rec)
    for b in range(B):
        def L_amp(e):
            a = amps[b] * (1 + e)
            return ob.rk4_impulse(X[b], DT, steps, a)[tip] + sum(
                c[k] * ob.rk4_impulse(X[b], DT, every * (k + 1), a)[tip] for k in range(4))

        def L_held(e):
            u = U[b] + e * dU[b]
            return ob.rk4_held(X[b], DT, steps, u)[tip] + sum(
                c[k] * ob.rk4_held(X[b], DT, every * (k + 1), u)[tip] for k in range(4))

        fd_scalar(float(np_(ab)[b]) * amps[b], L_amp, 1e-3, f"amplitude beam {b}")
        fd_scalar(float(np.sum(np_(fb)[b] * dU[b])), L_held, 1e-3, f"held force beam {b}")


# ---- 6. autograd
def test_rollout_gradcheck_and_backward():
    cols = nitinol_columns(4, "nonlinear")
    B, steps = 2, 10
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    X = rollout_state(ens, 40)
    x0 = torch.tensor(X, dtype=torch.float64, device=ens.device, requires_grad=True)
    amp = torch.tensor([0.1, 0.2], dtype=torch.float64, device=ens.device, requires_grad=True)
    held = torch.zeros((B, ens.n), dtype=torch.float64, device=ens.device)
    held[:, 1::3] = 0.01
    held.requires_grad_(True)
    f = lambda x, a, h: ens.rollout(x, steps, DT, impulse_amp=a, held_force=h)   # noqa: E731
    assert torch.autograd.gradcheck(f, (x0, amp, held), eps=1e-6)
    # loss.backward() on a recorded-tip loss = step_adjoint
    weights = torch.linspace(0.5, 2.0, 5, dtype=torch.float64, device=ens.device)
    xT, samples = ens.rollout(x0, steps, DT, impulse_amp=amp, held_force=held, record=(ens.n_elem, "w"), record_every=2)
    loss = xT[:, ens.n - 2].sum() + (samples * weights).sum()
    loss.backward()
    lam = np.zeros((B, 2 * ens.n))
    lam[:, ens.n - 2] = 1.0
    xb, ab, fb = ens.step_adjoint(steps, DT, lam, x0_red=X, impulse_amp=[0.1, 0.2], held_force=np_(held), t0=0.0,
                                  record=(ens.n_elem, "w"), record_every=2,
                                  lam_record=np_(weights)[None].repeat(B, 0))
    assert torch.equal(x0.grad, xb)
    assert torch.equal(amp.grad, ab)
    assert torch.equal(held.grad, fb)


# ---- 7. determinism: checkpoint intervals, cotangent batching, repeated calls
def test_bitwise_independent_of_checkpoint_interval_and_batching():
    cols = nitinol_columns(20, "nonlinear")
    B, steps = 3, 60
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    rng = np.random.default_rng(41)
    X = rollout_state(ens)
    lam = directions(X, rng, 3, ens.free_index)
    amps = np.array([0.1, 0.2, 0.3])
    U = rng.normal(0.0, 0.01, (B, ens.n))
    run = lambda lm, ce: ens.step_adjoint(steps, DT, lm, x0_red=X, impulse_amp=amps, held_force=U, t0=0.0,   # noqa: E731
                                          record=(ens.n_elem, "phi"), record_every=7,
                                          lam_record=np.ones((B, steps // 7)), checkpoint_every=ce)
    ref = run(lam, 1)
    for ce in (7, steps, None):
        got = run(lam, ce)
        for r, g in zip(ref, got):
            assert torch.equal(r, g), ce
    for d in range(3):
        one = run(lam[d], 7)
        for r, g in zip(ref, one):
            assert torch.equal(r[d], g), d
    again = run(lam, 1)
    for r, g in zip(ref, again):
        assert torch.equal(r, g)


# ---- 8. side effects and the forward value
def test_no_side_effects_and_rollout_matches_step():
    cols = nitinol_columns(16, "nonlinear")
    B, steps = 3, 100
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    X = rollout_state(ens)
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    lam = np.ones((B, 2 * ens.n))
    ens.step_adjoint(steps, DT, lam, impulse_amp=np.array([0.1, 0.2, 0.3]))
    xT = np_(ens.rollout(X, steps, DT, impulse_amp=np.array([0.1, 0.2, 0.3]), t0=ens.time))
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)
    ens.set_state(X, time0)
    ens.step(steps, DT, impulse_amp=np.array([0.1, 0.2, 0.3]))
    want = ens.unpack_state().cpu().numpy()
    n = ens.n
    fi = ens.free_index % 3
    for b in range(B):
        for pl in (0, n):
            for k in range(3):
                sel = pl + np.nonzero(fi == k)[0]
                if sel.size == 0:
                    continue
                scale = max(np.max(np.abs(want[b, sel])), 1e-300)
                assert np.max(np.abs(xT[b, sel] - want[b, sel])) <= 1e-12 * scale, (b, pl, k)


# ---- 9. heterogeneous ensembles
def test_heterogeneous_ensemble_matches_each_beam_alone():
    sets = [nitinol_columns(6, "nonlinear"),
            nitinol_columns(10, "linear", bcs=["PINNED"] + ["NONE"] * 9),
            nitinol_columns(8, "nonlinear", bcs=["FIXED", "NONE", "NONE", "PINNED", "NONE", "NONE", "NONE", "NONE"])]
    fps = [force_params(True, True), force_params(False, True), force_params(True, False)]
    ens = BeamEnsemble(sets, 3, force_params=fps)
    assert ens.mixed_topology
    rng = np.random.default_rng(9)
    singles = [BeamEnsemble(s, 1, force_params=f) for s, f in zip(sets, fps)]
    states = [rollout_state(s)[0] for s in singles]
    lams = [directions(x[None], rng, 1, s.free_index)[0, 0] for x, s in zip(states, singles)]
    helds = [rng.normal(0.0, 0.01, s.n) for s in singles]
    amps = np.array([0.1, 0.2, 0.3])
    X = ens.pad_states(states)
    Lm = ens.pad_states(lams)
    H = np.zeros((3, ens.n))
    for b, h in enumerate(helds):
        H[b, :h.size] = h
    xb, ab, fb = ens.step_adjoint(50, DT, Lm, x0_red=X, impulse_amp=amps, held_force=H, t0=0.0)
    xb, ab, fb = np_(xb), np_(ab), np_(fb)
    for b, s in enumerate(singles):
        wx, wa, wf = s.step_adjoint(50, DT, lams[b][None], x0_red=states[b][None], impulse_amp=amps[b:b + 1],
                                    held_force=helds[b][None], t0=0.0)
        nb = int(ens.n_per_beam[b])
        got = ens.beam_state(b, xb)
        np.testing.assert_allclose(got, np_(wx)[0], rtol=0, atol=1e-13 * np.max(np.abs(np_(wx))))
        np.testing.assert_allclose(fb[b, :nb], np_(wf)[0], rtol=0, atol=1e-13 * np.max(np.abs(np_(wf))))
        np.testing.assert_allclose(ab[b], np_(wa)[0], rtol=1e-13)
        assert np.all(xb[b, nb:ens.n] == 0.0) and np.all(xb[b, ens.n + nb:] == 0.0) and np.all(fb[b, nb:] == 0.0)
    _, ub = ens.rhs_vjp(Lm, X)
    for b in range(3):
        assert np.all(np_(ub)[b, int(ens.n_per_beam[b]):] == 0.0)


# ---- 10. full size
def test_full_size_4096_beams_of_256_elements():
    cols = nitinol_columns(256, "nonlinear")
    B, steps = 4096, 20
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    rng = np.random.default_rng(10)
    X = rollout_state(ens)
    amps = np.linspace(0.1, 0.5, B)
    dX = directions(X, rng, 1, ens.free_index)[0]
    ens.set_state(X)
    dT = np_(ens.step_tangent(steps, DT, dX, impulse_amp=amps))
    lam = directions(dT, rng, 1, ens.free_index)[0]
    xb, ab, fb = ens.step_adjoint(steps, DT, lam, x0_red=X, impulse_amp=amps, t0=0.0)
    xb, ab, fb = np_(xb), np_(ab), np_(fb)
    assert np.isfinite(xb).all() and np.isfinite(ab).all() and np.isfinite(fb).all()
    for b in (0, 2047, 4095):
        dot_check([(lam[b], dT[b])], [(xb[b], dX[b])], 1e-10, f"full size beam {b}")


# ---- 11. a non-finite cotangent stays in its beam
def test_non_finite_cotangent_stays_in_its_beam():
    for n in (6, 100):
        cols = nitinol_columns(n, "nonlinear")
        B = 12
        ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
        rng = np.random.default_rng(12)
        X = rollout_state(ens)
        lam = directions(X, rng, 2, ens.free_index)
        clean = ens.step_adjoint(30, DT, lam, x0_red=X, impulse_amp=np.full(B, 0.1), t0=0.0)
        bad = lam.copy()
        bad[1, 3, 5] = np.nan
        bad[0, 3, 1] = np.inf
        dirty = ens.step_adjoint(30, DT, bad, x0_red=X, impulse_amp=np.full(B, 0.1), t0=0.0)
        others = [b for b in range(B) if b != 3]
        for c, d in zip(clean, dirty):
            assert torch.equal(c[:, others], d[:, others])
        assert not torch.isfinite(dirty[0][1, 3]).all()
        cx, _ = ens.rhs_vjp(lam, X)
        dx, _ = ens.rhs_vjp(bad, X)
        assert torch.equal(cx[:, others], dx[:, others])
