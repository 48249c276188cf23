"""Adjoint of the implicit stepper on the GPU (BeamEnsemble.step_implicit_adjoint / rollout_implicit, crb_implicit_adjoint.h):
the transposed state-transition matrix of the linear rod against step_implicit itself, nonlinear gradients against central
differences of the oracle's `implicit`, autograd, bitwise independence of the checkpoint interval and of cotangent batching,
forward agreement with step_implicit, side effects, heterogeneous ensembles, isolation of non-finite cotangents, full size."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from tests.helpers import block_errs, nitinol_columns, oracle_beam
from tests.test_adjoint import fd_scalar, np_
from tests.test_tangent_linear import directions, force_params, oracle_kw

pytestmark = pytest.mark.gpu


def blockwise(got, want, n):
    """worst relative error over the n x n blocks of [.., rows, cols] matrices whose rows and columns come in planes of n"""
    worst = 0.0
    for r0 in range(0, want.shape[0], n):
        for c0 in range(0, want.shape[1], n):
            blk = want[r0:r0 + n, c0:c0 + n]
            worst = max(worst, float(np.max(np.abs(got[r0:r0 + n, c0:c0 + n] - blk)) / max(np.max(np.abs(blk)), 1e-300)))
    return worst


# ---- 1. the adjoint of 2n identity cotangents is the transposed state-transition matrix of step_implicit (linear rod: the
#         map is linear), and f_held_bar its response to unit held forces.
# Worst per-block relative error measured on one MI355X (40 steps, n_iter = 2), Phi^T / G^T:
STM_CASES = {
    "packed_6": dict(n=6, h=1e-4, measured=(5.96e-15, 2.82e-15)),
    "two_waves_65": dict(n=65, h=2e-4, measured=(3.16e-14, 5.49e-15)),
    "four_waves_130_padding": dict(n=130, h=5e-4, measured=(6.45e-14, 1.99e-14)),
    "all_8_levels_256": dict(n=256, h=1e-3, measured=(3.11e-13, 7.94e-14)),
    # the mappings the first four leave out (bcs: the boundary conditions; B: beams of the ensemble the adjoint runs on, every
    # one of them given the identity cotangents and compared).  The 65-slot and the 128-slot rod repeat the figures of the 65-
    # and the 130-element rods above: the worst entries sit at the free end, forty steps away from what differs at the root.
    "one_element_70_beams": dict(n=1, h=1e-4, B=70, measured=(2.58e-15, 3.47e-14)),
    "packed_pinned_10": dict(n=10, h=2e-4, bcs=["PINNED"] + ["NONE"] * 9, measured=(1.80e-14, 1.23e-14)),
    "two_waves_65_slots_pinned_64": dict(n=64, h=2e-4, bcs=["PINNED"] + ["NONE"] * 63, measured=(3.16e-14, 5.49e-15)),
    "pin_on_the_seam_128": dict(n=128, h=5e-4, bcs=["FIXED"] + ["NONE"] * 63 + ["PINNED"] + ["NONE"] * 63, measured=(6.45e-14, 1.99e-14)),
}
STM_CAP = 1e-7   # the bound test_implicit_stepper_matches_oracle uses for the same conditioning of A


@pytest.mark.parametrize("name", list(STM_CASES))
def test_adjoint_of_identity_cotangents_is_the_transposed_transition_matrix(name):
    c = STM_CASES[name]
    cols = nitinol_columns(c["n"], "linear", bcs=c.get("bcs"))
    steps, h, B = 40, c["h"], c.get("B", 1)
    one = BeamEnsemble(cols, B, force_params=force_params(False, False))
    n, n2 = one.n, 2 * one.n
    eye = np.eye(n2)
    ref = BeamEnsemble(cols, n2, force_params=force_params(False, False))
    ref.set_state(eye)
    ref.step_implicit(steps, h, n_iter=2, t0=0.0)
    Phi = ref.unpack_state().cpu().numpy().T                       # Phi[row, col]: beam `col` started from e_col
    frc = BeamEnsemble(cols, n, force_params=force_params(False, False))
    frc.zero_state()
    frc.step_implicit(steps, h, n_iter=2, held_force=np.eye(n), t0=0.0)
    G = frc.unpack_state().cpu().numpy().T                         # G[row, j]: the response to the unit held force e_j
    xb, _, fb = one.step_implicit_adjoint(steps, h, np.repeat(eye[:, None, :], B, axis=1), n_iter=2, x0_red=np.zeros((B, n2)), t0=0.0)
    # row d of beam b: Phi^T e_d = Phi[d, :], G^T e_d = G[d, :]
    e_phi = max(blockwise(np_(xb)[:, b, :], Phi, n) for b in range(B))
    e_g = max(blockwise(np_(fb)[:, b, :], G, n) for b in range(B))
    print(f"{name}: Phi^T {e_phi:.2e}  G^T {e_g:.2e}")
    for err, measured, what in ((e_phi, c["measured"][0], "Phi^T"), (e_g, c["measured"][1], "G^T")):
        assert err <= min(16.0 * measured, STM_CAP), (name, what, err)


# ---- 2. nonlinear gradients against central differences of the oracle's implicit()
FD_CASES = {
    "n8_drag_grav": dict(n=8, kind="nonlinear", drag=True, grav=True, h=1e-4, n_iter=2),
    "n32_one_iteration": dict(n=32, kind="nonlinear", drag=True, grav=True, h=2e-4, n_iter=1),
    "n32_two_iterations": dict(n=32, kind="nonlinear", drag=True, grav=True, h=2e-4, n_iter=2),
    "n64_drag_three_iterations": dict(n=64, kind="nonlinear", drag=True, grav=False, h=5e-4, n_iter=3),
    "n10_mixed_kinds": dict(n=10, kind=["linear", "nonlinear"] * 5, drag=True, grav=True, h=1e-4, n_iter=2),
    "n8_pinned_root_grav": dict(n=8, kind="nonlinear", drag=False, grav=True, h=1e-4, n_iter=2,
                                bcs=["PINNED"] + ["NONE"] * 7),
}
FD_STEPS, FD_EVERY = 40, 10
FD_WEIGHTS = np.array([0.5, -1.0, 2.0, 0.25])     # of the recorded tip samples (steps 10, 20, 30, 40)


def fd_inputs(c):
    """The oracle, the loss and the inputs of one FD case, CPU only: amp with the impulse switching off on a step boundary inside
    the run; a held force and its direction on the w DOFs; x0 = the oracle's state after 30 steps under the impulse and a
    direction scaled per DOF block by that state's own block maxima (test_tangent_linear.directions)."""
    cols = nitinol_columns(c["n"], c["kind"], bcs=c.get("bcs"))
    ob = oracle_beam(cols, **oracle_kw(c["drag"], c["grav"]))
    fi = ob.red2full()
    n = ob.n
    rng = np.random.default_rng(1000 + c["n"] + c["n_iter"])
    w = fi % 3 == 1
    inp = dict(cols=cols, ob=ob, fi=fi, n=n, tip=n - 2, amp=0.15, dur=10.0 * c["h"],
               U=np.where(w, rng.normal(0.0, 0.05, n), 0.0), dU=np.where(w, rng.normal(0.0, 0.05, n), 0.0))
    inp["X"] = ob.implicit(np.zeros(2 * n), c["h"], 30, n_iter=c["n_iter"], amp=inp["amp"], duration=inp["dur"])
    inp["dX"] = directions(inp["X"][None], rng, 1, fi)[0, 0]

    def loss(x0, amp=0.0, u=None):
        run = lambda k: ob.implicit(x0, c["h"], k, n_iter=c["n_iter"], amp=amp, duration=inp["dur"], u_held=u)[inp["tip"]]   # noqa: E731
        return run(FD_STEPS) + sum(FD_WEIGHTS[k] * run(FD_EVERY * (k + 1)) for k in range(4))

    inp["L_amp"] = lambda e: loss(inp["X"], amp=inp["amp"] * (1 + e))
    inp["L_held"] = lambda e: loss(inp["X"], u=inp["U"] + e * inp["dU"])
    inp["L_x0"] = lambda e: loss(inp["X"] + e * inp["dX"], amp=inp["amp"])
    return inp


@pytest.mark.parametrize("name", list(FD_CASES))
def test_gradients_match_central_differences_of_the_oracle(name):
    c = FD_CASES[name]
    i = fd_inputs(c)
    ens = BeamEnsemble(i["cols"], 1, force_params=force_params(c["drag"], c["grav"]))
    assert ens.n == i["n"] and np.array_equal(ens.free_index, i["fi"])
    n = ens.n
    lam = np.zeros((1, 2 * n))
    lam[0, i["tip"]] = 1.0
    kw = dict(n_iter=c["n_iter"], x0_red=i["X"][None], t0=0.0, record=(ens.n_elem, "w"), record_every=FD_EVERY,
              lam_record=FD_WEIGHTS[None], checkpoint_every=7)
    xb, ab, _ = ens.step_implicit_adjoint(FD_STEPS, c["h"], lam, impulse_amp=[i["amp"]], impulse_duration=i["dur"], **kw)
    _, _, fb = ens.step_implicit_adjoint(FD_STEPS, c["h"], lam, held_force=i["U"][None], **kw)
    fd_scalar(float(np_(ab)[0]) * i["amp"], i["L_amp"], 1e-3, f"{name}: amplitude")
    fd_scalar(float(np.sum(np_(fb)[0] * i["dU"])), i["L_held"], 1e-3, f"{name}: held force")
    fd_scalar(float(np.sum(np_(xb)[0] * i["dX"])), i["L_x0"], 1e-4, f"{name}: x0")


# ---- 3. autograd
def test_rollout_implicit_gradcheck_and_backward():
    cols = nitinol_columns(4, "nonlinear")
    B, steps, h = 2, 6, 1e-4
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    ens.zero_state()
    ens.step_implicit(40, h, impulse_amp=[0.1, 0.2], t0=0.0)
    X = ens.unpack_state().cpu().numpy()
    x0 = torch.tensor(X, dtype=torch.float64, device=ens.device, requires_grad=True)
    amp = torch.tensor([0.1, 0.2], dtype=torch.float64, device=ens.device, requires_grad=True)
    held = torch.zeros((B, ens.n), dtype=torch.float64, device=ens.device)
    held[:, 1::3] = 0.01
    held.requires_grad_(True)
    f = lambda x, a, u: ens.rollout_implicit(x, steps, h, impulse_amp=a, held_force=u, checkpoint_every=4)   # noqa: E731
    assert torch.autograd.gradcheck(f, (x0, amp, held), eps=1e-6)
    weights = torch.linspace(0.5, 2.0, 3, dtype=torch.float64, device=ens.device)
    xT, samples = ens.rollout_implicit(x0, steps, h, impulse_amp=amp, held_force=held, record=(ens.n_elem, "w"), record_every=2)
    loss = xT[:, ens.n - 2].sum() + (samples * weights).sum()
    loss.backward()
    lam = np.zeros((B, 2 * ens.n))
    lam[:, ens.n - 2] = 1.0
    xb, ab, fb = ens.step_implicit_adjoint(steps, h, lam, x0_red=X, impulse_amp=[0.1, 0.2], held_force=np_(held), t0=0.0,
                                           record=(ens.n_elem, "w"), record_every=2, lam_record=np_(weights)[None].repeat(B, 0))
    assert torch.equal(x0.grad, xb) and torch.equal(amp.grad, ab) and torch.equal(held.grad, fb)
    assert float(x0.grad.abs().max()) > 0 and float(amp.grad.abs().max()) > 0 and float(held.grad.abs().max()) > 0


# ---- 4. bitwise independence of the checkpoint interval and of cotangent batching (n_iter = 1: the carry between segments)
@pytest.mark.parametrize("n_iter", [1, 2])
def test_bitwise_independent_of_checkpoint_interval_and_batching(n_iter):
    cols = nitinol_columns(20, "nonlinear")
    B, steps, h = 3, 30, 2e-4
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    rng = np.random.default_rng(41)
    ens.zero_state()
    ens.step_implicit(20, h, impulse_amp=[0.1, 0.15, 0.2], t0=0.0)
    X = ens.unpack_state().cpu().numpy()
    lam = directions(X, rng, 3, ens.free_index)
    amps = np.array([0.1, 0.2, 0.3])
    U = rng.normal(0.0, 0.01, (B, ens.n))
    run = lambda lm, ce: ens.step_implicit_adjoint(steps, h, lm, n_iter=n_iter, x0_red=X, impulse_amp=amps, held_force=U,   # noqa: E731
                                                   t0=0.0, impulse_duration=12 * h, record=(ens.n_elem, "phi"), record_every=7,
                                                   lam_record=np.ones((B, steps // 7)), checkpoint_every=ce)
    ref = run(lam, 1)
    for ce in (7, steps, 11, None):            # (11 does not divide 30)
        for r, g in zip(ref, run(lam, ce)):
            assert torch.equal(r, g), ce
    for d in range(3):
        for r, g in zip(ref, run(lam[d], 7)):
            assert torch.equal(r[d], g), d
    assert all(torch.isfinite(r).all() and float(r.abs().max()) > 0 for r in ref)


# ---- 5. forward agreement with step_implicit, recorded samples, no side effects
def test_forward_matches_step_implicit_and_leaves_the_ensemble_alone():
    """rollout_implicit's forward against step_implicit (the lean kernel here), per DOF block: measured 3.0e-13 on one MI355X
    (recorded samples 4.0e-16), against the 1e-7 bound of test_implicit_stepper_matches_oracle"""
    cols = nitinol_columns(64, "nonlinear")
    B, steps, h = 3, 50, 2e-4
    amps = np.array([0.1, 0.2, 0.3])
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    ens.zero_state()
    ens.step_implicit(20, h, impulse_amp=amps, t0=0.0)
    X = ens.unpack_state().cpu().numpy()
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    ens.step_implicit_adjoint(steps, h, np.ones((B, 2 * ens.n)), impulse_amp=amps)
    xT, samples = ens.rollout_implicit(X, steps, h, impulse_amp=amps, t0=time0, record=(ens.n_elem, "w"), record_every=5)
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)
    _, want_samples = ens.step_implicit(steps, h, impulse_amp=amps, record=(ens.n_elem, "w"), record_every=5)
    want = ens.unpack_state().cpu().numpy()
    errs = block_errs(np_(xT), want, ens.free_index)
    worst = max(errs.values())
    rec_err = float(np.max(np.abs(np_(samples) - np_(want_samples))) / np.max(np.abs(np_(want_samples))))
    print(f"forward vs step_implicit: worst block {worst:.2e}, samples {rec_err:.2e}")
    assert worst <= 1e-7, errs
    assert samples.shape == want_samples.shape and rec_err <= 1e-7


# ---- 6. heterogeneous ensembles: each beam as alone, to the tolerance the RK4 counterpart uses (1e-13 of the largest entry:
#         the ensemble's per-beam tables are built by the same assembly, its slots sit in other lanes)
def test_heterogeneous_ensemble_matches_each_beam_alone():
    sets = [nitinol_columns(6, "nonlinear"),
            nitinol_columns(10, "linear", bcs=["PINNED"] + ["NONE"] * 9),
            nitinol_columns(8, "nonlinear", bcs=["FIXED", "NONE", "NONE", "PINNED", "NONE", "NONE", "NONE", "NONE"])]
    fps = [force_params(True, True), force_params(False, True), force_params(True, False)]
    ens = BeamEnsemble.from_dataframes(sets, force_params=fps)
    assert ens.mixed_topology
    rng = np.random.default_rng(9)
    singles = [BeamEnsemble(s, 1, force_params=f) for s, f in zip(sets, fps)]
    h, steps = 1e-4, 25
    states = []
    for s in singles:
        s.zero_state()
        s.step_implicit(20, h, impulse_amp=[0.1], t0=0.0)
        states.append(s.unpack_state().cpu().numpy()[0])
    lams = [directions(x[None], rng, 1, s.free_index)[0, 0] for x, s in zip(states, singles)]
    helds = [rng.normal(0.0, 0.01, s.n) for s in singles]
    amps = np.array([0.1, 0.2, 0.3])
    X, Lm = ens.pad_states(states), ens.pad_states(lams)
    H = np.zeros((3, ens.n))
    for b, u in enumerate(helds):
        H[b, :u.size] = u
    xb, ab, fb = ens.step_implicit_adjoint(steps, h, Lm, x0_red=X, impulse_amp=amps, held_force=H, t0=0.0, checkpoint_every=10)
    xb, ab, fb = np_(xb), np_(ab), np_(fb)
    for b, s in enumerate(singles):
        wx, wa, wf = s.step_implicit_adjoint(steps, h, lams[b][None], x0_red=states[b][None], impulse_amp=amps[b:b + 1],
                                             held_force=helds[b][None], t0=0.0, checkpoint_every=10)
        nb = int(ens.n_per_beam[b])
        np.testing.assert_allclose(ens.beam_state(b, xb), np_(wx)[0], rtol=0, atol=1e-13 * np.max(np.abs(np_(wx))))
        np.testing.assert_allclose(fb[b, :nb], np_(wf)[0], rtol=0, atol=1e-13 * np.max(np.abs(np_(wf))))
        np.testing.assert_allclose(ab[b], np_(wa)[0], rtol=1e-13)
        assert np.all(xb[b, nb:ens.n] == 0.0) and np.all(xb[b, ens.n + nb:] == 0.0) and np.all(fb[b, nb:] == 0.0)


# ---- 7. a non-finite cotangent stays in its beam (6 elements: ten beams share a wave)
def test_non_finite_cotangent_stays_in_its_beam():
    for n in (6, 100):
        cols = nitinol_columns(n, "nonlinear")
        B, h = 12, 1e-4
        ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
        rng = np.random.default_rng(12)
        ens.zero_state()
        ens.step_implicit(20, h, impulse_amp=np.linspace(0.1, 0.2, B), t0=0.0)
        X = ens.unpack_state().cpu().numpy()
        lam = directions(X, rng, 2, ens.free_index)
        run = lambda lm: ens.step_implicit_adjoint(15, h, lm, x0_red=X, impulse_amp=np.full(B, 0.1), t0=0.0, checkpoint_every=6)  # noqa: E731
        clean = run(lam)
        bad = lam.copy()
        bad[1, 3, 5] = np.nan
        bad[0, 3, 1] = np.inf
        dirty = run(bad)
        others = [b for b in range(B) if b != 3]
        for c, d in zip(clean, dirty):
            assert torch.equal(c[:, others], d[:, others])
        assert not torch.isfinite(dirty[0][1, 3]).all()


# ---- 8. full size
def test_full_size_4096_beams_of_256_elements():
    cols = nitinol_columns(256, "nonlinear")
    B, steps, h = 4096, 20, 1e-4
    fp = force_params(True, False)
    ens = BeamEnsemble(cols, B, force_params=fp)
    amps = np.linspace(0.1, 0.5, B)
    ens.zero_state()
    ens.step_implicit(20, h, impulse_amp=amps, t0=0.0)
    X = ens.unpack_state().cpu().numpy()
    rng = np.random.default_rng(10)
    lam = directions(X, rng, 1, ens.free_index)[0]
    xb, ab, fb = ens.step_implicit_adjoint(steps, h, lam, x0_red=X, impulse_amp=amps, t0=0.0)
    assert torch.isfinite(xb).all() and torch.isfinite(ab).all() and torch.isfinite(fb).all()
    pick = [0, 2047, 4095]
    small = BeamEnsemble(cols, 3, force_params=fp)
    sx, sa, sf = small.step_implicit_adjoint(steps, h, lam[pick], x0_red=X[pick], impulse_amp=amps[pick], t0=0.0)
    assert torch.equal(xb[pick], sx) and torch.equal(ab[pick], sa) and torch.equal(fb[pick], sf)
    assert float(sx.abs().max()) > 0
