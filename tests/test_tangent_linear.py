"""Tangent-linear model on the GPU (BeamEnsemble.rhs_jvp / linearize / step_tangent, crb_tangent.h): forward-mode derivatives
of the right-hand side and of the fused RK4 rollout, checked against central differences of the C oracle (rhs, rk4_impulse,
rk4_held), the reference's LQR state space, the tangent stiffness kernel and the plain stepper."""
import numpy as np
import pytest
import torch

from continuum_robot import _native as nat
from continuum_robot.batched import BeamEnsemble
from continuum_robot.control.linear_quadratic_regulator import LinearQuadraticRegulator
from continuum_robot.models.force_params import ForceParams
from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu


def force_params(drag, grav):
    return ForceParams(fluid_density=1000.0 if drag else 0.0, enable_fluid_effects=drag, enable_gravity_effects=grav)


def oracle_kw(drag, grav):
    return dict(fluid_density=1000.0 if drag else 0.0, enable_fluid=drag, enable_gravity=grav)


def bent_state(ens, rng, amp=2e-2):
    """[B, 2n]: a smooth bend (w ~ amp s^2, phi = dw/ds, u ~ 1e-6 amp s), beam by beam a little different, velocities zero"""
    fi = ens.free_index
    node, dof = fi // 3, fi % 3
    s = node / ens.n_elem
    X = np.zeros((ens.n_beams, 2 * ens.n))
    for b in range(ens.n_beams):
        a = amp * (1.0 + 0.3 * rng.uniform(-1, 1))
        L = 0.25 * ens.n_elem
        X[b, :ens.n] = np.where(dof == 1, a * s**2, np.where(dof == 2, 2 * a * s / L, 1e-6 * a * s))
    return X


def directions(X, rng, D, fi):
    """[D, B, 2n] random directions scaled per DOF block of X (each block by its largest entry, floor 1e-12 of its plane), so
    that every block is exercised at its own size"""
    B, n2 = X.shape
    n = n2 // 2
    dof = np.concatenate([fi % 3] * 2)
    S = np.empty_like(X)
    for b in range(B):
        for pl in range(2):
            sl = np.zeros(n2, bool)
            sl[pl * n:(pl + 1) * n] = True
            pmax = np.max(np.abs(X[b, sl]))
            for k in range(3):
                sel = sl & (dof == k)
                if sel.any():
                    S[b, sel] = max(np.max(np.abs(X[b, sel])), 1e-12 * pmax, 1e-300)
    return rng.normal(0.0, 1.0, (D, B, n2)) * S[None]


def fd_check(jvp, F, h, free_index, what):
    """|JVP - FD(h/4)| <= max(1e-7, 4 |FD(h) - FD(h/4)|) per DOF block (relative to the block, helpers.block_errs), never
    more than the 1e-6 bar.  F(e) = the function at the point + e * direction."""
    fd1 = (F(h) - F(-h)) / (2 * h)
    fd4 = (F(h / 4) - F(-h / 4)) / (h / 2)
    e_fd = block_errs(fd1, fd4, free_index)
    e_jvp = block_errs(jvp, fd4, free_index)
    for k, e in e_jvp.items():
        allowed = min(max(1e-7, 4 * e_fd[k]), 1e-6)
        assert e <= allowed, (what, k, e, allowed, e_jvp, e_fd)
    assert_blocks(jvp, fd4, free_index, min(max(1e-7, 4 * max(e_fd.values())), 1e-6), what=what)
    return e_jvp


def rollout_state(ens, steps=20):
    """[B, 2n]: the state of a short rollout from rest under the examples' tip impulse (non-zero velocities: drag is
    exercised).  (Bent initial shapes are no start for a dynamic test: the shipped nonlinear element, segments.py:178-208,
    lets their axial DOFs run away within a few hundred steps -- SURVEY App. B-1.)"""
    ens.zero_state()
    ens.step(steps, 2e-5, impulse_amp=np.linspace(0.1, 0.2, ens.n_beams))
    return ens.unpack_state().cpu().numpy()


RHS_CASES = {
    "linear_fixed": dict(n=6, kind="linear", drag=False, grav=False),
    "linear_drag_grav": dict(n=6, kind="linear", drag=True, grav=True),
    "nonlinear_fixed": dict(n=6, kind="nonlinear", drag=False, grav=False),
    "nonlinear_drag_grav": dict(n=6, kind="nonlinear", drag=True, grav=True),
    "corrected_drag_grav": dict(n=6, kind="nonlinear", drag=True, grav=True, corrected=True),
    "pinned_root_grav": dict(n=6, kind="nonlinear", drag=True, grav=True, bcs=["PINNED"] + ["NONE"] * 5),
    "interior_pinned_grav": dict(n=8, kind="nonlinear", drag=True, grav=True,
                                 bcs=["FIXED", "NONE", "NONE", "PINNED", "NONE", "NONE", "NONE", "NONE"]),
    "one_wave_50": dict(n=50, kind="nonlinear", drag=True, grav=True),
    "two_waves_100_pinned_root": dict(n=100, kind="nonlinear", drag=True, grav=True, bcs=["PINNED"] + ["NONE"] * 99),
    "four_waves_200": dict(n=200, kind=["linear", "nonlinear"] * 100, drag=True, grav=True),
}


@pytest.mark.parametrize("name", list(RHS_CASES))
def test_rhs_jvp_matches_finite_differences_of_the_oracle(name):
    c = dict(RHS_CASES[name])
    corrected = c.pop("corrected", False)
    cols = nitinol_columns(c["n"], c["kind"], bcs=c.get("bcs"))
    B, D = 2, 2
    ens = BeamEnsemble(cols, B, force_params=force_params(c["drag"], c["grav"]), corrected_axial=corrected)
    ob = oracle_beam(cols, corrected_axial=corrected, **oracle_kw(c["drag"], c["grav"]))
    rng = np.random.default_rng(7)
    X = rollout_state(ens)
    assert np.max(np.abs(X[:, ens.n:])) > 0.0
    U = rng.normal(0.0, 0.05, (B, ens.n))
    dX = directions(X, rng, D, ens.free_index)
    dU = rng.normal(0.0, 0.05, (D, B, ens.n))
    xdot, dxdot = ens.rhs_jvp(dX, X, U, dU)
    xdot, dxdot = xdot.cpu().numpy(), dxdot.cpu().numpy()
    for b in range(B):
        assert_blocks(xdot[b], ob.rhs(X[b], U[b]), ens.free_index, 1e-10, what=f"{name} xdot")
        for d in range(D):
            F = lambda e: ob.rhs(X[b] + e * dX[d, b], U[b] + e * dU[d, b])   # noqa: E731
            fd_check(dxdot[d, b], F, 1e-4, ens.free_index, f"{name} beam {b} dir {d}")


def lqr_blocks(got, ref, fi, tol):
    """per (row DOF kind, column DOF kind) sub-block of every quadrant, relative to the sub-block's largest entry (floor
    1e-9 of the quadrant's); a zero reference sub-block must come out zero to 1e-15 of the quadrant"""
    n = fi.size
    dof = np.concatenate([fi % 3, fi % 3])
    half = np.concatenate([np.zeros(n, int), np.ones(n, int)])
    cdof = dof[:got.shape[1]]
    chalf = half[:got.shape[1]]
    for rh in range(2):
        for ch in range(int(chalf.max()) + 1):
            quad = ref[np.ix_(half == rh, chalf == ch)]
            qmax = np.max(np.abs(quad))
            for r in range(3):
                for c in range(3):
                    rs, cs = (half == rh) & (dof == r), (chalf == ch) & (cdof == c)
                    sub, subr = got[np.ix_(rs, cs)], ref[np.ix_(rs, cs)]
                    if subr.size == 0:
                        continue
                    m = np.max(np.abs(subr))
                    if m == 0.0:
                        assert np.max(np.abs(sub)) <= 1e-15 * max(qmax, 1.0), (rh, ch, r, c)
                        continue
                    scale = max(m, 1e-9 * qmax)
                    assert np.max(np.abs(sub - subr)) / scale <= tol, (rh, ch, r, c, np.max(np.abs(sub - subr)) / scale)


@pytest.mark.parametrize("bcs", [None, ["FIXED", "NONE", "NONE", "PINNED", "NONE", "NONE", "NONE", "NONE", "NONE", "NONE"]])
def test_linearize_at_rest_of_a_linear_beam_is_the_reference_state_space(bcs):
    cols = nitinol_columns(10, "linear", bcs=bcs)
    ens = BeamEnsemble(cols, 3)
    A, Bu = ens.linearize()
    K, M = ens.plan.stiffness(), ens.plan.mass()
    n = ens.n
    lqr = LinearQuadraticRegulator(K, M, np.eye(2 * n), np.eye(n))
    for b in range(3):
        lqr_blocks(A[b].cpu().numpy(), lqr.get_A(), ens.free_index, 1e-10)
        lqr_blocks(Bu[b].cpu().numpy(), lqr.get_B(), ens.free_index, 1e-10)


@pytest.mark.parametrize("kind,corrected,n", [("nonlinear", False, 8), ("nonlinear", True, 8), ("nonlinear", False, 60)])
def test_linearize_agrees_with_the_tangent_stiffness(kind, corrected, n):
    cols = nitinol_columns(n, kind)
    B = 2
    ens = BeamEnsemble(cols, B, corrected_axial=corrected)
    rng = np.random.default_rng(5)
    Q = rng.normal(0.0, 2e-2, (B, ens.n))
    X = np.concatenate([Q, np.zeros_like(Q)], axis=1)
    A, Bu = ens.linearize(X)
    Kt = ens.tangent_stiffness(Q).cpu().numpy()
    M = ens.plan.mass()
    fi = ens.free_index
    dof = fi % 3
    for b in range(B):
        got = M @ A[b, ens.n:, :ens.n].cpu().numpy()
        ref = -Kt[b]
        for r in range(3):
            for c in range(3):
                sub, subr = got[np.ix_(dof == r, dof == c)], ref[np.ix_(dof == r, dof == c)]
                scale = max(np.max(np.abs(subr)), 1e-9 * np.max(np.abs(ref)))
                assert np.max(np.abs(sub - subr)) / scale <= 1e-9, (b, r, c)
        # the position rows are [0, I] whatever the point
        assert torch.equal(A[b, :ens.n, ens.n:].cpu(), torch.eye(ens.n, dtype=torch.float64))
        assert float(A[b, :ens.n, :ens.n].abs().max()) == 0.0


def test_tangent_of_a_linear_beam_is_the_rollout_of_the_perturbation():
    cols = nitinol_columns(12, "linear")
    B, steps, dt = 4, 150, 2e-5
    ens = BeamEnsemble(cols, B)
    rng = np.random.default_rng(1)
    X = bent_state(ens, rng)
    dX = directions(X, rng, 1, ens.free_index)[0]
    ens.set_state(X)
    dT = ens.step_tangent(steps, dt, dX, impulse_amp=np.linspace(0.1, 0.4, B), impulse_index=1).cpu().numpy()
    ref = BeamEnsemble(cols, B)
    ref.set_state(dX)
    ref.step(steps, dt)
    assert_blocks(dT, ref.unpack_state().cpu().numpy(), ens.free_index, 1e-12, what="linear tangent")


@pytest.mark.parametrize("case", ["nonlinear_drag_grav_32", "packed_pinned_6", "four_waves_200"])
def test_base_state_and_clock_match_step(case):
    # (the lean stepper that step() runs for canonical gravity rounds differently from the general one: the axial blocks of the
    #  shipped element amplify that -- 5e-11 in u after 420 steps at 32 elements -- so that case is held to 2 x 60 steps)
    n, bcs, grav, steps = {"nonlinear_drag_grav_32": (32, None, True, 60),
                           "packed_pinned_6": (6, ["PINNED"] + ["NONE"] * 5, True, 200),
                           "four_waves_200": (200, None, False, 100)}[case]
    cols = nitinol_columns(n, "nonlinear", bcs=bcs)
    B, dt = 5, 2e-5
    fp = force_params(True, grav)
    a, b = BeamEnsemble(cols, B, force_params=fp), BeamEnsemble(cols, B, force_params=fp)
    rng = np.random.default_rng(2)
    X = rollout_state(a)
    amps = np.linspace(0.1, 0.3, B)
    U = np.where((a.free_index % 3 == 1)[None], rng.normal(0.0, 0.05, (B, a.n)), 0.0)
    a.set_state(X, time=1e-3)
    b.set_state(X, time=1e-3)
    for _ in range(2):   # (the clock carries over between calls)
        a.step_tangent(steps, dt, directions(X, rng, 3, a.free_index), impulse_amp=amps, held_force=U, impulse_duration=2.5e-3)
        b.step(steps, dt, impulse_amp=amps, held_force=U, impulse_duration=2.5e-3)
        assert a.time == b.time
    assert_blocks(a.unpack_state().cpu().numpy(), b.unpack_state().cpu().numpy(), a.free_index, 1e-12, what=case)


def nonlinear_rollout_setup():
    cols = nitinol_columns(32, "nonlinear")
    B = 2
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    ob = oracle_beam(cols, **oracle_kw(True, True))
    rng = np.random.default_rng(4)
    X = rollout_state(ens)
    return ens, ob, X, rng


STEPS, DT = 200, 2e-5


def test_rollout_tangent_of_the_state_matches_oracle_rk4():
    ens, ob, X, rng = nonlinear_rollout_setup()
    amps = np.array([0.15, 0.3])
    dX = directions(X, rng, 2, ens.free_index)
    ens.set_state(X)
    dT = ens.step_tangent(STEPS, DT, dX, impulse_amp=amps).cpu().numpy()
    for b in range(2):
        for d in range(2):
            F = lambda e: ob.rk4_impulse(X[b] + e * dX[d, b], DT, STEPS, amps[b])   # noqa: E731
            fd_check(dT[d, b], F, 1e-5, ens.free_index, f"state beam {b} dir {d}")


def test_rollout_tangent_of_the_impulse_amplitude_matches_oracle_rk4():
    ens, ob, X, rng = nonlinear_rollout_setup()
    amps = np.array([0.15, 0.3])
    ens.set_state(X)
    zero = np.zeros((2, 2 * ens.n))
    dT = ens.step_tangent(STEPS, DT, zero, impulse_amp=amps, d_impulse_amp=np.ones(2)).cpu().numpy()
    for b in range(2):
        F = lambda e: ob.rk4_impulse(X[b], DT, STEPS, amps[b] + e * amps[b])   # noqa: E731
        fd_check(amps[b] * dT[b], F, 1e-3, ens.free_index, f"amplitude beam {b}")


def test_rollout_tangent_of_the_held_force_matches_oracle_rk4():
    ens, ob, X, rng = nonlinear_rollout_setup()
    w = (ens.free_index % 3 == 1)[None]   # transverse loads (axial ones excite the shipped element's runaway axial modes)
    U = np.where(w, rng.normal(0.0, 0.05, (2, ens.n)), 0.0)
    dU = np.where(w, rng.normal(0.0, 0.05, (2, ens.n)), 0.0)
    ens.set_state(X)
    dT = ens.step_tangent(STEPS, DT, np.zeros((2, 2 * ens.n)), held_force=U, d_held_force=dU).cpu().numpy()
    for b in range(2):
        F = lambda e: ob.rk4_held(X[b], DT, STEPS, U[b] + e * dU[b])   # noqa: E731
        fd_check(dT[b], F, 1e-3, ens.free_index, f"held force beam {b}")


def test_tangent_is_linear_in_the_direction_and_directions_are_independent():
    cols = nitinol_columns(24, "nonlinear")
    B = 3
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    rng = np.random.default_rng(9)
    X = rollout_state(ens)
    dX = directions(X, rng, 3, ens.free_index)
    dX[2] = 0.7 * dX[0] - 1.9 * dX[1]
    amps = np.linspace(0.1, 0.2, B)
    ens.set_state(X)
    together = ens.step_tangent(100, DT, dX, impulse_amp=amps)
    a = together.cpu().numpy()
    assert_blocks(a[2], 0.7 * a[0] - 1.9 * a[1], ens.free_index, 1e-12, what="linearity")
    base = ens.state.clone()
    for d in range(3):
        ens.set_state(X)
        one = ens.step_tangent(100, DT, dX[d], impulse_amp=amps)
        assert torch.equal(one, together[d]), d
        assert torch.equal(ens.state, base)


def test_state_transition_matrix_of_64_short_rods():
    cols = nitinol_columns(6, "nonlinear")
    B, steps = 64, 100
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    ob = oracle_beam(cols, **oracle_kw(True, False))
    X = rollout_state(ens)
    amps = np.linspace(0.05, 0.5, B)
    n2 = 2 * ens.n
    seeds = np.ascontiguousarray(np.broadcast_to(np.eye(n2)[:, None, :], (n2, B, n2)))
    ens.set_state(X)
    Phi = ens.step_tangent(steps, DT, seeds, impulse_amp=amps).cpu().numpy()   # [2n, B, 2n]: column d of beam b at [d, b]
    for b in (0, 21, 42, 63):
        for d in range(n2):
            e = np.zeros(n2)
            e[d] = 1.0
            F = lambda h: ob.rk4_impulse(X[b] + h * e, DT, steps, amps[b])   # noqa: E731
            h = 1e-8 if d < ens.n else 1e-5   # (unit seeds: the FD error estimate is <= 3e-7 at these steps)
            fd_check(Phi[d, b], F, h, ens.free_index, f"STM beam {b} column {d}")


def test_heterogeneous_ensemble_matches_each_beam_alone():
    sets = [nitinol_columns(6, "nonlinear"),
            nitinol_columns(10, "linear", bcs=["PINNED"] + ["NONE"] * 9),
            nitinol_columns(8, "nonlinear", bcs=["FIXED", "NONE", "NONE", "PINNED", "NONE", "NONE", "NONE", "NONE"])]
    fps = [force_params(True, True), force_params(False, True), force_params(True, False)]
    ens = BeamEnsemble(sets, 3, force_params=fps)
    assert ens.mixed_topology
    rng = np.random.default_rng(8)
    singles = [BeamEnsemble(s, 1, force_params=f) for s, f in zip(sets, fps)]
    states = [rollout_state(s)[0] for s in singles]
    dirs = [directions(x[None], rng, 2, s.free_index)[:, 0] for x, s in zip(states, singles)]
    amps = np.array([0.1, 0.2, 0.3])
    ens.set_state(ens.pad_states(states))
    A, Bu = ens.linearize()
    dX = np.stack([ens.pad_states([d[k] for d in dirs]) for k in range(2)])
    got = ens.step_tangent(50, DT, dX, impulse_amp=amps, d_impulse_amp=np.ones(3)).cpu().numpy()
    for b, s in enumerate(singles):
        s.set_state(states[b][None])
        want = s.step_tangent(50, DT, dirs[b][:, None], impulse_amp=amps[b:b + 1], d_impulse_amp=np.ones(1)).cpu().numpy()
        nb = int(ens.n_per_beam[b])
        for k in range(2):
            assert_blocks(ens.beam_state(b, got[k]), want[k, 0], s.free_index, 1e-13, what=f"hetero beam {b}")
            pad = np.concatenate([got[k, b, nb:ens.n], got[k, b, ens.n + nb:]])
            assert np.all(pad == 0.0)
        assert_blocks(ens.beam_state(b), s.unpack_state().cpu().numpy()[0], s.free_index, 1e-13, what=f"hetero base {b}")
        # linearize (at the start): the beam's own Jacobian in its corner, zero padding rows and columns
        s.set_state(states[b][None])
        As, Bs = s.linearize()
        sel = np.r_[0:nb, ens.n:ens.n + nb]
        Ab = A[b].cpu().numpy()
        np.testing.assert_allclose(Ab[np.ix_(sel, sel)], As[0].cpu().numpy(), rtol=0, atol=1e-13 * np.max(np.abs(Ab)))
        assert np.all(np.delete(np.delete(Ab, sel, axis=0), sel, axis=1) == 0.0)
        np.testing.assert_allclose(Bu[b].cpu().numpy()[np.ix_(sel, np.arange(nb))], Bs[0].cpu().numpy(), rtol=0,
                                   atol=1e-13 * np.max(np.abs(Bs[0].cpu().numpy())))


def test_full_size_4096_beams_of_256_elements():
    cols = nitinol_columns(256, "nonlinear")
    B, steps = 4096, 20
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    ob = oracle_beam(cols, **oracle_kw(True, False))
    rng = np.random.default_rng(10)
    X = rollout_state(ens)
    amps = np.linspace(0.1, 0.5, B)
    dX = directions(X, rng, 1, ens.free_index)[0]
    ens.set_state(X)
    dT = ens.step_tangent(steps, DT, dX, impulse_amp=amps).cpu().numpy()
    for b in (0, 2047, 4095):
        F = lambda e: ob.rk4_impulse(X[b] + e * dX[b], DT, steps, amps[b])   # noqa: E731
        fd_check(dT[b], F, 1e-4, ens.free_index, f"full size beam {b}")


def test_non_finite_direction_stays_in_its_beam():
    for n in (6, 100):   # packed beams (10 to a wave) and a two-wave beam
        cols = nitinol_columns(n, "nonlinear")
        B = 12
        ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
        rng = np.random.default_rng(12)
        X = rollout_state(ens)
        dX = directions(X, rng, 2, ens.free_index)
        ens.set_state(X)
        clean = ens.step_tangent(30, DT, dX).cpu()
        bad = dX.copy()
        bad[1, 3, 5] = np.nan
        bad[0, 3, 1] = np.inf
        ens.set_state(X)
        dirty = ens.step_tangent(30, DT, bad).cpu()
        others = [b for b in range(B) if b != 3]
        assert torch.equal(clean[:, others], dirty[:, others])
        assert not torch.isfinite(dirty[1, 3]).all()


def test_refusals():
    cols = nitinol_columns(6, "nonlinear")
    e32 = BeamEnsemble(cols, 2, dtype=torch.float32)
    with pytest.raises(nat.NativeError, match="error -4: .*fp64 plan"):
        e32.step_tangent(1, DT, np.zeros((2, 2 * e32.n)))
    with pytest.raises(nat.NativeError, match="error -4: .*fp64 plan"):
        e32.rhs_jvp(np.zeros((2, 2 * e32.n)))
    ens = BeamEnsemble(cols, 2)
    z = np.zeros((2, 2 * ens.n))
    with pytest.raises((ValueError, RuntimeError)):
        ens.step_tangent(1, DT, np.zeros((0, 2, 2 * ens.n)))
    with pytest.raises((ValueError, RuntimeError)):
        ens.rhs_jvp(np.zeros((0, 2, 2 * ens.n)))
    for dt in (0.0, -DT):
        with pytest.raises((ValueError, RuntimeError)):
            ens.step_tangent(1, dt, z)
    with pytest.raises((ValueError, RuntimeError)):
        ens.step_tangent(-1, DT, z)
    for shape in ((2, 2 * ens.n + 1), (3, 2 * ens.n), (2 * ens.n,), (1, 1, 2, 2 * ens.n)):
        with pytest.raises((ValueError, RuntimeError)):
            ens.step_tangent(1, DT, np.zeros(shape))
    with pytest.raises((ValueError, RuntimeError)):
        ens.step_tangent(1, DT, z, impulse_amp=np.ones(2), d_impulse_amp=np.ones((3, 2)))
    assert ens.time == 0.0 and float(ens.state.abs().max()) == 0.0   # refused calls leave the ensemble alone
