"""Every kernel family on beams whose properties vary along the span (helpers.graded_columns), each beam against its own
oracle per DOF block.  A table read one slot off, the left and the right element of a node swapped, a multiplier level
taken from its neighbour: none of these shows on the rods of equal elements that the rest of the suite steps.  The case
table, with the layout and the reduction levels that each case asserts (and so the kernel instance it runs), is
tests/test_graded_beams_cpu.py:CASES; the CPU file also shows every input here finite and conditioned below 2e-14 on the
oracle, so the bounds are the uniform-rod tests' own: 1e-9 RHS, 1e-8 RK4 rollouts of at most 40 steps, 1e-6 step_implicit
(n_iter = 3), 5e-9 controlled replay (implicit and closed loop), the tangent / adjoint figures of test_derivative_mappings.py."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from tests.helpers import assert_blocks, block_errs, graded_columns, nitinol_columns, oracle_beam
from tests.test_adjoint import dot_check
from tests.test_controlled_closed_loop_large import fits_lds, replay
from tests.test_graded_beams_cpu import (AMPS, CASES, DT, FP32_CASES, FP32_STEPS, STEPS, case_columns, case_dt, closed_loop_gain, mixed,
                                         seeded_gain)
from tests.test_gpu_parity import FP32_TOL, ensemble
from tests.test_static_equilibrium import numpy_newton
from tests.test_tangent_linear import directions, fd_check, force_params, oracle_kw, rollout_state

pytestmark = pytest.mark.gpu

DRAG = dict(fluid_density=1000.0, enable_fluid=True)
GRAV = dict(enable_gravity=True)
BOTH = dict(DRAG, **GRAV)


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def graded_ensemble(name, kw, dtype=None, B=None):
    """the ensemble of a case with its layout asserted, its columns and its oracle"""
    c = CASES[name]
    cols = case_columns(name)
    ens = ensemble(cols, B or c["B"], kw, dtype=dtype)
    got = layout_of(ens)
    want = c["layout"] if dtype in (None, torch.float64) else c["layout"][:3] + (c["lv32"], c["layout"][4])
    assert got == want, (name, got, want)
    return ens, cols, oracle_beam(cols, **kw)


def transverse(ens):
    return (ens.free_index % 3 == 1)[None]


def layout_of(ens):
    lay = ens.plan.layout
    return (lay.n_slots, lay.beams_per_group, lay.threads, lay.pcr_levels, lay.pcr_levels_full)


def report(row, errs):
    """one line per check for the table of tests/README.md: the worst block error (or the figure itself)"""
    worst = max(errs.values()) if isinstance(errs, dict) else float(errs)
    print(f"[graded] {row} | {worst:.1e}")
    return worst


# ---- 1. rhs() and step(): tip and mid-span impulse, held force; drag, canonical gravity, both; lean and general kernels
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_rhs_and_step_match_the_oracle(name, lean, monkeypatch):
    if not lean:
        monkeypatch.setenv("CRB_DISABLE_LEAN", "1")
    c, dt = CASES[name], case_dt(name)
    B = c["B"]
    amps = AMPS[:B]
    rng = np.random.default_rng(sum(map(ord, name)))
    for what, kw, imp in (("drag, tip", DRAG, None), ("gravity, mid-span", GRAV, (c["mid"], "w")), ("both, mid-span", BOTH, (c["mid"], "w")),
                          ("both, tip", BOTH, None)):
        ens, cols, ob = graded_ensemble(name, kw)
        idx = -2 if imp is None else ens.reduced_index(*imp)
        ens.step(STEPS, dt, impulse_amp=amps, impulse_index=idx)
        got = np_(ens.unpack_state())
        ref, _ = ob.rk4_impulse_batch(np.zeros((B, 2 * ob.n)), dt, STEPS, amps, idx=idx)
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
        errs = assert_blocks(got, ref, ens.free_index, 1e-8, what=(name, what, lean))
        report("step " + ("lean" if lean else "general"), errs)
        if what == "both, tip":
            # rhs() at the rolled-out state under a random input; then a held transverse load from that state
            U = rng.normal(0.0, 0.05, (B, ens.n))
            xd = np_(ens.rhs(ref, U))
            for b in range(B):
                report("rhs", assert_blocks(xd[b], ob.rhs(ref[b], U[b]), ens.free_index, 1e-9, what=(name, "rhs", b, lean)))
            H = np.where(transverse(ens), rng.normal(0.0, 0.05, (B, ens.n)), 0.0)
            ens.set_state(ref)
            ens.step(STEPS // 2, dt, held_force=H)
            want = np.array([ob.rk4_held(ref[b], dt, STEPS // 2, H[b]) for b in range(B)])
            report("held", assert_blocks(np_(ens.unpack_state()), want, ens.free_index, 1e-8, what=(name, "held", lean)))


# ---- 2. fp32 step() on the fp32 rows of the table: the per-block bounds and the horizon (200 steps, nonlinear rods with drag from
# rest under the tip impulse) of test_fp32_plan_tracks_fp64_within_measured_drift
@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_step_tracks_the_oracle(name):
    c = CASES[name]
    B = c["B"]
    cols = graded_columns(c["n"], "nonlinear", c["family"])
    ens = ensemble(cols, B, DRAG, dtype=torch.float32)
    lay = ens.plan.layout
    assert (lay.n_slots, lay.beams_per_group, lay.threads, lay.pcr_levels) == c["layout"][:3] + (c["lv32"],)
    amps = np.linspace(0.1, 0.2, B)     # (test_graded_beams_cpu.py: the same rollouts finite and conditioned on the oracle)
    ens.step(FP32_STEPS, DT, impulse_amp=amps)
    got = ens.unpack_state().double().cpu().numpy()
    ref, _ = oracle_beam(cols, **DRAG).rk4_impulse_batch(np.zeros((B, 2 * ens.n)), DT, FP32_STEPS, amps)
    errs = block_errs(got, ref, ens.free_index)
    print(name, "fp32", {k: f"{v:.1e}" for k, v in errs.items()})
    for k, e in errs.items():
        assert e <= FP32_TOL[k], (name, k, e, errs)


# ---- 3. rk4_stage / stage-split step_feedback with a seeded dense gain, lean and general stage kernels
@pytest.mark.parametrize("name", ["wave40_taper3", "wave64_step", "waves2_100_taper10", "waves2_128_step", "waves4_200_taper30",
                                  "waves4_256_taper10", "waves4_256_pinned_taper30"])
def test_stage_split_feedback_matches_the_oracle(name, monkeypatch):
    monkeypatch.setenv("CRB_FUSED_FEEDBACK", "0")
    monkeypatch.setenv("CRB_LOOP", "0")
    c = CASES[name]
    B, kw = c["B"], DRAG
    rng = np.random.default_rng(300 + c["n"])
    ens, cols, ob = graded_ensemble(name, kw)
    assert ens.feedback_path() == "stage-split"
    n = ens.n
    gain = seeded_gain(ob, rng)
    ref = rng.normal(0.0, 1e-4, (B, 2 * n))
    x0 = rng.normal(0.0, 1e-5, (B, 2 * n))
    amps = AMPS[:B]
    steps, dt = 20, 5e-6
    ens.set_state(x0)
    ens.step_feedback(steps, dt, gain, reference=ref, impulse_amp=amps)
    got = np_(ens.unpack_state())
    for b in range(B):
        want = ob.rk4_feedback(x0[b], dt, steps, gain, reference=ref[b], amp=amps[b])
        assert np.isfinite(want).all()
        report("stage-split lean", assert_blocks(got[b], want, ens.free_index, 1e-8, what=(name, b)))
    monkeypatch.setenv("CRB_DISABLE_LEAN_STAGE", "1")
    gen, _, _ = graded_ensemble(name, kw)
    gen.set_state(x0)
    gen.step_feedback(steps, dt, gain, reference=ref, impulse_amp=amps)
    for b in range(B):
        want = ob.rk4_feedback(x0[b], dt, steps, gain, reference=ref[b], amp=amps[b])
        report("stage-split general", assert_blocks(np_(gen.unpack_state())[b], want, ens.free_index, 1e-8, what=(name, b, "general")))


# ---- 4. the fused packed feedback stepper (5 levels) at 20 elements in fp64 and at 31 in fp32.  The fp64 gain of 31 elements
# (93 x 186 x 8 B = 135 KB, with the error vectors above the 144 KB that fused_feedback_ok grants) does not fit LDS: that plan is
# the stage-split path's, which is asserted and held to the same oracle.
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("name,dtype,path", [("packed20_taper3", torch.float64, "fused"), ("packed31_taper3", torch.float32, "fused"),
                                             ("packed31_taper3", torch.float64, "stage-split")])
def test_fused_packed_feedback_matches_the_oracle(name, dtype, path, lean, monkeypatch):
    monkeypatch.setenv("CRB_FUSED_FEEDBACK", "1")
    if not lean:
        monkeypatch.setenv("CRB_DISABLE_LEAN_FEEDBACK", "1")
    c = CASES[name]
    B, kw = c["B"], BOTH
    rng = np.random.default_rng(400 + c["n"])
    ens, cols, ob = graded_ensemble(name, kw, dtype=dtype)
    assert ens.feedback_path() == path
    n = ens.n
    gain = seeded_gain(ob, rng)
    ref = rng.normal(0.0, 1e-4, (B, 2 * n))
    x0 = rng.normal(0.0, 1e-5, (B, 2 * n))
    steps, dt = 40, 5e-6
    ens.set_state(x0)
    ens.step_feedback(steps, dt, gain, reference=ref, impulse_amp=AMPS[:B])
    got = ens.unpack_state().double().cpu().numpy()
    for b in range(B):
        want = ob.rk4_feedback(x0[b], dt, steps, gain, reference=ref[b], amp=AMPS[b])
        if dtype == torch.float32:   # (the bound of test_fused_feedback_stepper_in_single_precision, against the fp64 oracle here)
            assert report("fused fp32", block_errs(got[b], want, ens.free_index)) < 2e-3, (name, b, lean)    # (per block here)
        else:
            report(f"feedback {path} fp64", assert_blocks(got[b], want, ens.free_index, 1e-8, what=(name, b, lean)))


# ---- 5. the persistent closed loop at 6 levels: loop_built(6, 0) at 64 elements, loop_built(6, 1) at 100, 64 beams
@pytest.mark.parametrize("name", ["wave64_taper3", "waves2_100_taper3"])
def test_persistent_closed_loop_at_six_levels(name, monkeypatch):
    monkeypatch.setenv("CRB_LOOP", "1")
    B, kw = 64, DRAG
    rng = np.random.default_rng(500 + CASES[name]["n"])
    ens, cols, ob = graded_ensemble(name, kw, B=B)
    assert ens.plan.layout.pcr_levels == 6 and ens.feedback_path() == "persistent"
    n = ens.n
    gain = seeded_gain(ob, rng)
    ref = rng.normal(0.0, 1e-4, (B, 2 * n))
    x0 = rng.normal(0.0, 1e-5, (B, 2 * n))
    amps = 0.05 * (1.0 + np.arange(B) / B)
    steps, dt = 14, 5e-6
    ens.set_state(x0)
    t = ens.step_feedback(steps, dt, gain, reference=ref, impulse_amp=amps, impulse_duration=6.5 * dt)
    assert ens.feedback_status() == 0
    got = np_(ens.unpack_state())
    for b in (0, 1, 31, 62, 63):
        want = ob.rk4_feedback(x0[b], dt, steps, gain, reference=ref[b], amp=amps[b], duration=6.5 * dt)
        report("persistent loop", assert_blocks(got[b], want, ens.free_index, 1e-8, what=(name, b)))
    monkeypatch.setenv("CRB_LOOP", "0")
    split, _, _ = graded_ensemble(name, kw, B=B)
    assert split.feedback_path() == "stage-split"
    split.set_state(x0)
    assert split.step_feedback(steps, dt, gain, reference=ref, impulse_amp=amps, impulse_duration=6.5 * dt) == t
    report("persistent loop against stage-split", assert_blocks(np_(split.unpack_state()), got, ens.free_index, 1e-8, what=(name, "stage-split")))


# ---- 6. solve_rk45 against scipy over the oracle RHS: the same accepted steps and nfev (no gravity: the lean RK45 RHS)
@pytest.mark.parametrize("name", ["wave40_taper3", "waves2_100_taper10", "waves4_200_taper10"])
def test_adaptive_rk45_takes_scipys_steps(name):
    from scipy.integrate import solve_ivp

    c = CASES[name]
    B = c["B"]
    ens, cols, ob = graded_ensemble(name, DRAG)
    n = ob.n
    amps = AMPS[:B]
    dur, t_end, rtol, atol = 1e-4, 3e-4, 1e-6, 1e-9
    st = ens.solve_rk45(t_end, rtol=rtol, atol=atol, impulse_amp=amps, impulse_duration=dur)
    got = np_(ens.unpack_state())
    assert np.all(st["status"] == 0)
    for b in range(B):
        def fun(t, x, b=b):
            u = np.zeros(n)
            if t < dur:
                u[-2] = amps[b]
            return ob.rhs(x, u)

        sol = solve_ivp(fun, (0.0, t_end), np.zeros(2 * n), method="RK45", rtol=rtol, atol=atol)
        assert st["accepted"][b] == len(sol.t) - 1 and st["nfev"][b] == sol.nfev, (b, st["accepted"][b], len(sol.t) - 1)
        report("rk45", assert_blocks(got[b], sol.y[:, -1], ens.free_index, 1e-8, what=(name, b)))


# ---- 7. step_implicit: one beam per workgroup at 64 / 128 / 256, packed at 20; the damped variant
@pytest.mark.parametrize("name,kw,rho", [("packed20_taper3", BOTH, None), ("wave64_taper3", DRAG, None), ("waves2_128_taper10", GRAV, None),
                                         ("waves4_256_taper30", DRAG, None), ("waves2_128_step", BOTH, 0.6),
                                         ("waves4_256_taper10", DRAG, 0.8)])
def test_implicit_steppers_match_the_oracle(name, kw, rho):
    c = CASES[name]
    B = c["B"]
    kind = "linear" if kw.get("enable_gravity") and c["n"] > 31 else None     # (as the uniform-rod tests: gravity on linear rods)
    cols = graded_columns(c["n"], kind, c["family"]) if kind else case_columns(name)
    ens = ensemble(cols, B, kw)
    assert layout_of(ens) == c["layout"], name      # (the element kinds do not move the layout)
    ob = oracle_beam(cols, **kw)
    # (from rest: the shipped nonlinear element lets a seeded state on the thin end of a taper run away at this step,
    #  on the oracle itself)
    x0 = np.zeros((B, 2 * ob.n))
    h, steps = 1e-4, 40
    amps = AMPS[:B]
    ens.set_state(x0)
    if rho is None:
        ens.step_implicit(steps, h, n_iter=3, impulse_amp=amps, impulse_duration=10.0 * h)
    else:
        ens.step_implicit(steps, h, n_iter=3, impulse_amp=amps, impulse_duration=10.3 * h, rho_inf=rho, t0=0.0)
    got = np_(ens.unpack_state())
    for b in range(B):
        want = (ob.implicit(x0[b], h, steps, n_iter=3, amp=amps[b], duration=10.0 * h) if rho is None else
                ob.implicit_alpha(x0[b], h, steps, rho, n_iter=3, amp=amps[b], duration=10.3 * h))
        assert np.isfinite(want).all()
        report("implicit" if rho is None else "implicit damped", assert_blocks(got[b], want, ens.free_index, 1e-6, what=(name, b, rho)))


# ---- 8. solve_controlled, replayed interval by interval on the oracle at the step counts the controller accepted.
# The implicit scheme solves with ALL levels of A (lean_controlled_ok asks controlled_built for pcr_levels_full): the graded
# level count selects nothing there, the per-slot tables of a graded rod are what this adds -- 6 levels at one wave, 7 at two.
@pytest.mark.parametrize("name,full", [("wave64_taper3", 6), ("waves2_100_taper10", 7)])
def test_controlled_implicit_kernel_replays_on_the_oracle(name, full):
    c = CASES[name]
    B, kw = c["B"], dict(GRAV)
    cols = graded_columns(c["n"], "linear", c["family"])
    ens = ensemble(cols, B, kw)
    assert layout_of(ens) == c["layout"] and ens.plan.layout.pcr_levels_full == full
    ob = oracle_beam(cols, **kw)
    rng = np.random.default_rng(800 + c["n"])
    x0 = 1e-5 * rng.standard_normal((B, 2 * ens.n))
    ens.set_state(x0)
    amps = AMPS[:B]
    dt_eval, n_int = 1e-3, 3
    snaps, stats, used = ens.solve_controlled(n_int, dt_eval, rtol=1e-2, atol=1e-6, impulse_amp=amps, impulse_duration=1.5e-3,
                                              first_rate=4.0 / dt_eval, t0=0.0)
    assert np.all(stats[:, 2] == 0) and used.min() >= 2
    y = np_(ens.unpack_snapshots(snaps))
    for b in range(B):
        start = x0[b]
        for k in range(n_int):
            if k == 1:      # (the interval the impulse ends in is cut in two pieces with their own rungs: continue from the record)
                start = y[k, b]
                continue
            m = int(used[b, k])
            want = ob.implicit(start, dt_eval / m, m, n_iter=1, amp=amps[b], duration=1.5e-3, t0=k * dt_eval)
            report("controlled implicit", assert_blocks(y[k, b], want, ens.free_index, 5e-9, what=(name, b, k, m)))
            start = y[k, b]


# The closed loop solves with the mass matrix's truncated tables: pcr_levels = 6 is controlled_built(6, feedback, one wave), the
# instance no uniform rod reaches (they stop at 5).  A gain of 40 elements and more does not fit LDS, so this is the streamed
# form; lean and, under CRB_DISABLE_LEAN_FEEDBACK, the general right-hand side.
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("name", ["wave40_taper3", "wave64_taper3"])
def test_controlled_closed_loop_at_six_levels_replays_on_the_oracle(name, lean, monkeypatch):
    if not lean:
        monkeypatch.setenv("CRB_DISABLE_LEAN_FEEDBACK", "1")
    c = CASES[name]
    B, kw = c["B"], DRAG
    ens, cols, ob = graded_ensemble(name, kw)
    assert ens.plan.layout.pcr_levels == 6 and ens.plan.layout.threads == 64 and not fits_lds(ens)
    K = closed_loop_gain(ob, np.random.default_rng(850 + c["n"]))
    x0 = np.zeros((B, 2 * ens.n))
    amps = AMPS[:B]
    dt_eval, n_int, t_switch = 1e-3, 3, 1.5e-3
    snaps, stats, used = ens.solve_controlled(n_int, dt_eval, rtol=1e-2, atol=1e-5, gain=K, impulse_amp=amps, impulse_duration=t_switch,
                                              t0=0.0)
    y = np_(ens.unpack_snapshots(snaps))
    assert np.all(stats[:, 2] == 0) and np.all(np.isfinite(y)) and np.array_equal(stats[:, 0], used.sum(axis=1))
    print(name, "lean" if lean else "general", "steps per interval", used.tolist())
    replay(ob, y, x0, K, amps, dt_eval, used, t_switch, 1, ens.free_index, tol=5e-9)
    worst = 0.0
    for b in range(B):
        for k in (0, 2):
            m = int(used[b, k])
            want = ob.rk4_feedback(x0[b] if k == 0 else y[k - 1, b], dt_eval / m, m, K, amp=amps[b], duration=t_switch, t0=k * dt_eval)
            worst = max(worst, max(block_errs(y[k, b], want, ens.free_index).values()))
    report("controlled closed loop " + ("lean" if lean else "general"), worst)
    assert np.array_equal(np_(ens.unpack_state()), y[-1])


# ---- 9. derivatives and statics on allcols at 40 and 100 elements
ALLCOLS_LAYOUT = {40: (40, 1, 64, 6, 6), 100: (100, 1, 128, 5, 7)}


@pytest.mark.parametrize("n_e", [40, 100])
def test_derivatives_on_a_rod_whose_every_column_varies(n_e):
    cols = graded_columns(n_e, mixed(n_e), "allcols")
    B, steps = 2, 40
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    assert layout_of(ens) == ALLCOLS_LAYOUT[n_e]
    ob = oracle_beam(cols, **oracle_kw(True, True))
    fi = ens.free_index
    rng = np.random.default_rng(900 + n_e)
    X = rollout_state(ens)
    w = transverse(ens)
    U = np.where(w, rng.normal(0.0, 0.05, (B, ens.n)), 0.0)
    dX = directions(X, rng, 1, fi)
    dU = np.where(w, rng.normal(0.0, 0.05, (1, B, ens.n)), 0.0)
    # rhs_jvp against central differences of the oracle RHS; rhs_vjp by the dot-product identity
    xdot, Jv = ens.rhs_jvp(dX, X, U, dU)
    lam = directions(np_(Jv)[0] + X, rng, 1, fi)
    xb, ub = ens.rhs_vjp(lam, X, U)
    for b in range(B):
        assert_blocks(np_(xdot)[b], ob.rhs(X[b], U[b]), fi, 1e-9, what=("xdot", n_e, b))
        report("rhs_jvp", fd_check(np_(Jv)[0, b], lambda e: ob.rhs(X[b] + e * dX[0, b], U[b] + e * dU[0, b]), 1e-4, fi,
                                   f"allcols {n_e} rhs_jvp {b}"))
        report("rhs_vjp", dot_check([(lam[0, b], np_(Jv)[0, b])], [(np_(xb)[0, b], dX[0, b]), (np_(ub)[0, b], dU[0, b])], 1e-12,
                                    f"rhs_vjp {n_e} {b}"))
    # step_tangent against central differences of the oracle rollout; step_adjoint by the identity
    amps = np.array([0.5, 1.0])
    damp = rng.normal(0.0, 1.0, B)
    ens.set_state(X)
    dT = np_(ens.step_tangent(steps, DT, dX[0], impulse_amp=amps, held_force=U, d_impulse_amp=damp, d_held_force=dU[0], t0=0.0))
    ens.set_state(X)
    dTx = np_(ens.step_tangent(steps, DT, dX[0], impulse_amp=amps, t0=0.0))
    for b in range(B):
        report("step_tangent", fd_check(dTx[b], lambda e: ob.rk4_impulse(X[b] + e * dX[0, b], DT, steps, amps[b]), 1e-5, fi,
                                        f"allcols {n_e} tangent {b}"))
    lamT = directions(dT, rng, 1, fi)[0]
    xb, ab, fb = ens.step_adjoint(steps, DT, lamT, x0_red=X, impulse_amp=amps, held_force=U, t0=0.0)
    for b in range(B):
        report("step_adjoint", dot_check([(lamT[b], dT[b])], [(np_(xb)[b], dX[0, b]), (np_(ab)[b], damp[b]), (np_(fb)[b], dU[0, b])],
                                         1e-10, f"allcols {n_e} adjoint {b}"))


@pytest.mark.parametrize("n_e,tip", [(40, 1e-2), (100, 1e-3)])
def test_statics_on_a_rod_whose_every_column_varies(n_e, tip):
    cols = graded_columns(n_e, "nonlinear", "allcols")
    B = 2
    ens = BeamEnsemble(cols, B)
    assert layout_of(ens) == ALLCOLS_LAYOUT[n_e]
    ob = oracle_beam(cols, enable_gravity=True, gravity=(0.0, 0.0, 0.0))   # (numpy_newton reads the oracle's gravity term: zeros)
    U = np.zeros((B, ens.n))
    U[:, -2] = -tip * np.array([0.5, 1.0])
    sol = ens.solve_static(held_force=U, rtol=1e-7)
    assert bool(sol.converged.all()), (sol.iterations, sol.residual)
    got = np_(sol.q)
    ref = np.array([numpy_newton(ob, U[b]) for b in range(B)])
    errs = assert_blocks(got, ref, ens.free_index, 1e-6, what=f"allcols {n_e}")
    report("solve_static", errs)
    # the tangent stiffness at the equilibrium against central differences of the oracle's k(q), per block of rows and columns
    K = np_(ens.tangent_stiffness(ref))
    dof = ens.free_index % 3
    worst = 0.0
    for b in range(B):
        J = np.empty((ens.n, ens.n))
        for j in range(ens.n):
            h = 1e-6 * max(1e-2, abs(ref[b, j]))
            e = np.zeros(ens.n)
            e[j] = h
            J[:, j] = (ob.internal_force(ref[b] + e) - ob.internal_force(ref[b] - e)) / (2 * h)
        for r in range(3):
            for cc in range(3):
                sub, subr = K[b][np.ix_(dof == r, dof == cc)], J[np.ix_(dof == r, dof == cc)]
                scale = max(np.max(np.abs(subr)), 1e-9 * np.max(np.abs(J)))
                worst = max(worst, np.max(np.abs(sub - subr)) / scale)
                assert np.max(np.abs(sub - subr)) / scale <= 1e-6, (n_e, b, r, cc)
    report("tangent_stiffness", worst)


# ---- 10. one ensemble of a uniform, a taper10 and an allcols rod: the plan's level count is the largest of its beams'
@pytest.mark.parametrize("sizes,layout", [((100, 100, 100), (100, 1, 128, 6, 7)), ((31, 64, 128), (128, 1, 128, 6, 7))])
def test_mixed_ensemble_of_uniform_and_graded_rods(sizes, layout):
    sets = [nitinol_columns(sizes[0], "nonlinear"), graded_columns(sizes[1], "nonlinear", "taper10"),
            graded_columns(sizes[2], "nonlinear", "allcols")]
    ens = BeamEnsemble.from_dataframes(sets, force_params=[force_params(True, False)] * 3)
    assert layout_of(ens) == layout, layout_of(ens)       # (one mapping for all beams: the longest beam's slots, the deepest beam's levels)
    alone = [BeamEnsemble(s, 1, force_params=force_params(True, False)).plan.layout.pcr_levels for s in sets]
    assert ens.plan.layout.pcr_levels == max(alone) == 6 and alone[0] == 5      # the uniform rod runs one level deeper here
    amps = np.array([0.1, 0.2, 0.3])
    ens.step(STEPS, DT, impulse_amp=amps)
    got = np_(ens.unpack_state())
    for b, s in enumerate(sets):
        ob = oracle_beam(s, **DRAG)
        want = ob.rk4_impulse(np.zeros(2 * ob.n), DT, STEPS, amps[b])
        report("mixed ensemble step", assert_blocks(ens.beam_state(b, got), want, ob.red2full(), 1e-8, what=(sizes, b)))
    rng = np.random.default_rng(sum(sizes))
    x = [rng.normal(0.0, 1e-3, 6 * n_e) for n_e in sizes]
    xd = np_(ens.rhs(ens.pad_states(x)))
    for b, s in enumerate(sets):
        ob = oracle_beam(s, **DRAG)
        report("mixed ensemble rhs", assert_blocks(ens.beam_state(b, xd), ob.rhs(x[b]), ob.red2full(), 1e-9, what=(sizes, b, "rhs")))


# ---- 11. the blocked stepper's uniformity gate
def _step_256(cols, blocked, monkeypatch):
    if blocked:
        monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    else:
        monkeypatch.setenv("CRB_DISABLE_BLOCKED", "1")
    B = 3
    ens = ensemble(cols, B, DRAG)
    ens.step(STEPS, DT, impulse_amp=AMPS[:B])
    return np_(ens.unpack_state()), ens.free_index


def test_blocked_stepper_takes_only_bitwise_uniform_rods(monkeypatch):
    B = 3
    # an almost uniform rod (length[100] x 1.01) runs the one-node-per-lane stepper: bitwise the run with the blocked one off
    cols = graded_columns(256, "nonlinear", "nearly_uniform")
    got, fi = _step_256(cols, True, monkeypatch)
    off, _ = _step_256(cols, False, monkeypatch)
    assert np.array_equal(got, off)
    ref, _ = oracle_beam(cols, **DRAG).rk4_impulse_batch(np.zeros((B, got.shape[1])), DT, STEPS, AMPS[:B])
    report("gate nearly_uniform", assert_blocks(got, ref, fi, 1e-8, what="nearly_uniform"))
    # so does a rod whose mass matrix is uniform and whose stiffness is not (one element's modulus x 1.01)
    cols = nitinol_columns(256, "nonlinear")
    cols["elastic_modulus"][100] *= 1.01
    got, fi = _step_256(cols, True, monkeypatch)
    off, _ = _step_256(cols, False, monkeypatch)
    assert np.array_equal(got, off)
    ref, _ = oracle_beam(cols, **DRAG).rk4_impulse_batch(np.zeros((B, got.shape[1])), DT, STEPS, AMPS[:B])
    report("gate modulus", assert_blocks(got, ref, fi, 1e-8, what="modulus of one element"))
    # the switch is live: the uniform rod's two steppers agree to rounding (test_blocked_stage_arith.py: 1e-10 from rest), not bitwise
    cols = nitinol_columns(256, "nonlinear")
    got, fi = _step_256(cols, True, monkeypatch)
    off, _ = _step_256(cols, False, monkeypatch)
    assert not np.array_equal(got, off)
    assert report("gate uniform blocked against lean", block_errs(got, off, fi)) <= 1e-10
    ref, _ = oracle_beam(cols, **DRAG).rk4_impulse_batch(np.zeros((B, got.shape[1])), DT, STEPS, AMPS[:B])
    report("gate uniform", assert_blocks(got, ref, fi, 1e-8, what="uniform"))


@pytest.mark.parametrize("family", ["taper30", "step"])
def test_graded_256_slot_rods_match_the_oracle(family, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    B = 3
    cols = graded_columns(256, "nonlinear", family)
    got, fi = _step_256(cols, True, monkeypatch)
    ref, _ = oracle_beam(cols, **DRAG).rk4_impulse_batch(np.zeros((B, got.shape[1])), DT, STEPS, AMPS[:B])
    report("graded 256", assert_blocks(got, ref, fi, 1e-8, what=family))
