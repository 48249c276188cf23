"""Parameter gradients of the implicit adjoint on the GPU (BeamEnsemble.step_implicit_adjoint_params,
crb_step_implicit_adjoint_params, crb_implicit_paramgrad.h): stiffness, drag and gravity gradients of a recorded-tip loss against
central differences of the C oracle's `implicit` with perturbed constructor columns -- the iteration matrix A = M + h^2/4 K0
rebuilt with them -- on every thread mapping and with a control schedule; the test that fails without the iteration-matrix
term; bitwise independence of the checkpoint interval and of cotangent batching; exact zeros; heterogeneous ensembles; side
effects; the full-size ensemble.

Central differences.  The rule is test_adjoint.py's: |g - FD(eps/4)| <= min(max(1e-7, 4 |FD(eps) - FD(eps/4)|), 1e-6) |FD(eps/4)|.
The cases, the losses and the step sizes are those of tests/test_implicit_param_gradients_cpu.py, which proves on the CPU that the
oracle's own two differences agree to 2.5e-7 for every case and direction asserted here."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from tests.helpers import nitinol_columns
from tests.test_implicit_param_gradients_cpu import (ALL_DIRECTIONS, EVERY, MAPPING_CASES, MAPPING_DIRECTIONS, MATRIX_CASES,
                                                     ORACLE_CASES, SCHED_CASE, SCHED_DIRECTIONS, SCHED_HOLD, STEPS, TAG, WINDOW,
                                                     columns, oracle_differences, schedule)
from tests.test_param_gradients import AMPS, C_REC, directional, force_params, interior_pin, np_, pinned_root

pytestmark = pytest.mark.gpu


def tip_loss_gradients(ens, c, amps, steps=STEPS, every=EVERY, **kw):
    """step_implicit_adjoint_params for the loss of the CPU file's oracle_loss: from rest, the tip impulse, four samples"""
    B, n = ens.n_beams, ens.n
    lam = np.zeros((B, 2 * n))
    lam[:, n - 2] = 1.0
    rec = dict(record=(ens.n_elem, "w"), record_every=every, lam_record=np.broadcast_to(C_REC, (B, len(C_REC))).copy())
    return ens.step_implicit_adjoint_params(steps, c["h"], lam, n_iter=c["n_iter"], x0_red=np.zeros((B, 2 * n)), impulse_amp=amps,
                                            impulse_duration=WINDOW * c["h"], t0=0.0, **rec, **kw)


def check_against_oracle(table, name, c, directions, **kw):
    cols = columns(c)
    ens = BeamEnsemble(cols, len(AMPS), force_params=force_params(c["drag"], c["grav"]))
    grads = tip_loss_gradients(ens, c, AMPS, **kw)[3]
    for direction in directions:
        for b, (fd1, fd4) in enumerate(oracle_differences(table, name, direction)):
            g = directional(grads, cols, direction, b)
            allowed = min(max(1e-7, 4 * abs(fd1 - fd4) / abs(fd4)), 1e-6)
            err = abs(g - fd4) / abs(fd4)
            print(f"{TAG} {table} {name} beam {b} {direction}: g {g:.12e} FD(eps/4) {fd4:.12e} err {err:.2e} allowed {allowed:.2e} "
                  f"|FD(eps)-FD(eps/4)| {abs(fd1 - fd4) / abs(fd4):.2e}")
            assert err <= allowed, (table, name, b, direction, g, fd4, err, allowed)


# ---- 1. every direction against differences of the oracle
@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_parameter_gradients_match_oracle_differences(name):
    check_against_oracle("oracle", name, ORACLE_CASES[name], ALL_DIRECTIONS)


# ---- 2. the iteration matrix: with one iteration on a linear, drag-free, gravity-free rod the term
#         alpha gbar^T (dK0/dI) (a^i - a^{i+1}) is 8.8e-2 (6 elements, h = 1e-4) and 2.4e-2 (32 elements, h = 2e-4) of the
#         derivative with respect to I: a gradient without it misses the bound by five orders of magnitude
@pytest.mark.parametrize("name", list(MATRIX_CASES))
def test_moment_inertia_gradient_includes_the_iteration_matrix(name):
    check_against_oracle("matrix", name, MATRIX_CASES[name], ("moment_inertia",))


# ---- 3. every thread mapping
@pytest.mark.parametrize("name", list(MAPPING_CASES))
def test_parameter_gradients_on_every_mapping(name):
    check_against_oracle("mapping", name, MAPPING_CASES[name], MAPPING_DIRECTIONS)


# ---- 4. a control schedule: the chain of one oracle call per interval, the iterate restarting with each
@pytest.mark.parametrize("every", [7, 40])   # (7: interval boundaries inside segments and on none of their edges but step 0)
def test_parameter_gradients_with_a_control_schedule(every):
    c = SCHED_CASE
    n = 3 * c["n"]
    U = np.repeat(schedule(n)[:, None, :], len(AMPS), axis=1)
    check_against_oracle("schedule", "nonlinear_8", c, SCHED_DIRECTIONS, control=U, control_hold=SCHED_HOLD, checkpoint_every=every)


# ---- 5. bitwise: the plain path's returns, checkpoint intervals, cotangent batching, accumulation
def same(a, b, pick=lambda t: t):
    for r, g in zip(a[:3], b[:3]):
        assert torch.equal(pick(r), g)
    assert set(a[3]) == set(b[3])
    for key in a[3]:
        assert torch.equal(pick(a[3][key]), b[3][key]), key


@pytest.mark.parametrize("n_iter", [1, 2])
@pytest.mark.parametrize("scheduled", [False, True])
def test_bitwise_properties(n_iter, scheduled):
    cols = nitinol_columns(20, "nonlinear")
    B, steps, h = 3, 30, 2e-4
    ens = BeamEnsemble(cols, B, force_params=force_params())
    rng = np.random.default_rng(41)
    ens.zero_state()
    ens.step_implicit(20, h, impulse_amp=[0.1, 0.15, 0.2], t0=0.0)
    X = np_(ens.unpack_state())
    lam = rng.normal(0.0, 1.0, (3, B, 2 * ens.n)) * np.max(np.abs(X))
    amps = np.array([0.1, 0.2, 0.3])
    forcing = (dict(control=rng.normal(0.0, 0.01, (5, B, ens.n)) * (np.arange(ens.n) % 3 == 1), control_hold=6) if scheduled
               else dict(held_force=rng.normal(0.0, 0.01, (B, ens.n))))
    common = dict(n_iter=n_iter, x0_red=X, impulse_amp=amps, t0=0.0, impulse_duration=12 * h, record=(ens.n_elem, "phi"),
                  record_every=7, lam_record=np.ones((B, steps // 7)))

    def run(lm, ce, pg=True):
        if pg:
            return ens.step_implicit_adjoint_params(steps, h, lm, checkpoint_every=ce, **common, **forcing)
        from continuum_robot.batched import ControlSchedule
        held = ControlSchedule(forcing["control"], forcing["control_hold"]) if scheduled else forcing["held_force"]
        return ens.step_implicit_adjoint(steps, h, lm, checkpoint_every=ce, held_force=held, **common)

    ref = run(lam, 1)
    assert all(torch.isfinite(v).all() for v in ref[3].values())
    assert all(float(ref[3][k].abs().max()) > 0 for k in ("EA_scale", "EI_scale", "drag_scale", "gravity"))
    for ce in (7, 11, steps, None):            # (11 does not divide 30)
        same(ref, run(lam, ce))
    for d in range(3):
        same(ref, run(lam[d], 7), pick=lambda t: t[d])
    plain = run(lam, 7, False)
    assert len(plain) == 3
    for r, g in zip(ref[:3], plain):
        assert torch.equal(r, g)


def test_param_bar_accumulates_exactly():
    """crb_step_implicit_adjoint_params ADDS to param_bar (the Python method always hands it zeros, so this goes through the
    C ABI): a sweep with a zero cotangent leaves a filled buffer as it is, bit for bit; a second sweep of the same cotangent
    from the first's result doubles it to the rounding of its own additions (steps * n_iter of them per accumulator); records
    5 .. 7 stay zero."""
    import ctypes as C

    from continuum_robot import _native as nat

    cols = nitinol_columns(12, "nonlinear")
    B, steps, h, n_iter, every = 2, 12, 2e-4, 2, 5
    ens = BeamEnsemble(cols, B, force_params=force_params())
    lam = np.zeros((1, B, 2 * ens.n))
    lam[:, :, ens.n - 2] = 1.0
    desc, keep = ens._input_desc(AMPS, 10 * h, -2, None)
    x = ens.pack_state(np.zeros((B, 2 * ens.n)))
    ckpt = torch.empty((-(-steps // every), B, 3, ens.n_node, 4), dtype=torch.float64, device=ens.device)
    t_end = C.c_double(0.0)
    with ens._on_device():
        nat.check(ens._lib.crb_step_implicit_checkpoint(ens.plan.h, ens._ptr(x), 0.0, h, steps, n_iter, every, C.byref(desc), None,
                                                        ens._ptr(ckpt), C.byref(t_end), ens._stream()))
    work = torch.empty(ens._lib.crb_implicit_adjoint_params_work_bytes(ens.plan.h, every, n_iter, 1) // 8, dtype=torch.float64,
                       device=ens.device)

    def sweep(cot, pbar):
        lamd = ens._pack_dirs(torch.as_tensor(cot, dtype=torch.float64, device=ens.device), True)
        pg = nat.ParamCotangent()
        pg.param_bar = pbar.data_ptr()
        with ens._on_device():
            nat.check(ens._lib.crb_step_implicit_adjoint_params(ens.plan.h, ens._ptr(ckpt), ens._ptr(lamd), 1, 0.0, h, steps, n_iter,
                                                                every, C.byref(desc), None, None, C.byref(pg), ens._ptr(work),
                                                                ens._stream()))
        torch.cuda.synchronize()

    pbar = torch.zeros((1, B, ens.n_node, 8), dtype=torch.float64, device=ens.device)
    sweep(lam, pbar)
    first = pbar.clone()
    assert float(first[..., 0].abs().max()) > 0 and float(first[..., 2].abs().max()) > 0
    sweep(0.0 * lam, pbar)
    assert torch.equal(pbar, first)
    sweep(lam, pbar)
    assert torch.all(pbar[..., 5:] == 0)
    for c in range(5):
        scale = float(first[..., c].abs().max())
        assert float((pbar[..., c] - 2.0 * first[..., c]).abs().max()) <= 8 * steps * n_iter * np.finfo(float).eps * scale, c
    del keep


# ---- 6. exact zeros
def test_exact_zeros():
    cols = nitinol_columns(12, "nonlinear")
    B, steps, h = 2, 20, 2e-4
    lam = np.ones((B, 72))
    kw = dict(x0_red=np.zeros((B, 72)), impulse_amp=AMPS, t0=0.0, checkpoint_every=6)
    g = BeamEnsemble(cols, B, force_params=force_params(False, True)).step_implicit_adjoint_params(steps, h, lam, **kw)[3]
    for key in ("drag_scale", "fluid_density", "drag_coef"):
        assert torch.all(g[key] == 0), key
    assert float(g["gravity"].abs().max()) > 0 and float(g["EA_scale"].abs().max()) > 0
    g = BeamEnsemble(cols, B, force_params=force_params(True, False)).step_implicit_adjoint_params(steps, h, lam, **kw)[3]
    assert torch.all(g["gravity"] == 0)
    assert float(g["drag_scale"].abs().max()) > 0
    # node 0 of a plan whose node 0 is FIXED in every beam (off == 1): no slot, written zero
    assert torch.all(g["drag_scale"][:, 0] == 0)
    # padding of a mixed ensemble
    sets = [nitinol_columns(6, "nonlinear"), nitinol_columns(12, "linear", bcs=pinned_root(12))]
    ens = BeamEnsemble(sets, 2, force_params=[force_params(), force_params()])
    g = ens.step_implicit_adjoint_params(steps, h, np.ones((2, 2 * ens.n)), x0_red=np.zeros((2, 2 * ens.n)), impulse_amp=AMPS,
                                         t0=0.0)[3]
    for key in ("EA_scale", "EI_scale", "elastic_modulus", "moment_inertia", "drag_coef"):
        assert tuple(g[key].shape) == (2, 12)
        assert torch.all(g[key][0, 6:] == 0), key
        assert float(g[key][0, :6].abs().max()) > 0, key
    assert tuple(g["drag_scale"].shape) == (2, 13) and torch.all(g["drag_scale"][0, 7:] == 0)
    assert float(g["drag_scale"][0, :7].abs().max()) > 0


# ---- 7. heterogeneous ensemble: packed, two-wave and four-wave members, per-beam ForceParams
def test_heterogeneous_ensemble_matches_each_beam_alone():
    sets = [nitinol_columns(6, "nonlinear"), nitinol_columns(100, "nonlinear", bcs=pinned_root(100)),
            nitinol_columns(200, ["linear", "nonlinear"] * 100, bcs=interior_pin(200))]
    fps = [force_params(True, True), force_params(False, True), force_params(True, False)]
    ens = BeamEnsemble.from_dataframes(sets, force_params=fps)
    singles = [BeamEnsemble(s, 1, force_params=f) for s, f in zip(sets, fps)]
    amps = np.array([0.1, 0.2, 0.3])
    steps, h = 25, 2e-4
    lams = []
    for s in singles:
        lm = np.zeros(2 * s.n)
        lm[s.n - 2] = 1.0
        lm[2 * s.n - 2] = 1e-4
        lams.append(lm)
    X = np.zeros((3, 2 * ens.n))
    got = ens.step_implicit_adjoint_params(steps, h, ens.pad_states(lams), x0_red=X, impulse_amp=amps, t0=0.0, checkpoint_every=10)[3]
    for b, s in enumerate(singles):
        want = s.step_implicit_adjoint_params(steps, h, lams[b][None], x0_red=np.zeros((1, 2 * s.n)), impulse_amp=amps[b:b + 1],
                                              t0=0.0, checkpoint_every=10)[3]
        for key, w in want.items():
            w = np_(w)[0]
            g = np_(got[key])[b]
            if w.ndim == 1:
                assert np.all(g[w.size:] == 0), (b, key)
                g = g[:w.size]
            scale = np.max(np.abs(w))
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-13 * scale, err_msg=f"beam {b} {key}")


# ---- 8. side effects
def test_no_side_effects():
    cols = nitinol_columns(16, "nonlinear")
    B, h = 3, 2e-4
    ens = BeamEnsemble(cols, B, force_params=force_params())
    ens.step_implicit(20, h, impulse_amp=np.array([0.1, 0.2, 0.3]))
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    out = ens.step_implicit_adjoint_params(30, h, np.ones((B, 2 * ens.n)), impulse_amp=np.array([0.1, 0.2, 0.3]))
    assert len(out) == 4 and float(out[3]["elastic_modulus"].abs().max()) > 0
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)


# ---- 9. full size
def test_full_size_4096_beams_of_256_elements():
    cols = nitinol_columns(256, "nonlinear")
    B, steps, h = 4096, 4, 1e-4
    fp = force_params(True, False)
    ens = BeamEnsemble(cols, B, force_params=fp)
    amps = np.linspace(0.1, 0.5, B)
    lam = np.zeros((B, 2 * ens.n))
    lam[:, ens.n - 2] = 1.0
    out = ens.step_implicit_adjoint_params(steps, h, lam, x0_red=np.zeros((B, 2 * ens.n)), impulse_amp=amps, t0=0.0,
                                           impulse_duration=2 * h)
    for v in out[3].values():
        assert torch.isfinite(v).all()
    pick = [0, 2047, 4095]
    small = BeamEnsemble(cols, 3, force_params=fp)
    want = small.step_implicit_adjoint_params(steps, h, lam[pick], x0_red=np.zeros((3, 2 * ens.n)), impulse_amp=amps[pick], t0=0.0,
                                              impulse_duration=2 * h)
    # bitwise: the three plain returns and every per-element / per-node entry of the records.  fluid_density, drag_coef and gravity
    # are torch sums over nodes of those records, whose reduction order torch chooses by the tensor's shape: to rounding.
    for r, g in zip(out[:3], want[:3]):
        assert torch.equal(r[pick], g)
    for key in ("EA_scale", "EI_scale", "elastic_modulus", "moment_inertia", "drag_scale"):
        assert torch.equal(out[3][key][pick], want[3][key]), key
    for key in ("fluid_density", "drag_coef", "gravity"):
        assert torch.allclose(out[3][key][pick], want[3][key], rtol=1e-13, atol=0.0), key
    assert float(want[3]["elastic_modulus"].abs().max()) > 0 and float(want[3]["drag_coef"].abs().max()) > 0
