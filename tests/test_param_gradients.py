"""Parameter gradients of the adjoint rollout on the GPU (BeamEnsemble.step_adjoint_params,
crb_step_rk4_adjoint_params, crb_paramgrad.h): stiffness, drag and gravity gradients of a recorded-tip loss against central
differences of the C oracle with perturbed constructor columns, on every thread mapping; bitwise independence of the checkpoint
interval and of cotangent batching; exact zeros; heterogeneous ensembles; side effects; the full-size ensemble.

Central differences.  The rule is test_adjoint.py's: |g - FD(h/4)| <= min(max(1e-7, 4 |FD(h) - FD(h/4)|), 1e-6) |FD(h/4)|.  The
step sizes are those at which the ORACLE'S OWN two differences agree (run on the CPU with the losses of this file, before
any kernel was compared): h = 1e-4 for the stiffness directions and g_x, 1e-3 for drag, fluid density and g_y.  The figures of
that run are in the docstrings of the tests."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams
from tests.helpers import nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu

DT = 2e-5
RHO_F, G_Y = 1000.0, -9.81
C_REC = np.array([0.5, -1.0, 2.0, 0.25])          # weights of the four recorded tip samples
AMPS = np.array([0.15, 0.3])
STEP_SIZE = {"elastic_modulus": 1e-4, "moment_inertia": 1e-4, "drag_coef": 1e-3, "fluid_density": 1e-3, "g_y": 1e-3, "g_x": 1e-4}
ALL_DIRECTIONS = tuple(STEP_SIZE)
# the 32-element nonlinear rod answers g_x steeply (the shipped f1 makes its axial response stiff): with this file's loss the
# oracle's two differences at h = 1e-4 are 1.1e-3 apart, at 1e-5 1.1e-5, at 1e-6 1.1e-7 -- so that case differences g_x at 1e-6
STEP_SIZE_OF_CASE = {"nonlinear_32": {"g_x": 1e-6}}


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def force_params(drag=True, grav=True):
    return ForceParams(fluid_density=RHO_F if drag else 0.0, enable_fluid_effects=drag, enable_gravity_effects=grav)


def xi_of(n):
    """the seeded random element weights of the column directions: E_e (1 + eps xi_e)"""
    return np.random.default_rng(77).uniform(0.5, 1.5, n)


def perturbed_oracle(cols, direction, eps, drag=True, grav=True):
    """the oracle of the beam with one constructor input moved by eps along ``direction``"""
    c = {k: np.array(v, copy=True) for k, v in cols.items()}
    kw = dict(fluid_density=RHO_F if drag else 0.0, enable_fluid=drag, enable_gravity=grav, gravity=(0.0, G_Y, 0.0))
    if direction in ("elastic_modulus", "moment_inertia", "drag_coef"):
        c[direction] = c[direction] * (1.0 + eps * xi_of(len(c[direction])))
    elif direction == "fluid_density":
        kw["fluid_density"] = RHO_F * (1.0 + eps)
    elif direction == "g_y":
        kw["gravity"] = (0.0, G_Y * (1.0 + eps), 0.0)
    elif direction == "g_x":
        kw["gravity"] = (eps * 9.81, G_Y, 0.0)
    else:
        raise KeyError(direction)
    return oracle_beam(c, **kw)


def oracle_loss(ob, amp, steps, every, weights):
    """w_tip(T) + sum_k weights[k] w_tip(t_k), t_k the end of step every (k + 1): the rollout from rest under the tip impulse,
    continued from sample to sample (the clock only decides the impulse window, which outlasts every rollout here)"""
    tip = ob.n - 2
    x, k, loss = np.zeros(2 * ob.n), 0, 0.0
    for j, wj in enumerate(weights):
        x = ob.rk4_impulse(x, DT, every * (j + 1) - k, amp, t0=k * DT)
        k = every * (j + 1)
        loss += wj * x[tip]
    if k < steps:
        x = ob.rk4_impulse(x, DT, steps - k, amp, t0=k * DT)
    return loss + x[tip]


def oracle_differences(cols, direction, amp, steps, every, weights, drag=True, grav=True, what=None):
    """(FD(h), FD(h/4)) of the loss along ``direction``, h = STEP_SIZE[direction] unless the case ``what`` has its own"""
    h = STEP_SIZE_OF_CASE.get(what, {}).get(direction, STEP_SIZE[direction])
    L = lambda e: oracle_loss(perturbed_oracle(cols, direction, e, drag, grav), amp, steps, every, weights)   # noqa: E731
    return (L(h) - L(-h)) / (2 * h), (L(h / 4) - L(-h / 4)) / (h / 2)


def directional(grads, cols, direction, b):
    """the derivative of the loss of beam ``b`` along ``direction`` from step_adjoint_params' dict"""
    if direction in ("elastic_modulus", "moment_inertia", "drag_coef"):
        n = len(cols[direction])
        return float(np.sum(xi_of(n) * cols[direction] * np_(grads[direction])[b, :n]))
    if direction == "fluid_density":
        return RHO_F * float(np_(grads["fluid_density"])[b])
    if direction == "g_y":
        return G_Y * float(np_(grads["gravity"])[b, 1])
    return 9.81 * float(np_(grads["gravity"])[b, 0])


def tip_loss_gradients(ens, steps, every, weights, amps, **kw):
    """step_adjoint_params for the loss of oracle_loss"""
    B, n = ens.n_beams, ens.n
    lam = np.zeros((B, 2 * n))
    lam[:, n - 2] = 1.0
    rec = dict(record=(ens.n_elem, "w"), record_every=every, lam_record=np.broadcast_to(weights, (B, len(weights))).copy())
    return ens.step_adjoint_params(steps, DT, lam, x0_red=np.zeros((B, 2 * n)), impulse_amp=amps, t0=0.0, **rec, **kw)


def check_against_oracle(cols, directions, steps, every, weights, what, amps=AMPS, beams=None):
    ens = BeamEnsemble(cols, len(amps), force_params=force_params())
    grads = tip_loss_gradients(ens, steps, every, weights, amps)[3]
    for b in (range(len(amps)) if beams is None else beams):
        for direction in directions:
            fd1, fd4 = oracle_differences(cols, direction, amps[b], steps, every, weights, what=what)
            g = directional(grads, cols, direction, b)
            allowed = min(max(1e-7, 4 * abs(fd1 - fd4) / abs(fd4)), 1e-6)
            err = abs(g - fd4) / abs(fd4)
            print(f"[param-grad] {what} beam {b} {direction}: g {g:.12e} FD(h/4) {fd4:.12e} err {err:.2e} allowed {allowed:.2e} "
                  f"|FD(h)-FD(h/4)| {abs(fd1 - fd4) / abs(fd4):.2e}")
            assert err <= allowed, (what, b, direction, g, fd4, err, allowed)


# ---- 1. the recorded-tip loss of test_adjoint.py, 200 steps from rest, every direction
ORACLE_CASES = {"nonlinear_32": (32, "nonlinear"), "linear_32": (32, "linear"), "nonlinear_8_packed": (8, "nonlinear")}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_parameter_gradients_match_oracle_differences(name):
    """The oracle's own |FD(h) - FD(h/4)| / |FD(h/4)| with this loss, on the CPU, both amplitudes (bar: 2.5e-7): elastic_modulus and
    moment_inertia <= 6.7e-8 (32 nonlinear), 6.2e-8 (32 linear), 1.1e-7 (8 nonlinear); drag_coef <= 6.7e-10; fluid_density <=
    5.2e-10; g_y <= 6.8e-11; g_x 1.1e-7 on 32 nonlinear at its own h = 1e-6 (STEP_SIZE_OF_CASE), 2.7e-8 on 32 linear and
    1.7e-7 on 8 nonlinear at 1e-4.  No direction was dropped."""
    n, kind = ORACLE_CASES[name]
    check_against_oracle(nitinol_columns(n, kind), ALL_DIRECTIONS, 200, 50, C_REC, name)


# ---- 2. every thread mapping, 100 steps (samples every 25)
def pinned_root(n):
    return ["PINNED"] + ["NONE"] * (n - 1)


def interior_pin(n):
    return ["FIXED"] + ["NONE"] * (n // 2 - 1) + ["PINNED"] + ["NONE"] * (n - n // 2 - 1)


MAPPING_CASES = {
    "linear_1": (1, "linear", None), "linear_6": (6, "linear", None), "linear_33": (33, "linear", None),
    "linear_64": (64, "linear", None), "linear_65": (65, "linear", None), "linear_129": (129, "linear", None),
    "linear_256": (256, "linear", None),
    "pinned_root_32_slots": (31, "linear", pinned_root), "interior_pin_32_slots": (32, "linear", interior_pin),
    "nonlinear_64": (64, "nonlinear", None),
}


@pytest.mark.parametrize("name", list(MAPPING_CASES))
def test_parameter_gradients_on_every_mapping(name):
    """The oracle's own |FD(h) - FD(h/4)| / |FD(h/4)| on these ten beams, both amplitudes (bar: 2.5e-7): elastic_modulus <= 4.5e-8,
    fluid_density <= 9.0e-10, g_y <= 1.3e-8.  No case was dropped."""
    n, kind, bcs = MAPPING_CASES[name]
    cols = nitinol_columns(n, kind, bcs=bcs(n) if bcs else None)
    check_against_oracle(cols, ("elastic_modulus", "fluid_density", "g_y"), 100, 25, C_REC, name)


# ---- 3. bitwise: checkpoint intervals, cotangent batching, repeated calls, and the plain path's returns
def test_bitwise_properties():
    cols = nitinol_columns(20, "nonlinear")
    B, steps = 3, 60
    ens = BeamEnsemble(cols, B, force_params=force_params())
    rng = np.random.default_rng(41)
    ens.step(20, DT, impulse_amp=np.linspace(0.1, 0.2, B))
    X = np_(ens.unpack_state())
    lam = rng.normal(0.0, 1.0, (3, B, 2 * ens.n)) * np.max(np.abs(X))
    amps = np.array([0.1, 0.2, 0.3])
    U = rng.normal(0.0, 0.01, (B, ens.n))
    run = lambda lm, ce, pg=True: (ens.step_adjoint_params if pg else ens.step_adjoint)(   # noqa: E731
        steps, DT, lm, x0_red=X, impulse_amp=amps, held_force=U, t0=0.0, record=(ens.n_elem, "phi"), record_every=7,
        lam_record=np.ones((B, steps // 7)), checkpoint_every=ce)

    def same(a, b, pick=lambda t: t):
        for r, g in zip(a[:3], b[:3]):
            assert torch.equal(pick(r), g)
        assert set(a[3]) == set(b[3])
        for key in a[3]:
            assert torch.equal(pick(a[3][key]), b[3][key]), key

    ref = run(lam, 1)
    assert any(float(v.abs().max()) > 0 for v in ref[3].values())
    for ce in (7, steps, None):
        same(ref, run(lam, ce))
    for d in range(3):
        same(ref, run(lam[d], 7), pick=lambda t: t[d])
    same(ref, run(lam, 1))
    plain = run(lam, 7, False)
    assert len(plain) == 3
    for r, g in zip(ref[:3], plain):
        assert torch.equal(r, g)


# ---- 4. exact zeros
def test_exact_zeros():
    cols = nitinol_columns(12, "nonlinear")
    B, steps = 2, 40
    lam = np.ones((B, 2 * 36))
    kw = dict(x0_red=np.zeros((B, 72)), impulse_amp=AMPS, t0=0.0)
    g = BeamEnsemble(cols, B, force_params=force_params(False, True)).step_adjoint_params(steps, DT, lam, **kw)[3]
    for key in ("drag_scale", "fluid_density", "drag_coef"):
        assert torch.all(g[key] == 0), key
    assert float(g["gravity"].abs().max()) > 0 and float(g["EA_scale"].abs().max()) > 0
    g = BeamEnsemble(cols, B, force_params=force_params(True, False)).step_adjoint_params(steps, DT, lam, **kw)[3]
    assert torch.all(g["gravity"] == 0)
    assert float(g["drag_scale"].abs().max()) > 0
    g = BeamEnsemble(cols, B, force_params=force_params()).step_adjoint_params(steps, DT, 0.0 * lam, **kw)[3]
    for key, v in g.items():
        assert torch.all(v == 0), key
    # padding of a mixed ensemble
    sets = [nitinol_columns(6, "nonlinear"), nitinol_columns(12, "linear", bcs=pinned_root(12))]
    ens = BeamEnsemble(sets, 2, force_params=[force_params(), force_params()])
    g = ens.step_adjoint_params(steps, DT, np.ones((2, 2 * ens.n)), x0_red=np.zeros((2, 2 * ens.n)), impulse_amp=AMPS,
                                t0=0.0)[3]
    for key in ("EA_scale", "EI_scale", "elastic_modulus", "moment_inertia", "drag_coef"):
        assert tuple(g[key].shape) == (2, 12)
        assert torch.all(g[key][0, 6:] == 0), key
        assert float(g[key][0, :6].abs().max()) > 0, key
    assert tuple(g["drag_scale"].shape) == (2, 13) and torch.all(g["drag_scale"][0, 7:] == 0)
    assert float(g["drag_scale"][0, :7].abs().max()) > 0


# ---- 5. heterogeneous ensemble: packed, two-wave and four-wave members, per-beam ForceParams
def test_heterogeneous_ensemble_matches_each_beam_alone():
    sets = [nitinol_columns(6, "nonlinear"), nitinol_columns(100, "linear", bcs=pinned_root(100)),
            nitinol_columns(200, "nonlinear", bcs=interior_pin(200))]
    fps = [force_params(True, True), force_params(False, True), force_params(True, False)]
    ens = BeamEnsemble(sets, 3, force_params=fps)
    singles = [BeamEnsemble(s, 1, force_params=f) for s, f in zip(sets, fps)]
    amps = np.array([0.1, 0.2, 0.3])
    steps = 50
    lams = []
    for s in singles:
        lm = np.zeros(2 * s.n)
        lm[s.n - 2] = 1.0
        lm[2 * s.n - 2] = 1e-4
        lams.append(lm)
    X = np.zeros((3, 2 * ens.n))
    got = ens.step_adjoint_params(steps, DT, ens.pad_states(lams), x0_red=X, impulse_amp=amps, t0=0.0)[3]
    for b, s in enumerate(singles):
        want = s.step_adjoint_params(steps, DT, lams[b][None], x0_red=np.zeros((1, 2 * s.n)), impulse_amp=amps[b:b + 1],
                                     t0=0.0)[3]
        for key, w in want.items():
            w = np_(w)[0]
            g = np_(got[key])[b]
            if w.ndim == 1:
                assert np.all(g[w.size:] == 0), (b, key)
                g = g[:w.size]
            scale = np.max(np.abs(w))
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-13 * scale, err_msg=f"beam {b} {key}")


# ---- 6. side effects
def test_no_side_effects():
    cols = nitinol_columns(16, "nonlinear")
    B = 3
    ens = BeamEnsemble(cols, B, force_params=force_params())
    ens.step(20, DT, impulse_amp=np.array([0.1, 0.2, 0.3]))
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    out = ens.step_adjoint_params(100, DT, np.ones((B, 2 * ens.n)), impulse_amp=np.array([0.1, 0.2, 0.3]))
    assert len(out) == 4 and float(out[3]["elastic_modulus"].abs().max()) > 0
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)


# ---- 7. full size
def test_full_size_4096_beams_of_256_elements():
    """The loss keeps its four samples (every 5 steps).  The oracle's own |FD(h) - FD(h/4)| / |FD(h/4)| on the three beams:
    elastic_modulus <= 7.6e-10, fluid_density <= 6.5e-9."""
    cols = nitinol_columns(256, "nonlinear")
    B, steps = 4096, 20
    ens = BeamEnsemble(cols, B, force_params=force_params(True, False))
    amps = np.linspace(0.1, 0.5, B)
    grads = tip_loss_gradients(ens, steps, 5, C_REC, amps)[3]
    for v in grads.values():
        assert torch.isfinite(v).all()
    for b in (0, 2047, 4095):
        for direction in ("elastic_modulus", "fluid_density"):
            fd1, fd4 = oracle_differences(cols, direction, amps[b], steps, 5, C_REC, True, False)
            g = directional(grads, cols, direction, b)
            allowed = min(max(1e-7, 4 * abs(fd1 - fd4) / abs(fd4)), 1e-6)
            err = abs(g - fd4) / abs(fd4)
            print(f"[param-grad] full size beam {b} {direction}: g {g:.12e} FD(h/4) {fd4:.12e} err {err:.2e} allowed {allowed:.2e}")
            assert err <= allowed, (b, direction, g, fd4, err, allowed)
