"""Tangent of the implicit stepper on the GPU (BeamEnsemble.step_implicit_tangent / linearize_implicit,
crb_implicit_tangent.h).  tests/test_implicit_tangent_cpu.py proves the inputs of the finite-difference test and the dense
Cayley recursion on the oracle alone; tests/README_implicit_tangent.md lists the measured figures.

  1. tangent and adjoint are transposes: identity seeds against identity cotangents on the linear rods, the dot-product identity
     <lam, J v> = <J^T lam, v> on the nonlinear ones -- two exact derivatives of one statement of the map, by different functions;
  2. on a linear rod the tangent is step_implicit's rollout of the perturbation;
  3. central differences of the oracle under fd_check's rule;
  4. the base state against step_implicit, the clock, the status;
  5. the dot-product identity on every thread mapping, and the impulse window's edges;
  6. bitwise: batching, broadcasting, the chain of one call per schedule interval; linearity in the seed;
  7. linearize_implicit against the Cayley recursion of linearize()'s (A, B), its side effects, padding;
  8. a digital LQR designed on linearize_implicit closes the loop that the recursion predicts;
  9. edges: non-finite seeds, 257 slots, no steps, full size.

A bound written min(16 x measured, STM_CAP) takes `measured` from MEASURED below: the figure of the first run on one MI355X.
Every such comparison prints ``[implicit-tangent] key | err | allowed`` (pytest -s)."""
import numpy as np
import pytest
import torch

from continuum_robot import _native as nat
from continuum_robot.batched import BeamEnsemble, ControlSchedule
from tests.helpers import assert_blocks, block_errs, nitinol_columns
from tests.test_adjoint import np_
from tests.test_control_schedule import Case
from tests.test_derivative_mappings import clock
from tests.test_implicit_adjoint import FD_CASES, FD_STEPS, STM_CAP, STM_CASES, blockwise
from tests.test_implicit_adjoint_mappings_cpu import AMP_SCALE, CASES, HELD_SCALE, T0, _Ones, case_columns
from tests.test_implicit_tangent_cpu import LINEAR_RODS, TAG, cayley, fd_case
from tests.test_tangent_linear import directions, fd_check, force_params

pytestmark = pytest.mark.gpu

# key -> the figure of the first run on one MI355X (tests/README_implicit_tangent.md)
MEASURED = {
    "transpose packed_6 Phi": 6.41e-15,
    "transpose packed_6 G": 6.95e-15,
    "transpose two_waves_65 Phi": 3.23e-14,
    "transpose two_waves_65 G": 4.83e-15,
    "transpose four_waves_130_padding Phi": 6.97e-14,
    "transpose four_waves_130_padding G": 1.05e-14,
    "transpose all_8_levels_256 Phi": 3.33e-13,
    "transpose all_8_levels_256 G": 6.66e-14,
    "transpose one_element_70_beams Phi": 2.19e-15,
    "transpose one_element_70_beams G": 6.30e-15,
    "transpose packed_pinned_10 Phi": 1.96e-14,
    "transpose packed_pinned_10 G": 1.18e-14,
    "transpose two_waves_65_slots_pinned_64 Phi": 3.23e-14,
    "transpose two_waves_65_slots_pinned_64 G": 4.83e-15,
    "transpose pin_on_the_seam_128 Phi": 6.90e-14,
    "transpose pin_on_the_seam_128 G": 1.05e-14,
    "duality n8_drag_grav": 1.37e-14,
    "duality n32_one_iteration": 8.20e-14,
    "duality n32_two_iterations": 9.27e-14,
    "duality n64_drag_three_iterations": 1.02e-14,
    "duality n10_mixed_kinds": 1.63e-15,
    "duality n8_pinned_root_grav": 3.55e-15,
    "rollout packed_6 Phi": 5.01e-15,
    "rollout packed_6 G": 4.13e-15,
    "rollout two_waves_65 Phi": 8.30e-15,
    "rollout two_waves_65 G": 1.48e-15,
    "rollout four_waves_130_padding Phi": 6.46e-14,
    "rollout four_waves_130_padding G": 2.21e-14,
    "rollout all_8_levels_256 Phi": 2.83e-13,
    "rollout all_8_levels_256 G": 7.42e-14,
    "mapping one_element": 4.35e-15,
    "mapping packed_partial": 3.42e-13,
    "mapping packed_pinned": 4.14e-14,
    "mapping two_per_wave_pin": 8.71e-14,
    "mapping one_wave_full": 6.06e-15,
    "mapping two_waves_min": 2.00e-15,
    "mapping two_waves_pin_on_seam": 3.95e-13,
    "mapping four_waves_min": 2.78e-14,
    "mapping four_waves_padded": 5.83e-14,
    "mapping four_waves_full": 2.72e-14,
    "window packed_partial on_the_midpoint": 1.04e-13,
    "window packed_partial one_ulp_past_the_midpoint": 4.82e-14,
    "window packed_partial on_the_first_midpoint": 3.64e-13,
    "window packed_partial beyond_the_end": 6.14e-14,
    "window two_waves_padded on_the_midpoint": 1.48e-14,
    "window two_waves_padded one_ulp_past_the_midpoint": 1.80e-14,
    "window two_waves_padded on_the_first_midpoint": 1.57e-14,
    "window two_waves_padded beyond_the_end": 1.25e-14,
    "linearize n6_h1e-4 1 step(s) A_d": 1.16e-12,
    "linearize n6_h1e-4 1 step(s) B_d": 7.19e-14,
    "linearize n6_h1e-4 3 step(s) A_d": 7.00e-13,
    "linearize n6_h1e-4 3 step(s) B_d": 4.52e-14,
    "linearize n10_h1e-3 1 step(s) A_d": 1.07e-12,
    "linearize n10_h1e-3 1 step(s) B_d": 4.84e-13,
    "linearize n64_h1e-3 1 step(s) A_d": 1.98e-12,
    "linearize n64_h1e-3 1 step(s) B_d": 1.09e-12,
    "closed loop 50 samples": 7.10e-13,
}


def allowed(key, err):
    """min(16 x measured, STM_CAP), with the figure printed"""
    tol = min(16.0 * MEASURED[key], STM_CAP)
    print(f"{TAG} {key} | err {err:.2e} | allowed {tol:.2e}")
    return tol


def dev(ens, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64, device=ens.device)


def block_scales(X, fi):
    """[B, 2n]: the per-DOF-block sizes `directions` scales by"""
    return directions(X, _Ones(), 1, fi)[0]


def duality_error(lam, Jv, pairs):
    """| <lam, J v> - sum of <cotangent, seed> over `pairs` | / sum of |the terms on the right|, per beam (axis 1 of [D, B, .]
    arrays), worst over directions and beams"""
    lhs = np.sum(lam * Jv, axis=-1)
    terms = [np.sum(a * b, axis=-1) if a.ndim == 3 else a * b for a, b in pairs]
    rhs, scale = sum(terms), sum(np.abs(t) for t in terms)
    assert np.all(scale > 0.0)
    return float(np.max(np.abs(lhs - rhs) / scale))


# ------------------------------------------------------------------ 1. tangent and adjoint are transposes
@pytest.mark.parametrize("name", list(STM_CASES))
def test_identity_seeds_and_identity_cotangents_give_transposed_matrices(name):
    c = STM_CASES[name]
    cols = nitinol_columns(c["n"], "linear", bcs=c.get("bcs"))
    steps, h, B = 40, c["h"], c.get("B", 1)
    ens = BeamEnsemble(cols, B, force_params=force_params(False, False))
    n, n2 = ens.n, 2 * ens.n
    eye2, eye1 = np.eye(n2), np.eye(n)
    ens.zero_state()
    Tx = np_(ens.step_implicit_tangent(steps, h, np.repeat(eye2[:, None, :], B, axis=1), n_iter=2, t0=0.0))     # [2n, B, 2n]
    ens.zero_state()
    Tu = np_(ens.step_implicit_tangent(steps, h, np.zeros((n, B, n2)), n_iter=2, t0=0.0,
                                       d_held_force=np.repeat(eye1[:, None, :], B, axis=1)))                    # [n, B, 2n]
    xb, _, fb = ens.step_implicit_adjoint(steps, h, np.repeat(eye2[:, None, :], B, axis=1), n_iter=2, x0_red=np.zeros((B, n2)), t0=0.0)
    xb, fb = np_(xb), np_(fb)
    # Tx[d, b, :] = Phi e_d (column d), xb[d, b, :] = Phi^T e_d (row d); Tu[j, b, :] = G e_j, fb[d, b, :] = G^T e_d
    e_phi = max(blockwise(Tx[:, b, :].T, xb[:, b, :], n) for b in range(B))
    e_g = max(blockwise(Tu[:, b, :].T, fb[:, b, :], n) for b in range(B))
    assert np.max(np.abs(xb)) > 0 and np.max(np.abs(fb)) > 0
    assert e_phi <= allowed(f"transpose {name} Phi", e_phi), (name, e_phi)
    assert e_g <= allowed(f"transpose {name} G", e_g), (name, e_g)


class Nonlinear:
    """An FD case on the GPU: the oracle's start state, the impulse closing inside the run, the held force"""

    def __init__(self, name, B=1):
        self.k = k = fd_case(name)
        self.c, self.i = k.c, k.i
        self.ens = ens = BeamEnsemble(k.i["cols"], B, force_params=force_params(k.c["drag"], k.c["grav"]))
        assert ens.n == k.n and np.array_equal(ens.free_index, k.fi)
        self.B, self.n, self.h = B, k.n, k.c["h"]
        self.X = np.repeat(k.i["X"][None], B, axis=0)
        self.amps = np.full(B, k.i["amp"])
        self.U = np.repeat(k.i["U"][None], B, axis=0)
        self.kw = dict(n_iter=k.c["n_iter"], impulse_duration=k.i["dur"], t0=0.0)

    def tangent(self, dx0, **kw):
        self.ens.set_state(self.X, 0.0)
        return self.ens.step_implicit_tangent(FD_STEPS, self.h, dx0, **dict(self.kw, **kw))


@pytest.mark.parametrize("name", list(FD_CASES))
def test_dot_product_identity_with_the_adjoint_on_nonlinear_rods(name):
    s = Nonlinear(name)
    ens, n, D = s.ens, s.n, 3
    rng = np.random.default_rng(500 + n)
    S = block_scales(s.X, ens.free_index)
    dx0 = rng.normal(0.0, 1.0, (D, 1, 2 * n)) * S[None]
    lam = rng.normal(0.0, 1.0, (D, 1, 2 * n)) / S[None]
    d_amp = rng.normal(0.0, s.i["amp"], (D, 1))
    d_held = np.where(ens.free_index % 3 == 1, rng.normal(0.0, 0.05, (D, 1, n)), 0.0)
    Jv = np_(s.tangent(dx0, impulse_amp=s.amps, held_force=s.U, d_impulse_amp=d_amp, d_held_force=d_held))
    xb, ab, fb = ens.step_implicit_adjoint(FD_STEPS, s.h, lam, x0_red=s.X, impulse_amp=s.amps, held_force=s.U, checkpoint_every=7, **s.kw)
    err = duality_error(lam, Jv, [(np_(xb), dx0), (np_(ab), d_amp), (np_(fb), d_held)])
    assert np.max(np.abs(Jv)) > 0 and np.max(np.abs(np_(ab))) > 0 and np.max(np.abs(np_(fb))) > 0
    assert err <= allowed(f"duality {name}", err), (name, err)


# ------------------------------------------------------------------ 2. linear rod: the tangent is the rollout of the perturbation
@pytest.mark.parametrize("name", list(STM_CASES)[:4])
def test_tangent_of_a_linear_rod_is_the_rollout_of_the_perturbation(name):
    c = STM_CASES[name]
    cols = nitinol_columns(c["n"], "linear")
    steps, h = 40, c["h"]
    fp = force_params(False, False)
    one = BeamEnsemble(cols, 1, force_params=fp)
    n, n2 = one.n, 2 * one.n
    ref = BeamEnsemble(cols, n2, force_params=fp)
    ref.set_state(np.eye(n2))
    ref.step_implicit(steps, h, n_iter=2, t0=0.0)
    Phi = ref.unpack_state().cpu().numpy().T
    frc = BeamEnsemble(cols, n, force_params=fp)
    frc.zero_state()
    frc.step_implicit(steps, h, n_iter=2, held_force=np.eye(n), t0=0.0)
    G = frc.unpack_state().cpu().numpy().T
    one.zero_state()
    Tx = np_(one.step_implicit_tangent(steps, h, np.eye(n2)[:, None, :], n_iter=2, t0=0.0))[:, 0, :].T
    one.zero_state()
    Tu = np_(one.step_implicit_tangent(steps, h, np.zeros((n, 1, n2)), n_iter=2, t0=0.0, d_held_force=np.eye(n)[:, None, :]))[:, 0, :].T
    e_phi, e_g = blockwise(Tx, Phi, n), blockwise(Tu, G, n)
    assert e_phi <= allowed(f"rollout {name} Phi", e_phi), (name, e_phi)
    assert e_g <= allowed(f"rollout {name} G", e_g), (name, e_g)


# ------------------------------------------------------------------ 3. central differences of the oracle
@pytest.mark.parametrize("name", list(FD_CASES))
def test_tangent_matches_central_differences_of_the_oracle(name):
    s = Nonlinear(name)
    k, i, n = s.k, s.i, s.n
    zero = np.zeros((1, 2 * n))
    runs = {
        "x0": lambda: s.tangent(i["dX"][None], impulse_amp=s.amps),
        "amp": lambda: s.tangent(zero, impulse_amp=s.amps, d_impulse_amp=s.amps),
        "held": lambda: s.tangent(zero, held_force=s.U, d_held_force=i["dU"][None]),
    }
    for kind, run in runs.items():
        jvp = np_(run())[0]
        errs = fd_check(jvp, k.F(kind), k.eps[kind], k.fi, f"{name}: {kind}")
        print(f"{TAG} fd {name} {kind} | " + " ".join(f"{b} {e:.1e}" for b, e in errs.items()))


# ------------------------------------------------------------------ 4. the base state, the clock, the status
@pytest.mark.parametrize("name", list(FD_CASES))
def test_base_state_clock_and_status_are_step_implicits(name):
    s = Nonlinear(name, B=2)
    ens = s.ens
    twin = BeamEnsemble(s.i["cols"], 2, force_params=force_params(s.c["drag"], s.c["grav"]))
    inp = dict(impulse_amp=s.amps, held_force=s.U, n_iter=s.c["n_iter"], impulse_duration=s.i["dur"])
    for e in (ens, twin):
        e.set_state(s.X, 3e-4)
        assert int(e.status.abs().max()) == 0
    ens.step_implicit_tangent(FD_STEPS, s.h, np.ones((2, 2 * s.n)), **inp)
    twin.step_implicit(FD_STEPS, s.h, **inp)
    assert ens.time == twin.time == clock(3e-4, s.h, FD_STEPS)
    errs = assert_blocks(np_(ens.unpack_state()), np_(twin.unpack_state()), ens.free_index, 1e-7, what=f"{name}: base")
    print(f"{TAG} base {name} | worst block {max(errs.values()):.2e} | allowed 1.00e-07")
    assert int(ens.status.abs().max()) == 0
    # the status: a beam that goes non-finite is marked with the ensemble's step count, as step_implicit marks it
    for e in (ens, twin):
        x = e.unpack_state()
        x[1, 0] = float("nan")
        e.state = e.pack_state(x)
    ens.step_implicit_tangent(5, s.h, np.ones((2, 2 * s.n)), n_iter=s.c["n_iter"])
    twin.step_implicit(5, s.h, n_iter=s.c["n_iter"])
    assert ens.status.tolist() == twin.status.tolist() == [0, FD_STEPS + 5]
    assert ens.time == twin.time


# ------------------------------------------------------------------ 5. every mapping
MAP_STEPS, MAP_WINDOW = 30, 12.3
MAP_CASES = {"one_element": 2, "packed_partial": 1, "packed_pinned": 3, "two_per_wave_pin": 2, "one_wave_full": 1, "two_waves_min": 3,
             "two_waves_pin_on_seam": 2, "four_waves_min": 1, "four_waves_padded": 3, "four_waves_full": 2}     # name -> n_iter


class Mapped:
    """A rod of tests/test_implicit_adjoint_mappings_cpu.CASES on the GPU, drag and gravity on, set up without the oracle: the
    start state is step_implicit's after the case's warm-up under the impulse, the clock starts at T0"""

    def __init__(self, name, n_iter=None):
        c = self.c = CASES[name]
        self.ens = ens = BeamEnsemble(case_columns(c), c["B"], force_params=force_params(True, True), corrected_axial=c["corrected"])
        lay = ens.plan.layout
        assert (lay.n_slots, lay.beams_per_group, lay.threads) == c["layout"], name
        self.B, self.n, self.h = c["B"], ens.n, c["h"]
        self.n_iter = MAP_CASES.get(name, c["n_iter"]) if n_iter is None else n_iter
        self.idx = ens.reduced_index(c["imp"], c["imp_dof"])
        self.amps = c["load"] * AMP_SCALE * np.linspace(1.0, 2.0, self.B)
        self.rng = rng = np.random.default_rng(700 + sum(map(ord, name)))
        self.transverse = (ens.free_index % 3 == 1) if c["kind"] != "linear" else np.ones(ens.n, bool)
        self.U = np.where(self.transverse, rng.normal(0.0, c["load"] * HELD_SCALE, (self.B, ens.n)), 0.0)
        ens.zero_state()
        ens.step_implicit(c["warm"], self.h, n_iter=self.n_iter, impulse_amp=self.amps, impulse_duration=10.0 * self.h,
                          impulse_index=self.idx, t0=0.0)
        self.X = np_(ens.unpack_state())
        assert np.all(np.isfinite(self.X)) and np.max(np.abs(self.X[:, self.n:])) > 0
        self.kw = dict(n_iter=self.n_iter, impulse_index=self.idx, t0=T0, impulse_duration=T0 + MAP_WINDOW * self.h)

    def seeds(self, D=1):
        rng, n, B = self.rng, self.n, self.B
        S = block_scales(self.X, self.ens.free_index)
        return dict(dx0=rng.normal(0.0, 1.0, (D, B, 2 * n)) * S[None], lam=rng.normal(0.0, 1.0, (D, B, 2 * n)) / S[None],
                    d_amp=rng.normal(0.0, 1.0, (D, B)) * self.amps[None],
                    d_held=np.where(self.transverse, rng.normal(0.0, self.c["load"] * HELD_SCALE, (D, B, n)), 0.0))

    def tangent(self, dx0, steps=MAP_STEPS, **kw):
        self.ens.set_state(self.X, T0)
        return self.ens.step_implicit_tangent(steps, self.h, dx0, **dict(self.kw, impulse_amp=self.amps, held_force=self.U, **kw))

    def duality(self, v, **kw):
        Jv = np_(self.tangent(v["dx0"], d_impulse_amp=v["d_amp"], d_held_force=v["d_held"], **kw))
        assert np.all(np.isfinite(Jv)) and np.max(np.abs(Jv)) > 0
        xb, ab, fb = self.ens.step_implicit_adjoint(MAP_STEPS, self.h, v["lam"], x0_red=self.X, impulse_amp=self.amps, held_force=self.U,
                                                    checkpoint_every=7, **dict(self.kw, **kw))
        return duality_error(v["lam"], Jv, [(np_(xb), v["dx0"]), (np_(ab), v["d_amp"]), (np_(fb), v["d_held"])])


@pytest.mark.parametrize("name", list(MAP_CASES))
def test_dot_product_identity_on_every_mapping(name):
    m = Mapped(name)
    on = [clock(T0, m.h, s) + 0.5 * m.h < m.kw["impulse_duration"] for s in range(MAP_STEPS)]
    assert on == [s < 12 for s in range(MAP_STEPS)]                       # the window closes inside step 12: midpoint 11 is the last forced
    err = m.duality(m.seeds())
    assert err <= allowed(f"mapping {name}", err), (name, err)


K_EDGE = 21
EDGES = {
    "on_the_midpoint": lambda h: clock(T0, h, K_EDGE) + 0.5 * h,                                 # step K off (tm < duration fails)
    "one_ulp_past_the_midpoint": lambda h: np.nextafter(clock(T0, h, K_EDGE) + 0.5 * h, np.inf),   # step K on
    "on_the_first_midpoint": lambda h: T0 + 0.5 * h,                                             # off throughout
    "beyond_the_end": lambda h: clock(T0, h, MAP_STEPS) + 3.0 * h,                               # on throughout
}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("name", ["packed_partial", "two_waves_padded"])
def test_impulse_window_edges(name, edge):
    m = Mapped(name, n_iter=CASES[name]["n_iter"])
    dur = float(EDGES[edge](m.h))
    if edge.endswith("the_midpoint"):
        assert (clock(T0, m.h, K_EDGE) + 0.5 * m.h < dur) == (edge == "one_ulp_past_the_midpoint")
    v = m.seeds()
    # the tangent along the amplitude alone: the response of the forced midpoints, exactly 0 when none is forced
    alone = m.tangent(np.zeros_like(v["dx0"]), d_impulse_amp=v["d_amp"], impulse_duration=dur)
    if edge == "on_the_first_midpoint":
        assert torch.equal(alone, torch.zeros_like(alone))
        v["d_amp"] = np.zeros_like(v["d_amp"])       # (and the adjoint's amp_bar is exactly 0 there: no term on the right)
    else:
        assert float(alone.abs().max()) > 0.0
    err = m.duality(v, impulse_duration=dur)
    assert err <= allowed(f"window {name} {edge}", err), (name, edge, err)
    if edge == "one_ulp_past_the_midpoint":          # the two durations differ by step K's forcing: the tangent tells them apart
        off = m.tangent(np.zeros_like(v["dx0"]), d_impulse_amp=v["d_amp"], impulse_duration=float(EDGES["on_the_midpoint"](m.h)))
        assert float((alone - off).abs().max()) > 1e-4 * float(alone.abs().max())


# ------------------------------------------------------------------ 6. bitwise: batching, broadcasting, schedules; linearity
def test_directions_batch_and_broadcast_bitwise_and_the_tangent_is_linear_in_the_seed():
    m = Mapped("two_waves_padded")
    v = m.seeds(D=3)
    kw = dict(d_impulse_amp=v["d_amp"], d_held_force=v["d_held"])
    ref = m.tangent(v["dx0"], **kw)
    base = m.ens.state.clone()
    for d in range(3):
        one = m.tangent(v["dx0"][d], d_impulse_amp=v["d_amp"][d], d_held_force=v["d_held"][d])
        assert torch.equal(one, ref[d]) and torch.equal(m.ens.state, base), d
    # a [B, .] tangent of the inputs serves every direction
    got = m.tangent(v["dx0"], d_impulse_amp=v["d_amp"][0], d_held_force=v["d_held"][0])
    want = m.tangent(v["dx0"], d_impulse_amp=np.stack([v["d_amp"][0]] * 3), d_held_force=np.stack([v["d_held"][0]] * 3))
    assert torch.equal(got, want) and not torch.equal(got, ref)
    # linear in the seed
    a, b = 0.75, -1.5
    mix = np_(m.tangent(a * v["dx0"][0] + b * v["dx0"][1], d_impulse_amp=a * v["d_amp"][0] + b * v["d_amp"][1],
                        d_held_force=a * v["d_held"][0] + b * v["d_held"][1]))
    lin = a * np_(ref[0]) + b * np_(ref[1])
    errs = block_errs(mix, lin, m.ens.free_index)
    print(f"{TAG} linearity | worst block {max(errs.values()):.2e} | allowed 1.00e-12")
    assert max(errs.values()) <= 1e-12, errs


SCHED_STEPS, SCHED_K, SCHED_HOLD = 33, 5, 7
SCHED_CHUNKS = [(k, min(SCHED_HOLD, SCHED_STEPS - k * SCHED_HOLD)) for k in range(SCHED_K)]
SCHED_RUNS = {"packed_6": (1e-4, 2), "two_waves_65": (1e-4, 1), "four_waves_256": (1e-3, 2)}     # mapping -> (h, n_iter)


@pytest.mark.parametrize("name", list(SCHED_RUNS))
def test_scheduled_call_is_bitwise_the_chain_of_one_call_per_interval(name):
    h, n_iter = SCHED_RUNS[name]
    c = Case(name)
    ens, D, B = c.ens, 3, c.ens.n_beams
    X = c.start()
    dX = c.cotangents(D) * 1e-3
    dU = np.stack([c.schedule(SCHED_K) for _ in range(D)])          # [D, K, B, n]
    damp = c.rng.normal(0.0, 1.0, (D, B))
    imp = dict(impulse_amp=c.amps, impulse_duration=12.3 * h, n_iter=n_iter)
    ens.set_state(X, 0.0)
    got = ens.step_implicit_tangent(SCHED_STEPS, h, dX, held_force=ControlSchedule(c.U, SCHED_HOLD), d_held_force=dU, d_impulse_amp=damp, **imp)
    xa, ta = ens.state.clone(), ens.time
    assert torch.isfinite(got).all() and torch.isfinite(xa).all() and float(got.abs().max()) > 0.0
    ens.set_state(X, 0.0)
    d = dX
    for k, n in SCHED_CHUNKS:
        d = ens.step_implicit_tangent(n, h, d, held_force=c.U[k], d_held_force=dU[:, k], d_impulse_amp=damp, **imp)
    assert torch.equal(got, d)
    assert torch.equal(xa, ens.state) and ta == ens.time == clock(0.0, h, SCHED_STEPS)
    # one tangent [K, B, n] serves every direction
    ens.set_state(X, 0.0)
    one = ens.step_implicit_tangent(SCHED_STEPS, h, dX, held_force=ControlSchedule(c.U, SCHED_HOLD), d_held_force=dU[0], **imp)
    ens.set_state(X, 0.0)
    rep = ens.step_implicit_tangent(SCHED_STEPS, h, dX, held_force=ControlSchedule(c.U, SCHED_HOLD), d_held_force=np.stack([dU[0]] * D), **imp)
    assert torch.equal(one, rep)


def test_schedule_of_equal_vectors_differs_from_the_held_force_call():
    """every interval's first step starts from a^0 = 0 and da^0 = 0: K equal vectors are the chain of K calls, not the one call"""
    c = Case("two_waves_65")
    ens, h = c.ens, 1e-4
    X = c.start()
    dX = c.cotangents(1)[0] * 1e-3
    U, dU = c.U[0], c.schedule(1)[0]
    ens.set_state(X, 0.0)
    held = ens.step_implicit_tangent(SCHED_STEPS, h, dX, n_iter=1, held_force=U, d_held_force=dU)
    xh = ens.state.clone()
    ens.set_state(X, 0.0)
    sch = ens.step_implicit_tangent(SCHED_STEPS, h, dX, n_iter=1, held_force=ControlSchedule(np.stack([U] * SCHED_K), SCHED_HOLD),
                                    d_held_force=np.stack([dU] * SCHED_K))
    assert not torch.equal(held, sch) and not torch.equal(xh, ens.state)
    assert float((held - sch).abs().max()) <= 1e-2 * float(held.abs().max())


# ------------------------------------------------------------------ 7. linearize_implicit
LIN_RUNS = [("n6_h1e-4", 1), ("n6_h1e-4", 3), ("n10_h1e-3", 1), ("n64_h1e-3", 1)]


@pytest.mark.parametrize("rod, n_steps", LIN_RUNS, ids=[f"{r}-{s}" for r, s in LIN_RUNS])
def test_linearize_implicit_is_the_cayley_recursion_on_linear_rods(rod, n_steps):
    n_elem, h = LINEAR_RODS[rod]
    ens = BeamEnsemble(nitinol_columns(n_elem, "linear"), 2, force_params=force_params(False, False))
    n = ens.n
    rng = np.random.default_rng(n_elem)
    ens.set_state(1e-3 * rng.normal(0.0, 1.0, (2, 2 * n)), 0.125)
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    A, Bu = (np_(t) for t in ens.linearize())
    got = {it: tuple(np_(t) for t in ens.linearize_implicit(h, n_steps=n_steps, n_iter=it)) for it in (1, 2)}
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)
    for it in (1, 2):
        assert got[it][0].shape == (2, 2 * n, 2 * n) and got[it][1].shape == (2, 2 * n, n)
        for b in range(2):
            Ad, Bd = cayley(A[b], Bu[b], h, n_steps)
            e_a, e_b = blockwise(got[it][0][b], Ad, n), blockwise(got[it][1][b], Bd, n)
            key = f"linearize {rod} {n_steps} step(s)"
            assert e_a <= allowed(f"{key} A_d", e_a), (rod, n_steps, it, b, e_a)
            assert e_b <= allowed(f"{key} B_d", e_b), (rod, n_steps, it, b, e_b)
    # the status reporting goes on where it stood: a later non-finite beam is marked with the ensemble's own step count
    ens.step_implicit(2, h)
    x = ens.unpack_state()
    x[0, 0] = float("nan")
    ens.state = ens.pack_state(x)
    ens.step_implicit(3, h)
    assert ens.status.tolist() == [5, 0]


def test_linearize_implicit_about_an_equilibrium_is_the_tangent_on_identity_seeds():
    cols = nitinol_columns(12, "nonlinear")
    B, h, n_steps = 2, 1e-3, 2
    ens = BeamEnsemble(cols, B, force_params=force_params(True, True))
    n = ens.n
    U = np.where(ens.free_index % 3 == 1, 0.05, 0.0)[None].repeat(B, 0) * np.array([[1.0], [2.0]])
    sol = ens.solve_static(held_force=U)
    assert bool(sol.converged.all())
    x_eq = torch.cat([sol.q, torch.zeros_like(sol.q)], dim=1)
    ens.set_state(np.zeros((B, 2 * n)), 0.5)
    Ad, Bd = ens.linearize_implicit(h, n_steps=n_steps, n_iter=2, x_red=x_eq, held_force=U)
    assert float(ens.state.abs().max()) == 0.0 and ens.time == 0.5
    eye2 = torch.eye(2 * n, dtype=torch.float64, device=ens.device)
    ens.set_state(x_eq, 0.0)
    T = ens.step_implicit_tangent(n_steps, h, eye2[:, None, :].expand(2 * n, B, 2 * n), n_iter=2, held_force=U)
    assert torch.equal(Ad, T.permute(1, 2, 0))
    ens.set_state(x_eq, 0.0)
    Tu = ens.step_implicit_tangent(n_steps, h, torch.zeros((n, B, 2 * n), dtype=torch.float64, device=ens.device), n_iter=2,
                                   held_force=U, d_held_force=torch.eye(n, dtype=torch.float64, device=ens.device)[:, None, :].expand(n, B, n))
    assert torch.equal(Bd, Tu.permute(1, 2, 0))
    # the equilibrium is a fixed point of the map up to the solver's residual, and the two beams differ
    assert float((ens.unpack_state() - x_eq).abs().max()) <= 1e-6 * float(x_eq.abs().max())
    assert not torch.equal(Ad[0], Ad[1]) and float(Bd.abs().max()) > 0


def test_linearize_implicit_pads_mixed_ensembles_with_zeros_and_each_beam_is_as_alone():
    sets = [nitinol_columns(6, "linear"), nitinol_columns(10, "linear")]
    fp = force_params(False, False)
    ens = BeamEnsemble.from_dataframes(sets, force_params=[fp, fp])
    assert ens.mixed_topology
    h, n = 1e-3, ens.n
    Ad, Bd = (np_(t) for t in ens.linearize_implicit(h, n_iter=1))
    for b, cols in enumerate(sets):
        single = BeamEnsemble(cols, 1, force_params=fp)
        wa, wb = (np_(t)[0] for t in single.linearize_implicit(h, n_iter=1))
        nb = single.n
        assert int(ens.n_per_beam[b]) == nb
        rows = np.concatenate([np.arange(nb), n + np.arange(nb)])
        np.testing.assert_allclose(Ad[b][np.ix_(rows, rows)], wa, rtol=0, atol=1e-13 * np.max(np.abs(wa)))
        np.testing.assert_allclose(Bd[b][np.ix_(rows, np.arange(nb))], wb, rtol=0, atol=1e-13 * np.max(np.abs(wb)))
        pad = np.ones(2 * n, bool)
        pad[rows] = False
        assert np.all(Ad[b][pad, :] == 0.0) and np.all(Ad[b][:, pad] == 0.0)
        assert np.all(Bd[b][pad, :] == 0.0) and np.all(Bd[b][:, nb:] == 0.0)
    assert n > 18 - 1 and np.any(Ad[0] != 0.0)


# ------------------------------------------------------------------ 8. closed loop, end to end
def test_digital_lqr_on_the_linearisation_closes_the_loop_the_recursion_predicts():
    scipy_linalg = pytest.importorskip("scipy.linalg")
    h, samples, B = 1e-3, 50, 4
    ens = BeamEnsemble(nitinol_columns(6, "linear"), B, force_params=force_params(False, False))
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
    rho_open, rho = np.max(np.abs(np.linalg.eigvals(Ad))), np.max(np.abs(np.linalg.eigvals(Acl)))
    print(f"{TAG} closed loop | spectral radius open {rho_open:.6f} closed {rho:.6f}")
    assert rho < 1.0
    rng = np.random.default_rng(8)
    x0 = 1e-3 * rng.normal(0.0, 1.0, (B, 2 * n))
    Kd = dev(ens, K)
    ens.set_state(x0, 0.0)
    want = x0.copy()
    tip = n - 2
    worst = 0.0
    for _ in range(samples):
        u = -(ens.unpack_state() @ Kd.T)
        ens.step_implicit(1, h, n_iter=1, held_force=u)
        want = want @ Acl.T
        worst = max(worst, max(block_errs(np_(ens.unpack_state()), want, ens.free_index).values()))
    assert worst <= allowed("closed loop 50 samples", worst), worst
    open_loop = x0.copy()
    for _ in range(samples):
        open_loop = open_loop @ Ad.T
    closed_tip, open_tip = np.abs(np_(ens.unpack_state())[:, tip]), np.abs(open_loop[:, tip])
    assert np.all(np.isfinite(closed_tip)) and np.max(closed_tip) < np.max(open_tip)
    assert np.linalg.norm(want) < np.linalg.norm(open_loop)


# ------------------------------------------------------------------ 9. edges
@pytest.mark.parametrize("name", ["packed_partial", "two_waves_padded"])
def test_non_finite_seed_stays_in_its_beam_and_direction(name):
    m = Mapped(name)
    v = m.seeds(D=3)
    ref = m.tangent(v["dx0"], d_impulse_amp=v["d_amp"], d_held_force=v["d_held"])
    base = m.ens.state.clone()
    bad = {k: a.copy() for k, a in v.items()}
    bad["dx0"][1, 1, m.n + 1] = float("nan")
    got = m.tangent(bad["dx0"], d_impulse_amp=bad["d_amp"], d_held_force=bad["d_held"])
    assert torch.equal(m.ens.state, base) and int(m.ens.status.abs().max()) == 0
    assert not torch.isfinite(got[1, 1]).all()
    keep = torch.ones(got.shape[:2], dtype=torch.bool)
    keep[1, 1] = False
    assert torch.equal(got[keep], ref[keep]) and torch.isfinite(got[keep]).all()


def test_257_slots_are_refused_and_no_steps_change_nothing():
    big = BeamEnsemble(nitinol_columns(257, "linear"), 1, force_params=force_params(False, False))
    big.set_state(1e-3 * np.ones((1, 2 * big.n)), 0.25)
    state0 = big.state.clone()
    with pytest.raises(nat.NativeError) as e:
        big.step_implicit_tangent(3, 1e-4, np.ones((1, 2 * big.n)))
    assert e.value.code == nat.CRB_EUNSUPPORTED and "256" in str(e.value) and "crb_step_implicit_tangent" in str(e.value)
    assert torch.equal(big.state, state0) and big.time == 0.25
    m = Mapped("packed_partial")
    m.ens.set_state(m.X, T0)
    state0 = m.ens.state.clone()
    dx0 = m.seeds()["dx0"]
    got = m.ens.step_implicit_tangent(0, m.h, dx0, impulse_amp=m.amps, held_force=m.U)
    assert torch.equal(m.ens.state, state0) and m.ens.time == T0
    assert torch.equal(got, dev(m.ens, dx0))
    for kw, word in ((dict(n_iter=0), "n_iter"), (dict(n_iter=17), "n_iter")):
        with pytest.raises(nat.NativeError, match=word):
            m.ens.step_implicit_tangent(3, m.h, dx0, **kw)
        assert torch.equal(m.ens.state, state0) and m.ens.time == T0
    with pytest.raises(ValueError, match="step_implicit_tangent: dx0_red"):
        m.ens.step_implicit_tangent(3, m.h, dx0[0, :, :-1])


def test_full_size_4096_beams_of_256_elements():
    cols = nitinol_columns(256, "nonlinear")
    fp = force_params(True, True)
    B, steps, h = 4096, 10, 1e-4
    amps = np.linspace(0.1, 0.2, B)
    pick = [0, 2047, 4095]
    rng = np.random.default_rng(12)
    big = BeamEnsemble(cols, B, force_params=fp)
    n = big.n
    dx0 = np.zeros((B, 2 * n))
    dx0[pick] = 1e-3 * rng.normal(0.0, 1.0, (3, 2 * n))
    big.zero_state()
    got = big.step_implicit_tangent(steps, h, dx0, impulse_amp=amps, d_impulse_amp=amps)
    assert torch.isfinite(got).all() and torch.isfinite(big.state).all() and float(got.abs().max()) > 0
    small = BeamEnsemble(cols, 3, force_params=fp)
    small.zero_state()
    want = small.step_implicit_tangent(steps, h, dx0[pick], impulse_amp=amps[pick], d_impulse_amp=amps[pick])
    assert torch.equal(got[pick], want) and torch.equal(big.unpack_state()[pick], small.unpack_state())
