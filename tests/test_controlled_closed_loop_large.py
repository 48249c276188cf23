"""crb_solve_controlled's closed loop for gains that do not fit the LDS (beams of more than ~30 elements): the gain is read
from a transposed copy in global memory (csrc/crb_ctrl.h, SG) while every beam keeps its own step sequence.  Checked
against the CPU oracle's fixed-step closed loop at the step counts the kernel accepted, against the LDS form on the golden
G6 loops (CRB_CTRL_STREAM_GAIN=1), and through ``solve_ivp(gain=K, controller="device")``."""
import numpy as np
import pytest

from tests.helpers import assert_blocks, beam_columns, force_kwargs, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def ensemble(cols, n_beams, kw=None):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    kw = kw or {}
    fp = ForceParams(fluid_density=kw.get("fluid_density", 0.0), enable_fluid_effects=kw.get("enable_fluid", False),
                     gravity_vector=list(kw.get("gravity", [0.0, -9.81, 0.0])),
                     enable_gravity_effects=kw.get("enable_gravity", False))
    return BeamEnsemble(cols, n_beams, force_params=fp, dtype=torch.float64)


_CARE = {}


def care_gain(ens):
    """LQR gain of examples/lqr_control.py:46-84 (Q = diag(100 I, 10 I), R = I), solved once per rod."""
    from continuum_robot.control import LinearQuadraticRegulator

    key = (ens.n_elem, ens.n)
    if key not in _CARE:
        K, M = ens.plan.stiffness(), ens.plan.mass()
        n = K.shape[0]
        Q = np.eye(2 * n)
        Q[:n, :n] *= 100
        Q[n:, n:] *= 10
        _CARE[key] = LinearQuadraticRegulator(K, M, Q, np.eye(n)).compute_gain_matrix()
    return _CARE[key]


def pd_gain(n, kp=200.0, kd=2.0):
    """u = -kp q - kd v: a stabilising gain for rods whose CARE would take minutes."""
    return np.hstack([kp * np.eye(n), kd * np.eye(n)])


def fits_lds(ens):
    n2p = (2 * ens.n + 7) // 8 * 8
    return 14 * int(ens.plan.layout.threads) * 8 + (n2p + n2p * ens.n + 32) * 8 + 512 <= 160 * 1024


def replay(ob, y, x0, K, amps, dt_eval, used, t_switch, cut, free_index, tol=1e-9):
    """Every recorded interval but the cut one against the oracle's rk4_feedback at the accepted step count, each from the
    kernel's own state at the interval's start."""
    n_int, B = y.shape[0], y.shape[1]
    for b in range(B):
        for k in range(n_int):
            if k == cut:     # (its two pieces may sit on different rungs: used / 2 steps each is not what ran)
                continue
            start = x0[b] if k == 0 else y[k - 1, b]
            m = int(used[b, k])
            want = ob.rk4_feedback(start, dt_eval / m, m, K, amp=amps[b], duration=t_switch, t0=k * dt_eval)
            assert_blocks(y[k, b], want, free_index, tol, what=(b, k, m))


@pytest.mark.parametrize("n_e,kw,gain", [
    (40, dict(), "care"),                                                               # one wave: the lean RHS
    (96, dict(), "care"),                                                               # two waves: the general RHS
    (48, dict(fluid_density=1000.0, enable_fluid=True, enable_gravity=True), "care"),   # drag + gravity, lean
    (160, dict(fluid_density=1000.0, enable_fluid=True), "pd"),                         # four waves
])
def test_streamed_gain_kernel_takes_the_oracles_steps(n_e, kw, gain):
    """The kernel's recorded states are the oracle's closed-loop RK4 states for the step counts it accepted.  Loose
    tolerances let the controller halve the rate until the coarse solution crosses RK4's stability limit: at least one
    doubling happens with the LQR gains.  The impulse ends inside interval 2."""
    cols = nitinol_columns(n_e, "linear")
    B, dt_eval, n_int, t_switch = 3, 1e-3, 5, 0.0025
    ens = ensemble(cols, B, kw)
    assert not fits_lds(ens)
    K = care_gain(ens) if gain == "care" else pd_gain(ens.n)
    ob = oracle_beam(cols, **kw)
    x0 = np.zeros((B, 2 * ens.n))
    amps = np.array([1.0, 0.4, 0.1])
    snaps, stats, used = ens.solve_controlled(n_int, dt_eval, rtol=1e-2, atol=1e-5, gain=K, impulse_amp=amps, impulse_duration=t_switch,
                                              t0=0.0)
    y = ens.unpack_snapshots(snaps).cpu().numpy()
    assert np.all(stats[:, 2] == 0) and np.all(np.isfinite(y)) and np.array_equal(stats[:, 0], used.sum(axis=1))
    if gain == "care":
        assert stats[:, 1].max() >= 1, (used, stats)
    replay(ob, y, x0, K, amps, dt_eval, used, t_switch, 2, ens.free_index)
    assert np.array_equal(ens.unpack_state().cpu().numpy(), y[-1])


def test_streamed_gain_gives_every_beam_its_own_step_sequence():
    """In one launch the driven beams take more steps than the beam at rest, and each beam's trajectory and step counts are
    bit-identical to that beam run as an ensemble of one.  (This loop is linear and RK4's stability limit, not the tolerance,
    sets the driven beams' steps -- 256 per ms for the 10 N and the 1e-4 N beam alike at rtol 1e-8 ... 1e-12 -- so their
    counts agree; the beam at rest is not held back by that limit and drops to 64 per ms.)"""
    cols = nitinol_columns(40, "linear")
    amps = np.array([10.0, 1e-4, 0.0])
    B, n_int = 3, 3
    tol = dict(rtol=1e-8, atol=1e-10)      # (the example's)
    ens = ensemble(cols, B)
    K = care_gain(ens)
    snaps, stats, used = ens.solve_controlled(n_int, 1e-3, gain=K, impulse_amp=amps, impulse_duration=1.5e-3, t0=0.0, **tol)
    y = ens.unpack_snapshots(snaps).cpu().numpy()
    total = used.sum(axis=1)
    assert np.all(stats[:, 2] == 0) and total[0] >= total[1] > total[2] and used[2, -1] < used[0, -1], used
    for b in range(B):
        one = ensemble(cols, 1)
        s1, st1, u1 = one.solve_controlled(n_int, 1e-3, gain=K, impulse_amp=amps[b:b + 1], impulse_duration=1.5e-3, t0=0.0, **tol)
        assert np.array_equal(u1[0], used[b]) and np.array_equal(one.unpack_snapshots(s1).cpu().numpy()[:, 0], y[:, b]), b


@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("name", ["lqr6", "lqr24"])
def test_streamed_gain_on_small_gains_takes_the_same_steps(golden, name, lean, monkeypatch):
    """CRB_CTRL_STREAM_GAIN=1 forces the streamed form where the gain fits the LDS: on golden G6's loops it takes the same
    step counts as the LDS form (both form K e with the same multiply-adds in the same order), and its states replay on the
    oracle."""
    if not lean:
        monkeypatch.setenv("CRB_DISABLE_LEAN_FEEDBACK", "1")
    z = golden["g6_lqr_loop"]
    cols, kw = beam_columns(z, name), force_kwargs(z, name)
    K, amp = z[f"{name}/gain"], float(z[f"{name}/amp"])
    ob = oracle_beam(cols, **kw)
    B, dt_eval, n_int, t_switch = 2, 1e-3, 5, 0.0025
    amps = np.array([amp, 0.5 * amp])
    runs = []
    for streamed in (False, True):
        if streamed:
            monkeypatch.setenv("CRB_CTRL_STREAM_GAIN", "1")
        else:
            monkeypatch.delenv("CRB_CTRL_STREAM_GAIN", raising=False)
        ens = ensemble(cols, B, kw)
        assert fits_lds(ens)
        snaps, stats, used = ens.solve_controlled(n_int, dt_eval, rtol=1e-2, atol=1e-5, gain=K, impulse_amp=amps, impulse_duration=t_switch,
                                                  t0=0.0)
        assert np.all(stats[:, 2] == 0)
        runs.append((ens.unpack_snapshots(snaps).cpu().numpy(), used, ens.free_index))
    (y_lds, used_lds, _), (y_sg, used_sg, free_index) = runs
    assert np.array_equal(used_lds, used_sg), (used_lds, used_sg)
    replay(ob, y_sg, np.zeros((B, 2 * ob.n)), K, amps, dt_eval, used_sg, t_switch, 2, free_index)
    assert np.allclose(y_sg, y_lds, rtol=1e-12, atol=1e-15)


def test_solve_ivp_device_controller_with_a_gain_beyond_the_lds():
    """``solve_ivp(gain=K, controller="device")`` on a 64-element rod: one launch, per-beam step counts, positions inside the
    tolerance band of the host-loop controller on the same call; ``controller="auto"`` still takes the host loop there."""
    cols = nitinol_columns(64, "linear")
    B = 2
    t_eval = np.arange(0.0, 0.0035, 0.001)
    amps = np.array([1.0, 0.5])
    call = dict(method="LSODA", rtol=1e-8, atol=1e-10, impulse_amp=amps, impulse_duration=0.0015)
    dev = ensemble(cols, B)
    K = care_gain(dev)
    sd = dev.solve_ivp((0.0, t_eval[-1]), t_eval, gain=K, controller="device", **call)
    assert sd.controller == "device" and sd.substeps_per_beam.shape == (B, t_eval.size - 1)
    host = ensemble(cols, B)
    sh = host.solve_ivp((0.0, t_eval[-1]), t_eval, gain=K, controller="host", **call)
    assert sh.controller == "host"
    n = dev.n
    yd, yh = sd.y.cpu().numpy(), sh.y.cpu().numpy()
    assert np.all(np.isfinite(yd))
    assert np.max(np.abs(yd[:, :n] - yh[:, :n]) / (1e-6 + 1e-3 * np.abs(yh[:, :n]))) < 0.1
    sa = ensemble(cols, B).solve_ivp((0.0, t_eval[-1]), t_eval, gain=K, controller="auto", **call)
    assert sa.controller == "host"


def test_streamed_gain_series_output_and_refusals():
    """``record=(n_elem, "w")`` equals that DOF of the snapshots of the same run, bit for bit; a list of gains with
    ``controller="device"`` is still refused."""
    cols = nitinol_columns(40, "linear")
    B, n_int = 3, 4
    amps = np.array([0.3, 0.6, 0.9])
    a, b = ensemble(cols, B), ensemble(cols, B)
    K = care_gain(a)
    tol = dict(rtol=1e-6, atol=1e-9)
    snaps, _, used_a = a.solve_controlled(n_int, 1e-3, gain=K, impulse_amp=amps, impulse_duration=2.5e-3, t0=0.0, **tol)
    series, _, used_b = b.solve_controlled(n_int, 1e-3, gain=K, impulse_amp=amps, impulse_duration=2.5e-3, t0=0.0,
                                           record=(a.n_elem, "w"), **tol)
    assert tuple(series.shape) == (B, n_int) and np.array_equal(used_a, used_b)
    y = a.unpack_snapshots(snaps).cpu().numpy()
    idx = a.reduced_index(a.n_elem, "w")
    assert np.array_equal(series.cpu().numpy(), y[:, :, idx].T)
    assert np.array_equal(a.state.cpu().numpy(), b.state.cpu().numpy())
    with pytest.raises(ValueError, match="controller"):
        ensemble(cols, B).solve_ivp((0.0, 0.002), np.arange(0.0, 0.0025, 0.001), method="LSODA", gain=[K, K], controller="device",
                                    impulse_amp=amps)
