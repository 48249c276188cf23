"""GPU checks of the blocked stepper's shared-membrane element forces (crb_lean.h, lean_blocked_body with
elem_force_nonlinear_shared of crb_math.h: A1 = dw^2 - 2 L du and A2 = dw^2 - (2 L / 3) du formed once per element, the
plan's SK_N constants behind the folded ones in the blocked table buffer).  Against the one-node-per-lane stepper
(CRB_DISABLE_BLOCKED=1 in a fresh child process, one for all cases) at 1e-10 per block and against the oracle at 1e-9, the
bounds of the other blocked tests.  256 elements, B = 5: one full group of four waves and one partial; 40 steps.
  tip_w                  a tip w impulse from rest
  axial_first_node       an axial impulse on a lane's first node \\ the f1 exchange with the lane below / the difference of
  axial_last_node        ... and on a lane's last node           / f2 inside the lane carries it
  phi_last_node          a rotation impulse on a lane's last node
  window_closes          the tip impulse with a window that closes between stages 0 and 1 of step 21
  seeded_rates           test_blocked_chord_rk4.py's bumps of u, w, phi and their rates, with the drag: every monomial is live
  inextensible_bends     bends over lanes 0 .. 2, 30 .. 32 and 61 .. 63 (the root's, an interior and the tip's rows of the
                         wave) whose u follows du = dw^2 / (2 L) node by node: A1 cancels to rounding at the start
  length_0p3             seeded_rates on a rod of element length 0.3 (length and wetted_area scaled): the products with L round
  length_0p0731          ... of element length 0.0731, at a quarter of the step (RK4's stability limit falls with L^2)
The oracle carries every one of these states finitely over the horizon (asserted below).  Chunked stepping, snapshots, a
single-slot record and beam isolation stay bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, oracle_beam
from tests.test_blocked_chord_rk4 import seeded_rates
from tests.test_blocked_folded_forces import AMPS, B, DT, LANE, N, columns, five

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STEPS = 40
TOL_LEAN, TOL_ORACLE = 1e-10, 1e-9
BEND_LANES = (0, 30, 61)      # each bend spans three lanes: 12 nodes from the first node of the lane


def inextensible_bends(n, length=0.25):
    """Per region the rotation profile of test_blocked_chord_rk4.rigid_rotation (up to a plateau, through zero to the
    opposite plateau and back, so that w returns) with w_{j+1} = w_j - L (phi_j + phi_{j+1}) / 2, and
    u_{j+1} = u_j - dw^2 / (2 L): the element's chord keeps its length to second order, A1 = dw^2 - 2 L du = 0 up to the rounding of the running sum u (at
    most 2e-14 of dw^2; the CPU test has the cancellation to a few ulp)."""
    prof = np.array([0.5, 1.0, 1.0 + 1e-4, 1.0 - 1e-4, 0.5, 0.0, -0.5, -1.0, -1.0 - 1e-4, -1.0 + 1e-4, -0.5, 0.0])
    x0 = np.zeros((B, 2 * n))
    for b in range(B):
        phi = np.zeros(257)                  # node 0 is the fixed root; slot j is node j + 1
        for lane in BEND_LANES:
            phi[4 * lane + 1:4 * lane + 13] = 0.01 * (1.0 + 0.25 * b) * prof
        u, w = np.zeros(257), np.zeros(257)
        for j in range(256):
            dw = 0.5 * length * (phi[j] + phi[j + 1])
            w[j + 1] = w[j] - dw
            u[j + 1] = u[j] - dw * dw / (2.0 * length)
        x0[b, :n] = np.stack([u[1:], w[1:], phi[1:]], axis=1).reshape(-1)
    return x0


# name -> dict(rod (keywords of columns), idx: reduced position index of the impulse, duration, state, dt)
def case(idx=-2, duration=0.01, state=None, rod=None, dt=DT):
    return dict(rod=rod or {}, idx=idx, duration=duration, state=state, dt=dt)


CASES = {
    "tip_w": case(),
    "axial_first_node": case(idx=3 * (4 * LANE) + 0),
    "axial_last_node": case(idx=3 * (4 * LANE + 3) + 0),
    "phi_last_node": case(idx=3 * (4 * LANE + 3) + 2),
    "window_closes": case(duration=20.25 * DT),
    "seeded_rates": case(state=five(seeded_rates)),
    "inextensible_bends": case(state=inextensible_bends),
    "length_0p3": case(state=five(seeded_rates), rod=dict(length=0.3)),
    "length_0p0731": case(state=five(seeded_rates), rod=dict(length=0.0731), dt=DT / 4),
}


def initial_state(name):
    make = CASES[name]["state"]
    return np.zeros((B, 2 * N)) if make is None else make(N)


def make_ensemble(name="tip_w"):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True)
    return BeamEnsemble(columns("nonlinear", **CASES[name]["rod"]), B, dtype=torch.float64, force_params=fp)


def run_case(name, chunks=1):
    """Terminal states of case `name` on whatever stepper this process's environment selects."""
    c = CASES[name]
    ens = make_ensemble(name)
    assert ens.n == N
    ens.set_state(initial_state(name))
    for _ in range(chunks):
        ens.step(STEPS // chunks, c["dt"], impulse_amp=AMPS, impulse_duration=c["duration"], impulse_index=c["idx"])
    return ens.unpack_state().cpu().numpy(), np.asarray(ens.free_index)


CHILD = """
import sys
import numpy as np
from tests import test_blocked_shared_forces as m
np.savez(sys.argv[1], **{name: m.run_case(name)[0] for name in m.CASES})
"""


@pytest.fixture(scope="module")
def lean_states(tmp_path_factory):
    """Every case on the one-node-per-lane stepper, from one fresh child process."""
    out = str(tmp_path_factory.mktemp("lean") / "lean.npz")
    env = dict(os.environ, CRB_DISABLE_BLOCKED="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, "-c", CHILD, out], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    return np.load(out)


def oracle_run(name):
    c = CASES[name]
    ob = oracle_beam(columns("nonlinear", **c["rod"]), fluid_density=1000.0, enable_fluid=True)
    ref, _ = ob.rk4_impulse_batch(initial_state(name), c["dt"], STEPS, AMPS, duration=c["duration"], idx=c["idx"])
    return ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_forces_against_the_lean_stepper_and_the_oracle(name, lean_states, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    got, free = run_case(name)
    lean = lean_states[name]
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(got, lean)
    errs = block_errs(got, lean, free)
    print(name, "against the one-node-per-lane stepper:", errs)
    assert max(errs.values()) <= TOL_LEAN, errs
    ref = oracle_run(name)
    assert np.isfinite(ref).all()
    print(name, "against the oracle:", block_errs(got, ref, free))
    assert_blocks(got, ref, free, TOL_ORACLE, what=name)


def test_the_bends_start_with_a1_cancelled_on_the_three_lane_rows():
    """In every element of the nine lanes dw^2 and 2 L du agree to a few ulp of dw^2 while dw itself is of the bend's size."""
    x0 = inextensible_bends(N)
    u = np.concatenate([np.zeros((B, 1)), x0[:, 0:N:3]], axis=1)
    w = np.concatenate([np.zeros((B, 1)), x0[:, 1:N:3]], axis=1)
    du, dw = u[:, :-1] - u[:, 1:], w[:, :-1] - w[:, 1:]
    live = np.zeros(256, dtype=bool)
    for lane in BEND_LANES:
        live[4 * lane:4 * lane + 12] = True
    assert (np.abs(dw[:, live]) > 1e-5).mean() > 0.8
    a1 = dw * dw - 2 * 0.25 * du
    # (u is a running sum: a node's du carries half an ulp of u itself, which is up to 12 elements' worth of dw^2 / (2 L))
    assert (np.abs(a1[:, live]) <= 2.0 ** -52 * 16 * np.abs(u[:, 1:][:, live] * 0.5 + dw[:, live] ** 2)).all()
    assert (a1[:, ~live] == 0).all()


def test_the_window_closes_inside_step_21():
    """The window's end lies between the first and the second stage time of step 21 and changes the answer."""
    assert 20 * DT < CASES["window_closes"]["duration"] < 20.5 * DT < STEPS * DT
    assert not np.array_equal(oracle_run("window_closes"), oracle_run("tip_w"))


@pytest.mark.parametrize("name", ["window_closes", "length_0p3", "inextensible_bends"])
def test_one_launch_equals_two_launches_bitwise(name, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    one, _ = run_case(name, chunks=1)
    two, _ = run_case(name, chunks=2)
    assert np.array_equal(one, two)


def test_snapshots_and_a_single_slot_record_equal_chunked_stepping(monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    x0 = initial_state("inextensible_bends")
    k, n_rec = 10, 4
    ens, ref, one = (make_ensemble("inextensible_bends") for _ in range(3))
    for e in (ens, ref, one):
        e.set_state(x0)
    _, snaps = ens.step(k * n_rec + 3, DT, impulse_amp=AMPS, record="all", record_every=k)
    red = ens.unpack_snapshots(snaps)
    _, series = one.step(k * n_rec, DT, impulse_amp=AMPS, record=(4 * LANE + 4, "dphi_dt"), record_every=k)
    for i in range(n_rec):
        ref.step(k, DT, impulse_amp=AMPS)
        assert torch.equal(red[i], ref.unpack_state()), i
        assert torch.equal(series[:, i], ref.unpack_state()[:, N + 3 * (4 * LANE + 3) + 2]), i
    ref.step(3, DT, impulse_amp=AMPS)
    assert torch.equal(ens.unpack_state(), ref.unpack_state())


def test_a_nan_seeded_beam_changes_no_other_beam(monkeypatch):
    """Beam 2 shares its workgroup with beams 0, 1 and 3; beam 4 walks alone in the partial group."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    clean = make_ensemble("seeded_rates")
    x0 = initial_state("seeded_rates")
    clean.set_state(x0)
    clean.step(STEPS, DT, impulse_amp=AMPS)
    ens = make_ensemble("seeded_rates")
    x0 = x0.copy()
    x0[2, N + 3 * (4 * LANE + 3) + 1] = np.nan     # (a w rate: it enters the drag and the position sums)
    ens.set_state(x0)
    ens.step(STEPS, DT, impulse_amp=AMPS)
    good = np.arange(B) != 2
    got, want = ens.unpack_state(), clean.unpack_state()
    assert torch.equal(got[good], want[good])
    assert not torch.isfinite(got[2]).all() and torch.isfinite(got[good]).all()
