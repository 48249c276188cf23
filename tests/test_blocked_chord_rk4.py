"""GPU checks of the blocked stepper's chord-relative element forces and of its RK4 bookkeeping without stage velocities of u
and phi (crb_lean.h, lean_blocked_body with elem_force_nonlinear_chord and the Rk4Pos stage ends of crb_math.h): the next
stage's positions are carried on the accelerations, the drag alone reads a stage velocity (w), and the rate update is the
one it was.  Against the one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1 in a fresh child process, one for all cases) and
the oracle: 1e-10 from rest, 1e-9 from seeded states (the tolerances of test_blocked_stage_arith.py).
  tip_w                  a tip w impulse from rest
  phi_last_node_closes   a rotation impulse on a lane's last node whose window closes between stages 0 and 1 of step 51
  seeded_rates           smooth bumps of u, w, phi and of their RATES on a few lanes, dw/dt of 1 m/s: the drag moves the result
                         by more than 1e5 tolerances, so a wrong stage velocity of w, or one of u / phi leaking into the
                         drag, shows here
  rigid_rotation         lanes 0 .. 2, 30 .. 32 and 61 .. 63 carry near-rigid rotations: phi constant to 1e-4 over plateaus, w
                         falling by L (phi1 + phi2) / 2 per element, u by what keeps the axial strain E at zero -- so e = s - 2 dw
                         cancels to rounding, d ~ 0, and dw^2 / 2 stands against U in E
  linear_seeded          the linear blocked instance (the RK4 bookkeeping is shared) from the seeded state
The oracle carries every one of these states finitely over the horizon (checked on the CPU before they were fixed, and
asserted below); large_state's docstring in test_blocked_axial_regrouped.py says why that needs checking.
Chunked stepping, snapshots, a single-slot record and beam isolation stay bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam
from tests.test_blocked_stage_arith import seeded_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT = 2e-5
B = 4
AMPS = 0.05 * (1.0 + np.arange(B))
LANE = 30
N = 3 * 256
ELEM_L = 0.25
REGIONS = (0, 120, 244)        # first slots of the twelve-node regions: lanes 0 .. 2, 30 .. 32, 61 .. 63


def seeded_rates(n):
    """sin^2 bumps of displacements and RATES over lanes 28 .. 33 and the last six: u 1e-6, w 1e-4, phi 1e-3 with du/dt 1e-3,
    dw/dt 1, dphi/dt 1.  (Smooth: a random state with rates of this size leaves RK4's stability region at this step within
    the horizon, and the shipped f1 amplifies any u -- the oracle carries this one with a forward sensitivity of 1e-13 to a
    one-ulp change of the state.)"""
    x0 = np.zeros((B, 2 * n))
    for lo, hi in ((112, 136), (232, 256)):
        env = np.sin(np.pi * (np.arange(hi - lo) + 1) / (hi - lo + 1)) ** 2
        for b in range(B):
            amp = 1.0 + 0.1 * b
            x0[b, 3 * lo:3 * hi] = np.stack([1e-6 * env, -1e-4 * amp * env, 1e-3 * env], axis=1).reshape(-1)
            x0[b, n + 3 * lo:n + 3 * hi] = np.stack([1e-3 * env, amp * env, -1.0 * env], axis=1).reshape(-1)
    return x0


def rigid_rotation(n):
    """Per region: phi rises to a plateau of three nodes (equal to 1e-4), falls through zero to the opposite plateau and back
    to zero, so that w returns; w_{j+1} = w_j - L (phi_j + phi_{j+1}) / 2 (e = 0 up to rounding) and
    u_{j+1} = u_j - (dw^2 / 2 + d^2 / 24) / L (E = 0 up to rounding: a rotation without axial strain)."""
    prof = np.array([0.5, 1.0, 1.0 + 1e-4, 1.0 - 1e-4, 0.5, 0.0, -0.5, -1.0, -1.0 - 1e-4, -1.0 + 1e-4, -0.5, 0.0])
    x0 = np.zeros((B, 2 * n))
    for b in range(B):
        phi = np.zeros(257)                  # node 0 is the fixed root; slot j is node j + 1
        for lo in REGIONS:
            phi[lo + 1:lo + 13] = 0.01 * (1.0 + 0.25 * b) * prof
        u, w = np.zeros(257), np.zeros(257)
        for j in range(256):
            a_, b_ = ELEM_L * phi[j], ELEM_L * phi[j + 1]
            dw = 0.5 * (a_ + b_)
            w[j + 1] = w[j] - dw
            u[j + 1] = u[j] - (0.5 * dw * dw + (a_ - b_) ** 2 / 24.0) / ELEM_L
        x0[b, :n] = np.stack([u[1:], w[1:], phi[1:]], axis=1).reshape(-1)
    return x0


# name -> (element kind, reduced position index of the impulse, impulse duration, initial state or None, steps, tolerance)
CASES = {
    "tip_w": ("nonlinear", -2, 0.01, None, 100, 1e-10),
    "phi_last_node_closes": ("nonlinear", 3 * (4 * LANE + 3) + 2, 50.25 * DT, None, 100, 1e-10),
    "seeded_rates": ("nonlinear", -2, 0.01, seeded_rates, 80, 1e-9),
    "rigid_rotation": ("nonlinear", -2, 0.01, rigid_rotation, 80, 1e-9),
    "linear_seeded": ("linear", 3 * (4 * LANE + 3) + 1, 0.01, lambda n: seeded_state(n, "linear_seeded"), 80, 1e-9),
}


def initial_state(name):
    make = CASES[name][3]
    return np.zeros((B, 2 * N)) if make is None else make(N)


def make_ensemble(kind="nonlinear", drag=True):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True) if drag else None
    return BeamEnsemble(nitinol_columns(256, kind), B, dtype=torch.float64, force_params=fp)


def run_case(name, chunks=1):
    """Terminal states of case `name` on whatever stepper this process's environment selects."""
    kind, idx, duration, _, steps, _ = CASES[name]
    ens = make_ensemble(kind)
    assert ens.n == N
    ens.set_state(initial_state(name))
    for _ in range(chunks):
        ens.step(steps // chunks, DT, impulse_amp=AMPS, impulse_duration=duration, impulse_index=idx)
    return ens.unpack_state().cpu().numpy(), np.asarray(ens.free_index)


CHILD = """
import sys
import numpy as np
from tests import test_blocked_chord_rk4 as m
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


def oracle_run(name, drag=True):
    kind, idx, duration, _, steps, _ = CASES[name]
    ob = oracle_beam(nitinol_columns(256, kind), fluid_density=1000.0, enable_fluid=drag)
    ref, _ = ob.rk4_impulse_batch(initial_state(name), DT, steps, AMPS, duration=duration, idx=idx)
    return ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_chord_forces_and_rk4_against_the_lean_stepper_and_the_oracle(name, lean_states, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    tol = CASES[name][5]
    got, free = run_case(name)
    lean = lean_states[name]
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(got, lean)
    errs = block_errs(got, lean, free)
    print(name, "against the one-node-per-lane stepper:", errs)
    assert max(errs.values()) <= tol, errs
    ref = oracle_run(name)
    assert np.isfinite(ref).all()
    print(name, "against the oracle:", block_errs(got, ref, free))
    assert_blocks(got, ref, free, tol, what=name)


def test_the_drag_matters_in_the_seeded_rates_case():
    """The oracle with and without drag: the w block moves by more than 1e5 times the case's tolerance, so a stage velocity
    that is wrong by a part in 1e4 is seen."""
    with_drag, without = oracle_run("seeded_rates"), oracle_run("seeded_rates", drag=False)
    w = np.arange(1, N, 3)
    moved = np.abs(with_drag[:, w] - without[:, w]).max() / np.abs(with_drag[:, w]).max()
    print("drag moves the w block by", moved)
    assert moved > 1e5 * CASES["seeded_rates"][5]


def test_rigid_rotation_state_cancels_e_on_the_end_lanes():
    x0 = rigid_rotation(N)[0, :N].reshape(256, 3)
    q = np.vstack([np.zeros((1, 3)), x0])
    a, b, dw = ELEM_L * q[:-1, 2], ELEM_L * q[1:, 2], q[:-1, 1] - q[1:, 1]
    s, d = a + b, a - b
    for lo in REGIONS:
        el = np.arange(lo, min(lo + 13, 256))          # the elements that touch the region's nodes
        assert np.abs(s[el] - 2 * dw[el]).max() <= 1e-12 * np.abs(s[el]).max()
        assert (np.abs(d[el]) <= 2.1e-4 * np.abs(a[el]).max()).sum() >= 4 and np.abs(a[el]).max() > 0
    assert x0[0:12, 2].any() and x0[244:256, 2].any() and x0[255, 2] == 0.0


@pytest.mark.parametrize("name", ["phi_last_node_closes", "seeded_rates"])
def test_one_launch_equals_five_launches_bitwise(name, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    one, _ = run_case(name, chunks=1)
    many, _ = run_case(name, chunks=5)
    assert np.array_equal(one, many)


def test_sixty_steps_equal_three_times_twenty(monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    a, b = make_ensemble(), make_ensemble()
    x0 = seeded_rates(N)
    a.set_state(x0)
    b.set_state(x0)
    idx = 3 * (4 * LANE + 3) + 2
    a.step(60, DT, impulse_amp=AMPS, impulse_duration=25.25 * DT, impulse_index=idx)
    for _ in range(3):
        b.step(20, DT, impulse_amp=AMPS, impulse_duration=25.25 * DT, impulse_index=idx)
    assert torch.equal(a.state, b.state)


def test_snapshots_and_a_single_slot_record_equal_chunked_stepping(monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    x0 = seeded_rates(N)
    k, n_rec = 10, 4
    ens, ref, one = make_ensemble(), make_ensemble(), make_ensemble()
    for e in (ens, ref, one):
        e.set_state(x0)
    _, snaps = ens.step(k * n_rec + 3, DT, impulse_amp=AMPS, record="all", record_every=k)
    red = ens.unpack_snapshots(snaps)
    # the rate of the rotation of lane 30's last node: a component whose stage velocity is no longer formed
    _, series = one.step(k * n_rec, DT, impulse_amp=AMPS, record=(4 * LANE + 4, "dphi_dt"), record_every=k)
    for i in range(n_rec):
        ref.step(k, DT, impulse_amp=AMPS)
        assert torch.equal(red[i], ref.unpack_state()), i
        assert torch.equal(series[:, i], ref.unpack_state()[:, N + 3 * (4 * LANE + 3) + 2]), i
    ref.step(3, DT, impulse_amp=AMPS)
    assert torch.equal(ens.unpack_state(), ref.unpack_state())


def test_a_nan_seeded_beam_changes_no_other_beam_of_its_workgroup(monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    clean = make_ensemble()
    x0 = seeded_rates(N)
    clean.set_state(x0)
    clean.step(40, DT, impulse_amp=AMPS)
    ens = make_ensemble()
    x0 = x0.copy()
    x0[2, N + 3 * (4 * LANE + 3) + 1] = np.nan     # (a w rate: it enters the drag and the position sums)
    ens.set_state(x0)
    ens.step(40, DT, impulse_amp=AMPS)
    good = np.arange(B) != 2
    got, want = ens.unpack_state(), clean.unpack_state()
    assert torch.equal(got[good], want[good])
    assert not torch.isfinite(got[2]).all() and torch.isfinite(got[good]).all()
