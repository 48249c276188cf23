"""GPU checks of the blocked stepper's regrouped axial right-hand side (crb_lean.h, lean_blocked_body with
elem_force_nonlinear_regrouped): a lane's nodes get r_u = (f2(k+1) - f2(k)) - cA1 W(k+1), its last node -f2(3) - f1 with the
explicit f1 = cA1 W - f2 of lane+1's first element, and the axial impulse lands on the difference f2(k) - f2(k+1) (on the
shifted-in f1 for the last node).  Axial impulses on a lane's first and last node, on the first free node (nothing to its left
but the root) and on the tip (nothing shifted in), a window that closes between two stages, seeded states around lane 30 and
on the last four lanes, and a seeded state large enough for the nonlinear terms of the axial force to matter, against the
one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1 in a fresh child process, one for all cases) and the oracle: 1e-10 from
rest, 1e-9 for seeded states (the tolerances of test_blocked_stage_arith.py).  Chunked stepping and beam isolation stay bitwise."""
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
STEPS = 100
SEEDED_STEPS = 80
N = 3 * 256


def large_state(n):
    """Rotations of 1e-1 and axial displacements of 1e-4 in smooth bumps over the nodes of lanes 28 .. 33 and of the last six
    lanes, at rest: s^2 / 15 = 1.7e-4 and s dw / 10 of the regrouped E stand against L du = 1e-5, 0.05 s against L in LT.
    (Smooth and at rest, w of 1e-3: a random state of this size, or one with velocities, leaves RK4's stability region at
    this step within the horizon -- the oracle itself returns NaN; this one the oracle carries with a forward sensitivity of
    2e-13 to a one-ulp change of the state.)"""
    j = np.arange(1, n // 3 + 1)
    env = np.zeros(n // 3)
    for lo, hi in ((112, 136), (232, 256)):
        k = np.arange(hi - lo)
        env[lo:hi] = np.sin(np.pi * (k + 1) / (hi - lo + 1)) ** 2
    x0 = np.zeros((B, 2 * n))
    for b in range(B):
        q = np.stack([1e-4 * env * np.cos(2 * np.pi * j / 16), 1e-3 * env, 0.1 * (1.0 + 0.1 * b) * env], axis=1)
        x0[b, :n] = q.reshape(-1)
    return x0


# name -> (reduced position index of the impulse, impulse duration, initial state or None, tolerance)
CASES = {
    "axial_lane_first_node": (3 * (4 * LANE), 0.01, None, 1e-10),
    "axial_lane_last_node": (3 * (4 * LANE + 3), 0.01, None, 1e-10),
    "axial_first_free_node": (0, 0.01, None, 1e-10),
    "axial_tip": (N - 3, 0.01, None, 1e-10),
    "axial_last_node_closes_between_stages": (3 * (4 * LANE + 3), 50.25 * DT, None, 1e-10),
    "axial_first_node_closes_between_stages": (3 * (4 * LANE), 30.75 * DT, None, 1e-10),
    "seeded_axial_last_node": (3 * (4 * LANE + 3), 0.01, "seeded", 1e-9),
    "seeded_tip_w": (-2, 40.5 * DT, "seeded", 1e-9),
    "large_axial_first_node": (3 * (4 * LANE), 0.01, "large", 1e-9),
    "large_tip_w": (-2, 0.01, "large", 1e-9),
}


def initial_state(name):
    kind = CASES[name][2]
    if kind is None:
        return np.zeros((B, 2 * N))
    return seeded_state(N, name) if kind == "seeded" else large_state(N)


def steps_of(name):
    return STEPS if CASES[name][2] is None else SEEDED_STEPS


def make_ensemble(corrected=False):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    return BeamEnsemble(nitinol_columns(256, "nonlinear"), B, dtype=torch.float64, corrected_axial=corrected,
                        force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))


def run_case(name, chunks=1):
    """Terminal states of case `name` on whatever stepper this process's environment selects."""
    idx, duration, _, _ = CASES[name]
    ens = make_ensemble()
    assert ens.n == N
    ens.set_state(initial_state(name))
    for _ in range(chunks):
        ens.step(steps_of(name) // chunks, DT, impulse_amp=AMPS, impulse_duration=duration, impulse_index=idx)
    return ens.unpack_state().cpu().numpy(), np.asarray(ens.free_index)


def run_corrected():
    ens = make_ensemble(True)
    ens.set_state(seeded_state(N, "corrected"))
    ens.step(40, DT, impulse_amp=AMPS, impulse_index=3 * (4 * LANE + 3))
    return ens.unpack_state().cpu().numpy()


CHILD = """
import sys
import numpy as np
from tests import test_blocked_axial_regrouped as m
out = {name: m.run_case(name)[0] for name in m.CASES}
out["corrected"] = m.run_corrected()
np.savez(sys.argv[1], **out)
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


@pytest.mark.parametrize("name", sorted(CASES))
def test_regrouped_axial_rhs_against_the_lean_stepper_and_the_oracle(name, lean_states, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    idx, duration, _, tol = CASES[name]
    got, free = run_case(name)
    lean = lean_states[name]
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(got, lean)
    errs = block_errs(got, lean, free)
    print(name, "against the one-node-per-lane stepper:", errs)
    assert max(errs.values()) <= tol, errs
    ob = oracle_beam(nitinol_columns(256, "nonlinear"), fluid_density=1000.0, enable_fluid=True)
    ref, _ = ob.rk4_impulse_batch(initial_state(name), DT, steps_of(name), AMPS, duration=duration, idx=idx)
    assert np.isfinite(ref).all()
    print(name, "against the oracle:", block_errs(got, ref, free))
    assert_blocks(got, ref, free, tol, what=name)


def test_an_axial_impulse_moves_the_axial_block(monkeypatch):
    """The axial impulse reaches u (its sign and its node: the same case with the impulse one node further differs)."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    a, free = run_case("axial_lane_last_node")
    b, _ = run_case("axial_lane_first_node")
    u = free % 3 == 0
    assert np.abs(a[:, :N][:, u]).max() > 1e-12 and not np.array_equal(a, b)


@pytest.mark.parametrize("name", ["axial_last_node_closes_between_stages", "large_axial_first_node"])
def test_chunked_stepping_is_bitwise(name, monkeypatch):
    """One launch equals the same steps in several launches, bit for bit (the window closes inside the second of them)."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    one, _ = run_case(name, chunks=1)
    many, _ = run_case(name, chunks=5 if name.startswith("axial") else 4)
    assert np.array_equal(one, many)


def test_sixty_steps_equal_three_times_twenty(monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    a, b = make_ensemble(), make_ensemble()
    idx = 3 * (4 * LANE + 3)
    a.step(60, DT, impulse_amp=AMPS, impulse_duration=25.25 * DT, impulse_index=idx)
    for _ in range(3):
        b.step(20, DT, impulse_amp=AMPS, impulse_duration=25.25 * DT, impulse_index=idx)
    assert torch.equal(a.state, b.state)


def test_a_nan_seeded_beam_changes_no_other_beam_of_its_workgroup(monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    idx = 3 * (4 * LANE)
    clean = make_ensemble()
    x0 = large_state(N)
    clean.set_state(x0)
    clean.step(40, DT, impulse_amp=AMPS, impulse_index=idx)
    ens = make_ensemble()
    x0 = x0.copy()
    x0[2, 3 * (4 * LANE + 3)] = np.nan     # (an axial displacement: it enters f2 and W of two lanes)
    ens.set_state(x0)
    ens.step(40, DT, impulse_amp=AMPS, impulse_index=idx)
    good = np.arange(B) != 2
    got, want = ens.unpack_state(), clean.unpack_state()
    assert torch.equal(got[good], want[good])
    assert not torch.isfinite(got[2]).all() and torch.isfinite(got[good]).all()


def test_corrected_axial_plans_keep_the_one_node_per_lane_stepper(lean_states, monkeypatch):
    """f1 = -f2 has no regrouped form: such a plan is not the blocked stepper's, so both processes ran the same kernel."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    assert np.array_equal(run_corrected(), lean_states["corrected"])
