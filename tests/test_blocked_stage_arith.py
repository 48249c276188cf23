"""GPU checks of the blocked stepper's stage arithmetic (crb_lean.h, lean_blocked_body): the impulse enters the right-hand side
of ONE (node, dof) of one lane behind wave-uniform scalar branches, every other component is -f_right - f_left(next) with the
drag folded in, and stage 0 starts the RK4 sums.  An impulse on each of a lane's four node positions and each dof, an impulse
window that closes inside a launch (between the stages of a step), drag on and off and seeded states are compared with the
one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1 in a fresh child process, one for all cases) and with the oracle, at the
tolerances of test_blocked_strip_edges.py: 1e-10 from rest, 1e-9 for seeded states."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT = 2e-5
B = 4
AMPS = 0.05 * (1.0 + np.arange(B))
LANE = 30          # slots 120 .. 123: a lane in the middle of the wave
STEPS = 120
SEEDED_STEPS = 80   # (the horizon of the seeded case of test_blocked_strip_edges.py)

# name -> (reduced position index of the impulse, drag, impulse duration, seeded state, tolerance)
CASES = {}
for _k in range(4):
    for _dof in range(3):
        CASES[f"node{_k}_dof{_dof}"] = (3 * (4 * LANE + _k) + _dof, True, 0.01, False, 1e-10)
# the window closes after stage 0 of step 50 (t = 50 DT is inside, the half and the full step are not), and on a step boundary
CASES["closes_between_stages"] = (3 * (4 * LANE + 1) + 1, True, 50.25 * DT, False, 1e-10)
CASES["closes_on_a_step"] = (-2, True, 70.0 * DT, False, 1e-10)
CASES["closes_before_the_launch"] = (-2, True, 0.0, True, 1e-9)
CASES["tip_no_drag"] = (-2, False, 0.01, False, 1e-10)
CASES["node2_dof1_no_drag"] = (3 * (4 * LANE + 2) + 1, False, 0.01, False, 1e-10)
CASES["seeded_drag"] = (3 * (4 * LANE + 3) + 1, True, 0.01, True, 1e-9)
CASES["seeded_no_drag"] = (3 * (4 * LANE) + 2, False, 40.5 * DT, True, 1e-9)   # (closes inside the seeded horizon)


def seeded_state(n, name):
    """Positions and rates on the nodes of lanes 28 .. 33 and of the last four lanes (as test_blocked_strip_edges.py seeds the
    ends: a state seeded on every node of the beam excites its stiffest modes beyond what RK4 at this step integrates)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    x0 = np.zeros((B, 2 * n))
    for lo, hi in ((3 * 112, 3 * 136), (3 * 240, n)):
        x0[:, lo:hi] = rng.normal(0.0, 1e-5, (B, hi - lo))
        x0[:, n + lo:n + hi] = rng.normal(0.0, 1e-2, (B, hi - lo))
    return x0


def run_case(name):
    """Terminal states of case `name` on whatever stepper this process's environment selects, and the free index."""
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    idx, drag, duration, seeded, _ = CASES[name]
    cols = nitinol_columns(256, "nonlinear")
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True) if drag else None
    ens = BeamEnsemble(cols, B, force_params=fp, dtype=torch.float64)
    n = ens.n
    x0 = seeded_state(n, name) if seeded else np.zeros((B, 2 * n))
    ens.set_state(x0)
    steps = SEEDED_STEPS if seeded else STEPS
    ens.step(steps, DT, impulse_amp=AMPS, impulse_duration=duration, impulse_index=idx)
    return ens.unpack_state().cpu().numpy(), np.asarray(ens.free_index), x0


CHILD = """
import sys
import numpy as np
from tests import test_blocked_stage_arith as m
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


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_arithmetic_against_the_lean_stepper_and_the_oracle(name, lean_states, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    idx, drag, duration, seeded, tol = CASES[name]
    got, free, x0 = run_case(name)
    lean = lean_states[name]
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(got, lean)
    errs = block_errs(got, lean, free)
    print(name, "against the one-node-per-lane stepper:", errs)
    assert max(errs.values()) <= tol, errs
    ob = oracle_beam(nitinol_columns(256, "nonlinear"), **(dict(fluid_density=1000.0, enable_fluid=True) if drag else {}))
    ref, _ = ob.rk4_impulse_batch(x0, DT, SEEDED_STEPS if seeded else STEPS, AMPS, duration=duration, idx=idx)
    print(name, "against the oracle:", block_errs(got, ref, free))
    assert_blocks(got, ref, free, tol, what=name)


def test_the_impulse_reaches_the_state_only_inside_its_window(lean_states, monkeypatch):
    """The same seeded state with the window closed from the start and with no impulse at all: bitwise equal."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    a, _, _ = run_case("closes_before_the_launch")
    # (as above: equal to the other stepper bit for bit would mean the blocked stepper did not run)
    assert not np.array_equal(a, lean_states["closes_before_the_launch"])
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    ens = BeamEnsemble(nitinol_columns(256, "nonlinear"), B, dtype=torch.float64,
                       force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    ens.set_state(seeded_state(ens.n, "closes_before_the_launch"))
    ens.step(SEEDED_STEPS, DT)
    assert np.array_equal(a, ens.unpack_state().cpu().numpy())
