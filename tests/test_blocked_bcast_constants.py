"""GPU checks of the blocked stepper's wave-uniform solve constants (crb_lean.h, lean_blocked_body; layout in crb_blocked.h):
the 75 constants sit in five fp64 registers per lane, constant k in lane k % 16 of EVERY 16-lane row of register k / 16, and
enter the mass solve as DPP row broadcasts inside multiply-adds.  What can go wrong is a row without its table, a constant
read from the wrong lane or register, and table registers that do not survive a beam switch.  Compared with the
one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1 in a fresh child process, one for all cases) and with the oracle, at the
tolerances of test_blocked_stage_arith.py: 1e-10 from rest, 1e-9 for seeded states.

The seeds, checked on the oracle alone before they were used (its response to a relative perturbation of 2^-50 of every
entry of the seeded state, worst DOF block): four rows, 80 steps: 2.6e-15; whole span, 2 steps: 1.9e-15 (nonlinear + drag) and
2.7e-15 (linear) -- an input change of 4 ulp comes out as 12 ulp at most, so the rounding differences between two solves stay
orders below 1e-9 from these states."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT = 2e-5
ROW_LANES = (5, 21, 37, 53)   # one lane in each of the wave's four 16-lane rows
N_RED = 3 * 256               # reduced positions of the 256-slot beam: lane l owns 12 l .. 12 l + 11

# name -> (element kind, drag, beams, steps, seed, tolerance)
CASES = {
    "four_rows": ("nonlinear", True, 4, 80, "rows", 1e-9),
    "every_constant_nonlinear_drag": ("nonlinear", True, 4, 2, "span", 1e-9),
    "every_constant_linear": ("linear", False, 4, 2, "span", 1e-9),
    "one_beam": ("nonlinear", True, 1, 20, None, 1e-10),      # three idle waves
    "three_beams": ("nonlinear", True, 3, 20, None, 1e-10),   # one idle wave
    "five_beams": ("nonlinear", True, 5, 20, None, 1e-10),    # a second group of one beam
}


def amps_of(n_beams):
    return 0.05 * (1.0 + np.arange(n_beams))


def seeded_state(name):
    """rows: positions and rates as test_blocked_stage_arith.py's seeded_state draws them, on the nodes of one lane per
    16-lane row.  span: the whole span at a tenth of that amplitude, for two steps only (a state seeded on every node
    excites the stiffest modes beyond what RK4 at this step integrates over a long horizon), so that every entry of every
    constant pack multiplies a non-zero value."""
    _, _, n_beams, _, seed, _ = CASES[name]
    x0 = np.zeros((n_beams, 2 * N_RED))
    if seed is None:
        return x0
    rng = np.random.default_rng(sum(map(ord, name)))
    if seed == "rows":
        for lane in ROW_LANES:
            lo, hi = 12 * lane, 12 * lane + 12
            x0[:, lo:hi] = rng.normal(0.0, 1e-5, (n_beams, hi - lo))
            x0[:, N_RED + lo:N_RED + hi] = rng.normal(0.0, 1e-2, (n_beams, hi - lo))
    else:
        x0[:, :N_RED] = rng.normal(0.0, 1e-6, (n_beams, N_RED))
        x0[:, N_RED:] = rng.normal(0.0, 1e-3, (n_beams, N_RED))
        assert np.all(x0 != 0.0)
    return x0


def ensemble(kind, drag, n_beams):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True) if drag else None
    ens = BeamEnsemble(nitinol_columns(256, kind), n_beams, force_params=fp, dtype=torch.float64)
    assert ens.n == N_RED
    return ens


def run_case(name):
    """Terminal states of case `name` on whatever stepper this process's environment selects, the free index, the seed."""
    kind, drag, n_beams, steps, _, _ = CASES[name]
    ens = ensemble(kind, drag, n_beams)
    x0 = seeded_state(name)
    ens.set_state(x0)
    ens.step(steps, DT, impulse_amp=amps_of(n_beams))
    return ens.unpack_state().cpu().numpy(), np.asarray(ens.free_index), x0


CHILD = """
import sys
import numpy as np
from tests import test_blocked_bcast_constants as m
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
def test_broadcast_constants_against_the_lean_stepper_and_the_oracle(name, lean_states, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    kind, drag, n_beams, steps, seed, tol = CASES[name]
    got, free, x0 = run_case(name)
    lean = lean_states[name]
    assert got.shape == lean.shape == (n_beams, 2 * N_RED)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(got, lean)
    errs = block_errs(got, lean, free)
    print(name, "against the one-node-per-lane stepper:", errs)
    assert max(errs.values()) <= tol, errs
    ob = oracle_beam(nitinol_columns(256, kind), **(dict(fluid_density=1000.0, enable_fluid=True) if drag else {}))
    ref, _ = ob.rk4_impulse_batch(x0, DT, steps, amps_of(n_beams))
    print(name, "against the oracle:", block_errs(got, ref, free))
    assert_blocks(got, ref, free, tol, what=name)


def test_table_registers_survive_the_beam_switch(monkeypatch):
    """4100 beams, 4 steps: 1025 groups of four beams, more than the workgroups that are resident, so a workgroup walks over
    several groups with the table loaded once, and the last round is a single group.  Four amplitudes in turn: beams of equal
    amplitude are bitwise equal wherever and whenever they ran; beams 0, 2047, 2048 and 4099 against the oracle."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    n_beams, steps = 4100, 4
    amps = 0.05 * (1.0 + np.arange(n_beams) % 4)
    ens = ensemble("nonlinear", True, n_beams)
    ens.step(steps, DT, impulse_amp=amps)
    got = ens.unpack_state()
    assert torch.isfinite(got).all()
    for k in range(4):
        same = got[k::4]
        assert torch.equal(same, same[:1].expand_as(same)), k
    assert not torch.equal(got[0], got[1])
    pick = [0, 2047, 2048, 4099]
    ob = oracle_beam(nitinol_columns(256, "nonlinear"), fluid_density=1000.0, enable_fluid=True)
    ref, _ = ob.rk4_impulse_batch(np.zeros((len(pick), 2 * N_RED)), DT, steps, amps[pick])
    assert_blocks(got[pick].cpu().numpy(), ref, np.asarray(ens.free_index), 1e-10, what="beam switch")


def test_one_launch_equals_five_launches_bitwise(monkeypatch):
    """100 steps in one launch against 5 launches of 20: the table and the broadcast copies are per launch, the results are
    bit for bit the same."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    n_beams = 6
    one, five = ensemble("nonlinear", True, n_beams), ensemble("nonlinear", True, n_beams)
    one.step(100, DT, impulse_amp=amps_of(n_beams))
    for _ in range(5):
        five.step(20, DT, impulse_amp=amps_of(n_beams))
    assert torch.isfinite(one.state).all() and one.state.abs().max() > 0
    assert torch.equal(one.state, five.state)
