"""GPU checks of the blocked stepper's twisted interior solve and of its one right-neighbour exchange per stage (crb_lean.h,
lean_blocked_body: CRB_BLK_TWIST, CRB_BLK_ONE_RIGHT).  A lane's nodes 0 and 2 are eliminated into its centre node, and what a
lane owes the separator of lane-1 -- the left halves of its first element and C_s y_0 -- crosses the lane boundary as one sum,
so the impulse on the axial dof of a lane's last node lands on the local right half.  Both are the nonlinear instance's; the
linear instance keeps its parent's code (tests/test_blocked_folded_forces.py holds its output to the parent's bit for bit) and
runs the same cases here.  256-element rods with 1 beam and with 5 (a second group with one live wave), 12 steps, the
nonlinear + drag instance and the linear one:
  * an impulse on the tip's transverse dof, on the axial dof of a lane's last node (slot 4l + 3) and of its first (slot 4l)
    for lanes 0, 1 and 63, and on the last node's transverse dof and moment at the boundary of lanes 1 and 2;
  * a large-amplitude state, as test_blocked_exchange_strips.py uses;
  * a clock that starts inside the impulse window (which then closes between two stages) and one that starts after it;
  * a rod of element length 0.3 / 256, whose device-assembled node blocks lack the mirror structure bitwise (a rounding residue
    in B's off-diagonals): it runs the block-Thomas instance, with the one exchange.
Which instance a plan runs is asserted, not assumed (crb_plan_get_blocked_form): the twisted one for the default nonlinear
rod -- the benchmark's -- and block Thomas for the 0.3 rod and for every linear plan.
Every run is compared with the one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1 in a fresh child process, one for all cases)
and with the oracle, at the bounds of the existing blocked tests: 1e-10 per DOF block from rest, 1e-9 for seeded states.  A
rollout cut into several launches is bitwise the single launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT = 2e-5
STEPS = 12
DRAG = dict(fluid_density=1000.0, enable_fluid=True)


def case(idx=-2, duration=0.01, state=None, t0=0.0, tol=1e-10, length=0.25):
    return dict(idx=idx, duration=duration, state=state, t0=t0, tol=tol, length=length)


def columns(kind, name):
    cols = nitinol_columns(256, kind)
    scale = CASES[name]["length"] / 0.25
    cols["length"] = cols["length"] * scale
    cols["wetted_area"] = cols["wetted_area"] * scale
    return cols


# name -> reduced position index of the impulse (3 * slot + dof, fixed root; -2: the tip's w), its window, the initial state,
# the clock at the start, the tolerance
CASES = {"tip_w": case()}
for _lane in (0, 1, 63):
    CASES[f"last_node_axial_lane{_lane}"] = case(idx=3 * (4 * _lane + 3))
    CASES[f"first_node_axial_lane{_lane}"] = case(idx=3 * (4 * _lane))
CASES["last_node_w_lane1"] = case(idx=3 * 7 + 1)
CASES["last_node_phi_lane1"] = case(idx=3 * 7 + 2)
CASES["large_state"] = case(state="large", tol=1e-9)
# the clock starts at 2 DT inside a window of 5.25 DT: open for three steps and the first stage of the fourth
CASES["clock_inside_window"] = case(idx=3 * 7, duration=5.25 * DT, t0=2.0 * DT)
CASES["clock_after_window"] = case(duration=5.25 * DT, t0=6.0 * DT, state="ends", tol=1e-9)
CASES["length_0p3_last_node_axial"] = case(idx=3 * 7, length=0.3)
CASES["length_0p3_large_state"] = case(state="large", tol=1e-9, length=0.3)
KINDS = ("nonlinear", "linear")
BEAMS = (1, 5)


def amps_of(B):
    return 0.05 * (1.0 + np.arange(B)) * np.where(np.arange(B) % 2, -1.0, 1.0)   # (both signs)


def initial_state(name, B, n):
    """None: at rest.  "ends": test_blocked_exchange_strips.seeded_ends (lanes 60 .. 63 and 0 .. 3).  "large": that file's large
    state, the seeded ends with every other node moving too."""
    what = CASES[name]["state"]
    x0 = np.zeros((B, 2 * n))
    if what is None:
        return x0
    rng = np.random.default_rng(sum(map(ord, name)) + B)
    x0[:, 3 * 240:n] = rng.normal(0.0, 1e-5, (B, n - 3 * 240))
    x0[:, n + 3 * 240:] = rng.normal(0.0, 1e-2, (B, n - 3 * 240))
    x0[:, :48] = rng.normal(0.0, 1e-5, (B, 48))
    if what == "large":
        x0[:, :n] += rng.normal(0.0, 1e-8, (B, n))
        x0[:, n:] += rng.normal(0.0, 1e-5, (B, n))
    return x0


def large_amps(name, B):
    # (the large state is driven as test_blocked_exchange_strips.test_no_stale_value_at_beam_start drives it: up to 1.0)
    return amps_of(B) * (4.0 if CASES[name]["state"] == "large" else 1.0)


def run_case(kind, B, name, chunks=(STEPS,)):
    """Terminal states of a case on whatever stepper this process's environment selects, the free index, the initial state."""
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    c = CASES[name]
    ens = BeamEnsemble(columns(kind, name), B, dtype=torch.float64,
                       force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    x0 = initial_state(name, B, ens.n)
    ens.set_state(x0, time=c["t0"])
    for n in chunks:
        ens.step(n, DT, impulse_amp=large_amps(name, B), impulse_duration=c["duration"], impulse_index=c["idx"])
    return ens.unpack_state().cpu().numpy(), np.asarray(ens.free_index), x0


THOMAS, TWISTED = 1, 2   # (crb_plan_get_blocked_form)


def expected_form(kind, name):
    return TWISTED if kind == "nonlinear" and CASES[name]["length"] == 0.25 else THOMAS


@pytest.mark.parametrize("name", ["tip_w", "length_0p3_large_state"])
@pytest.mark.parametrize("B", BEAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_plan_runs_the_instance_it_should(kind, B, name):
    """The default nonlinear rod (the benchmark's config 3) holds the twisted tables, three separator levels; the linear
    instance and the rod whose assembled blocks lack the mirror structure bitwise hold block Thomas's."""
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    ens = BeamEnsemble(columns(kind, name), B, dtype=torch.float64,
                       force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    assert ens.plan.blocked_form() == (expected_form(kind, name), 3)


def test_the_benchmark_plan_runs_the_twisted_instance():
    """config 3 as bench.py builds it: 4096 beams x 256 nonlinear elements + drag, fp64."""
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    ens = BeamEnsemble(nitinol_columns(256, "nonlinear"), 4096, dtype=torch.float64,
                       force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    assert ens.plan.blocked_form() == (TWISTED, 3)


CHILD = """
import sys
import numpy as np
from tests import test_blocked_twist_solve as m
np.savez(sys.argv[1], **{f"{kind}_{B}_{name}": m.run_case(kind, B, name)[0] for kind in m.KINDS for B in m.BEAMS for name in m.CASES})
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


@pytest.fixture(scope="module")
def oracles():
    return {(kind, length): oracle_beam(columns(kind, name), **DRAG)
            for kind in KINDS for length, name in {c["length"]: n for n, c in CASES.items()}.items()}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("B", BEAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_lean_stepper_and_the_oracle(kind, B, name, lean_states, oracles, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    c = CASES[name]
    got, free, x0 = run_case(kind, B, name)
    lean = lean_states[f"{kind}_{B}_{name}"]
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(got, lean)
    errs = block_errs(got, lean, free)
    print(kind, B, name, "against the one-node-per-lane stepper:", errs)
    assert max(errs.values()) <= c["tol"], errs
    ref, _ = oracles[kind, c["length"]].rk4_impulse_batch(x0, DT, STEPS, large_amps(name, B), duration=c["duration"], idx=c["idx"], t0=c["t0"])
    print(kind, B, name, "against the oracle:", block_errs(got, ref, free))
    assert_blocks(got, ref, free, c["tol"], what=(kind, B, name))


@pytest.mark.parametrize("name", ["last_node_axial_lane1", "large_state", "clock_inside_window", "length_0p3_large_state"])
@pytest.mark.parametrize("kind", KINDS)
def test_chunked_launches_equal_a_single_launch(kind, name, monkeypatch):
    """12 steps in one launch, as 5 + 7 and as 12 x 1: the state between launches is (q, v) and nothing else."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    one, _, _ = run_case(kind, 5, name)
    two, _, _ = run_case(kind, 5, name, chunks=(5, 7))
    each, _, _ = run_case(kind, 5, name, chunks=(1,) * STEPS)
    assert np.isfinite(one).all() and np.abs(one).max() > 0.0
    assert np.array_equal(one, two)
    assert np.array_equal(one, each)


def test_the_window_closed_from_the_start_is_no_impulse_at_all(monkeypatch):
    """The clock starts behind the window: bitwise the run without an impulse."""
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    a, _, x0 = run_case("nonlinear", 5, "clock_after_window")
    ens = BeamEnsemble(nitinol_columns(256, "nonlinear"), 5, dtype=torch.float64,
                       force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    ens.set_state(x0, time=CASES["clock_after_window"]["t0"])
    ens.step(STEPS, DT)
    assert np.array_equal(a, ens.unpack_state().cpu().numpy())
