"""GPU checks of the blocked stepper's folded element forces (crb_lean.h, lean_blocked_body with elem_force_nonlinear_folded
of crb_math.h: the pack's prefactors multiplied into the polynomial coefficients when the plan is built, the constants behind
the blocked tables).  Against the one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1 in a fresh child process, one for all
cases) and the oracle, with the tolerances of test_blocked_chord_rk4.py: 1e-10 from rest, 1e-9 from seeded states.  256
elements, B = 5: one full group of four waves and one partial.
  tip_w                  a tip w impulse from rest
  axial_first_node       an axial impulse on a lane's first node \\ the f1 exchange with the lane below / the difference of
  axial_last_node        ... and on a lane's last node           / f2 inside the lane carries it
  phi_last_node_closes   a rotation impulse on a lane's last node whose window closes between stages 0 and 1 of step 51
  seeded_rates           test_blocked_chord_rk4.py's bumps of u, w, phi and their rates: every monomial and the drag are live
  rigid_rotation         its near-rigid rotations: eps = sigma - (2/L) dw cancels to rounding, delta ~ 0
  seeded_no_drag         seeded_rates without the drag
  linear_seeded          the linear blocked instance, which does not take the folded form: bitwise the stored output of
                         the parent build (tests/golden/blocked_folded_linear_seeded.npy)
New for the folded constants, each with the drag on, from seeded_rates' state:
  length_0p3             element length 0.3 (length and wetted_area scaled): the products with L round
  length_0p0731          element length 0.0731, at a quarter of the step (RK4's stability limit falls with L^2)
  modulus_0p1            the modulus scaled by 0.1: the cD and cA terms change weight
The oracle carries every one of these states finitely over the horizon (checked on the CPU before they were fixed, and
asserted below).  Chunked stepping, snapshots, a single-slot record and beam isolation stay bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam
from tests.test_blocked_chord_rk4 import rigid_rotation, seeded_rates
from tests.test_blocked_stage_arith import seeded_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT = 2e-5
B = 5
AMPS = 0.05 * (1.0 + np.arange(B))
LANE = 30
N = 3 * 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blocked_folded_linear_seeded.npy")


def five(make):
    """The four beams of an imported initial state and the first of them again (it takes another impulse amplitude)."""
    def state(n):
        x0 = make(n)
        return np.vstack([x0, x0[:1]])
    return state


def columns(kind="nonlinear", length=0.25, modulus=1.0):
    cols = nitinol_columns(256, kind)
    cols["length"] = cols["length"] * (length / 0.25)
    cols["wetted_area"] = cols["wetted_area"] * (length / 0.25)
    cols["elastic_modulus"] = cols["elastic_modulus"] * modulus
    return cols


# name -> dict(kind, rod (keywords of columns), idx: reduced position index of the impulse, duration, state, steps, dt, tol, drag)
def case(idx=-2, duration=0.01, state=None, steps=100, tol=1e-10, kind="nonlinear", rod=None, dt=DT, drag=True):
    return dict(kind=kind, rod=rod or {}, idx=idx, duration=duration, state=state, steps=steps, dt=dt, tol=tol, drag=drag)


CASES = {
    "tip_w": case(),
    "axial_first_node": case(idx=3 * (4 * LANE) + 0, steps=60),
    "axial_last_node": case(idx=3 * (4 * LANE + 3) + 0, steps=60),
    "phi_last_node_closes": case(idx=3 * (4 * LANE + 3) + 2, duration=50.25 * DT),
    "seeded_rates": case(state=five(seeded_rates), steps=80, tol=1e-9),
    "rigid_rotation": case(state=five(rigid_rotation), steps=80, tol=1e-9),
    "seeded_no_drag": case(state=five(seeded_rates), steps=80, tol=1e-9, drag=False),
    "linear_seeded": case(idx=3 * (4 * LANE + 3) + 1, state=five(lambda n: seeded_state(n, "linear_seeded")), steps=80, tol=1e-9,
                          kind="linear"),
    "length_0p3": case(state=five(seeded_rates), steps=80, tol=1e-9, rod=dict(length=0.3)),
    "length_0p0731": case(state=five(seeded_rates), steps=80, tol=1e-9, rod=dict(length=0.0731), dt=DT / 4),
    "modulus_0p1": case(state=five(seeded_rates), steps=80, tol=1e-9, rod=dict(modulus=0.1)),
}


def initial_state(name):
    make = CASES[name]["state"]
    return np.zeros((B, 2 * N)) if make is None else make(N)


def make_ensemble(name="tip_w"):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    c = CASES[name]
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True) if c["drag"] else None
    return BeamEnsemble(columns(c["kind"], **c["rod"]), B, dtype=torch.float64, force_params=fp)


def run_case(name, chunks=1):
    """Terminal states of case `name` on whatever stepper this process's environment selects."""
    c = CASES[name]
    ens = make_ensemble(name)
    assert ens.n == N
    ens.set_state(initial_state(name))
    for _ in range(chunks):
        ens.step(c["steps"] // chunks, c["dt"], impulse_amp=AMPS, impulse_duration=c["duration"], impulse_index=c["idx"])
    return ens.unpack_state().cpu().numpy(), np.asarray(ens.free_index)


CHILD = """
import sys
import numpy as np
from tests import test_blocked_folded_forces as m
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
    ob = oracle_beam(columns(c["kind"], **c["rod"]), fluid_density=1000.0, enable_fluid=c["drag"])
    ref, _ = ob.rk4_impulse_batch(initial_state(name), c["dt"], c["steps"], AMPS, duration=c["duration"], idx=c["idx"])
    return ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_folded_forces_against_the_lean_stepper_and_the_oracle(name, lean_states, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    tol = CASES[name]["tol"]
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


def test_the_linear_instance_is_bitwise_its_parents(monkeypatch):
    """The linear blocked kernel is the parent's instruction for instruction; its output is the parent build's, stored."""
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    got, _ = run_case("linear_seeded")
    assert np.array_equal(got, np.load(GOLDEN))


def test_the_axial_impulses_reach_the_neighbouring_lanes():
    """The oracle's axial displacement right of and left of the struck node moves: the exchange of f1 with the lane below and
    the shifted-in f1 of the lane above are both on the path of these two cases."""
    for name, slot in (("axial_first_node", 4 * LANE), ("axial_last_node", 4 * LANE + 3)):
        ref = oracle_run(name)
        assert (np.abs(ref[:, 3 * (slot - 1)]) > 0).all() and (np.abs(ref[:, 3 * (slot + 1)]) > 0).all()


def test_the_new_rods_change_the_answer():
    """Each new rod moves seeded_rates' terminal w block by far more than the tolerance: a constant folded from the wrong
    length or modulus would be seen.  The short rod runs at a quarter of the step, so its base is the shipped rod at that step."""
    w = np.arange(1, N, 3)
    for name in ("length_0p3", "length_0p0731", "modulus_0p1"):
        c = CASES[name]
        ob = oracle_beam(columns(c["kind"]), fluid_density=1000.0, enable_fluid=c["drag"])
        base, _ = ob.rk4_impulse_batch(initial_state(name), c["dt"], c["steps"], AMPS, duration=c["duration"], idx=c["idx"])
        assert np.isfinite(base).all()
        moved = np.abs(oracle_run(name)[:, w] - base[:, w]).max() / np.abs(base[:, w]).max()
        print(name, "moves the w block by", moved)
        assert moved > 1e5 * c["tol"]


@pytest.mark.parametrize("name", ["phi_last_node_closes", "length_0p3"])
def test_one_launch_equals_two_launches_bitwise(name, monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    one, _ = run_case(name, chunks=1)
    two, _ = run_case(name, chunks=2)
    assert np.array_equal(one, two)


def test_snapshots_and_a_single_slot_record_equal_chunked_stepping(monkeypatch):
    monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    x0 = initial_state("length_0p3")
    k, n_rec = 10, 4
    ens, ref, one = (make_ensemble("length_0p3") for _ in range(3))
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
    clean.step(40, DT, impulse_amp=AMPS)
    ens = make_ensemble("seeded_rates")
    x0 = x0.copy()
    x0[2, N + 3 * (4 * LANE + 3) + 1] = np.nan     # (a w rate: it enters the drag and the position sums)
    ens.set_state(x0)
    ens.step(40, DT, impulse_amp=AMPS)
    good = np.arange(B) != 2
    got, want = ens.unpack_state(), clean.unpack_state()
    assert torch.equal(got[good], want[good])
    assert not torch.isfinite(got[2]).all() and torch.isfinite(got[good]).all()
