"""GPU checks of the blocked stepper's exchanges between neighbouring lanes and of the transverse force's sign (crb_lean.h,
lean_blocked_body): q of lane-1's last node and the left half of lane+1's first element cross a lane boundary every stage
by DPP lane shifts (0 comes in past the fixed root and past the tip; routing them through LDS strips of their own was
measured and not taken, DESIGN.md §4, so the stride-4 level's strip is the only one), the right transverse half is carried as
+f3 through the impulse block, and the wave's strip and the lane's separator-table address, formed once per launch, serve
every beam the workgroup walks over.  Impulses sit on every dof at lane boundaries
and at the beam's ends, with both signs; one workgroup walks over every beam; launches are chunked; a beam at rest follows a
beam with a large state.  Every run is compared with the one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1) and with the
oracle at 1e-10 per DOF block."""
import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DRAG = dict(fluid_density=1000.0, enable_fluid=True)
DT = 2e-5
TOL = 1e-10


def ensemble(cols, n_beams):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True)
    return BeamEnsemble(cols, n_beams, force_params=fp, dtype=torch.float64)


def run(monkeypatch, cols, x0, chunks, amps, idx, blocked=True, max_groups=None):
    """the state after stepping `chunks` (a list of step counts, one launch each) from x0, and the free index"""
    if blocked:
        monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
    else:
        monkeypatch.setenv("CRB_DISABLE_BLOCKED", "1")
    if max_groups is None:
        monkeypatch.delenv("CRB_LEAN_MAX_GROUPS", raising=False)
    else:
        monkeypatch.setenv("CRB_LEAN_MAX_GROUPS", str(max_groups))
    ens = ensemble(cols, x0.shape[0])
    ens.set_state(x0)
    for n in chunks:
        ens.step(n, DT, impulse_amp=amps, impulse_index=idx)
    return ens.unpack_state().cpu().numpy(), ens.free_index


def check_against_both(monkeypatch, cols, ob, got, free, x0, steps, amps, idx, what):
    """`got` against the one-node-per-lane stepper and against the oracle, each figure printed before it is asserted"""
    lean, _ = run(monkeypatch, cols, x0, [steps], amps, idx, blocked=False)
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(got, lean)
    errs = block_errs(got, lean, free)
    print(what, "vs one node per lane:", errs)
    assert max(errs.values()) <= TOL, errs
    ref, _ = ob.rk4_impulse_batch(x0, DT, steps, amps, idx=idx)
    print(what, "vs oracle:", block_errs(got, ref, free))
    assert_blocks(got, ref, free, TOL, what=what)


def seeded_ends(B, n, seed):
    """the state of test_blocked_strip_edges.test_state_seeded_near_the_tip_and_the_root: lanes 60 .. 63 and 0 .. 3"""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 2 * n))
    x0[:, 3 * 240:n] = rng.normal(0.0, 1e-5, (B, n - 3 * 240))       # positions of slots 240 .. 255
    x0[:, n + 3 * 240:] = rng.normal(0.0, 1e-2, (B, n - 3 * 240))    # their rates
    x0[:, :48] = rng.normal(0.0, 1e-5, (B, 48))                      # positions of slots 0 .. 15
    return x0


# reduced position index = 3 * slot + dof (fixed root), lane = slot // 4: slot 3 is lane 0's last node and slot 4 lane 1's
# first, 251 / 252 the same between lanes 62 and 63; slot 0 meets the root's pad, slot 255 the pad past the tip
@pytest.mark.parametrize("slot", [3, 4, 251, 252, 0, 255])
@pytest.mark.parametrize("dof", [0, 1, 2])
@pytest.mark.parametrize("kind", ["nonlinear", "linear"])
def test_impulse_on_each_dof_at_lane_boundaries(slot, dof, kind, monkeypatch):
    cols = nitinol_columns(256, kind)
    B, steps = 4, 60
    amps = np.array([0.05, -0.1, 0.15, -0.2])   # both signs
    idx = 3 * slot + dof
    ob = oracle_beam(cols, **DRAG)
    x0 = np.zeros((B, 2 * ob.n))
    got, free = run(monkeypatch, cols, x0, [steps], amps, idx)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    check_against_both(monkeypatch, cols, ob, got, free, x0, steps, amps, idx, (kind, slot, dof))


def test_strips_reused_from_beam_to_beam_by_one_workgroup(monkeypatch):
    """One workgroup walks over all three groups of B = 9 (the last with one beam): its waves' strips carry one beam's values
    when the next begins.  Bitwise the default grid's result."""
    cols = nitinol_columns(256, "nonlinear")
    B, steps = 9, 40
    ob = oracle_beam(cols, **DRAG)
    x0 = seeded_ends(B, ob.n, 11)
    amps = 0.03 * (1.0 + np.arange(B)) * np.where(np.arange(B) % 2, -1.0, 1.0)
    walked, free = run(monkeypatch, cols, x0, [steps], amps, -2, max_groups=1)
    default, _ = run(monkeypatch, cols, x0, [steps], amps, -2)
    assert np.isfinite(walked).all()
    assert np.array_equal(walked, default)
    check_against_both(monkeypatch, cols, ob, walked, free, x0, steps, amps, -2, "strip reuse")


def test_chunked_launches_equal_a_single_launch(monkeypatch):
    """7 steps in one launch, as 3 + 4 and as 7 x 1: the q that rides a stage's exchange crosses the launch boundary."""
    cols = nitinol_columns(256, "nonlinear")
    B = 5
    ob = oracle_beam(cols, **DRAG)
    x0 = seeded_ends(B, ob.n, 12)
    amps = np.array([0.1, -0.05, 0.0, 0.2, -0.3])
    one, free = run(monkeypatch, cols, x0, [7], amps, -2)
    two, _ = run(monkeypatch, cols, x0, [3, 4], amps, -2)
    seven, _ = run(monkeypatch, cols, x0, [1] * 7, amps, -2)
    assert np.isfinite(one).all()
    assert np.array_equal(one, two)
    assert np.array_equal(one, seven)
    check_against_both(monkeypatch, cols, ob, one, free, x0, 7, amps, -2, "chunked")


def test_no_stale_value_at_beam_start(monkeypatch):
    """Each wave of the one workgroup steps a beam with a large state (the seeded ends, and every other node moving too),
    then a beam at rest with no forcing: whatever the first left in the strips, the second must stay exactly zero."""
    cols = nitinol_columns(256, "nonlinear")
    B, steps = 8, 40
    ob = oracle_beam(cols, **DRAG)
    n = ob.n
    rng = np.random.default_rng(13)
    x0 = np.zeros((B, 2 * n))
    x0[:4] = seeded_ends(4, n, 14)
    x0[:4, :n] += rng.normal(0.0, 1e-8, (4, n))
    x0[:4, n:] += rng.normal(0.0, 1e-5, (4, n))
    amps = np.array([0.5, -0.5, 1.0, -1.0, 0.0, 0.0, 0.0, 0.0])
    got, free = run(monkeypatch, cols, x0, [steps], amps, -2, max_groups=1)
    assert np.isfinite(got).all() and np.abs(got[:4]).max() > 0.0
    assert not got[4:].any()
    check_against_both(monkeypatch, cols, ob, got, free, x0, steps, amps, -2, "stale")
