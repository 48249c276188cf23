"""GPU checks of the blocked stepper's separator levels at the beam's ends (crb_lean.h, lean_blocked_body): the level at lane
stride 4 reads its neighbours from a per-wave LDS strip whose zeroed pads stand in for the lanes past the fixed root and the
tip.  Forcing and state sit in the first and the last four lanes, where those pads are read; every run is compared with the
one-node-per-lane stepper (CRB_DISABLE_BLOCKED=1) and with the oracle."""
import numpy as np
import pytest

from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DRAG = dict(fluid_density=1000.0, enable_fluid=True)
DT = 2e-5


def ensemble(cols, n_beams):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True)
    return BeamEnsemble(cols, n_beams, force_params=fp, dtype=torch.float64)


def both_kernels(monkeypatch, cols, x0, steps, amps, idx):
    """(blocked stepper, one-node-per-lane stepper, free index) after `steps` steps from x0"""
    outs = []
    for disable in (False, True):
        if disable:
            monkeypatch.setenv("CRB_DISABLE_BLOCKED", "1")
        else:
            monkeypatch.delenv("CRB_DISABLE_BLOCKED", raising=False)
        ens = ensemble(cols, x0.shape[0])
        ens.set_state(x0)
        ens.step(steps, DT, impulse_amp=amps, impulse_index=idx)
        outs.append(ens.unpack_state().cpu().numpy())
    # (two different solves agree to rounding, not bit for bit: equal outputs would mean the blocked stepper did not run)
    assert not np.array_equal(outs[0], outs[1])
    return outs[0], outs[1], ens.free_index


# reduced position index = 3 * slot + dof (fixed root), lane = slot // 4: slots 0 .. 15 are lanes 0 .. 3, 240 .. 255 lanes 60 .. 63
@pytest.mark.parametrize("idx", [1, 3 * 5 + 2, 3 * 14, 3 * 241 + 1, 3 * 250 + 2, 3 * 255])
@pytest.mark.parametrize("kind", ["nonlinear", "linear"])
def test_impulse_in_the_first_or_last_four_lanes(idx, kind, monkeypatch):
    cols = nitinol_columns(256, kind)
    B, steps = 4, 120
    amps = 0.05 * (1.0 + np.arange(B))
    ob = oracle_beam(cols, **DRAG)
    x0 = np.zeros((B, 2 * ob.n))
    got, lean, free = both_kernels(monkeypatch, cols, x0, steps, amps, idx)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    errs = block_errs(got, lean, free)
    assert max(errs.values()) <= 1e-10, errs
    ref, _ = ob.rk4_impulse_batch(x0, DT, steps, amps, idx=idx)
    assert_blocks(got, ref, free, 1e-10, what=(kind, idx))


def test_state_seeded_near_the_tip_and_the_root(monkeypatch):
    """A state seeded on the last four lanes' nodes (rates large against the impulse's) and on the first four lanes': the pads
    past the tip and the root must contribute exactly nothing whatever the values next to them are."""
    cols = nitinol_columns(256, "nonlinear")
    B, steps = 3, 80
    ob = oracle_beam(cols, **DRAG)
    n = ob.n
    rng = np.random.default_rng(7)
    x0 = np.zeros((B, 2 * n))
    x0[:, 3 * 240:n] = rng.normal(0.0, 1e-5, (B, n - 3 * 240))       # positions of slots 240 .. 255
    x0[:, n + 3 * 240:] = rng.normal(0.0, 1e-2, (B, n - 3 * 240))    # their rates
    x0[:, :48] = rng.normal(0.0, 1e-5, (B, 48))                      # positions of slots 0 .. 15
    amps = np.array([0.0, 0.1, 1.0])
    got, lean, free = both_kernels(monkeypatch, cols, x0, steps, amps, -2)
    assert np.isfinite(got).all()
    errs = block_errs(got, lean, free)
    assert max(errs.values()) <= 1e-9, errs
    ref, _ = ob.rk4_impulse_batch(x0, DT, steps, amps)
    assert_blocks(got, ref, free, 1e-9, what="seeded ends")
