"""The tangent of the sampled-data implicit loop on the GPU (BeamEnsemble.step_implicit_feedback_tangent /
linearize_implicit_feedback; crb_step_implicit_feedback_tangent), on the rods of tests/test_implicit_feedback_tangent_cpu.py,
which proves their inputs and the finite-difference reference on the oracle alone.

  1. the transpose of the merged adjoint: <lam, dx(T)> against the five terms of step_implicit_feedback_adjoint, on every rod,
     then each input family alone;
  2. linear rods: linearize_implicit_feedback is A_d - B_d K and B_d K of linearize_implicit, and their powers;
  3. central differences of the oracle's chain under fd_check's rule;
  4. the bitwise properties, the replay through step_implicit_tangent, the control against rollout_implicit_feedback's;
  5. the base state against step_implicit_feedback on both of its paths, the clock, the status, the padding, junk in the seeds;
  6. edges: non-finite seeds, 257 slots, fp32, mixed topology, no steps, hold > n_steps, 4096 x 256.
Measured figures and the bounds derived from them: tests/README_implicit_feedback_tangent.md.  Every comparison against a
measured bound prints ``[implicit-feedback-tangent] key | err | allowed`` (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from continuum_robot import _native as nat
from continuum_robot.batched import BeamEnsemble, ControlSchedule
from tests.helpers import assert_blocks, block_errs, nitinol_columns, oracle_beam
from tests.test_adjoint import np_
from tests.test_derivative_mappings import clock
from tests.test_implicit_adjoint import blockwise
from tests.test_implicit_adjoint_mappings_cpu import CASES, T0
from tests.test_implicit_feedback_cpu import gain_scales, sample_response
from tests.test_implicit_feedback_tangent_cpu import ALONE_RODS, FAMILIES, FD_RODS, RODS, TAG, fd_step, loop
from tests.test_implicit_tangent import MEASURED as OPEN_MEASURED
from tests.test_implicit_tangent_cpu import LINEAR_RODS
from tests.test_tangent_linear import fd_check, force_params, oracle_kw

pytestmark = pytest.mark.gpu

FLOOR, CAP = 1e-13, 1e-9
# Test 1's allowance per rod: 16 x the mismatch of the OPEN-loop pair the project had before this call -- step_implicit_tangent
# against step_implicit_adjoint on the same rod, steps and hold, the closed-loop run's own control fed as a ControlSchedule,
# the same seeds (open_loop_mismatch below) -- measured on one MI355X; never below FLOOR (rods whose figure is at rounding),
# never above CAP (a dropped or mis-signed term shows at 1e-2 ... 1).  tests/README_implicit_feedback_tangent.md.
OPEN_LOOP_MISMATCH = {
    "one_element": 3.11e-15,
    "packed_partial": 1.23e-14,
    "packed_pinned": 3.62e-15,
    "two_per_wave_pin": 1.87e-15,
    "two_waves_min": 2.46e-15,
    "four_waves_min": 5.61e-15,
    "four_waves_full": 4.32e-14,
}
# Test 2's allowance per rod: 16 x the larger figure tests/README_implicit_tangent.md records for linearize_implicit against
# the Cayley recursion on the same rod (tests/test_implicit_tangent.py: MEASURED), never above CAP.  rod -> (hold, n_iter)
LINEAR_RUNS = {"n6_h1e-4": (3, 2), "n10_h1e-3": (1, 1), "n64_h1e-3": (1, 2)}


def transpose_allowed(name):
    m = OPEN_LOOP_MISMATCH[name]
    assert m is not None, f"no open-loop figure recorded for {name}"
    return min(max(16.0 * m, FLOOR), CAP)


def linear_allowed(rod):
    figs = [v for k, v in OPEN_MEASURED.items() if k.startswith(f"linearize {rod} ")]
    assert len(figs) >= 2
    return min(16.0 * max(figs), CAP)


class Rod:
    """A rod of the CPU file on the GPU: its ensemble, and the calls on the oracle's inputs from the clock T0"""

    def __init__(self, name):
        self.name, self.lp = name, loop(name)
        lp, c = self.lp, CASES[name]
        self.ens = BeamEnsemble(lp.cols, lp.B, force_params=force_params(True, True), corrected_axial=c["corrected"])
        lay = self.ens.plan.layout
        assert (lay.n_slots, lay.beams_per_group, lay.threads) == c["layout"], name
        assert self.ens.n == lp.n and np.array_equal(self.ens.free_index, lp.fi)
        assert self.ens.reduced_index(c["imp"], c["imp_dof"]) == lp.idx
        self.inp = dict(impulse_amp=lp.amps, impulse_duration=lp.duration, impulse_index=lp.idx, held_force=lp.U)
        self.loop_kw = dict(reference=lp.R, hold=lp.hold, n_iter=lp.n_iter, **self.inp)

    def tangent(self, s, steps=None, **kw):
        """dx(T) along the seeds ``s`` (Loop.seeds) from the oracle's start state; ``state`` and ``time`` advance"""
        lp = self.lp
        self.ens.set_state(lp.X, T0)
        args = dict(self.loop_kw, d_gain=s["gain"], d_reference=s["reference"], d_held_force=s["held"], d_impulse_amp=s["amp"])
        args.update(kw)
        return self.ens.step_implicit_feedback_tangent(lp.steps if steps is None else steps, lp.h, s["x0"], lp.K, **args)

    def adjoint(self, lam):
        lp = self.lp
        return self.ens.step_implicit_feedback_adjoint(lp.steps, lp.h, lam, lp.K, x0_red=lp.X, t0=T0, **self.loop_kw)


@functools.lru_cache(maxsize=None)
def rod(name):
    return Rod(name)


def take(s, d):
    return {k: v[d] for k, v in s.items()}


def mismatch(lam, Jv, pairs):
    """| <lam, dx(T)> - sum of <cotangent, seed> | / (|<lam, dx(T)>| + sum of |<cotangent, seed>|) per direction (axis 0), each
    inner product over the whole ensemble (gain_bar is a sum over the beams); the worst direction"""
    D = lam.shape[0]
    lhs = np.sum((lam * Jv).reshape(D, -1), axis=1)
    terms = [np.sum((a * b).reshape(D, -1), axis=1) for a, b in pairs]
    scale = np.abs(lhs) + sum(np.abs(t) for t in terms)
    assert np.all(scale > 0.0) and np.all(np.isfinite(scale))
    return float(np.max(np.abs(lhs - sum(terms)) / scale))


def open_loop_mismatch(g):
    """The same figure for the pair the closed-loop pair is held against: step_implicit_tangent and step_implicit_adjoint on
    the rod, steps and hold of ``g``, the closed-loop run's own control as the schedule, seeds on x0, the schedule and amp."""
    lp, ens = g.lp, g.ens
    _, control = ens.rollout_implicit_feedback(lp.X, lp.steps, lp.h, lp.K, reference=lp.R, hold=lp.hold, n_iter=lp.n_iter, t0=T0,
                                               return_control=True, **g.inp)
    K = control.shape[0]
    sched = ControlSchedule(control, lp.hold)
    rng = np.random.default_rng(77)
    dU = np.where(lp.transverse, rng.normal(0.0, 1.0, (lp.D, K, lp.B, lp.n)), 0.0) * np.max(np.abs(lp.dF))
    kw = dict(n_iter=lp.n_iter, impulse_amp=lp.amps, impulse_duration=lp.duration, impulse_index=lp.idx, held_force=sched, t0=T0)
    ens.set_state(lp.X, T0)
    Jv = np_(ens.step_implicit_tangent(lp.steps, lp.h, lp.dX, d_impulse_amp=lp.dA, d_held_force=dU, **kw))
    xb, ab, sb = ens.step_implicit_adjoint(lp.steps, lp.h, lp.lam, x0_red=lp.X, **kw)
    return mismatch(lp.lam, Jv, [(np_(xb), lp.dX), (np_(ab), lp.dA), (np_(sb), dU)])


# ------------------------------------------------------------------ 1. the transpose of the merged adjoint
def transpose_figure(g, s):
    lp = g.lp
    Jv = np_(g.tangent(s))
    assert np.all(np.isfinite(Jv)) and np.max(np.abs(Jv)) > 0.0
    xb, gb, rb, ab, fb = (np_(t) for t in g.adjoint(lp.lam))
    return mismatch(lp.lam, Jv, [(xb, s["x0"]), (gb, s["gain"]), (rb, s["reference"]), (fb, s["held"]), (ab, s["amp"])])


@pytest.mark.parametrize("name", list(RODS))
def test_tangent_is_the_transpose_of_the_merged_adjoint(name):
    g = rod(name)
    err = transpose_figure(g, g.lp.seeds())
    own = open_loop_mismatch(g)
    print(f"{TAG} transpose {name} | err {err:.2e} | open-loop pair here {own:.2e} | recorded {OPEN_LOOP_MISMATCH[name]} | "
          f"allowed {transpose_allowed(name):.2e}")
    assert err <= transpose_allowed(name), (name, err)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", ALONE_RODS)
def test_each_input_family_alone_is_the_transpose(name, family):
    g = rod(name)
    s = g.lp.seeds(family)
    assert sum(bool(np.any(v != 0.0)) for v in s.values()) == 1
    err = transpose_figure(g, s)
    print(f"{TAG} transpose {name} {family} alone | err {err:.2e} | allowed {transpose_allowed(name):.2e}")
    assert err <= transpose_allowed(name), (name, family, err)


# ------------------------------------------------------------------ 2. linear rods: exact composition
def linear_gain(cols, n, h, hold, n_iter, rng):
    ob = oracle_beam(cols, **oracle_kw(False, False))
    scale, damp = gain_scales(sample_response(ob, h, hold, n_iter), n)
    K = scale * rng.normal(0.0, 1.0, (n, 2 * n))
    K[np.arange(n), n + np.arange(n)] += damp
    return K


@pytest.mark.parametrize("name", list(LINEAR_RUNS))
def test_linearisation_of_a_linear_rod_is_the_composition_of_the_open_loop_pair(name):
    n_elem, h = LINEAR_RODS[name]
    hold, n_iter = LINEAR_RUNS[name]
    cols = nitinol_columns(n_elem, "linear")
    ens = BeamEnsemble(cols, 2, force_params=force_params(False, False))
    n = ens.n
    rng = np.random.default_rng(40 + n_elem)
    K = linear_gain(cols, n, h, hold, n_iter, rng)
    x0, R = 1e-3 * rng.normal(0.0, 1.0, (2, 2 * n)), 1e-3 * rng.normal(0.0, 1.0, (2, 2 * n))
    ens.set_state(x0, 0.125)
    _ = ens.status
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    Ad, Bd = (np_(t) for t in ens.linearize_implicit(h, n_steps=hold, n_iter=n_iter))
    tol = linear_allowed(name)
    for n_samples in (1, 3):
        Phi, G = (np_(t) for t in ens.linearize_implicit_feedback(h, K, reference=R, hold=hold, n_samples=n_samples, n_iter=n_iter))
        assert Phi.shape == G.shape == (2, 2 * n, 2 * n)
        for b in range(2):
            Acl, BK = Ad[b] - Bd[b] @ K, Bd[b] @ K
            want_phi, want_g = np.linalg.matrix_power(Acl, n_samples), sum(np.linalg.matrix_power(Acl, j) for j in range(n_samples)) @ BK
            e_phi, e_g = blockwise(Phi[b], want_phi, n), blockwise(G[b], want_g, n)
            print(f"{TAG} linear {name} {n_samples} sample(s) beam {b} | Phi_cl {e_phi:.2e} G_ref {e_g:.2e} | allowed {tol:.2e}")
            assert e_phi <= tol and e_g <= tol, (name, n_samples, b, e_phi, e_g)
            assert blockwise(Phi[b], np.linalg.matrix_power(Ad[b], n_samples), n) > 1e-3      # (the gain is what it measures)
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)
    # the status reporting goes on where it stood
    ens.step_implicit(2, h)
    x = ens.unpack_state()
    x[0, 0] = float("nan")
    ens.state = ens.pack_state(x)
    ens.step_implicit(3, h)
    assert ens.status.tolist() == [5, 0]


# ------------------------------------------------------------------ 3. central differences of the oracle's chain
@pytest.mark.parametrize("name", FD_RODS)
def test_tangent_matches_central_differences_of_the_oracles_chain(name):
    g = rod(name)
    lp = g.lp
    for family in FAMILIES:
        jvp = np_(g.tangent(take(lp.seeds(family), slice(0, 1))))[0]
        errs = fd_check(jvp, lp.F(family), fd_step(name, family), lp.fi, f"{name}: {family}")
        print(f"{TAG} fd {name} {family} | " + " ".join(f"{b} {e:.1e}" for b, e in errs.items()))


# ------------------------------------------------------------------ 4. bitwise properties
@pytest.mark.parametrize("name", ["packed_partial", "packed_pinned", "two_waves_min"])
def test_batching_broadcasting_repetition_and_the_skipped_gain_product_are_bitwise(name):
    g = rod(name)
    lp, ens = g.lp, g.ens
    s = lp.seeds()
    ref, (U, dU) = g.tangent(s, return_control=True)
    base = ens.state.clone()
    assert torch.isfinite(ref).all() and tuple(dU.shape) == (lp.D,) + tuple(U.shape) == (lp.D, -(-lp.steps // lp.hold), lp.B, lp.n)
    # two identical calls; D directions in one call are D calls of one
    again, (U2, dU2) = g.tangent(s, return_control=True)
    assert torch.equal(again, ref) and torch.equal(U2, U) and torch.equal(dU2, dU) and torch.equal(ens.state, base)
    for d in range(lp.D):
        one, (U1, dU1) = g.tangent(take(s, d), return_control=True)
        assert torch.equal(one, ref[d]) and torch.equal(U1, U) and torch.equal(dU1[0], dU[d]) and torch.equal(ens.state, base), d
    # a [B, .] seed serves every direction
    first = take(s, 0)
    got = g.tangent(dict(s, gain=first["gain"], reference=first["reference"], held=first["held"], amp=first["amp"]))
    want = g.tangent({k: (v if k == "x0" else np.stack([first[k]] * lp.D)) for k, v in s.items()})
    assert torch.equal(got, want) and not torch.equal(got, ref)
    # d_gain=None: the product is skipped, the state is the same, and dx equals that of a zero d_gain
    none = g.tangent(dict(s, gain=None))
    state_none = ens.state.clone()
    zero = g.tangent(dict(s, gain=np.zeros_like(s["gain"])))
    assert torch.equal(state_none, base) and torch.equal(ens.state, base)
    assert torch.equal(none, zero) and not torch.equal(none, ref)
    # the replay through the open-loop tangent with the call's own control and its tangent
    kw = dict(n_iter=lp.n_iter, impulse_amp=lp.amps, impulse_duration=lp.duration, impulse_index=lp.idx)
    ens.set_state(lp.X, T0)
    replay = ens.step_implicit_tangent(lp.steps, lp.h, s["x0"], held_force=ControlSchedule(U, lp.hold), d_held_force=dU,
                                       d_impulse_amp=s["amp"], **kw)
    assert torch.equal(replay, ref) and torch.equal(ens.state, base)


@pytest.mark.parametrize("name", list(RODS))
def test_control_is_the_differentiable_rollouts(name):
    g = rod(name)
    lp = g.lp
    _, (U, dU) = g.tangent(take(lp.seeds(), 0), return_control=True)
    _, want = g.ens.rollout_implicit_feedback(lp.X, lp.steps, lp.h, lp.K, reference=lp.R, hold=lp.hold, n_iter=lp.n_iter, t0=T0,
                                              return_control=True, **g.inp)
    errs = block_errs(np_(U).reshape(-1, lp.n), np_(want).reshape(-1, lp.n), lp.fi)
    print(f"{TAG} control {name} | worst block {max(errs.values()):.2e} | allowed 1.00e-07")
    assert_blocks(np_(U).reshape(-1, lp.n), np_(want).reshape(-1, lp.n), lp.fi, 1e-7, what=f"{name} control")
    assert float(dU.abs().max()) > 0.0


# ------------------------------------------------------------------ 5. base state and side effects
@pytest.mark.parametrize("path", ["0", "1"])
@pytest.mark.parametrize("name", list(RODS))
def test_base_state_clock_and_status_are_step_implicit_feedbacks(name, path, monkeypatch):
    g = rod(name)
    lp, ens = g.lp, g.ens
    monkeypatch.setenv("CRB_IMPLICIT_FEEDBACK", path)
    twin = BeamEnsemble(lp.cols, lp.B, force_params=force_params(True, True), corrected_axial=CASES[name]["corrected"])
    s = take(lp.seeds(), 0)
    for e in (ens, twin):
        e.set_state(lp.X, T0)
        assert int(e.status.abs().max()) == 0
    args = dict(g.loop_kw, d_gain=s["gain"], d_reference=s["reference"], d_held_force=s["held"], d_impulse_amp=s["amp"])
    ens.step_implicit_feedback_tangent(lp.steps, lp.h, s["x0"], lp.K, **args)
    twin.step_implicit_feedback(lp.steps, lp.h, lp.K, **g.loop_kw)
    assert ens.time == twin.time == clock(T0, lp.h, lp.steps)
    errs = assert_blocks(np_(ens.unpack_state()), np_(twin.unpack_state()), lp.fi, 1e-7, what=f"{name}: base")
    print(f"{TAG} base {name} path {twin.implicit_feedback_path()} | worst block {max(errs.values()):.2e} | allowed 1.00e-07")
    assert int(ens.status.abs().max()) == 0 and int(twin.status.abs().max()) == 0
    # a beam that goes non-finite is marked with the ensemble's step count at the end of the call, as step_implicit_feedback marks it
    # (from the start state again, 3 + 5 steps: the pinned 65-slot rod does not stay finite for 5 steps more after its 40,
    #  on the oracle either)
    last = lp.B - 1
    for e in (ens, twin):
        e.set_state(lp.X, T0)
    ens.step_implicit_feedback_tangent(3, lp.h, s["x0"], lp.K, **args)
    twin.step_implicit_feedback(3, lp.h, lp.K, **g.loop_kw)
    for e in (ens, twin):
        x = e.unpack_state()
        x[last, 0] = float("nan")
        e.state = e.pack_state(x)
    ens.step_implicit_feedback_tangent(5, lp.h, s["x0"], lp.K, **args)
    twin.step_implicit_feedback(5, lp.h, lp.K, **g.loop_kw)
    want = [0] * last + [3 + 5]
    assert ens.status.tolist() == want and twin.status.tolist() == want and ens.time == twin.time


@pytest.mark.parametrize("name", ["packed_partial", "packed_pinned", "four_waves_min"])
def test_padding_holds_zeros_and_junk_in_the_seeds_changes_nothing(name):
    g = rod(name)
    lp, ens = g.lp, g.ens
    s = take(lp.seeds(), slice(0, 2))
    ref, (U, dU) = g.tangent(s, return_control=True)
    # the device buffers of the last call: dx, u_out, du_out
    dxd, u_out, du_out = ens._keep[-4], ens._keep[-3], ens._keep[-2]
    free = torch.zeros(ens.n_node * 4, dtype=torch.bool, device=ens.device)
    fi = torch.as_tensor(np.asarray(lp.fi), device=ens.device)
    free[(fi // 3) * 4 + fi % 3] = True
    assert dxd.shape[-2:] == (ens.n_node, 4) and du_out.shape[-2:] == (ens.n_node, 4)
    for t in (dxd, u_out, du_out):
        flat = t.reshape(-1, ens.n_node * 4)
        assert bool((flat[:, ~free] == 0).all()) and bool((flat[:, free] != 0).any())
    # junk in component 3 and at constrained DOFs of the packed seeds: through the C ABI, since the Python packing never writes there
    K = ens._dev(lp.K)
    R = ens._dev(lp.R)

    def native(junk):
        ens.set_state(lp.X, T0)
        dx = ens._pack_dirs(ens._dev(s["x0"]), True)
        df = ens._pack_dirs(ens._dev(s["held"]), False)
        if junk:
            dx.reshape(-1, ens.n_node * 4)[:, ~free] = 7.25
            df.reshape(-1, ens.n_node * 4)[:, ~free] = float("nan")
        desc, keep = ens._input_desc(lp.amps, lp.duration, lp.idx, lp.U)
        fbt, tan = nat.FeedbackTangent(), nat.InputTangent()
        dK, dR, dA = ens._dev(s["gain"]), ens._dev(s["reference"]), ens._dev(s["amp"])
        fbt.d_gain, fbt.d_ref, tan.d_amp, tan.df_held = dK.data_ptr(), dR.data_ptr(), dA.data_ptr(), df.data_ptr()
        work = torch.empty(int(ens._lib.crb_implicit_feedback_tangent_work_bytes(ens.plan.h, 2)), dtype=torch.uint8, device=ens.device)
        t_end = C.c_double(0.0)
        nat.check(ens._lib.crb_step_implicit_feedback_tangent(
            ens.plan.h, ens._ptr(ens.state), ens._ptr(dx), 2, T0, lp.h, lp.steps, lp.n_iter, lp.hold, ens._ptr(K), ens._ptr(R),
            C.byref(fbt), C.byref(desc), C.byref(tan), None, None, ens._ptr(work), C.byref(t_end), ens._stream()))
        torch.cuda.synchronize()
        return ens._unpack_dirs(dx), ens.state.clone()

    clean, x_clean = native(False)
    dirty, x_dirty = native(True)
    assert torch.equal(clean, ref)                       # (u_out and du_out NULL: the work buffer's records, the same results)
    assert torch.equal(dirty, clean) and torch.equal(x_dirty, x_clean)


# ------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("name", ["packed_partial", "two_waves_min"])
def test_non_finite_seed_stays_in_its_beam_and_direction(name):
    g = rod(name)
    lp, ens = g.lp, g.ens
    s = lp.seeds()
    ref = g.tangent(s)
    base = ens.state.clone()
    for family, entry in (("x0", (1, 1, lp.n + 1)), ("reference", (1, 1, 2)), ("held", (1, 1, int(np.flatnonzero(lp.transverse)[0])))):
        bad = {k: v.copy() for k, v in s.items()}
        bad[family][entry] = float("nan")
        got = g.tangent(bad)
        assert torch.equal(ens.state, base) and int(ens.status.abs().max()) == 0, family
        assert not torch.isfinite(got[1, 1]).all(), family
        keep = torch.ones(got.shape[:2], dtype=torch.bool)
        keep[1, 1] = False
        assert torch.equal(got[keep], ref[keep]) and torch.isfinite(got[keep]).all(), family
    # a non-finite gain direction stays in its direction
    bad = {k: v.copy() for k, v in s.items()}
    bad["gain"][2, 0, 0] = float("inf")
    got = g.tangent(bad)
    assert torch.equal(got[:2], ref[:2]) and not torch.isfinite(got[2]).all() and torch.equal(ens.state, base)


def test_refusals_leave_state_and_time_alone_and_no_steps_change_nothing():
    big = BeamEnsemble(nitinol_columns(257, "linear"), 1, force_params=force_params(False, False))
    big.set_state(1e-3 * np.ones((1, 2 * big.n)), 0.25)
    state0 = big.state.clone()
    with pytest.raises(nat.NativeError) as e:
        big.step_implicit_feedback_tangent(3, 1e-4, np.ones((1, 2 * big.n)), np.zeros((big.n, 2 * big.n)))
    assert e.value.code == nat.CRB_EUNSUPPORTED and "256" in str(e.value) and "crb_step_implicit_feedback_tangent" in str(e.value)
    assert torch.equal(big.state, state0) and big.time == 0.25
    f32 = BeamEnsemble(nitinol_columns(6, "linear"), 2, force_params=force_params(False, False), dtype=torch.float32)
    f32.set_state(1e-3 * np.ones((2, 2 * f32.n)), 0.25)
    state0 = f32.state.clone()
    with pytest.raises(nat.NativeError) as e:
        f32.step_implicit_feedback_tangent(3, 1e-4, np.ones((2, 2 * f32.n)), np.zeros((f32.n, 2 * f32.n)))
    assert e.value.code == nat.CRB_EUNSUPPORTED and "fp64" in str(e.value)
    assert torch.equal(f32.state, state0) and f32.time == 0.25
    mixed = BeamEnsemble([nitinol_columns(6, "nonlinear"), nitinol_columns(9, "nonlinear")], 2, force_params=force_params(True, False))
    assert mixed.mixed_topology
    mixed.zero_state()
    state0 = mixed.state.clone()
    with pytest.raises(nat.NativeError, match="crb_step_implicit_feedback_tangent") as e:
        mixed.step_implicit_feedback_tangent(4, 1e-4, np.zeros((2, 2 * mixed.n)), np.zeros((mixed.n, 2 * mixed.n)), hold=2)
    assert e.value.code == nat.CRB_EUNSUPPORTED and "one free-DOF set" in str(e.value)
    assert torch.equal(mixed.state, state0) and mixed.time == 0.0
    # n_steps = 0: the identity on the seeds, nothing else touched; n_iter out of range: refused
    g = rod("packed_partial")
    lp, ens = g.lp, g.ens
    s = lp.seeds()
    ens.set_state(lp.X, T0)
    state0 = ens.state.clone()
    got, (U, dU) = ens.step_implicit_feedback_tangent(0, lp.h, s["x0"], lp.K, d_gain=s["gain"], return_control=True, **g.loop_kw)
    assert torch.equal(ens.state, state0) and ens.time == T0
    assert torch.equal(got, torch.as_tensor(s["x0"], device=got.device))
    assert tuple(U.shape) == (0, lp.B, lp.n) and tuple(dU.shape) == (lp.D, 0, lp.B, lp.n)
    for kw, word in ((dict(n_iter=0), "n_iter"), (dict(n_iter=17), "n_iter")):
        with pytest.raises(nat.NativeError, match=word):
            ens.step_implicit_feedback_tangent(3, lp.h, s["x0"], lp.K, **kw)
        assert torch.equal(ens.state, state0) and ens.time == T0


@pytest.mark.parametrize("name", ["packed_partial", "two_per_wave_pin"])
def test_hold_longer_than_the_call_is_one_sample_of_the_open_loop_tangent(name):
    g = rod(name)
    lp, ens = g.lp, g.ens
    s = lp.seeds()
    got, (U, dU) = g.tangent(s, hold=lp.steps + 3, return_control=True)
    base = ens.state.clone()
    assert tuple(U.shape) == (1, lp.B, lp.n) and tuple(dU.shape) == (lp.D, 1, lp.B, lp.n)
    kw = dict(n_iter=lp.n_iter, impulse_amp=lp.amps, impulse_duration=lp.duration, impulse_index=lp.idx)
    ens.set_state(lp.X, T0)
    want = ens.step_implicit_tangent(lp.steps, lp.h, s["x0"], held_force=U[0], d_held_force=dU[:, 0], d_impulse_amp=s["amp"], **kw)
    assert torch.equal(got, want) and torch.equal(ens.state, base)
    # u and du in extended precision: the device's sums of 2n products, the subtraction and the additions around them
    ld, eps = np.longdouble, 2.0 ** -53
    e0 = lp.R.astype(ld) - lp.X.astype(ld)
    u_want = lp.U.astype(ld) + e0 @ lp.K.T.astype(ld)
    u_bound = (2 * lp.n + 3) * eps * (np.abs(lp.U) + np.abs(lp.R - lp.X) @ np.abs(lp.K.T) + np.abs(lp.X) @ np.abs(lp.K.T))
    assert np.all(np.abs(np_(U)[0] - u_want) <= u_bound)
    for d in range(lp.D):
        de = s["reference"][d].astype(ld) - s["x0"][d].astype(ld)
        du_want = s["held"][d].astype(ld) + de @ lp.K.T.astype(ld) + e0 @ s["gain"][d].T.astype(ld)
        mag = (np.abs(s["held"][d]) + (np.abs(s["reference"][d]) + np.abs(s["x0"][d])) @ np.abs(lp.K.T)
               + (np.abs(lp.R) + np.abs(lp.X)) @ np.abs(s["gain"][d].T))
        assert np.all(np.abs(np_(dU)[d, 0] - du_want) <= (4 * lp.n + 4) * eps * mag), d
    assert np.any(np_(dU) != 0.0)


def test_full_size_4096_beams_of_256_elements():
    lp = loop("four_waves_full")
    fp = force_params(True, True)
    B, steps, h = 4096, 3, lp.h
    amps = np.linspace(0.1, 0.2, B)
    pick = [0, 2047, 4095]
    rng = np.random.default_rng(12)
    big = BeamEnsemble(lp.cols, B, force_params=fp)
    n = big.n
    assert n == lp.n and big.plan.layout.n_slots == 256
    X = np.zeros((B, 2 * n))
    X[:] = lp.X[0]
    dx0 = np.zeros((B, 2 * n))
    dx0[pick] = 1e-3 * rng.normal(0.0, 1.0, (3, 2 * n))
    R = 0.3 * X
    kw = dict(hold=2, n_iter=2, d_gain=lp.dK[0], impulse_index=lp.idx)
    big.set_state(X, 0.0)
    got = big.step_implicit_feedback_tangent(steps, h, dx0, lp.K, reference=R, impulse_amp=amps, d_impulse_amp=amps, **kw)
    assert torch.isfinite(got).all() and torch.isfinite(big.state).all() and float(got.abs().max()) > 0
    small = BeamEnsemble(lp.cols, 3, force_params=fp)
    small.set_state(X[pick], 0.0)
    want = small.step_implicit_feedback_tangent(steps, h, dx0[pick], lp.K, reference=R[pick], impulse_amp=amps[pick],
                                                d_impulse_amp=amps[pick], **kw)
    assert torch.equal(got[pick], want) and torch.equal(big.unpack_state()[pick], small.unpack_state())
