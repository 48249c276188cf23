"""Tangent and adjoint rollouts (crb_tangent.h, crb_adjoint.h) on every thread mapping they accept -- 1 slot, packed waves
with a partial last group, one wave, two and four waves with and without padding lanes, 256 slots -- and on the input edges
the rollout kernels own: the impulse window closing inside a step and before the start, a clock that does not start at 0,
impulses on interior nodes, on phi and on u, recorded samples of phi, u and rates, whole-state snapshots, heterogeneous
ensembles whose members run different mappings, and the refusal beyond 256 thread-carried nodes.

References: central differences of the C oracle (rk4_impulse / rk4_held) under the fd_check rule of test_tangent_linear.py,
the dot-product identity between step_tangent and step_adjoint (recorded samples included), step() for the values, and each
beam alone for heterogeneous ensembles."""
import numpy as np
import pytest
import torch

from continuum_robot import _native as nat
from continuum_robot.batched import BeamEnsemble
from tests.helpers import assert_blocks, nitinol_columns, oracle_beam
from tests.test_adjoint import dot_check, fd_scalar
from tests.test_tangent_linear import directions, fd_check, force_params, oracle_kw, rollout_state

pytestmark = pytest.mark.gpu

DT = 2e-5
T0 = 7e-4   # every rollout here starts on a clock that is not 0


def pinned_root(n):
    return ["PINNED"] + ["NONE"] * (n - 1)


def interior_pin(n, at):
    bcs = ["FIXED"] + ["NONE"] * (n - 1)
    bcs[at] = "PINNED"
    return bcs


def mixed(n):
    return ["linear", "nonlinear"] * (n // 2)


# One table for the file.  layout = (n_slots, beams_per_group, threads, pcr_levels) of the plan; imp / rec = (node, param) of
# the impulse and of the recorded DOF (rec: never the tip where there is another node, and in another wave than the impulse
# on multi-wave beams).  Nonlinear beams get transverse impulses and held loads only (axial ones excite the shipped element's
# runaway axial modes); axial impulses go on linear beams.  record_every never divides steps.
CASES = {
    "one_element": dict(n=1, kind="linear", bcs=None, drag=True, grav=False, B=70, steps=160, every=45,
                        imp=(1, "u"), rec=(1, "dw_dt"), layout=(1, 64, 64, 0)),           # 64 per wave, 0 levels, 2nd group of 6
    "packed_partial": dict(n=6, kind="nonlinear", bcs=None, drag=True, grav=True, B=13, steps=160, every=45,
                           imp=(6, "w"), rec=(3, "phi"), layout=(6, 10, 64, 3)),          # 10 per wave, last group of 3
    "packed_pinned": dict(n=10, kind="linear", bcs=pinned_root(10), drag=False, grav=True, B=7, steps=160, every=45,
                          imp=(10, "u"), rec=(4, "u"), layout=(11, 5, 64, 4)),            # band-breaking gravity
    "two_per_wave_max": dict(n=32, kind="nonlinear", bcs=interior_pin(32, 16), drag=True, grav=True, B=3, steps=160,
                             every=45, imp=(32, "w"), rec=(8, "dphi_dt"), layout=(32, 2, 64, 5)),   # G = 2 at full width
    "one_wave_min": dict(n=33, kind="linear", bcs=None, drag=True, grav=True, B=2, steps=160, every=45,
                         imp=(20, "w"), rec=(5, "phi"), layout=(33, 1, 64, 5)),           # G = 1, 31 idle lanes
    "one_wave_full": dict(n=63, kind="nonlinear", bcs=pinned_root(63), drag=True, grav=True, B=2, steps=100, every=30,
                          imp=(63, "w"), rec=(10, "w"), layout=(64, 1, 64, 5)),           # 64 slots, one wave exactly
    "two_waves_min": dict(n=64, kind="linear", bcs=pinned_root(64), drag=True, grav=True, B=2, steps=100, every=30,
                          imp=(64, "u"), rec=(20, "u"), layout=(65, 1, 128, 5)),          # 65 slots: 2 waves
    "two_waves_padded": dict(n=100, kind="nonlinear", bcs=pinned_root(100), drag=True, grav=True, B=3, steps=100,
                             every=30, imp=(100, "w"), rec=(30, "phi"), layout=(101, 1, 128, 5)),   # 101 of 128
    "two_waves_full": dict(n=128, kind=mixed(128), bcs=interior_pin(128, 64), drag=True, grav=False, B=2, steps=100,
                           every=30, imp=(128, "w"), rec=(40, "dw_dt"), layout=(128, 1, 128, 5)),   # 128 of 128
    "four_waves_min": dict(n=129, kind="nonlinear", bcs=None, drag=True, grav=True, B=2, steps=60, every=25,
                           imp=(129, "w"), rec=(70, "phi"), layout=(129, 1, 256, 5)),     # 129 of 256
    "four_waves_padded": dict(n=200, kind=mixed(200), bcs=None, drag=True, grav=True, B=2, steps=60, every=25,
                              imp=(200, "w"), rec=(60, "dphi_dt"), layout=(200, 1, 256, 5)),   # 200 of 256
    "four_waves_max_pinned": dict(n=255, kind="linear", bcs=pinned_root(255), drag=True, grav=True, B=2, steps=60,
                                  every=25, imp=(255, "u"), rec=(100, "u"), layout=(256, 1, 256, 5)),   # 256 of 256, PINNED
}


class Case:
    """A case of the table set up: the ensemble (its mapping asserted), the oracle, the start state (a short rollout from rest
    under the tip impulse), the inputs and their directions"""

    def __init__(self, name, seed=0):
        c = CASES[name]
        self.name, self.c = name, c
        self.cols = nitinol_columns(c["n"], c["kind"], bcs=c["bcs"])
        self.fp = force_params(c["drag"], c["grav"])
        self.B, self.steps, self.every = c["B"], c["steps"], c["every"]
        self.ens = ens = BeamEnsemble(self.cols, self.B, force_params=self.fp)
        lay = ens.plan.layout
        assert (lay.n_slots, lay.beams_per_group, lay.threads, lay.pcr_levels) == c["layout"], name
        self.ob = oracle_beam(self.cols, **oracle_kw(c["drag"], c["grav"]))
        self.n, self.fi = ens.n, ens.free_index
        self.rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
        self.X = rollout_state(ens)
        self.idx = ens.reduced_index(*c["imp"])
        node, param = c["rec"]
        vel = param.startswith("d") and param.endswith("_dt")
        self.rec_i = ens.reduced_index(node, param[1:-3] if vel else param) + (self.n if vel else 0)
        self.amps = np.linspace(1.0, 2.0, self.B)
        self.duration = T0 + (self.steps // 2 + 0.3) * DT        # the window closes inside a step, halfway through
        # held loads: every DOF of a linear beam, the transverse ones of the others
        w = np.ones((1, self.n), bool) if c["kind"] == "linear" else (self.fi % 3 == 1)[None]
        self.U = np.where(w, self.rng.normal(0.0, 0.05, (self.B, self.n)), 0.0)
        # state directions scaled per block by the start state; on linear beams by the start plus the end (an axial impulse
        # fills the u block of a beam that starts with u = 0: scaled by the start alone, it would sit at the FD noise)
        scale = self.X
        if c["kind"] == "linear":
            xT = self.ob.rk4_impulse(self.X[0], DT, self.steps, self.amps[0], self.duration, self.idx, T0)
            scale = np.abs(self.X) + np.abs(xT)[None]
        self.dX = directions(scale, self.rng, 1, self.fi)[0]
        self.damp = self.rng.normal(0.0, 1.0, self.B)
        self.dU = np.where(w, self.rng.normal(0.0, 0.05, (self.B, self.n)), 0.0)

    @property
    def tol(self):
        """the rollout identity's: 1e-10 with drag or gravity, 1e-12 for linear beams with neither"""
        c = self.c
        return 1e-12 if (c["kind"] == "linear" and not c["drag"] and not c["grav"]) else 1e-10

    @property
    def nonlinear_gravity(self):
        return self.c["grav"] and (self.c["kind"] != "linear")

    def inputs(self, **over):
        kw = dict(impulse_amp=self.amps, impulse_duration=self.duration, impulse_index=self.idx, held_force=self.U)
        kw.update(over)
        return kw

    def tangent(self, m, dX=None, **over):
        """step_tangent of m steps from (X, T0) along (dX, damp, dU), all inputs on"""
        self.ens.set_state(self.X, T0)
        return np_(self.ens.step_tangent(m, DT, self.dX if dX is None else dX, d_impulse_amp=self.damp, d_held_force=self.dU,
                                         t0=T0, **self.inputs(**over)))

    def beams(self):
        return sorted({0, self.B // 2, self.B - 1})


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def clock(t0, dt, k):
    """the clock after k steps: t0 plus dt, added k times in fp64 (clock_after in crbeam.hip, the kernels' stage times)"""
    t = t0
    for _ in range(k):
        t = t + dt
    return t


def free_mask(ens):
    """[B, 2, n_node, 4] bool: the device-layout entries that hold a free DOF"""
    m = np.zeros((ens.n_beams, 2, ens.n_node, 4), dtype=bool)
    for b in range(ens.n_beams):
        fi = ens.free_index_per_beam[b]
        for pl in range(2):
            m[b, pl, fi // 3, fi % 3] = True
    return m


def to_device_layout(ens, x_red):
    """reduced [B, 2n] -> [B, 2, n_node, 4], built here (not by pack_state): zero off the free entries"""
    out = np.zeros((ens.n_beams, 2, ens.n_node, 4))
    for b in range(ens.n_beams):
        fi = ens.free_index_per_beam[b]
        nb = fi.size
        out[b, 0, fi // 3, fi % 3] = x_red[b, :nb]
        out[b, 1, fi // 3, fi % 3] = x_red[b, ens.n:ens.n + nb]
    return out


def block_normalised(v, fi):
    """v [2n] with every DOF block (plane x u / w / phi) divided by its largest entry (blocks of zeros stay zero)"""
    out = np.array(v, dtype=np.float64)
    n = fi.size
    dof = fi % 3
    for pl in range(2):
        for k in range(3):
            sel = pl * n + np.nonzero(dof == k)[0]
            m = np.max(np.abs(out[sel])) if sel.size else 0.0
            if m > 0.0:
                out[sel] /= m
    return out


# ---- a. the tangent rollout against central differences of the oracle: state, amplitude, held force
@pytest.mark.parametrize("name", list(CASES))
def test_tangent_rollout_matches_oracle_differences(name):
    k = Case(name, 1)
    ens, ob, X, steps = k.ens, k.ob, k.X, k.steps
    zero = np.zeros_like(k.dX)
    # (5 .. 10 N: the u rates that the impulse drives on the PINNED-root rods under gravity grow as amps^2, and below ~5 N they
    #  sit at the rounding noise of the central differences next to the pendulum's own u -- FD error 1.6e-6 at 1 N)
    amps = 5.0 * k.amps
    # one launch: direction 0 along the state, direction 1 along the amplitude (window closing halfway, clock from T0)
    ens.set_state(X, T0)
    dT = np_(ens.step_tangent(steps, DT, np.stack([k.dX, zero]), impulse_amp=amps, impulse_duration=k.duration,
                              impulse_index=k.idx, d_impulse_amp=np.stack([np.zeros(k.B), np.ones(k.B)]), t0=T0))
    assert ens.time == clock(T0, DT, steps)
    for b in k.beams():
        def F_x(e):
            return ob.rk4_impulse(X[b] + e * k.dX[b], DT, steps, amps[b], k.duration, k.idx, T0)

        def F_a(e):
            return ob.rk4_impulse(X[b], DT, steps, amps[b] * (1 + e), k.duration, k.idx, T0)

        fd_check(dT[0, b], F_x, 1e-5, k.fi, f"{name} state beam {b}")
        fd_check(amps[b] * dT[1, b], F_a, 1e-3, k.fi, f"{name} amplitude beam {b}")
    # one launch: direction 0 along the state, direction 1 along a held force (transverse on nonlinear beams; x 10 for the
    # same reason as the amplitude: FD error 1.4e-6 in the PINNED-root rods' u rates at the table's 0.05 N)
    U, dU = 10.0 * k.U, 10.0 * k.dU
    ens.set_state(X, T0)
    dT = np_(ens.step_tangent(steps, DT, np.stack([k.dX, zero]), held_force=U,
                              d_held_force=np.stack([np.zeros_like(dU), dU]), t0=T0))
    for b in k.beams():
        def G_x(e):
            return ob.rk4_held(X[b] + e * k.dX[b], DT, steps, U[b])

        def G_u(e):
            return ob.rk4_held(X[b], DT, steps, U[b] + e * dU[b])

        fd_check(dT[0, b], G_x, 1e-5, k.fi, f"{name} state (held) beam {b}")
        fd_check(dT[1, b], G_u, 1e-3, k.fi, f"{name} held force beam {b}")


# ---- b. the rollout identity with recorded samples:
#   sum_k c_k <e_rec, dx(t_k)> + <lam, dx(T)> = <xbar0, dx0> + abar da + <fbar, df>,   t_k = T0 + (k + 1) every dt
def recorded_identity(k, lam, dT, dS, c, xb, ab, fb, what):
    for b in range(k.B):
        dot_check([(lam[b], dT[b]), (c[b], dS[b])], [(xb[b], k.dX[b]), (ab[b], k.damp[b]), (fb[b], k.dU[b])], k.tol,
                  f"{what} beam {b}")


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_identity_with_recorded_samples(name):
    k = Case(name, 2)
    n_s = k.steps // k.every
    assert k.steps % k.every != 0 and n_s >= 2
    dT = k.tangent(k.steps)
    dS = np.stack([k.tangent((j + 1) * k.every)[:, k.rec_i] for j in range(n_s)], axis=1)      # [B, n_s]
    assert np.all(np.max(np.abs(dS), axis=1) > 0.0), name
    lam = directions(dT, k.rng, 1, k.fi)[0]
    # sample cotangents sized so that the samples weigh about what the final state does in the identity
    final = np.sum(np.abs(lam * dT), axis=1)
    c = k.rng.normal(0.0, 1.0, (k.B, n_s)) * (final / (n_s * np.max(np.abs(dS), axis=1)))[:, None]
    xb, ab, fb = k.ens.step_adjoint(k.steps, DT, lam, x0_red=k.X, t0=T0, record=k.c["rec"], record_every=k.every,
                                    lam_record=c, **k.inputs())
    recorded_identity(k, lam, dT, dS, c, np_(xb), np_(ab), np_(fb), name)


# ---- b'. whole-state snapshot cotangents (record="all"): the free entries count, the padding component and the constrained
# DOFs do not (the sweep masks what it reads: crb_adjoint.h, the cotangent of the sample taken at the end of a step)
@pytest.mark.parametrize("name", ["packed_partial", "two_waves_padded", "four_waves_padded"])
def test_snapshot_cotangents(name):
    k = Case(name, 3)
    ens = k.ens
    n_s = k.steps // k.every
    dT = k.tangent(k.steps)
    dS = np.stack([k.tangent((j + 1) * k.every) for j in range(n_s)])                           # [n_s, B, 2n]
    lam = directions(dT, k.rng, 1, k.fi)[0]
    C_red = np.stack([directions(dS[j], k.rng, 1, k.fi)[0] for j in range(n_s)])
    C = np.stack([to_device_layout(ens, C_red[j]) for j in range(n_s)])                        # [n_s, B, 2, n_node, 4]
    run = lambda cot: ens.step_adjoint(k.steps, DT, lam, x0_red=k.X, t0=T0, record="all", record_every=k.every,  # noqa: E731
                                       lam_record=cot, **k.inputs())
    xb, ab, fb = run(C)
    for b in range(k.B):
        dot_check([(lam[b], dT[b])] + [(C_red[j, b], dS[j, b]) for j in range(n_s)],
                  [(np_(xb)[b], k.dX[b]), (np_(ab)[b], k.damp[b]), (np_(fb)[b], k.dU[b])], k.tol, f"{name} beam {b}")
    # junk on the 4th component and on every constrained DOF (node 0 of a FIXED root, a PINNED root's w and u): no effect
    junk = np.where(free_mask(ens)[None], 0.0, k.rng.normal(0.0, 1.0, C.shape) * np.max(np.abs(C)))
    assert np.count_nonzero(junk) > 0
    for r, g in zip((xb, ab, fb), run(C + junk)):
        assert torch.equal(r, g)
    # rollout(record="all") under loss.backward() is step_adjoint, bitwise
    x0 = torch.tensor(k.X, dtype=torch.float64, device=ens.device, requires_grad=True)
    amp = torch.tensor(k.amps, dtype=torch.float64, device=ens.device, requires_grad=True)
    held = torch.tensor(k.U, dtype=torch.float64, device=ens.device, requires_grad=True)
    xT, samples = ens.rollout(x0, k.steps, DT, impulse_amp=amp, held_force=held, impulse_duration=k.duration,
                              impulse_index=k.idx, t0=T0, record="all", record_every=k.every)
    assert tuple(samples.shape) == (n_s, k.B, 2, ens.n_node, 4)
    lam_t = torch.tensor(lam, dtype=torch.float64, device=ens.device)
    C_t = torch.tensor(C, dtype=torch.float64, device=ens.device)
    ((xT * lam_t).sum() + (samples * C_t).sum()).backward()
    assert torch.equal(x0.grad, xb) and torch.equal(amp.grad, ab) and torch.equal(held.grad, fb)


# ---- c. the values: step_tangent's base state and clock, rollout's x(T), against step()
@pytest.mark.parametrize("name", list(CASES))
def test_forward_values_match_step(name):
    k = Case(name, 4)
    # (the lean stepper that step() runs for canonical gravity rounds differently from the general one, and the shipped
    #  element's axial blocks amplify that -- test_tangent_linear.py::test_base_state_and_clock_match_step: such cases are held
    #  to 2 x 60 steps)
    m = min(k.steps, 60) if k.nonlinear_gravity else k.steps
    ref = BeamEnsemble(k.cols, k.B, force_params=k.fp)
    k.ens.set_state(k.X, T0)
    ref.set_state(k.X, T0)
    for _ in range(2):   # (the clock carries over between calls)
        k.ens.step_tangent(m, DT, np.stack([k.dX, -k.dX]), d_impulse_amp=k.damp, d_held_force=k.dU, **k.inputs())
        ref.step(m, DT, **k.inputs())
        assert k.ens.time == ref.time
    want = ref.unpack_state().cpu().numpy()
    assert ref.time == clock(T0, DT, 2 * m)
    assert_blocks(k.ens.unpack_state().cpu().numpy(), want, k.fi, 1e-12, what=f"{name} tangent base")
    state0, time0 = k.ens.state.clone(), k.ens.time
    xT = np_(k.ens.rollout(k.X, 2 * m, DT, t0=T0, **k.inputs()))
    assert torch.equal(k.ens.state, state0) and k.ens.time == time0
    assert_blocks(xT, want, k.fi, 1e-12, what=f"{name} rollout")


# ---- d. bitwise independence of the checkpoint interval and of batching the cotangents
@pytest.mark.parametrize("name", ["two_waves_padded", "four_waves_padded"])
def test_adjoint_bitwise_independent_of_checkpoints_and_batching(name):
    k = Case(name, 5)
    D, n_s = 3, k.steps // k.every
    lam = directions(k.X, k.rng, D, k.fi)
    c = k.rng.normal(0.0, 1.0, (D, k.B, n_s))
    run = lambda lm, cr, ce: k.ens.step_adjoint(k.steps, DT, lm, x0_red=k.X, t0=T0, record=k.c["rec"],  # noqa: E731
                                                record_every=k.every, lam_record=cr, checkpoint_every=ce, **k.inputs())
    assert k.steps % 7 != 0
    ref = run(lam, c, 1)
    for ce in (7, k.steps, None):
        for r, g in zip(ref, run(lam, c, ce)):
            assert torch.equal(r, g), ce
    for d in range(D):
        for r, g in zip(ref, run(lam[d], c[d], 7)):
            assert torch.equal(r[d], g), d


# ---- 3. the impulse window against the clock: durations on and between the stage times of step K, from T0 != 0
K_EDGE = 37
EDGES = {
    "quarter": lambda t_end: clock(T0, DT, K_EDGE) + 0.25 * DT,       # stage 1 of step K on, 2-4 off
    "three_quarters": lambda t_end: clock(T0, DT, K_EDGE) + 0.75 * DT,  # stages 1-3 on, 4 off
    "exact": lambda t_end: clock(T0, DT, K_EDGE),                     # stage 4 of step K - 1 and all of step K off
    "before_start": lambda t_end: 0.5 * T0,                           # off throughout
    "beyond_end": lambda t_end: t_end + 3 * DT,                       # on throughout
}
WINDOW_CASES = {"packed_partial/tip_phi": ("packed_partial", (6, "phi")),
                "two_waves_padded/wave0_w": ("two_waves_padded", (30, "w"))}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("where", list(WINDOW_CASES))
def test_impulse_window_edges(where, edge):
    name, imp = WINDOW_CASES[where]
    k = Case(name, 6)
    ens, ob, X, steps = k.ens, k.ob, k.X, k.steps
    assert K_EDGE < steps
    idx = -1 if imp == (k.c["n"], "phi") else ens.reduced_index(*imp)
    if idx == -1:
        assert ens.reduced_index(*imp) == k.n - 1
    t_end = clock(T0, DT, steps)
    dur = EDGES[edge](t_end)
    closed = dur <= T0
    kw = dict(impulse_amp=k.amps, impulse_duration=dur, impulse_index=idx)
    ens.set_state(X, T0)
    dT = np_(ens.step_tangent(steps, DT, np.zeros_like(X), d_impulse_amp=np.ones(k.B), t0=T0, **kw))
    lam = np.empty_like(X)
    for b in k.beams():
        def F(e):
            return ob.rk4_impulse(X[b], DT, steps, k.amps[b] * (1 + e), dur, idx, T0)

        if closed:
            assert np.all(F(1e-3) == F(-1e-3))   # (the oracle does not see the amplitude either)
            continue
        fd_check(k.amps[b] * dT[b], F, 1e-3, k.fi, f"{where} {edge} amplitude tangent beam {b}")
    for b in range(k.B):   # L = <lam, x(T)> with lam the tangent's own shape: dL/da without cancellation
        lam[b] = block_normalised(dT[b], k.fi) if not closed else directions(X, k.rng, 1, k.fi)[0, b]
    _, ab, _ = ens.step_adjoint(steps, DT, lam, x0_red=X, t0=T0, **kw)
    if closed:
        assert float(np.max(np.abs(dT))) == 0.0 and float(ab.abs().max()) == 0.0
    else:
        for b in k.beams():
            def L(e):
                return float(lam[b] @ ob.rk4_impulse(X[b], DT, steps, k.amps[b] * (1 + e), dur, idx, T0))

            fd_scalar(float(np_(ab)[b]) * k.amps[b], L, 1e-3, f"{where} {edge} amp_bar beam {b}")
    amp = torch.tensor(k.amps, dtype=torch.float64, device=ens.device, requires_grad=True)
    xT = ens.rollout(X, steps, DT, impulse_amp=amp, impulse_duration=dur, impulse_index=idx, t0=T0)
    (xT * torch.tensor(lam, dtype=torch.float64, device=ens.device)).sum().backward()
    assert torch.equal(amp.grad, ab)


# ---- 4. a heterogeneous ensemble whose members run three mappings: packed, two waves (PINNED root), four waves (mixed)
def test_heterogeneous_ensemble_across_mappings():
    sets = [nitinol_columns(6, "nonlinear"), nitinol_columns(100, "nonlinear", bcs=pinned_root(100)),
            nitinol_columns(200, mixed(200))]
    fps = [force_params(True, True), force_params(True, True), force_params(True, False)]
    ens = BeamEnsemble(sets, 3, force_params=fps)
    assert ens.mixed_topology
    singles = [BeamEnsemble(s, 1, force_params=f) for s, f in zip(sets, fps)]
    assert [int(s.plan.threads) for s in singles] == [64, 128, 256]
    assert [int(s.plan.beams_per_group) for s in singles] == [10, 1, 1]
    rng = np.random.default_rng(77)
    steps, dur = 60, T0 + 25.4 * DT
    states = [rollout_state(s)[0] for s in singles]
    dirs = [directions(x[None], rng, 1, s.free_index)[0, 0] for x, s in zip(states, singles)]
    trans = [(s.free_index % 3 == 1) for s in singles]
    helds = [np.where(t, rng.normal(0.0, 0.05, t.size), 0.0) for t in trans]
    dhelds = [np.where(t, rng.normal(0.0, 0.05, t.size), 0.0) for t in trans]
    amps, damp = np.array([0.1, 0.2, 0.3]), rng.normal(0.0, 1.0, 3)

    def pad_force(vs):
        out = np.zeros((3, ens.n))
        for b, v in enumerate(vs):
            out[b, :v.size] = v
        return out

    X, dX, H, dH = ens.pad_states(states), ens.pad_states(dirs), pad_force(helds), pad_force(dhelds)
    kw = dict(impulse_duration=dur, t0=T0)
    ens.set_state(X, T0)
    got = np_(ens.step_tangent(steps, DT, dX, impulse_amp=amps, held_force=H, d_impulse_amp=damp, d_held_force=dH, **kw))
    wants, lams = [], []
    for b, s in enumerate(singles):
        s.set_state(states[b][None], T0)
        want = np_(s.step_tangent(steps, DT, dirs[b][None], impulse_amp=amps[b:b + 1], held_force=helds[b][None],
                                  d_impulse_amp=damp[b:b + 1], d_held_force=dhelds[b][None], **kw))[0]
        nb = int(ens.n_per_beam[b])
        assert_blocks(ens.beam_state(b, got), want, s.free_index, 1e-13, what=f"hetero tangent beam {b}")
        assert np.all(got[b, nb:ens.n] == 0.0) and np.all(got[b, ens.n + nb:] == 0.0)
        wants.append(want)
        lams.append(directions(want[None], rng, 1, s.free_index)[0, 0])
    xb, ab, fb = ens.step_adjoint(steps, DT, ens.pad_states(lams), x0_red=X, impulse_amp=amps, held_force=H, **kw)
    xb, ab, fb = np_(xb), np_(ab), np_(fb)
    for b, s in enumerate(singles):
        wx, wa, wf = s.step_adjoint(steps, DT, lams[b][None], x0_red=states[b][None], impulse_amp=amps[b:b + 1],
                                    held_force=helds[b][None], **kw)
        wx, wa, wf = np_(wx)[0], np_(wa)[0], np_(wf)[0]
        nb = int(ens.n_per_beam[b])
        np.testing.assert_allclose(ens.beam_state(b, xb), wx, rtol=0, atol=1e-13 * np.max(np.abs(wx)))
        np.testing.assert_allclose(fb[b, :nb], wf, rtol=0, atol=1e-13 * np.max(np.abs(wf)))
        np.testing.assert_allclose(ab[b], wa, rtol=1e-13)
        assert np.all(xb[b, nb:ens.n] == 0.0) and np.all(xb[b, ens.n + nb:] == 0.0) and np.all(fb[b, nb:] == 0.0)
        # the identity against the forward kernel, beam by beam
        dot_check([(lams[b], wants[b])], [(ens.beam_state(b, xb), dirs[b]), (ab[b], damp[b]), (fb[b, :nb], dhelds[b])],
                  1e-10, f"hetero identity beam {b}")


# ---- 5. 257 slots (256 elements, PINNED root): refused by every derivative entry point, the ensemble left alone
def test_refused_beyond_256_thread_carried_nodes():
    cols = nitinol_columns(256, "linear", bcs=pinned_root(256))
    B = 2
    ens = BeamEnsemble(cols, B)
    assert (ens.plan.n_slots, ens.plan.threads) == (257, 512)
    rng = np.random.default_rng(5)
    ens.set_state(rng.normal(0.0, 1e-3, (B, 2 * ens.n)), 3e-4)
    state0, time0 = ens.state.clone(), ens.time
    v = rng.normal(0.0, 1.0, (B, 2 * ens.n))
    amps = np.array([0.1, 0.2])
    calls = {
        "rhs_jvp": lambda: ens.rhs_jvp(v),
        "step_tangent": lambda: ens.step_tangent(5, DT, v, impulse_amp=amps, t0=1e-3),
        "rhs_vjp": lambda: ens.rhs_vjp(v),
        "step_adjoint": lambda: ens.step_adjoint(5, DT, v, impulse_amp=amps, t0=1e-3),
        "rollout": lambda: ens.rollout(np_(ens.unpack_state()), 5, DT, impulse_amp=amps, t0=1e-3),
    }
    for what, call in calls.items():
        with pytest.raises(nat.NativeError, match="more than 256 thread-carried nodes") as err:
            call()
        assert err.value.code == nat.CRB_EUNSUPPORTED, what
        assert torch.equal(ens.state, state0) and ens.time == time0, what
