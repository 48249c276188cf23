"""Adjoint of the closed-loop RK4 rollout on the GPU (BeamEnsemble.rollout_feedback / step_feedback_adjoint;
crb_step_rk4_feedback_checkpoint / _adjoint, csrc/crb_feedback_adjoint.h).

  1. forward: x(T) is bitwise step_feedback's stage-split path, 1e-12 per block from whichever path step_feedback picks, and the
     recorded samples are bitwise the chain of shorter calls;
  2. the backward sweep against the same sweep composed on the host from ens.rhs (stage states), ens.rhs_vjp and torch.matmul
     for the two matrix products -- this checks the new kernels and the orchestration, not the existing ones -- per block at
     1e-10, the project's figure for rollout identities with drag and gravity;
  3. gain and reference gradients against central differences of the C oracle's closed loop (fd_scalar's rule, h = 1e-2);
  4. autograd: gradcheck over (x0, gain, reference), and loss.backward() bitwise step_feedback_adjoint;
  5. bitwise independence of the checkpoint interval, of cotangent batching and of repetition;
  6. side effects, isolation of a non-finite cotangent, want_gain=False, refusals that need a device plan;
  7. one full-size shape, 2048 x 128 elements.

Common inputs (the issue's): nitinol_columns rods, closed_loop_gain / seeded_gain of tests/test_graded_beams_cpu.py, DT = 2e-5,
the start state 40 steps of the tip impulse at amp 0.2, references N(0, 1e-3).  An unscaled PD gain gives NaN within 10 steps."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from tests.helpers import BLOCK_FLOOR, assert_blocks, block_errs, nitinol_columns, oracle_beam
from tests.test_graded_beams_cpu import closed_loop_gain, seeded_gain
from tests.test_tangent_linear import directions, force_params, oracle_kw

pytestmark = pytest.mark.gpu

DT = 2e-5
TOL = 1e-10   # rollout identities with drag and gravity


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def start_state(ens, steps=40, amp=0.2):
    ens.zero_state()
    ens.step(steps, DT, impulse_amp=np.full(ens.n_beams, amp) * (1.0 + 0.1 * np.arange(ens.n_beams) / ens.n_beams))
    x = ens.unpack_state().cpu().numpy()
    ens.zero_state()
    return x


class Case:
    """an ensemble, its oracle beam, a stabilising dense gain, references, a start state and cotangents"""

    def __init__(self, n_elem, B, D=1, kind="nonlinear", drag=True, grav=True, bcs=None, seed=0, with_ref=True):
        self.cols = nitinol_columns(n_elem, kind, bcs=bcs)
        self.ens = BeamEnsemble(self.cols, B, force_params=force_params(drag, grav))
        self.ob = oracle_beam(self.cols, **oracle_kw(drag, grav))
        rng = np.random.default_rng(100 + seed)
        self.rng = rng
        n = self.ens.n
        assert self.ob.n == n
        self.K = closed_loop_gain(self.ob, rng)
        self.R = rng.normal(0.0, 1e-3, (B, 2 * n)) if with_ref else None
        self.X0 = start_state(self.ens)
        # cotangents scaled per block of the start state, so that every block is exercised at its own size
        self.lam = directions(self.X0, rng, D, self.ens.free_index)
        self.amps = 0.1 * (1.0 + np.arange(B) / B)


def gain_block_errs(got, ref, fi):
    """per block (row DOF kind x column DOF kind and plane) of a [n, 2n] gain gradient: max |got - ref| over the block relative
    to the block's largest reference magnitude (floored at BLOCK_FLOOR x the matrix's largest, as helpers.block_errs floors
    a block at its plane's)"""
    got, ref = np.asarray(got), np.asarray(ref)
    n = fi.size
    rk, ck = fi % 3, np.concatenate([fi % 3, 3 + fi % 3])
    top = max(np.max(np.abs(ref)), 1e-300)
    out = {}
    for a in range(3):
        for b in range(6):
            blk = np.ix_(rk == a, ck == b)
            if ref[blk].size == 0:
                continue
            with np.errstate(invalid="ignore"):
                e = np.max(np.abs(got[blk] - ref[blk])) / max(np.max(np.abs(ref[blk])), BLOCK_FLOOR * top)
            out[(a, b)] = float(e) if np.isfinite(e) else float("inf")
    assert n * 2 == ref.shape[1]
    return out


def compare(got, want, fi, tol, what):
    """(xbar0, gain_bar, ref_bar) [D, ...] against the host-composed ones, per block; prints the worst figures before asserting"""
    worst = {}
    for d in range(np_(want[0]).shape[0]):
        ex = block_errs(np_(got[0])[d], np_(want[0])[d], fi)
        er = block_errs(np_(got[2])[d], np_(want[2])[d], fi)
        eg = gain_block_errs(np_(got[1])[d], np_(want[1])[d], fi) if got[1] is not None else {}
        for name, e in (("xbar0", ex), ("ref_bar", er), ("gain_bar", eg)):
            if e:
                worst[name] = max(worst.get(name, 0.0), max(e.values()))
    print(f"[feedback adjoint] {what}: worst block errors " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= tol, (what, k, v, tol)
    return worst


def host_sweep(ens, X0, K, R, steps, lam, amps=None, held=None, duration=0.01, rec=None, t0=0.0):
    """The closed-loop rollout and its transposed sweep composed on the host: stage states from ens.rhs, (xbar, ubar) from
    ens.rhs_vjp, the two matrix products by torch.matmul.  rec = (reduced state index, every, lam_rec [D, B, n_rec]).
    Returns x(T) and (xbar0 [D, B, 2n], gain_bar [D, n, 2n], ref_bar [D, B, 2n])."""
    dev, f8 = ens.device, torch.float64
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=f8, device=dev)   # noqa: E731
    n, B = ens.n, ens.n_beams
    K, x = T(K), T(X0)
    R = torch.zeros((B, 2 * n), dtype=f8, device=dev) if R is None else T(R)
    imp = n - 2   # impulse_index -2: the tip's w
    dt, t = DT, t0
    stages = []
    for _ in range(steps):
        ts = (t, t + 0.5 * dt, t + 0.5 * dt, t + dt)
        Xs, ks, xs = [], [], x
        for s in range(4):
            u = (R - xs) @ K.T
            if held is not None:
                u = u + T(held)
            if amps is not None and ts[s] < duration:
                u = u.clone()
                u[:, imp] += T(amps)
            k = ens.rhs(xs, u)
            Xs.append(xs)
            ks.append(k)
            if s < 3:
                xs = x + (dt if s == 2 else 0.5 * dt) * k
        x = x + (dt / 6.0) * (ks[0] + 2.0 * ks[1] + 2.0 * ks[2] + ks[3])
        stages.append(Xs)
        t = t + dt
    lam = T(lam).clone()
    D = lam.shape[0]
    gain_bar = torch.zeros((D, n, 2 * n), dtype=f8, device=dev)
    ref_bar = torch.zeros((D, B, 2 * n), dtype=f8, device=dev)
    ca = (None, dt / 6.0, dt / 3.0, dt / 3.0)
    cb = (None, 0.5 * dt, 0.5 * dt, dt)
    for k in range(steps - 1, -1, -1):
        if rec is not None and (k + 1) % rec[1] == 0 and (k + 1) // rec[1] <= steps // rec[1]:
            lam[:, :, rec[0]] += T(rec[2])[:, :, (k + 1) // rec[1] - 1]
        seed = (dt / 6.0) * lam
        total = torch.zeros_like(lam)
        for s in (3, 2, 1, 0):
            xb, ub = ens.rhs_vjp(seed, stages[k][s])
            P = ub @ K
            si = xb - P
            ref_bar += P
            gain_bar += torch.einsum("dbi,bj->dij", ub, R - stages[k][s])
            total = total + si
            if s > 0:
                seed = ca[s] * lam + cb[s] * si
        lam = lam + total
    return x, (lam, gain_bar, ref_bar)


# ---------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("n_elem,B,steps", [(6, 5, 40), (40, 3, 10)])
def test_forward_is_the_stage_split_closed_loop(n_elem, B, steps, monkeypatch):
    c = Case(n_elem, B)
    ens = c.ens
    xT = ens.rollout_feedback(c.X0, steps, DT, c.K, c.R, impulse_amp=c.amps)
    assert ens.time == 0.0 and torch.count_nonzero(ens.state) == 0          # (state and time are left alone)
    # whichever path step_feedback picks: to rounding
    ens.set_state(c.X0)
    ens.step_feedback(steps, DT, c.K, c.R, impulse_amp=c.amps)
    errs = assert_blocks(np_(ens.unpack_state()), np_(xT), ens.free_index, 1e-12, what=("forward", ens.feedback_path()))
    print(f"[feedback adjoint] forward {n_elem} x {B} x {steps} vs step_feedback ({ens.feedback_path()}): {max(errs.values()):.2e}")
    # forced to the stage-split launches: bitwise
    monkeypatch.setenv("CRB_FUSED_FEEDBACK", "0")
    monkeypatch.setenv("CRB_LOOP", "0")
    assert ens.feedback_path() == "stage-split"
    ens.set_state(c.X0)
    ens.step_feedback(steps, DT, c.K, c.R, impulse_amp=c.amps)
    assert torch.equal(ens.unpack_state(), xT)
    ens.set_state(c.X0)
    ens.step_feedback(steps, DT, c.K, None)
    assert torch.equal(ens.unpack_state(), ens.rollout_feedback(c.X0, steps, DT, c.K))


def test_recorded_samples_are_the_chain_of_shorter_calls():
    c = Case(6, 3)
    ens = c.ens
    steps, every = 20, 5
    tip = ens.n - 2
    for rec, idx in (((ens.n_elem, "w"), tip), ((ens.n_elem, "dphi_dt"), ens.n + ens.n - 1)):
        xT, samples = ens.rollout_feedback(c.X0, steps, DT, c.K, c.R, impulse_amp=c.amps, record=rec, record_every=every,
                                           checkpoint_every=7)
        assert tuple(samples.shape) == (3, steps // every)
        x, t = torch.as_tensor(c.X0, device=ens.device), 0.0
        for k in range(steps // every):
            x = ens.rollout_feedback(x, every, DT, c.K, c.R, impulse_amp=c.amps, t0=t)
            for _ in range(every):
                t = t + DT
            assert torch.equal(samples[:, k], x[:, idx]), (rec, k)
        assert torch.equal(x, xT)


# ---------------------------------------------------------------- 2. against the host-composed transpose
SHAPES = [   # (n_elem, B, steps, D)
    (5, 1, 3, 1),      # n = 15, odd
    (6, 3, 10, 2),     # n = 18: MFMA k-tail in the transposed product, 6 rows
    (6, 17, 3, 1),     # beam-reduction tail in the gain gradient
    (6, 33, 2, 1),     # beam-reduction tail past one K step
    (11, 5, 3, 1),     # n = 33: ragged 2 x 3 output tiles
    (100, 3, 2, 1),    # two-wave beams, 10 x 19 tiles
]


@pytest.mark.parametrize("n_elem,B,steps,D", SHAPES)
def test_sweep_matches_the_host_composed_transpose(n_elem, B, steps, D):
    c = Case(n_elem, B, D)
    ens = c.ens
    xT_host, want = host_sweep(ens, c.X0, c.K, c.R, steps, c.lam, amps=c.amps)
    xT = ens.rollout_feedback(c.X0, steps, DT, c.K, c.R, impulse_amp=c.amps)
    assert_blocks(np_(xT), np_(xT_host), ens.free_index, 1e-12, what="x(T)")
    got = ens.step_feedback_adjoint(steps, DT, c.lam if D > 1 else c.lam[0], c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, t0=0.0)
    if D == 1:
        got = tuple(g[None] for g in got)
    compare(got, want, ens.free_index, TOL, f"{n_elem} x {B} x {steps} x {D}")


VARIANTS = {
    "pinned_root": dict(n_elem=6, bcs=["PINNED"] + ["NONE"] * 5),
    # node_offset = 0 and other offset tables (on two pins the rod's rates reach 9 within the 40 start steps, linear or not:
    # the oracle's closed loop stays finite, 20 at most)
    "interior_pin": dict(n_elem=6, bcs=["PINNED", "NONE", "NONE", "PINNED", "NONE", "NONE"]),
    "interior_clamp": dict(n_elem=6, bcs=["PINNED", "NONE", "NONE", "FIXED", "NONE", "NONE"]),
    "linear": dict(n_elem=6, kind="linear"),
    "mixed_elements": dict(n_elem=7, kind=["linear", "nonlinear"] * 3 + ["linear"]),
    "no_drag_no_gravity": dict(n_elem=6, drag=False, grav=False),
    "drag_only": dict(n_elem=6, drag=True, grav=False),
    "gravity_only": dict(n_elem=6, drag=False, grav=True),
    "no_reference": dict(n_elem=6, with_ref=False),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_sweep_variants_match_the_host_composed_transpose(name):
    c = Case(B=3, D=2, **VARIANTS[name])
    ens = c.ens
    if name in ("interior_pin", "interior_clamp"):
        assert ens.plan.node_offset == 0
    steps = 5
    _, want = host_sweep(ens, c.X0, c.K, c.R, steps, c.lam, amps=c.amps)
    got = ens.step_feedback_adjoint(steps, DT, c.lam, c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, t0=0.0, checkpoint_every=2)
    compare(got, want, ens.free_index, TOL, name)


def test_record_cotangents_and_held_force_match_the_host_composed_transpose():
    c = Case(6, 3, D=2)
    ens = c.ens
    steps, every = 9, 2
    n = ens.n
    held = c.rng.normal(0.0, 0.02, (3, n)) * (ens.free_index % 3 == 1)[None]
    for rec, idx in (((ens.n_elem, "w"), n - 2), ((3, "phi"), ens.reduced_index(3, "phi"))):
        lam_rec = c.rng.normal(0.0, 1.0, (2, 3, steps // every)) * np.max(np.abs(c.lam))
        xT_host, want = host_sweep(ens, c.X0, c.K, c.R, steps, c.lam, amps=c.amps, held=held, rec=(idx, every, lam_rec))
        xT = ens.rollout_feedback(c.X0, steps, DT, c.K, c.R, impulse_amp=c.amps, held_force=held)
        assert_blocks(np_(xT), np_(xT_host), ens.free_index, 1e-12, what="x(T) with a held force")
        got = ens.step_feedback_adjoint(steps, DT, c.lam, c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, held_force=held, t0=0.0,
                                        record=rec, record_every=every, lam_record=lam_rec, checkpoint_every=4)
        compare(got, want, ens.free_index, TOL, f"record {rec}")


# ---------------------------------------------------------------- 3. against central differences of the C oracle
def fd_scalar(g, L, h, what):
    fd1 = (L(h) - L(-h)) / (2 * h)
    fd4 = (L(h / 4) - L(-h / 4)) / (h / 2)
    allowed = min(max(1e-7, 4 * abs(fd1 - fd4) / abs(fd4)), 1e-6)
    err = abs(g - fd4) / abs(fd4)
    print(f"[feedback adjoint] {what}: adjoint {g:.12e}, oracle differences {fd4:.12e}, err {err:.2e}, allowed {allowed:.2e}")
    assert err <= allowed, (what, g, fd4, err, allowed)


@pytest.mark.parametrize("n_elem,steps", [(4, 10), (6, 40), (20, 40)])
def test_gain_and_reference_gradients_match_oracle_differences(n_elem, steps):
    B = 2
    c = Case(n_elem, B, seed=3)
    ens, ob = c.ens, c.ob
    lam = c.lam[0]
    dK = seeded_gain(ob, c.rng)
    dR = c.rng.normal(0.0, 1e-3, (B, 2 * ens.n))
    _, gb, rb = ens.step_feedback_adjoint(steps, DT, lam, c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, t0=0.0)

    def loss(K, R):
        return sum(float(lam[b] @ ob.rk4_feedback(c.X0[b], DT, steps, K, R[b], amp=float(c.amps[b]))) for b in range(B))

    fd_scalar(float(np.sum(np_(gb) * dK)), lambda e: loss(c.K + e * dK, c.R), 1e-2, f"gain, {n_elem} x {steps}")
    fd_scalar(float(np.sum(np_(rb) * dR)), lambda e: loss(c.K, c.R + e * dR), 1e-2, f"reference, {n_elem} x {steps}")


# ---------------------------------------------------------------- 4. autograd
def test_gradcheck_over_state_gain_and_reference():
    c = Case(4, 2)
    ens = c.ens
    dev = ens.device
    x0 = torch.tensor(c.X0, dtype=torch.float64, device=dev, requires_grad=True)
    K = torch.tensor(c.K, dtype=torch.float64, device=dev, requires_grad=True)
    R = torch.tensor(c.R, dtype=torch.float64, device=dev, requires_grad=True)
    f = lambda x, k, r: ens.rollout_feedback(x, 10, DT, k, r, impulse_amp=c.amps)   # noqa: E731
    assert torch.autograd.gradcheck(f, (x0, K, R), eps=1e-6, nondet_tol=0.0)


def test_backward_equals_step_feedback_adjoint():
    c = Case(6, 3)
    ens = c.ens
    dev = ens.device
    steps, every = 12, 3
    rec = (ens.n_elem, "w")
    x0 = torch.tensor(c.X0, dtype=torch.float64, device=dev, requires_grad=True)
    K = torch.tensor(c.K, dtype=torch.float64, device=dev, requires_grad=True)
    R = torch.tensor(c.R, dtype=torch.float64, device=dev, requires_grad=True)
    w = torch.tensor([0.5, -1.0, 2.0, 0.25], dtype=torch.float64, device=dev)
    xT, samples = ens.rollout_feedback(x0, steps, DT, K, R, impulse_amp=c.amps, record=rec, record_every=every)
    loss = (samples * w).sum() + 0.5 * (xT * xT).sum()
    loss.backward()
    lam_rec = w[None].expand(3, 4).contiguous()
    xb, gb, rb = ens.step_feedback_adjoint(steps, DT, xT.detach(), c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, t0=0.0, record=rec,
                                           record_every=every, lam_record=lam_rec)
    assert torch.equal(x0.grad, xb) and torch.equal(K.grad, gb) and torch.equal(R.grad, rb)
    # without a reference, and a gain that needs no gradient
    x1 = torch.tensor(c.X0, dtype=torch.float64, device=dev, requires_grad=True)
    ens.rollout_feedback(x1, steps, DT, c.K).sum().backward()
    xb1, _, _ = ens.step_feedback_adjoint(steps, DT, np.ones_like(c.X0), c.K, x0_red=c.X0, t0=0.0)
    assert torch.equal(x1.grad, xb1)


# ---------------------------------------------------------------- 5. bitwise
def test_results_are_bitwise_independent_of_checkpoints_batching_and_repetition():
    c = Case(6, 5, D=2)
    ens = c.ens
    steps = 16
    rec = (ens.n_elem, "w")
    lam_rec = c.rng.normal(0.0, 1.0, (2, 5, steps // 3)) * np.max(np.abs(c.lam))
    run = lambda lam, lr, every: ens.step_feedback_adjoint(steps, DT, lam, c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, t0=0.0,   # noqa: E731
                                                           record=rec, record_every=3, lam_record=lr, checkpoint_every=every)
    base = run(c.lam, lam_rec, None)
    assert all(torch.isfinite(t).all() for t in base)
    for every in (1, 7, steps):
        got = run(c.lam, lam_rec, every)
        for a, b, name in zip(got, base, ("xbar0", "gain_bar", "ref_bar")):
            assert torch.equal(a, b), (every, name)
    again = run(c.lam, lam_rec, None)
    for d in range(2):
        one = run(c.lam[d], lam_rec[d], 7)
        for a, b, e, name in zip(one, base, again, ("xbar0", "gain_bar", "ref_bar")):
            assert torch.equal(a, b[d]), (d, name)
            assert torch.equal(e[d], b[d]), (d, name)


# ---------------------------------------------------------------- 6. side effects, isolation, refusals
def test_state_time_and_status_are_left_alone():
    c = Case(6, 3)
    ens = c.ens
    ens.set_state(c.X0, time=0.125)
    status = ens.status.clone()
    before = ens.state.clone()
    lam = c.lam[0].copy()
    lam[1, 0] = np.inf                 # (a diverging cotangent must not mark a beam either)
    ens.step_feedback_adjoint(8, DT, lam, c.K, c.R, impulse_amp=c.amps)
    ens.rollout_feedback(c.X0, 8, DT, c.K, c.R)
    assert torch.equal(ens.state, before) and ens.time == 0.125 and torch.equal(ens.status, status)
    # the resident state and clock are the defaults of x0_red and t0
    a = ens.step_feedback_adjoint(8, DT, c.lam[0], c.K, c.R, impulse_amp=c.amps, impulse_duration=0.125 + 3.5 * DT)
    b = ens.step_feedback_adjoint(8, DT, c.lam[0], c.K, c.R, x0_red=c.X0, t0=0.125, impulse_amp=c.amps,
                                  impulse_duration=0.125 + 3.5 * DT)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_non_finite_cotangent_stays_in_its_beam_and_want_gain_false_changes_nothing_else():
    c = Case(6, 5)
    ens = c.ens
    steps = 6
    run = lambda lam, **kw: ens.step_feedback_adjoint(steps, DT, lam, c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, t0=0.0, **kw)   # noqa: E731
    xb, gb, rb = run(c.lam[0])
    xb2, gb2, rb2 = run(c.lam[0], want_gain=False)
    assert gb2 is None and torch.equal(xb2, xb) and torch.equal(rb2, rb)
    bad = c.lam[0].copy()
    bad[2, 3] = np.nan
    xn, gn, rn = run(bad)
    keep = [0, 1, 3, 4]
    assert torch.equal(xn[keep], xb[keep]) and torch.equal(rn[keep], rb[keep])
    assert torch.isnan(xn[2]).any() and torch.isnan(rn[2]).any()
    assert torch.isnan(gn).any()       # (documented: the gain gradient is a sum over the beams)


def test_mixed_topology_and_gain_lists_are_refused():
    from continuum_robot import _native as nat

    c = Case(4, 2)
    ens = c.ens
    with pytest.raises(NotImplementedError, match="list of gains"):
        ens.rollout_feedback(c.X0, 2, DT, [c.K, c.K])
    with pytest.raises(NotImplementedError, match="list of gains"):
        ens.step_feedback_adjoint(2, DT, c.lam[0], [c.K, None])
    mixed = BeamEnsemble([nitinol_columns(4, "nonlinear"), nitinol_columns(6, "nonlinear")], 2)
    assert mixed.mixed_topology
    K = np.zeros((mixed.n, 2 * mixed.n))
    with pytest.raises(nat.NativeError, match="free-DOF set") as e:
        mixed.rollout_feedback(np.zeros((2, 2 * mixed.n)), 2, DT, K)
    assert e.value.code == nat.CRB_EUNSUPPORTED
    with pytest.raises(nat.NativeError, match="free-DOF set") as e:
        mixed.step_feedback_adjoint(2, DT, np.zeros((2, 2 * mixed.n)), K)
    assert e.value.code == nat.CRB_EUNSUPPORTED


# ---------------------------------------------------------------- 7. one full-size shape
def test_full_size_ensemble_is_finite_and_matches_the_host_sweep_on_sampled_beams():
    n_elem, B, steps = 128, 2048, 4
    c = Case(n_elem, B)
    ens = c.ens
    got = ens.step_feedback_adjoint(steps, DT, c.lam[0], c.K, c.R, x0_red=c.X0, impulse_amp=c.amps, t0=0.0)
    assert all(torch.isfinite(t).all() for t in got)
    _, want = host_sweep(ens, c.X0, c.K, c.R, steps, c.lam, amps=c.amps)
    pick = [0, 1027, 2047]
    ex = block_errs(np_(got[0])[pick], np_(want[0])[0][pick], ens.free_index)
    er = block_errs(np_(got[2])[pick], np_(want[2])[0][pick], ens.free_index)
    eg = gain_block_errs(np_(got[1]), np_(want[1])[0], ens.free_index)
    print(f"[feedback adjoint] 2048 x 128 x 4: worst block errors xbar0 {max(ex.values()):.2e}, ref_bar {max(er.values()):.2e}, "
          f"gain_bar {max(eg.values()):.2e}")
    assert max(ex.values()) <= TOL and max(er.values()) <= TOL
