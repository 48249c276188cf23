"""CPU side of the implicit adjoint's mapping tests (tests/test_implicit_adjoint_mappings.py holds the GPU side and imports the
case table, the inputs and the oracle's differences from here).

One table of rods for both files, one row per thread mapping of crb_implicit_adjoint.h -- 1 slot, packed waves with a partly
filled last group, one wave, two and four waves with and without padding lanes, 256 slots -- with PINNED roots, interior pins,
both values of the axial option, mixed element kinds and graded rods.  Every case runs STEPS steps of OracleBeam.implicit from
a clock T0 != 0, drag and gravity on, under a transverse impulse next to a wave seam (next to the beam's end where there is
none; never on the tip, except on the one-element rod, which has no other node) whose window closes inside a step, and a
seeded transverse held force.  The start state is the oracle's own after WARM steps from rest under that impulse.

This file proves the inputs before any kernel is compared.  For every case, checked beam, direction and DOF block:
  * self = max_r |FD_r(e) - FD_r(e/4)| / max_r |FD_r(e/4)| <= SELF_BAR = 2.5e-7 over the probe entries r of the block, FD the
    oracle's central difference along the direction: with it the GPU file's bound min(max(1e-7, 4 self), 1e-6) never reaches
    its cap from difference noise alone;
  * the largest probe entry of every asserted block is non-zero;
  * the smaller step moves the block's largest probe entry by at least RESOLVED ulps: a response that is linear to the last
    bit gives self = 0 however few bits it has (the u of the one-element linear rod under a held-force direction whose own u
    component was 1 % of the others: 4e-16 moved on 2.8e-7, self 0, the quantisation 1.3e-7).
The layouts the GPU file asserts on its ensembles are asserted here on host-only plans.

What was chosen on the oracle alone, before any kernel was compared, so that these hold:
  * Loads.  Impulses of 5 .. 10 N (AMP_SCALE) and held forces of 0.5 N per node (HELD_SCALE): the axial blocks answer a
    transverse input only through the deflection, and at 0.1 .. 0.2 N and 0.05 N their probe entries sat at the differences'
    rounding (self up to 6e-6).  ``load`` scales both per case: x 2 on the two small rods (the same reason, for unit
    directions), x 0.04 and x 0.003 on the graded rods, whose thin ends deflect far more (at x 1 the taper10 rod of 256
    elements is not finite after the warm start, the allcols rods reach self 9e-6).
  * n_iter = 1 does not hold on the rods with an interior pin (32 elements: not finite within 70 steps; 128: self 1e-2); they
    take 3 and 2, and n_iter = 1 goes to three other rows.
  * The two rods of 256 elements run 30 steps after a warm start of 5: after 30 + 40 steps at h = 1e-3 (the step that keeps all
    8 levels of A) gravity has bent the rod far enough that the two differences of the axial rates' response to a held force
    are 2e-6 apart at best over e = 1e-4 .. 4e-3 (rounding below, curvature above).
  * Steps.  HELD_STEP = 1e-3 sits between rounding (self grows as 1 / e below) and curvature (as e^2 above); ``held_step`` =
    3e-4 where curvature still showed at 1e-3 (the linear rod's drag, the 101-slot and the 256-slot rod).
  * The unit directions of the two small rods: an axial unit direction at the size of the axial block itself (1e-7 of the
    transverse one) moves the bending blocks by less than the oracle's rounding (self 5e-3).  FULL_AXIAL: the axial
    displacements take 0.2 x the scale of the w block, the axial rates 10 x that of the dw/dt block; FULL_STEP = 1.5e-4.
  * ``reseed`` moves a case's seed, as in test_param_gradients_dense_cpu.py: each of the one-element rod's first three seeds put the
    u block of a held-force direction below the first or the third condition (the first drew a direction whose own u
    component was 1 % of the others).

Difference steps: STATE_STEP along state directions (scaled per DOF block by the start state, test_tangent_linear.directions),
HELD_STEP along held-force directions, AMP_STEP relative to the amplitude.  The amplitude's one scalar is taken against the
block-normalised oracle tangent itself (test_derivative_mappings.block_normalised): it carries no cancellation."""
import functools

import numpy as np
import pytest

from tests.helpers import graded_columns, nitinol_columns, oracle_beam
from tests.test_derivative_mappings import block_normalised, clock
from tests.test_tangent_linear import directions, oracle_kw

TAG = "[implicit-adjoint-map]"
T0 = 7e-4                 # every rollout here starts on a clock that is not 0
STEPS, CKPT = 40, 7       # (7 does not divide 40: the last checkpoint segment is partial)
WARM = 30
WINDOW = 12.3             # the impulse window closes inside step 12 of the run: its midpoint is the last one forced
SELF_BAR = 2.5e-7
RESOLVED = 4e7            # the smaller difference step moves a block's largest probe entry by at least this many ulps of it (1 / 2.5e-8)
STATE_STEP, HELD_STEP, AMP_STEP = 2e-5, 1e-3, 2.5e-4
AMP_SCALE, HELD_SCALE = 5.0, 0.5
FULL_AXIAL = (0.2, 10.0)
FULL_STEP = 1.5e-4
SEAM_SLOTS = (63, 64, 127, 128, 191, 192)
BLOCKS = ("u", "w", "phi", "du_dt", "dw_dt", "dphi_dt")


def pinned_root(n):
    return ["PINNED"] + ["NONE"] * (n - 1)


def interior_pin(n, at):
    bcs = ["FIXED"] + ["NONE"] * (n - 1)
    bcs[at] = "PINNED"
    return bcs


def mixed(n):
    return (["linear", "nonlinear"] * n)[:n]


# layout = (n_slots, beams_per_group, threads) of the fp64 plan; imp = the node whose w (u on the linear rod) takes the
# impulse; pins = interior pinned nodes; full = every node is a probe and every unit vector a direction; load, steps, warm,
# held_step, reseed: see the head of the file.
CASES = {
    "one_element": dict(n=1, kind="linear", B=70, h=1e-4, n_iter=2, imp=1, imp_dof="u", layout=(1, 64, 64), held_step=3e-4, reseed=3),
    "packed_partial": dict(n=6, kind="nonlinear", B=13, h=1e-4, n_iter=2, imp=5, layout=(6, 10, 64), full=True, load=2.0),
    "packed_pinned": dict(n=10, kind=mixed(10), bcs=pinned_root(10), B=7, h=2e-4, n_iter=3, imp=9, layout=(11, 5, 64),
                          full=True, load=2.0),
    "two_per_wave_pin": dict(n=32, kind="nonlinear", bcs=interior_pin(32, 16), pins=(16,), B=3, h=2e-4, n_iter=3, imp=31,
                             layout=(32, 2, 64)),
    "one_wave_full": dict(n=63, kind="nonlinear", bcs=pinned_root(63), B=2, h=2e-4, n_iter=2, imp=62, layout=(64, 1, 64)),
    "two_waves_min": dict(n=64, kind="nonlinear", bcs=pinned_root(64), B=2, h=2e-4, n_iter=3, imp=63, layout=(65, 1, 128)),
    "two_waves_padded": dict(n=100, kind="nonlinear", bcs=pinned_root(100), B=3, h=5e-4, n_iter=2, imp=64,
                             layout=(101, 1, 128), held_step=3e-4),
    "two_waves_pin_on_seam": dict(n=128, kind=mixed(128), bcs=interior_pin(128, 64), pins=(64,), B=2, h=2e-4, n_iter=2, imp=65,
                                  layout=(128, 1, 128)),
    "four_waves_min": dict(n=129, kind="nonlinear", B=2, h=5e-4, n_iter=2, imp=64, layout=(129, 1, 256)),
    "four_waves_padded": dict(n=200, kind=mixed(200), B=2, h=5e-4, n_iter=3, imp=128, layout=(200, 1, 256)),
    "four_waves_full": dict(n=256, kind="nonlinear", B=2, h=1e-3, n_iter=2, imp=192, layout=(256, 1, 256), steps=30, warm=5,
                            held_step=3e-4),   # all 8 levels of A
    "corrected_40": dict(n=40, kind="nonlinear", corrected=True, B=2, h=2e-4, n_iter=1, imp=39, layout=(40, 1, 64)),
    "alternating_40": dict(n=40, kind=mixed(40), B=2, h=2e-4, n_iter=1, imp=39, layout=(40, 1, 64)),
    "graded_40_allcols": dict(n=40, kind="nonlinear", family="allcols", B=2, h=2e-4, n_iter=2, imp=39, layout=(40, 1, 64), load=0.04),
    "graded_100_allcols": dict(n=100, kind="nonlinear", family="allcols", B=2, h=2e-4, n_iter=1, imp=65, layout=(100, 1, 128), load=0.04),
    "graded_256_taper10": dict(n=256, kind="nonlinear", family="taper10", B=2, h=2e-4, n_iter=2, imp=193, layout=(256, 1, 256),
                               load=0.003, steps=30, warm=5),
}
for _c in CASES.values():
    for _k, _v in dict(bcs=None, pins=(), family=None, corrected=False, full=False, imp_dof="w", load=1.0, reseed=0, held_step=HELD_STEP, steps=STEPS, warm=WARM).items():
        _c.setdefault(_k, _v)
FULL_CASES = [k for k, c in CASES.items() if c["full"]]
SNAPSHOT_CASES = ("packed_partial", "two_waves_padded", "four_waves_padded")
WINDOW_CASES = ("packed_partial", "two_waves_padded")


def case_columns(c):
    if c["family"]:
        return graded_columns(c["n"], c["kind"], c["family"], bcs=c["bcs"])
    return nitinol_columns(c["n"], c["kind"], bcs=c["bcs"])


def slot_offset(c):
    """the node of slot 0: a FIXED root carries no thread, a PINNED one does"""
    return 0 if (c["bcs"] is not None and c["bcs"][0] == "PINNED") else 1


def probe_nodes(c):
    """the first slot's node (the root itself when it is PINNED) and the one after it, both sides of every wave seam, the last
    valid slot (the tip: the padding lanes follow it), a pin and its neighbours; every node of a ``full`` case"""
    n, off = c["n"], slot_offset(c)
    if c["full"]:
        return tuple(range(off, n + 1))
    nodes = {off, off + 1, n}
    nodes |= {s + off for s in SEAM_SLOTS if s + off <= n}
    for p in c["pins"]:
        nodes |= {p - 1, p, p + 1}
    return tuple(sorted(x for x in nodes if off <= x <= n))


def checked_beams(c):
    """the first and the last beam of a full group and the last beam of the partly filled group; every beam of B <= 3"""
    G, B = c["layout"][1], c["B"]
    return tuple(range(B)) if B <= 3 else tuple(sorted({0, G - 1, B - 1}))


def probe_wave(c):
    """the wave whose nodes carry the second state direction: the one (not the first listed among equals) that holds the
    fewest probes, None for a rod of one wave"""
    off, waves = slot_offset(c), c["layout"][2] // 64
    if waves == 1:
        return None
    count = [sum(1 for x in probe_nodes(c) if (x - off) // 64 == w) for w in range(waves)]
    most = int(np.argmax(count))
    return min((w for w in range(waves) if w != most and w * 64 + off <= c["n"]), key=lambda w: (count[w], -w))


def host_layout(cols, **kw):
    from continuum_robot import _native as nat

    p = nat.Plan(cols, n_beams=5, device=-1, dtype="f64", **kw)
    return (p.n_slots, p.beams_per_group, p.threads)


class _Ones:
    """in place of a random generator: ``directions`` then returns its per-block scales"""

    @staticmethod
    def normal(loc, scale, shape):
        return np.ones(shape)


class Inputs:
    """One beam of a case on the oracle alone: its start state, amplitude, held force, directions, probe entries, and the
    oracle's central differences, cached so that the CPU and the GPU file of one run compute each of them once."""

    def __init__(self, name, b):
        c = self.c = CASES[name]
        self.name, self.b = name, b
        self.cols = case_columns(c)
        self.ob = ob = oracle_beam(self.cols, corrected_axial=c["corrected"], **oracle_kw(True, True))
        self.fi = fi = ob.red2full()
        self.n = n = ob.n
        self.h, self.n_iter = c["h"], c["n_iter"]
        full = 3 * c["imp"] + "uwp".index(c["imp_dof"][0])
        self.idx = int(np.flatnonzero(fi == full)[0])
        if c["n"] > 1:
            assert self.idx != n - 2 and c["imp"] != c["n"]                 # (not the tip)
        self.amp = c["load"] * AMP_SCALE * float(np.linspace(1.0, 2.0, c["B"])[b])
        self.duration = T0 + WINDOW * self.h
        rng = np.random.default_rng(1000 * sum(map(ord, name)) + 10 * c["reseed"] + b)
        node, dof = fi // 3, fi % 3
        self.transverse = (dof == 1) if c["kind"] != "linear" else np.ones(n, bool)
        self.U = np.where(self.transverse, rng.normal(0.0, c["load"] * HELD_SCALE, n), 0.0)
        self.X = ob.implicit(np.zeros(2 * n), self.h, c["warm"], n_iter=self.n_iter, amp=self.amp, duration=10.0 * self.h, idx=self.idx)
        assert np.all(np.isfinite(self.X))
        on_probe = np.isin(node, probe_nodes(c))
        self.probes = np.flatnonzero(np.concatenate([on_probe, on_probe]))   # the reduced entries of the probe nodes, both planes
        self.block_of = np.concatenate([dof, 3 + dof])
        if c["full"]:
            S = directions(self.X[None], _Ones(), 1, fi)[0, 0]       # the per-block scales of ``directions`` alone
            axial = np.flatnonzero(self.block_of % 3 == 0)
            for pl in range(2):
                S[axial[axial // n == pl]] = FULL_AXIAL[pl] * S[pl * n + np.flatnonzero(dof == 1)[0]]
            self.state_dirs = [(f"unit {r}", S[r] * np.eye(2 * n)[r]) for r in range(2 * n)]
        else:
            dense = directions(self.X[None], rng, 3, fi)[:, 0]
            self.state_dirs = [("on the probes", np.where(np.concatenate([on_probe, on_probe]), dense[0], 0.0))]
            w = probe_wave(c)
            if w is not None:
                in_wave = (node - slot_offset(c)) // 64 == w
                self.state_dirs.append((f"on wave {w}", np.where(np.concatenate([in_wave, in_wave]), dense[1], 0.0)))
            elif not np.all(on_probe):
                self.state_dirs.append(("off the probes", np.where(np.concatenate([on_probe, on_probe]), 0.0, dense[1])))
            else:
                self.state_dirs.append(("dense again", dense[1]))
            self.state_dirs.append(("dense", dense[2]))
        dU = rng.normal(0.0, c["load"] * HELD_SCALE, (2, n))
        self.held_dirs = [("on the probes", np.where(self.transverse & on_probe, dU[0], 0.0)),
                          ("dense", np.where(self.transverse, dU[1], 0.0))]
        self._memo, self._fd = {}, {}

    # -- the oracle's map and its central differences
    def run(self, x0=None, amp=None, u=None, steps=None, duration=None):
        steps = self.c["steps"] if steps is None else steps
        return self.ob.implicit(self.X if x0 is None else x0, self.h, steps, n_iter=self.n_iter,
                                amp=self.amp if amp is None else amp, duration=self.duration if duration is None else duration,
                                idx=self.idx, t0=T0, u_held=self.U if u is None else u)

    def perturbed(self, kind, k, e, **kw):
        """the run with the input ``kind`` moved by e along its direction k (memoised: fd_check and fd_scalar ask again)"""
        key = (kind, k, e, tuple(sorted(kw.items())))
        if key not in self._memo:
            if kind == "state":
                out = self.run(x0=self.X + e * self.state_dirs[k][1], **kw)
            elif kind == "held":
                out = self.run(u=self.U + e * self.held_dirs[k][1], **kw)
            else:
                out = self.run(amp=self.amp * (1.0 + e), **kw)
            self._memo[key] = out
        return self._memo[key]

    def step_of(self, kind):
        return dict(state=FULL_STEP if self.c["full"] else STATE_STEP, held=self.c["held_step"], amp=AMP_STEP)[kind]

    def differences(self, kind, k=0, **kw):
        """(FD(e), FD(e / 4)) of the final state [2n] along direction k of ``kind`` (state / held / amp)"""
        key = (kind, k, tuple(sorted(kw.items())))
        if key not in self._fd:
            e = self.step_of(kind)
            self._fd[key] = tuple((self.perturbed(kind, k, s, **kw) - self.perturbed(kind, k, -s, **kw)) / (2 * s) for s in (e, e / 4))
        return self._fd[key]

    def amp_cotangent(self, **kw):
        """the block-normalised amplitude tangent of the oracle: <it, dx(T)/d amp> sums terms of one sign per block"""
        return block_normalised(self.differences("amp", **kw)[1], self.fi)


@functools.lru_cache(maxsize=None)
def inputs(name, b):
    return Inputs(name, b)


def probe_blocks(i, got, fd1, fd4, what, assert_bound=True):
    """fd_check's rule on the probe entries: per DOF block, relative to the block's largest probe entry of FD(e/4),
    err <= min(max(1e-7, 4 self), 1e-6), every probe entry asserted.  ``got`` = the kernel's figures at i.probes (None: the
    inputs alone are examined).  Prints one line per block; returns {block: (err, allowed, self)}."""
    out = {}
    for blk in range(6):
        sel = i.probes[i.block_of[i.probes] == blk]
        if sel.size == 0:
            continue
        top = float(np.max(np.abs(fd4[sel])))
        assert top > 0.0, (what, BLOCKS[blk], "the block's probe entries are all zero")
        self_err = float(np.max(np.abs(fd1[sel] - fd4[sel])) / top)
        allowed = min(max(1e-7, 4.0 * self_err), 1e-6)
        err = None
        if got is not None:
            pos = np.flatnonzero(i.block_of[i.probes] == blk)
            err = float(np.max(np.abs(np.asarray(got)[pos] - fd4[sel])) / top)
            print(f"{TAG} {i.name} beam {i.b} | {what} | {BLOCKS[blk]} | err {err:.2e} | allowed {allowed:.2e} | self {self_err:.2e}")
            if assert_bound:
                assert err <= allowed, (i.name, i.b, what, BLOCKS[blk], err, allowed, self_err)
        out[BLOCKS[blk]] = (err, allowed, self_err)
    return out


def scalar_figures(g, L, e):
    """fd_scalar's figures (err, allowed, self) for the gradient g of the scalar L(e)"""
    fd1 = (L(e) - L(-e)) / (2 * e)
    fd4 = (L(e / 4) - L(-e / 4)) / (e / 2)
    self_err = abs(fd1 - fd4) / abs(fd4)
    return (None if g is None else abs(g - fd4) / abs(fd4)), min(max(1e-7, 4 * self_err), 1e-6), self_err


# ---- 1. the layouts the GPU cases assert, on host plans; the probes sit where the table says
@pytest.mark.parametrize("name", list(CASES))
def test_case_layouts_on_host_plans(name):
    c = CASES[name]
    assert host_layout(case_columns(c), corrected_axial=c["corrected"]) == c["layout"], name
    off, S = slot_offset(c), c["layout"][0]
    assert S == c["n"] + 1 - off
    nodes = probe_nodes(c)
    for s in SEAM_SLOTS:
        assert (s + off in nodes) == (s < S), (name, s)
    assert off in nodes and c["n"] in nodes and (c["n"] == 1 or off + 1 in nodes)
    for p in c["pins"]:
        assert {p - 1, p + 1} <= set(nodes)
    if c["layout"][2] > 64:   # the impulse sits next to a wave seam
        assert (c["imp"] - off) % 64 in (0, 63), name
    assert STEPS % CKPT != 0 and T0 != 0.0
    i = inputs(name, 0)
    assert clock(T0, i.h, 12) + 0.5 * i.h > i.duration > clock(T0, i.h, 11) + 0.5 * i.h    # 12 midpoints forced, inside the run


def test_both_values_of_the_axial_option_are_in_the_table():
    assert CASES["corrected_40"]["corrected"] and CASES["corrected_40"]["kind"] == "nonlinear"
    assert not CASES["alternating_40"]["corrected"] and set(CASES["alternating_40"]["kind"]) == {"linear", "nonlinear"}
    assert sorted({c["n_iter"] for c in CASES.values()}) == [1, 2, 3]
    assert all(1e-4 <= c["h"] <= 1e-3 for c in CASES.values())


# ---- 2. the oracle's own differences: self-agreement on the probe entries, every asserted block non-zero
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_differences_agree_on_the_probe_entries(name):
    c = CASES[name]
    worst, least = 0.0, np.inf
    for b in checked_beams(c):
        i = inputs(name, b)
        if c["full"]:
            assert len(i.state_dirs) == 2 * i.n and i.probes.size == 2 * i.n
        else:
            assert len(i.state_dirs) >= 3
        for kind, dirs in (("state", i.state_dirs), ("held", i.held_dirs)):
            for k, (label, v) in enumerate(dirs):
                assert np.max(np.abs(v)) > 0.0, (name, kind, label)
                fd1, fd4 = i.differences(kind, k)
                figs = probe_blocks(i, None, fd1, fd4, f"{kind} {label}")
                for blk, (_, _, s) in figs.items():
                    assert s <= SELF_BAR, (name, b, kind, label, blk, s)
                    worst = max(worst, s)
                # what the smaller step moves is resolved by fp64: the two differences of a (nearly) linear response agree
                # to the last bit however few bits the moved amount has, so ``self`` cannot show this
                hi, lo = i.perturbed(kind, k, i.step_of(kind) / 4), i.perturbed(kind, k, -i.step_of(kind) / 4)
                for blk in range(6):
                    sel = i.probes[i.block_of[i.probes] == blk]
                    if sel.size:
                        moved, size = np.max(np.abs(hi[sel] - lo[sel])), np.max(np.abs(hi[sel]))
                        least = min(least, moved / size)
                        assert moved >= RESOLVED * np.finfo(np.float64).eps * size, (name, b, kind, label, BLOCKS[blk], moved / size)
        lam = i.amp_cotangent()
        _, _, s = scalar_figures(None, lambda e: float(lam @ i.perturbed("amp", 0, e)), AMP_STEP)
        assert s <= SELF_BAR, (name, b, "amplitude", s)
        worst = max(worst, s)
    print(f"{TAG} {name} | oracle differences | worst self {worst:.2e} | least moved {least:.1e} of its block")


# ---- 3. losses over whole-state snapshots (record="all") and over a recorded rate component
SNAP_EVERY = 17           # samples after steps 17 and 34 of 40 (17 does not divide 40)
RATE_CASE, RATE_NODE = "two_waves_padded", 30    # dw/dt of a node of wave 0; the impulse acts in wave 1


class SnapshotLoss:
    """L = <lam, x(T)> + sum_j <C_j, x(t_j)> of one beam on the oracle: seeded cotangents on every free entry of the final state
    and of every snapshot, each scaled per DOF block by the state it weighs (``directions``); with ``rate_node`` the C_j weigh
    dw/dt of that node alone.  The oracle reruns from the start for every sample time: the iteration's starting iterate is
    carried from step to step.  One dense direction per input."""

    def __init__(self, name, b, rate_node=None):
        i = self.i = inputs(name, b)
        n, fi = i.n, i.fi
        rng = np.random.default_rng(77000 + 100 * sum(map(ord, name)) + b + (5000 if rate_node is not None else 0))
        self.times = [SNAP_EVERY * (j + 1) for j in range(i.c["steps"] // SNAP_EVERY)]
        assert i.c["steps"] % SNAP_EVERY != 0 and len(self.times) >= 2
        base = self.outputs()
        self.lam = directions(base[0][None], rng, 1, fi)[0, 0]
        if rate_node is None:
            self.rec_idx = None
            self.C = np.stack([directions(s[None], rng, 1, fi)[0, 0] for s in base[1:]])
        else:
            self.rec_idx = n + int(np.flatnonzero(fi == 3 * rate_node + 1)[0])
            weight = np.sum(np.abs(self.lam * base[0])) / len(self.times)      # the samples weigh about what the final state does
            self.c = rng.normal(0.0, 1.0, len(self.times)) * weight / np.abs(base[1:, self.rec_idx])
            self.C = np.zeros((len(self.times), 2 * n))
            self.C[:, self.rec_idx] = self.c
        self.dX = directions(i.X[None], rng, 1, fi)[0, 0]
        self.dU = np.where(i.transverse, rng.normal(0.0, i.c["load"] * HELD_SCALE, n), 0.0)
        self._memo = {}

    def outputs(self, **kw):
        """[1 + n_samples, 2n]: x(T), then the snapshots"""
        return np.stack([self.i.run(**kw)] + [self.i.run(steps=t, **kw) for t in self.times])

    def loss(self, kind, e):
        if (kind, e) not in self._memo:
            i = self.i
            kw = dict(state=dict(x0=i.X + e * self.dX), held=dict(u=i.U + e * self.dU), amp=dict(amp=i.amp * (1.0 + e)))[kind]
            out = self.outputs(**kw)
            self._memo[(kind, e)] = float(self.lam @ out[0] + np.sum(self.C * out[1:]))
        return self._memo[(kind, e)]

    def gradient_along(self, kind, xb, ab, fb):
        """the kernel's figure for d loss / d e along this beam's direction of ``kind``"""
        return float(dict(state=lambda: xb @ self.dX, held=lambda: fb @ self.dU, amp=lambda: ab * self.i.amp)[kind]())


@functools.lru_cache(maxsize=None)
def snapshot_loss(name, b, rate_node=None):
    return SnapshotLoss(name, b, rate_node)


@pytest.mark.parametrize("name,rate_node", [(k, None) for k in SNAPSHOT_CASES] + [(RATE_CASE, RATE_NODE)])
def test_snapshot_loss_differences_agree(name, rate_node):
    c = CASES[name]
    if rate_node is not None:
        assert (rate_node - slot_offset(c)) // 64 != (c["imp"] - slot_offset(c)) // 64     # another wave than the impulse's
    for b in checked_beams(c):
        s = snapshot_loss(name, b, rate_node)
        for kind in ("state", "held", "amp"):
            _, _, self_err = scalar_figures(None, lambda e: s.loss(kind, e), s.i.step_of(kind) if kind != "state" else STATE_STEP)
            print(f"{TAG} {name} beam {b} | snapshot loss{' (rate)' if rate_node is not None else ''} {kind} | self {self_err:.2e}")
            assert self_err <= SELF_BAR, (name, b, kind, self_err)


# ---- 4. the impulse window against the midpoint clock: the clocks are built as the kernel and the oracle build them
K_EDGE = 21
WINDOW_CKPT = {"first_of_segment": 21, "last_of_segment": 11}     # step 21 opens the segment 21 .. 39 / closes the segment 11 .. 21
EDGES = {
    "on_the_midpoint": lambda h, steps: clock(T0, h, K_EDGE) + 0.5 * h,                       # step K off (tm < duration fails)
    "one_ulp_past_the_midpoint": lambda h, steps: np.nextafter(clock(T0, h, K_EDGE) + 0.5 * h, np.inf),   # step K on
    "on_the_first_midpoint": lambda h, steps: T0 + 0.5 * h,                                   # off throughout
    "beyond_the_end": lambda h, steps: clock(T0, h, steps) + 3.0 * h,                         # on throughout
}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("name", WINDOW_CASES)
def test_window_edge_inputs(name, edge):
    c = CASES[name]
    assert 0 < K_EDGE < c["steps"] - 1
    assert K_EDGE % WINDOW_CKPT["first_of_segment"] == 0 and (K_EDGE + 1) % WINDOW_CKPT["last_of_segment"] == 0
    assert all(c["steps"] % ce != 0 for ce in WINDOW_CKPT.values())
    for b in checked_beams(c):
        i = inputs(name, b)
        dur = float(EDGES[edge](i.h, c["steps"]))
        if edge == "on_the_first_midpoint":     # the oracle is bitwise blind to the amplitude
            assert np.array_equal(i.perturbed("amp", 0, AMP_STEP, duration=dur), i.perturbed("amp", 0, -AMP_STEP, duration=dur))
            continue
        lam = i.amp_cotangent(duration=dur)
        _, _, self_err = scalar_figures(None, lambda e: float(lam @ i.perturbed("amp", 0, e, duration=dur)), AMP_STEP)
        assert self_err <= SELF_BAR, (name, b, edge, self_err)
    i = inputs(name, 0)
    # the two durations around the midpoint of step K differ by that step's forcing: the oracle tells them apart
    on = i.run(duration=float(EDGES["one_ulp_past_the_midpoint"](i.h, c["steps"])))
    off = i.run(duration=float(EDGES["on_the_midpoint"](i.h, c["steps"])))
    assert np.max(np.abs(on - off)) > 1e-4 * np.max(np.abs(on))
