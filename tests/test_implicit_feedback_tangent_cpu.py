"""CPU side of the tangent of the sampled-data implicit loop (crb_step_implicit_feedback_tangent,
BeamEnsemble.step_implicit_feedback_tangent / linearize_implicit_feedback; the GPU side is
tests/test_implicit_feedback_tangent.py, which imports the rods, their inputs, the directions and the oracle's differences from
here).

  * the two entry points are declared in include/crbeam.h, exported and bound, and CRB_VERSION stays;
  * every refusal shows on a host-only plan in the documented order and names the entry point and the argument;
  * the work-buffer size follows the header's formula;
  * the Python argument errors need no device;
  * the inputs of the GPU file are proved on the oracle alone.  The CPU statement of the call is OracleBeam.implicit chained
    per sample with u_held = f + K (r - x_k) formed on the host (Loop.chain).  For every rod the chain stays finite and differs
    from the open loop (K = 0) by far more than any bound of the GPU file: the loop is driven by the gain.  On the three rods
    of the finite-difference test the central differences along one direction each of x0, gain, reference, held force and
    amplitude agree between the step e and e / 4 to SELF_BAR = 2.5e-7 on every DOF block of every beam, every block's response
    is non-zero, and the smaller step moves each block's largest entry by at least RESOLVED = 4e7 ulps.

The rods are rows of tests/test_implicit_adjoint_mappings_cpu.CASES (drag and gravity on, the clock starting at T0 = 7e-4, the
oracle's own warm start, a seeded transverse held force): the smallest shapes at which each thread mapping and each tile edge
of the boundary kernel can go wrong.  RODS adds the hold and the iteration count of the closed loop; the impulse window closes
inside step 13, which is no sample's first step under any hold used here.  The gain is tests/test_implicit_feedback_cpu.py's:
dense normal entries plus a velocity-damping diagonal, scaled by gain_scales from the sampled plant's own compliance."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests.helpers import BLOCKS, block_errs, nitinol_columns
from tests.test_derivative_mappings import clock
from tests.test_implicit_adjoint_mappings_cpu import CASES, HELD_SCALE, RESOLVED, SELF_BAR, T0
from tests.test_implicit_adjoint_mappings_cpu import inputs as rod_inputs
from tests.test_implicit_feedback_cpu import gain_scales, sample_response
from tests.test_tangent_linear import directions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "[implicit-feedback-tangent]"
NAMES = ("crb_implicit_feedback_tangent_work_bytes", "crb_step_implicit_feedback_tangent")
WHO = NAMES[1]
WINDOW = 13.3             # the impulse window closes inside step 13 of the run: midpoint 12 is the last one forced

# rod -> hold (1, 4, and 7, which cuts the last sample of 40 steps to 5; 4 cuts that of the 30 steps of the 256-slot rod to 2)
# and n_iter of the closed loop
RODS = {
    "one_element": dict(hold=1, n_iter=1),            # n = 3: far below one MFMA tile; 70 beams: 64 per wave plus a group of 6
    "packed_partial": dict(hold=7, n_iter=2),         # n = 18: a 16 + 2 tile edge; 13 beams: rows no multiple of 16
    "packed_pinned": dict(hold=4, n_iter=3),          # a PINNED root: a root DOF with a reduced index
    "two_per_wave_pin": dict(hold=4, n_iter=3),       # a pin mid-wave: n = 96 - 1
    "two_waves_min": dict(hold=4, n_iter=2),          # 65 slots: two waves (a pinned root: at hold = 7 the oracle's chain is not finite)
    "four_waves_min": dict(hold=1, n_iter=2),         # 129 slots
    "four_waves_full": dict(hold=4, n_iter=2),        # 256 slots at h = 1e-3: all eight levels
}
FD_RODS = ("packed_partial", "two_per_wave_pin", "two_waves_min")
FAMILIES = ("x0", "gain", "reference", "held", "amp")
ALONE_RODS = ("packed_partial", "two_waves_min")
# Steps of the central differences per family, relative to the family's direction (the smaller one is a quarter of it), chosen
# on the oracle alone between rounding (self grows as 1 / e below) and curvature (as e^2 above).  The reference and the
# amplitude reach the axial blocks only through the deflection: at the state's step 2e-5 the smaller step moved du/dt of the
# 65-slot rod by 7e4 ulps (self 1.5e-4); they take larger steps, the amplitude a larger one the longer the rod.
FD_STEP = dict(x0=2e-5, gain=1e-3, reference=1.6e-2, held=1e-3, amp=2.5e-4)
FD_STEP_OF = {("two_per_wave_pin", "amp"): 1e-3, ("two_waves_min", "amp"): 4e-3, ("two_waves_min", "held"): 5e-4}


def fd_step(name, family):
    return FD_STEP_OF.get((name, family), FD_STEP[family])


class Loop:
    """One rod on the oracle alone: the start states of all its beams, amplitudes, held forces, a reference, the gain, D seeded
    directions of every input family, and the oracle's chain."""
    D = 3

    def __init__(self, name):
        self.name, self.c = name, CASES[name]
        c, r = self.c, RODS[name]
        self.B, self.h, self.steps, self.hold, self.n_iter = c["B"], c["h"], c["steps"], r["hold"], r["n_iter"]
        per = [rod_inputs(name, b) for b in range(self.B)]
        self.ob, self.n, self.fi, self.idx = per[0].ob, per[0].n, per[0].fi, per[0].idx
        self.cols = per[0].cols
        n, B, D = self.n, self.B, self.D
        self.X = np.stack([i.X for i in per])
        self.amps = np.array([i.amp for i in per])
        self.U = np.stack([i.U for i in per])
        self.transverse = per[0].transverse
        self.duration = T0 + WINDOW * self.h
        self.R = 0.3 * np.roll(self.X, 1, axis=0)               # another beam's state, scaled: nonzero, of the state's size
        rng = np.random.default_rng(9000 + sum(map(ord, name)))
        self.resp = sample_response(self.ob, self.h, self.hold, self.n_iter)
        self.scale, self.damp = gain_scales(self.resp, n)
        self.K = self.scale * rng.normal(0.0, 1.0, (n, 2 * n))
        self.K[np.arange(n), n + np.arange(n)] += self.damp
        self.dX = directions(self.X, rng, D, self.fi)
        self.dK = self.scale * rng.normal(0.0, 1.0, (D, n, 2 * n))
        self.dR = 0.3 * directions(self.X, rng, D, self.fi)
        self.dF = np.where(self.transverse, rng.normal(0.0, c["load"] * HELD_SCALE, (D, B, n)), 0.0)
        self.dA = self.amps * rng.uniform(0.5, 1.5, (D, B))
        self.lam = rng.normal(0.0, 1.0, (D, B, 2 * n)) / directions(self.X, _ones(), 1, self.fi)
        self._memo = {}

    def seeds(self, family=None):
        """the D directions of every family (dx0, d_gain, d_reference, d_held_force, d_impulse_amp); ``family``: the others zero"""
        full = dict(x0=self.dX, gain=self.dK, reference=self.dR, held=self.dF, amp=self.dA)
        return {k: (v if family in (None, k) else np.zeros_like(v)) for k, v in full.items()}

    def chain(self, b, K=None, x0=None, r=None, u=None, amp=None, steps=None, hold=None):
        """OracleBeam.implicit chained per sample on beam b from the clock T0: (final state [2n], controls [samples, n])"""
        K = self.K if K is None else K
        x = (self.X[b] if x0 is None else x0).copy()
        r = self.R[b] if r is None else r
        u = self.U[b] if u is None else u
        amp = self.amps[b] if amp is None else amp
        left, hold = (self.steps if steps is None else steps), (self.hold if hold is None else hold)
        t, held = T0, []
        while left > 0:
            m = min(hold, left)
            uk = u + K @ (r - x)
            held.append(uk)
            x = self.ob.implicit(x, self.h, m, n_iter=self.n_iter, amp=amp, duration=self.duration, idx=self.idx, t0=t, u_held=uk)
            t, left = clock(t, self.h, m), left - m
        return x, np.array(held).reshape(-1, self.n)

    def moved(self, family, e, d=0):
        """[B, 2n]: the chain of every beam with the input ``family`` moved by e along its direction d (memoised)"""
        key = (family, e, d)
        if key not in self._memo:
            out = []
            for b in range(self.B):
                kw = {}
                if family == "x0":
                    kw["x0"] = self.X[b] + e * self.dX[d, b]
                elif family == "gain":
                    kw["K"] = self.K + e * self.dK[d]
                elif family == "reference":
                    kw["r"] = self.R[b] + e * self.dR[d, b]
                elif family == "held":
                    kw["u"] = self.U[b] + e * self.dF[d, b]
                else:
                    kw["amp"] = self.amps[b] + e * self.dA[d, b]
                out.append(self.chain(b, **kw)[0])
            self._memo[key] = np.stack(out)
        return self._memo[key]

    def F(self, family):
        return lambda e: self.moved(family, e)


class _Ones:
    @staticmethod
    def normal(loc, scale, shape):
        return np.ones(shape)


def _ones():
    return _Ones()


@functools.lru_cache(maxsize=None)
def loop(name):
    return Loop(name)


# ------------------------------------------------------------------ the inputs, on the oracle alone
def test_the_window_closes_inside_a_sample_under_every_hold_used():
    for name, r in RODS.items():
        lp_h, steps = CASES[name]["h"], CASES[name]["steps"]
        dur = T0 + WINDOW * lp_h
        on = [clock(T0, lp_h, s) + 0.5 * lp_h < dur for s in range(steps)]
        assert on == [s < 13 for s in range(steps)], name
        assert r["hold"] == 1 or 13 % r["hold"] != 0, name
    assert sorted({r["hold"] for r in RODS.values()}) == [1, 4, 7] and sorted({r["n_iter"] for r in RODS.values()}) == [1, 2, 3]
    assert 40 % 7 != 0 and 30 % 4 != 0 and CASES["four_waves_full"]["steps"] == 30 and CASES["packed_partial"]["steps"] == 40


@pytest.mark.parametrize("name", list(RODS))
def test_oracle_chain_is_finite_and_driven_by_the_gain(name):
    lp = loop(name)
    n = lp.n
    assert lp.K.shape == (n, 2 * n) and np.all(lp.K != 0.0) and lp.resp > 0.0
    assert lp.scale * lp.resp * (np.sqrt(n) + np.sqrt(2 * n)) == pytest.approx(0.2, rel=1e-12)
    assert np.any(lp.R != 0.0) and np.any(lp.U != 0.0) and np.all(np.isfinite(lp.X))
    least = np.inf
    for b in sorted({0, lp.B - 1}):
        xT, held = lp.chain(b)
        assert held.shape == (-(-lp.steps // lp.hold), n) and np.all(np.isfinite(xT)) and np.all(np.isfinite(held))
        open_loop, _ = lp.chain(b, K=np.zeros_like(lp.K))
        drive = max(block_errs(xT, open_loop, lp.fi).values())
        least = min(least, drive)
        assert drive > 1e-4, (name, b, drive)                # (every bound of the GPU file is 1e-6 or below)
        assert np.all(np.any(held != lp.U[b], axis=1))
    print(f"{TAG} {name} | hold {lp.hold} n_iter {lp.n_iter} | closed against open loop, worst block: {least:.2e}")


def fd_figures(lp, family):
    """per DOF block over all beams: (self = |FD(e) - FD(e / 4)| relative to the block, the ulps the smaller step moves the
    block's largest entry by, the block's largest |FD(e / 4)|)"""
    e = fd_step(lp.name, family)
    fd1 = (lp.moved(family, e) - lp.moved(family, -e)) / (2 * e)
    fd4 = (lp.moved(family, e / 4) - lp.moved(family, -e / 4)) / (e / 2)
    self_err = block_errs(fd1, fd4, lp.fi)
    hi, lo = lp.moved(family, e / 4), lp.moved(family, -e / 4)
    dof = np.concatenate([lp.fi % 3, 3 + lp.fi % 3])
    ulps, top = {}, {}
    for blk in range(6):
        sel = dof == blk
        if sel.any():
            moved = np.max(np.abs(hi[:, sel] - lo[:, sel]), axis=1)
            size = np.max(np.abs(hi[:, sel]), axis=1)
            ulps[BLOCKS[blk]] = float(np.min(moved / (np.finfo(np.float64).eps * size)))
            top[BLOCKS[blk]] = float(np.min(np.max(np.abs(fd4[:, sel]), axis=1)))
    return self_err, ulps, top


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", FD_RODS)
def test_oracle_differences_agree_and_are_resolved_on_every_block(name, family):
    lp = loop(name)
    self_err, ulps, top = fd_figures(lp, family)
    print(f"{TAG} {name} {family} | self " + " ".join(f"{k} {v:.1e}" for k, v in self_err.items())
          + " | ulps moved " + " ".join(f"{k} {v:.1e}" for k, v in ulps.items()))
    for blk in self_err:
        assert top[blk] > 0.0, (name, family, blk)
        assert self_err[blk] <= SELF_BAR, (name, family, blk, self_err[blk])
        assert ulps[blk] >= RESOLVED, (name, family, blk, ulps[blk])


# ------------------------------------------------------------------ symbols
def header():
    return open(os.path.join(ROOT, "include", "crbeam.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from continuum_robot import _native as nat
    from continuum_robot.batched import BeamEnsemble

    hdr, lib = header(), nat.load()
    for name, ret in zip(NAMES, ("size_t", "int")):
        assert re.search(rf"\b{ret} {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.crb_implicit_feedback_tangent_work_bytes.restype is C.c_size_t
    assert re.search(r"typedef struct crb_feedback_tangent \{\s*const void\* d_gain;[^}]*const void\* d_ref;[^}]*\} crb_feedback_tangent;", hdr)
    assert [f for f, _ in nat.FeedbackTangent._fields_] == ["d_gain", "d_ref"]
    assert lib.crb_version() == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1)) == 106
    # the implicit tangent's "not covered" note points to the new entry point; the new one lists what it leaves out
    assert "tangents of recorded samples, the closed loop, parameter tangents" not in hdr
    assert "crb_step_implicit_feedback_tangent below" in hdr
    for word in ("in-kernel (one-launch) form", "tangents of recorded samples", "gain groups", "damped variant", "fp32",
                 "parameter tangents", "RK4 closed loop"):
        assert word in hdr[hdr.index("---- Tangent of the sampled-data implicit loop"):], word
    sig = inspect.signature(BeamEnsemble.step_implicit_feedback_tangent).parameters
    assert list(sig)[1:] == ["n_steps", "h", "dx0_red", "gain", "reference", "hold", "n_iter", "d_gain", "d_reference", "impulse_amp",
                             "impulse_duration", "impulse_index", "held_force", "d_impulse_amp", "d_held_force", "t0",
                             "return_control"]
    assert (sig["hold"].default, sig["n_iter"].default, sig["return_control"].default, sig["impulse_index"].default) == (1, 2, False, -2)
    sig = inspect.signature(BeamEnsemble.linearize_implicit_feedback).parameters
    assert list(sig)[1:] == ["h", "gain", "reference", "hold", "n_samples", "n_iter", "x_red", "held_force"]
    assert (sig["hold"].default, sig["n_samples"].default, sig["n_iter"].default) == (1, 1, 2)


# ------------------------------------------------------------------ the work buffer
def test_work_bytes_formula_on_host_only_plans():
    from continuum_robot import _native as nat

    lib = nat.load()
    wb = lib.crb_implicit_feedback_tangent_work_bytes
    for n_elem, nb in ((4, 1), (6, 13), (40, 200)):
        plan = nat.Plan(nitinol_columns(n_elem, "nonlinear"), n_beams=nb, device=-1)
        F = nb * (n_elem + 1) * 4                          # doubles of one [B][n_node][4] record
        for n_dir in (1, 5, 36, 65535):
            assert wb(plan.h, n_dir) == (1 + n_dir) * F * 8, (n_elem, nb, n_dir)
        for bad in (0, -1, 65536):
            assert wb(plan.h, bad) == 0, bad
    assert wb(None, 1) == 0


# ------------------------------------------------------------------ refusals, before the device is touched
P = C.c_void_p
X_, DX, GAIN, REF, WORK, UOUT, DUOUT, DGAIN, DREF, HELD, AMP, DHELD, DAMP = (P(64 * k) for k in range(1, 14))   # never read
H_, STEPS_, HOLD_ = 1e-4, 22, 4


class Calls:
    def __init__(self, dtype, cols=None):
        from continuum_robot import _native as nat

        self.nat, self.lib = nat, nat.load()
        self.plan = nat.Plan(nitinol_columns(4, "nonlinear") if cols is None else cols, n_beams=2, device=-1, dtype=dtype)
        self.t_end = C.c_double(-1.0)

    def tan(self, x=X_, dx=DX, n_dir=3, h=H_, n=STEPS_, n_iter=2, hold=HOLD_, gain=GAIN, ref=REF, d_gain=DGAIN, d_ref=DREF, dfb=True,
            desc=None, d_amp=None, df_held=DHELD, din=True, u_out=UOUT, du_out=DUOUT, work=WORK, plan=True):
        fb, ti = self.nat.FeedbackTangent(), self.nat.InputTangent()
        fb.d_gain, fb.d_ref = getattr(d_gain, "value", None), getattr(d_ref, "value", None)
        ti.d_amp, ti.df_held = getattr(d_amp, "value", None), getattr(df_held, "value", None)
        return self.lib.crb_step_implicit_feedback_tangent(self.plan.h if plan else None, x, dx, n_dir, 0.0, h, n, n_iter, hold, gain,
                                                           ref, C.byref(fb) if dfb else None, desc, C.byref(ti) if din else None,
                                                           u_out, du_out, work, C.byref(self.t_end), None)

    def refused(self, rc, code, *words):
        msg = self.lib.crb_last_error().decode()
        assert rc == code, (rc, code, msg)
        for w in (WHO,) + words:
            assert w in msg, (w, msg)
        assert self.t_end.value == -1.0          # (*t_end is written only by a call that is not refused)


def bad_input(nat):
    d = nat.InputDesc()
    d.kind = 77
    return C.byref(d)


def impulse(nat, held=None):
    d = nat.InputDesc()
    d.kind, d.node, d.dof, d.duration, d.amp = nat.CRB_INPUT_IMPULSE, 4, 1, 1e-3, AMP.value
    d.f_held = getattr(held, "value", None)
    return C.byref(d)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_in_order_before_the_device(dtype):
    c = Calls(dtype)
    nat, inval = c.nat, c.nat.CRB_EINVAL
    last = (nat.CRB_ENODEV, "host-only") if dtype == "f64" else (nat.CRB_EUNSUPPORTED, "fp64")
    # every later fault of the documented order, next to which each earlier one must still be the one reported
    order = [("n_dir", 0, "n_dir"), ("n", -1, "n_steps"), ("n_iter", 17, "n_iter"), ("h", 0.0, "h must"), ("hold", 0, "hold must"),
             ("desc", bad_input(nat), "input kind")]

    def later(i):
        return {k: v for k, v, _ in order[i + 1:]}

    worst = later(-1)
    # 1. CRB_EINVAL: NULL plan and buffers, then aliasing, before every size
    c.refused(c.tan(plan=False, **worst), inval, "null plan")
    for key in ("x", "dx", "gain", "work"):
        c.refused(c.tan(**{**worst, key: None}), inval, "null")
    for kw, word in ((dict(dx=X_), "dx"), (dict(dx=GAIN), "dx"), (dict(dx=REF), "dx"), (dict(dx=DGAIN), "dx"), (dict(dx=DREF), "dx"),
                     (dict(dx=DHELD), "dx"), (dict(u_out=X_), "u_out"), (dict(u_out=GAIN), "u_out"), (dict(du_out=DREF), "du_out"),
                     (dict(du_out=DHELD), "du_out"), (dict(work=X_), "work"), (dict(work=REF), "work"), (dict(work=DGAIN), "work"),
                     (dict(u_out=DX), "dx"), (dict(du_out=DX), "dx"), (dict(work=DX), "dx"), (dict(du_out=UOUT), "u_out"),
                     (dict(work=UOUT), "u_out"), (dict(work=DUOUT), "du_out"),
                     (dict(desc=impulse(nat, held=DX)), "dx"), (dict(desc=impulse(nat), dx=AMP), "dx"),
                     (dict(desc=impulse(nat), d_amp=DAMP, work=DAMP), "work")):
        c.refused(c.tan(**{**worst, **kw}), inval, "alias", word)
    # ... then the sizes and the input, each next to every later one
    for i, (key, value, word) in enumerate(order):
        c.refused(c.tan(**{**later(i), key: value}), inval, word)
    for kw, word in ((dict(n_dir=-1), "n_dir"), (dict(n_dir=65536), "n_dir"), (dict(n_iter=0), "n_iter"), (dict(h=float("nan")), "h must"),
                     (dict(h=-1e-4), "h must"), (dict(hold=-1), "hold must")):
        c.refused(c.tan(**kw), inval, word)
    c.refused(c.tan(d_amp=DAMP), inval, "d_amp", "impulse")                          # no input at all
    c.refused(c.tan(d_amp=DAMP, desc=bad_input(nat)), inval, "input kind")          # (the input comes first)
    # 2. / 3. valid arguments: CRB_EUNSUPPORTED for fp32, else CRB_ENODEV -- also without what is optional
    c.refused(c.tan(), *last)
    c.refused(c.tan(ref=None, u_out=None, du_out=None, dfb=False, din=False), *last)
    c.refused(c.tan(d_gain=None, d_ref=None, df_held=None), *last)
    c.refused(c.tan(d_amp=DAMP, desc=impulse(nat, held=HELD)), *last)
    c.refused(c.tan(n=0), *last)
    c.refused(c.tan(hold=STEPS_ + 1, n_dir=65535, n_iter=16), *last)


def test_unsupported_plans_are_refused_before_the_device():
    from continuum_robot import _native as nat

    big = Calls("f64", nitinol_columns(300, "linear"))
    big.refused(big.tan(), nat.CRB_EUNSUPPORTED, "256")
    big.refused(big.tan(hold=0), nat.CRB_EINVAL, "hold must")               # (CRB_EINVAL comes first)
    big32 = Calls("f32", nitinol_columns(300, "linear"))
    big32.refused(big32.tan(), nat.CRB_EUNSUPPORTED, "fp64")                 # (the dtype is looked at first)
    # (a plan of mixed topology has no host-only form: its refusal is in the GPU file)


# ------------------------------------------------------------------ Python argument errors
def bare_ensemble():
    import torch

    from continuum_robot.batched import BeamEnsemble

    ens = BeamEnsemble.__new__(BeamEnsemble)
    ens.dtype, ens.device, ens.n_beams, ens.n = torch.float64, torch.device("cpu"), 2, 12
    return ens


@pytest.mark.parametrize("kw, error, word", [
    (dict(hold=0), ValueError, "hold must be"),
    (dict(hold=2.5), ValueError, "hold must be"),
    (dict(gain=np.zeros((11, 24))), ValueError, "expected shape"),
    (dict(dx0_red=np.zeros((2, 23))), ValueError, "dx0_red"),
    (dict(dx0_red=np.zeros((3, 2, 24)), d_gain=np.zeros((2, 12, 24))), ValueError, "d_gain must be"),
    (dict(d_gain=np.zeros((12, 23))), ValueError, "d_gain must be"),
    (dict(reference=np.zeros((3, 24))), ValueError, "expected shape"),
    (dict(dx0_red=np.zeros((3, 2, 24)), d_reference=np.zeros((2, 2, 24))), ValueError, "d_reference must have the directions"),
    (dict(d_reference=np.zeros((2, 23))), ValueError, "d_reference"),
])
def test_python_argument_checks_need_no_device(kw, error, word):
    ens = bare_ensemble()
    args = dict(dx0_red=np.zeros((2, 24)), gain=np.zeros((12, 24)))
    args.update(kw)
    with pytest.raises(error, match=word):
        ens.step_implicit_feedback_tangent(STEPS_, H_, **args)


def test_a_list_of_gains_is_refused_with_the_adjoints_message():
    ens = bare_ensemble()
    for gains in ([np.zeros((12, 24))] * 2, (None, np.zeros((12, 24)))):
        with pytest.raises(NotImplementedError, match="list of gains") as e:
            ens.step_implicit_feedback_tangent(STEPS_, H_, np.zeros((2, 24)), gains, hold=0)
        with pytest.raises(NotImplementedError, match="list of gains") as a:
            ens.step_implicit_feedback_adjoint(STEPS_, H_, np.zeros((2, 24)), gains, hold=0)
        assert str(e.value).split(": ", 1)[1] == str(a.value).split(": ", 1)[1]
    for kw, word in ((dict(n_samples=0), "n_samples"), (dict(n_samples=1.5), "n_samples"), (dict(hold=0), "hold must be")):
        with pytest.raises(ValueError, match=word):
            ens.linearize_implicit_feedback(H_, np.zeros((12, 24)), **kw)
