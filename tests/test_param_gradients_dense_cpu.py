"""CPU side of the dense parameter-gradient tests (tests/test_param_gradients_dense.py holds the GPU side and imports the case
table, the loss and the oracle's differences from here).

test_param_gradients.py differentiates the tip of a rod that starts at rest under a tip impulse: within its 20 to 200 steps the
disturbance stays in the last two or three elements, so every slot but those contributes 1e-7 of the asserted sums or less.
Here the loss makes every slot matter:

  x0    the oracle's rk4_held from rest, WARM = 400 steps of DT under a seeded held force on every free w DOF (+-50 N), with
        drag (RHO_F) and gravity (G_Y) on;
  L     = lam . x(T) + sum_k lam_record[k] w_rec(t_k) over STEPS = 60 further steps under the same held force (or, in the
        impulse cases, under a mid-span impulse whose window closes inside the rollout, from a clock T0 > 0): lam seeded
        normal on all 2 n reduced DOFs, each of the six DOF blocks divided by the largest |x0| of that block; a sample of a
        mid-span w every REC_EVERY = 7 steps (the last record interval and the last checkpoint segment are partial), seeded
        lam_record divided by the largest |x0| of the w block.  The oracle continues from sample to sample.  The recorded
        node is n_elem // 2, or the node after it where that one's w is constrained (the interior pins).

The loss is linear in (lam, lam_record), so one perturbed rollout serves every cotangent of a problem.

This file proves the inputs before any kernel is compared.  For every problem of the GPU file and every asserted column:
  * self = max_e |FD_e(h) - FD_e(h/4)| / max_e |FD_e(h/4)| <= 2.5e-7 (a quarter of the 1e-6 ceiling), FD_e the oracle's central
    difference with entry e of the column scaled by 1 +- h (so FD_e = c_e dL/dc_e);
  * every asserted entry has |FD_e| >= 1e-5 max_e |FD_e|, ten times the loosest allowed error: an entry that a kernel dropped
    entirely fails.  The only entries below are the exact zeros of the oracle, named per case (``zeros``): drag_coef[e] where
    the w of node e -- the only node that reads row e -- is constrained (element 0 under a FIXED or PINNED root, the element
    right of an interior pin).  They are asserted to be exact zeros, here of the oracle and in the GPU file of the kernel.

  * amp dL/d amp is one number, with no larger entry of a column to be measured against, so whatever its parts cancel counts in
    full against it: it must keep |sum_i t_i| >= AMP_KEPT = 0.1 of sum_i |t_i|, t_i = W_i amp d out_i / d amp over the 2 n final
    DOFs and the samples (at most one digit lost to the sum).  Of the first five seeds of the 129-element impulse case the
    first keeps 0.42 and 0.016 (beams 0, 1), the second 0.19 and 0.068, the fourth 0.0058 and 0.050 -- and there the
    oracle's own two differences are 7.2e-7 apart; the third seed (reseed=2) is the first that keeps a tenth in both beams.

Two departures from that recipe, both decided on the oracle alone, before any kernel was compared:
  * WARM_NL.  Uncorrected nonlinear ``allcols`` rods do not survive 460 steps on the oracle: under +-50 N (and just as well under
    +-5 N) the axial DOFs of the 40, 64, 100 and 256-element rods grow tenfold every 20 steps from about step 120 and are NaN at
    step 180 to 300, four seeds out of four (the instability of the shipped nonlinear element that helpers.assert_blocks
    describes); the 6 and 20-element rods stay finite but their differences no longer agree (g_x of 6 elements: 4.8e-7 at best
    over h = 1e-3 .. 1e-5).  These rods warm WARM_NL = 60 steps, so the differentiated rollout ends at step 120; the held force
    acts on every w DOF from the first step, so every element still carries its share (the floor below is asserted).  The
    alternating and the corrected 40-element rods and all linear rods warm the full 400 steps.
  * Step sizes.  This loss moves the rod a hundred times further than the tip impulse of test_param_gradients.py, and the
    oracle's two differences at that file's h = 1e-3 are 4e-7 to 2e-6 apart for drag_coef and fluid_density (curvature: a
    quarter of the step gives a sixteenth).  STEP_SIZE here: 1e-4 stiffness and g_x as there, 2.5e-4 drag_coef, 1e-4
    fluid_density, 1e-3 g_y; a direction moves all elements at once and takes a tenth of that; amp 2.5e-4; STEP_SIZE_OF_CASE
    names the cases with a step of their own.  Seeds: ``reseed`` in the table moves a case's seed where the first one put
    an entry below the floor, a column above the bar or the amplitude's derivative below AMP_KEPT.
Measured with these (worst beam, cotangent and case): self <= 1.75e-7 in every column, the smallest asserted entry >= 1.3e-5 of
its column's largest (the tests print every figure, pytest -s)."""
import functools

import numpy as np
import pytest

from tests.helpers import graded_columns, oracle_beam

DT = 2e-5
RHO_F, G_Y = 1000.0, -9.81
WARM, STEPS, REC_EVERY = 400, 60, 7
WARM_NL = 60
N_REC = STEPS // REC_EVERY
T0_IMPULSE = 3e-4
IMPULSE_DURATION = T0_IMPULSE + 23.3 * DT      # 23 whole steps forced, the window closes inside the 24th
STEP_SIZE = {"elastic_modulus": 1e-4, "moment_inertia": 1e-4, "drag_coef": 2.5e-4, "fluid_density": 1e-4, "g_y": 1e-3, "g_x": 1e-4}
# Cases with a step of their own; self = the oracle's two differences apart, at the file's step -> at the case's.  Where
# curvature sets the figure a smaller step divides it; g_x of the undamped rod is rounding, and takes a larger one.
#   the 6-element rod (alone and in the mixed ensemble): stiffness 9.4e-7 and 1.1e-6 at 1e-4; drag_coef 2.2e-7 -> 3.2e-8
#   the PINNED-root 64-slot rod: drag_coef 2.5e-7 -> 7.1e-8
#   the tapered several-wave rods: elastic_modulus 1.5e-7 -> 1.1e-8 (EA_scale 2.2e-7 -> 1.7e-8) at 100 elements
#   the undamped 100-element rod of the mixed ensemble: g_x 1.0e-6 at 1e-4, 4.9e-7 at 2.5e-5
_STEEP = {"elastic_modulus": 2.5e-5, "moment_inertia": 2.5e-5}
_STEEP6 = dict(_STEEP, drag_coef=1e-4)
STEP_SIZE_OF_CASE = {"mixed0": _STEEP6, "all6_allcols_nl": _STEEP6, "mixed1": {"g_x": 1e-3}, "pinned_root64_allcols_nl": {"drag_coef": 1e-4},
                     "waves100_taper10_lin": _STEEP, "waves129_taper10_lin": _STEEP, "waves256_taper10_lin": _STEEP}
DIRECTION_STEP = 0.1       # a direction moves every element at once: its differences take a tenth of STEP_SIZE (no case's own)
AMP_STEP = 2.5e-4
ELEMENT_COLUMNS = ("elastic_modulus", "moment_inertia", "drag_coef")
SCALARS = ("fluid_density", "g_x", "g_y")
SELF_BAR = 2.5e-7
FLOOR = 1e-5
AMP_KEPT = 0.1
SEAMS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193)


def pinned_root(n):
    return ["PINNED"] + ["NONE"] * (n - 1)


def interior_pin(n):
    return ["FIXED"] + ["NONE"] * (n // 2 - 1) + ["PINNED"] + ["NONE"] * (n - n // 2 - 1)


def alternating(n):
    return (["linear", "nonlinear"] * n)[:n]


def selected(n, extra=()):
    """the seam list of the several-wave cases within a rod of n elements, with the rod's last two and ``extra``"""
    return tuple(sorted({e for e in SEAMS + (n - 2, n - 1) + tuple(extra) if 0 <= e < n}))


def around(p):
    """the two elements either side of node p"""
    return (p - 2, p - 1, p, p + 1)


# One table for both files.  layout = (n_slots, beams_per_group, threads) of the fp64 plan; elements = "all" or the list of
# per-element differences; zeros = the named exact zeros of a column; B beams differ in the seed of their held force.
CASES = {
    # 1. per element, all elements
    "all6_allcols_nl": dict(warm=WARM_NL, n=6, family="allcols", kind="nonlinear", B=2, layout=(6, 10, 64)),
    "all20_allcols_nl": dict(reseed=3, warm=WARM_NL, n=20, family="allcols", kind="nonlinear", B=2, layout=(20, 3, 64)),
    "all31_taper10_lin": dict(n=31, family="taper10", kind="linear", B=2, layout=(31, 2, 64)),
    "all33_mesh4_lin": dict(n=33, family="mesh4", kind="linear", B=2, layout=(33, 1, 64)),
    "all40_allcols_nl": dict(warm=WARM_NL, n=40, family="allcols", kind="nonlinear", B=2, layout=(40, 1, 64)),
    "all64_allcols_nl": dict(reseed=20, warm=WARM_NL, n=64, family="allcols", kind="nonlinear", B=2, layout=(64, 1, 64)),
    "all65_mesh4_lin": dict(reseed=2, n=65, family="mesh4", kind="linear", B=2, layout=(65, 1, 128), n_cot=3),
    # 2. several waves: the seam elements, three seeded directions, the scalars
    "waves100_taper10_lin": dict(n=100, family="taper10", kind="linear", layout=(100, 1, 128)),
    "waves100_allcols_nl": dict(warm=WARM_NL, n=100, family="allcols", kind="nonlinear", layout=(100, 1, 128)),
    "waves129_taper10_lin": dict(n=129, family="taper10", kind="linear", layout=(129, 1, 256)),
    "waves200_taper10_lin": dict(reseed=4, n=200, family="taper10", kind="linear", layout=(200, 1, 256)),
    "waves256_taper10_lin": dict(reseed=2, n=256, family="taper10", kind="linear", layout=(256, 1, 256)),
    "waves256_allcols_nl": dict(reseed=1, warm=WARM_NL, n=256, family="allcols", kind="nonlinear", layout=(256, 1, 256)),
    # 3. boundary conditions at 64 and 200 slots (a PINNED root keeps node 0 as a slot)
    "pinned_root64_allcols_nl": dict(warm=WARM_NL, n=63, family="allcols", kind="nonlinear", bcs=pinned_root, layout=(64, 1, 64)),
    "pinned_root200_taper10_lin": dict(n=199, family="taper10", kind="linear", bcs=pinned_root, layout=(200, 1, 256)),
    "interior_pin64_allcols_nl": dict(reseed=1, warm=WARM_NL, n=64, family="allcols", kind="nonlinear", bcs=interior_pin, layout=(64, 1, 64),
                                      extra=around(32), zeros={"drag_coef": (0, 32)}),
    "interior_pin200_taper10_lin": dict(reseed=4, n=200, family="taper10", kind="linear", bcs=interior_pin, layout=(200, 1, 256),
                                        extra=around(100), zeros={"drag_coef": (0, 100)}),
    # 4. element kinds and the axial option
    "alternating40_allcols": dict(n=40, family="allcols", kind=alternating, layout=(40, 1, 64), elements="all"),
    "corrected40_allcols_nl": dict(n=40, family="allcols", kind="nonlinear", corrected=True, layout=(40, 1, 64), elements="all"),
    # 5. an impulse on the w of node 64 (a wave seam) whose window closes inside the rollout; no held force
    "impulse65_mesh4_lin": dict(n=65, family="mesh4", kind="linear", B=2, layout=(65, 1, 128), elements="all",
                                impulse=dict(node=64, amps=(20.0, 35.0))),
    "impulse129_taper10_lin": dict(reseed=2, n=129, family="taper10", kind="linear", B=2, layout=(129, 1, 256),
                                   impulse=dict(node=64, amps=(20.0, 35.0))),
}
for _name, _c in CASES.items():
    _c.setdefault("B", 1)
    _c.setdefault("n_cot", 1)
    _c.setdefault("elements", "all" if _name.startswith("all") else selected(_c["n"], _c.get("extra", ())))
    _c.setdefault("zeros", {"drag_coef": (0,)})
ALL_ELEMENT_CASES = [k for k in CASES if k.startswith("all")]
WAVE_CASES = [k for k in CASES if k.startswith("waves")]
BC_CASES = [k for k in CASES if "pin" in k]
KIND_CASES = ["alternating40_allcols", "corrected40_allcols_nl"]
IMPULSE_CASES = [k for k in CASES if k.startswith("impulse")]

# the mixed ensemble: (elements, family, kind, boundary conditions, drag, gravity); one recorded node for all three
MIXED = (dict(n=6, family="allcols", kind="nonlinear", drag=True, grav=True, warm=WARM_NL),
         dict(n=100, family="taper10", kind="linear", bcs=pinned_root, drag=False, grav=True),
         dict(n=200, family="allcols", kind="nonlinear", drag=True, grav=False, warm=WARM_NL, reseed=1))
MIXED_REC_NODE = 3


def case_columns(c):
    kind = c["kind"](c["n"]) if callable(c["kind"]) else c["kind"]
    return graded_columns(c["n"], kind, c["family"], bcs=c["bcs"](c["n"]) if c.get("bcs") else None)


def seed_of(name, b, reseed=0):
    return 1000 * sum(map(ord, name)) + 10 * reseed + b


class Problem:
    """One beam with its dense loss: the warm start, the held force (or the impulse), the cotangents, and the oracle's
    differences of the loss, cached so that the CPU and the GPU file of one run compute each of them once."""

    def __init__(self, cols, seed, drag=True, grav=True, corrected=False, impulse=None, n_cot=1, rec_node=None, warm=WARM):
        self.cols, self.drag, self.grav, self.corrected = cols, drag, grav, corrected
        self.n_elem = len(cols["length"])
        ob = self.oracle()
        n = self.n = ob.n
        r2f = ob.red2full()
        self.dof = r2f % 3
        rng = np.random.default_rng(seed)
        self.U = np.where(self.dof == 1, rng.uniform(-50.0, 50.0, n), 0.0)
        self.x0 = ob.rk4_held(np.zeros(2 * n), DT, warm, self.U)
        assert np.all(np.isfinite(self.x0))
        node = self.n_elem // 2 if rec_node is None else rec_node
        if 3 * node + 1 not in r2f:
            node += 1
        self.rec_node, self.rec_idx = node, int(np.flatnonzero(r2f == 3 * node + 1)[0])
        scale = np.zeros(2 * n)
        for plane in range(2):
            for d in range(3):
                sel = np.flatnonzero(self.dof == d) + plane * n
                scale[sel] = 1.0 / np.max(np.abs(self.x0[sel]))     # (no block of any case is at rest after the warm start)
        assert np.all(np.isfinite(scale)) and np.all(scale > 0)
        self.lam = rng.normal(0.0, 1.0, (n_cot, 2 * n)) * scale
        self.lam_record = rng.normal(0.0, 1.0, (n_cot, N_REC)) * scale[self.rec_idx]
        self.W = np.hstack([self.lam, self.lam_record])
        self.impulse_idx = self.amp = None
        if impulse is not None:
            self.impulse_idx, self.amp = int(np.flatnonzero(r2f == 3 * impulse["node"] + 1)[0]), float(impulse["amp"])
        self._fd = {}

    def oracle(self, column=None, weights=None, eps=0.0):
        """the oracle of the beam, ``column`` moved by eps: an element column scaled by 1 + eps weights, or a scalar"""
        c = {k: np.array(v, copy=True) for k, v in self.cols.items()}
        kw = dict(fluid_density=RHO_F if self.drag else 0.0, enable_fluid=self.drag, enable_gravity=self.grav,
                  gravity=(0.0, G_Y, 0.0), corrected_axial=self.corrected)
        if column in ELEMENT_COLUMNS:
            c[column] = c[column] * (1.0 + eps * weights)
        elif column == "fluid_density":
            kw["fluid_density"] = RHO_F * (1.0 + eps)
        elif column == "g_y":
            kw["gravity"] = (0.0, G_Y * (1.0 + eps), 0.0)
        elif column == "g_x":
            kw["gravity"] = (eps * 9.81, G_Y, 0.0)
        elif column is not None:
            raise KeyError(column)
        return oracle_beam(c, **kw)

    def advance(self, ob, x, k, steps, amp):
        if self.impulse_idx is None:
            return ob.rk4_held(x, DT, steps, self.U)
        return ob.rk4_impulse(x, DT, steps, amp, IMPULSE_DURATION, self.impulse_idx, T0_IMPULSE + k * DT)

    def outputs(self, ob, amp=None):
        """what the loss weighs, [2 n + N_REC]: the rollout from x0, continued from sample to sample, then the samples"""
        amp = self.amp if amp is None else amp
        x, k, rec = self.x0, 0, []
        for _ in range(N_REC):
            x = self.advance(ob, x, k, REC_EVERY, amp)
            k += REC_EVERY
            rec.append(x[self.rec_idx])
        x = self.advance(ob, x, k, STEPS - k, amp)
        return np.concatenate([x, rec])

    def losses(self, ob, amp=None):
        """the loss of every cotangent [n_cot]"""
        return self.W @ self.outputs(ob, amp)

    def amp_kept(self, h):
        """|sum_i t_i| / sum_i |t_i| per cotangent, t_i = W_i amp d out_i / d amp the parts of amp dL/d amp"""
        ob = self.oracle()
        t = self.W * (self.outputs(ob, self.amp * (1 + h)) - self.outputs(ob, self.amp * (1 - h))) / (2 * h)
        return np.abs(np.sum(t, axis=1)) / np.sum(np.abs(t), axis=1)

    def central(self, column, h, weights=None):
        if column == "amp":
            return (self.losses(self.oracle(), self.amp * (1 + h)) - self.losses(self.oracle(), self.amp * (1 - h))) / (2 * h)
        return (self.losses(self.oracle(column, weights, h)) - self.losses(self.oracle(column, weights, -h))) / (2 * h)

    def differences(self, column, h, elements=None, xi=None):
        """(FD(h), FD(h/4)), each [n_cot, len(elements)] per element, [n_cot] along the element weights ``xi`` or for a scalar"""
        key = (column, h, elements, None if xi is None else xi.tobytes())
        if key not in self._fd:
            out = []
            for hh in (h, h / 4):
                if elements is not None:
                    out.append(np.stack([self.central(column, hh, np.eye(self.n_elem)[e]) for e in elements], axis=1))
                else:
                    out.append(self.central(column, hh, xi))
            self._fd[key] = tuple(out)
        return self._fd[key]


@functools.lru_cache(maxsize=None)
def problem(name, b):
    c = CASES[name]
    imp = dict(node=c["impulse"]["node"], amp=c["impulse"]["amps"][b]) if c.get("impulse") else None
    return Problem(case_columns(c), seed_of(name, b, c.get("reseed", 0)), corrected=c.get("corrected", False), impulse=imp,
                   n_cot=c["n_cot"], warm=c.get("warm", WARM))


@functools.lru_cache(maxsize=None)
def mixed_problem(b):
    m = MIXED[b]
    return Problem(case_columns(m), seed_of("mixed", b, m.get("reseed", 0)), drag=m["drag"], grav=m["grav"], rec_node=MIXED_REC_NODE,
                   warm=m.get("warm", WARM))


def step_size(name, column):
    return STEP_SIZE_OF_CASE.get(name, {}).get(column, STEP_SIZE[column])


def elements_of(c):
    return tuple(range(c["n"])) if c["elements"] == "all" else tuple(c["elements"])


def directions_of(n):
    """the three seeded element weightings of the several-wave cases"""
    return np.random.default_rng(77).uniform(0.5, 1.5, (3, n))


def self_agreement(fd1, fd4):
    """max_e |FD_e(h) - FD_e(h/4)| / max_e |FD_e(h/4)| per cotangent (a scalar difference is a column of one entry)"""
    fd1, fd4 = np.atleast_2d(np.asarray(fd1).T).T, np.atleast_2d(np.asarray(fd4).T).T
    return np.max(np.abs(fd1 - fd4), axis=1) / np.max(np.abs(fd4), axis=1)


def column_error(g, fd4):
    g, fd4 = np.atleast_2d(np.asarray(g).T).T, np.atleast_2d(np.asarray(fd4).T).T
    return np.max(np.abs(g - fd4), axis=1) / np.max(np.abs(fd4), axis=1)


def allowed_error(self_err):
    """test_adjoint.py's rule, column-wise"""
    return np.minimum(np.maximum(1e-7, 4.0 * np.asarray(self_err)), 1e-6)


def element_table(p, name, columns, elements):
    """{column: (FD(h), FD(h/4))} of the element columns, with EA_scale = E dL/dE - I dL/dI and EI_scale = I dL/dI when both
    stiffness columns are asked for"""
    out = {col: p.differences(col, step_size(name, col), elements=elements) for col in columns}
    if "elastic_modulus" in out and "moment_inertia" in out:
        out["EA_scale"] = tuple(e - i for e, i in zip(out["elastic_modulus"], out["moment_inertia"]))
        out["EI_scale"] = out["moment_inertia"]
    return out


def scalar_table(p, name, scalars=SCALARS):
    return {col: p.differences(col, step_size(name, col)) for col in scalars}


def direction_table(p, name, xi):
    return {col: p.differences(col, DIRECTION_STEP * STEP_SIZE[col], xi=xi) for col in ELEMENT_COLUMNS}


def check_inputs(what, table, elements=None, zeros=None):
    """the two conditions of this file on {column: (FD(h), FD(h/4))}; returns the worst self-agreement"""
    worst = 0.0
    for col, (fd1, fd4) in table.items():
        s = self_agreement(fd1, fd4)
        line = f"[param-grad-dense-cpu] {what} | {col} | self {np.max(s):.2e}"
        if elements is not None:
            zero_at = [i for i, e in enumerate(elements) if e in (zeros or {}).get(col, ())]
            rel = np.abs(fd4) / np.max(np.abs(fd4), axis=1, keepdims=True)
            for i in zero_at:
                assert np.all(fd1[:, i] == 0.0) and np.all(fd4[:, i] == 0.0), (what, col, elements[i])
            rel = np.delete(rel, zero_at, axis=1)
            line += f" | smallest entry {np.min(rel):.1e} of the largest"
            print(line)
            kept = [e for i, e in enumerate(elements) if i not in zero_at]
            assert np.min(rel) >= FLOOR, (what, col, [kept[i] for i in np.flatnonzero(np.min(rel, axis=0) < FLOOR)])
        else:
            print(line)
            assert np.all(np.abs(fd4) > 0.0), (what, col)
        assert np.all(s <= SELF_BAR), (what, col, s)
        worst = max(worst, float(np.max(s)))
    return worst


def host_layout(cols, **kw):
    from continuum_robot import _native as nat

    p = nat.Plan(cols, n_beams=5, device=-1, dtype="f64", **kw)
    return (p.n_slots, p.beams_per_group, p.threads)


# ---- 1. the layouts the GPU cases assert, on host plans
@pytest.mark.parametrize("name", list(CASES))
def test_case_layouts_on_host_plans(name):
    c = CASES[name]
    assert host_layout(case_columns(c), corrected_axial=c.get("corrected", False)) == c["layout"], name
    if c.get("impulse"):
        assert c["impulse"]["node"] == 64 and c["layout"][2] > 64          # (a wave seam)


# ---- 2. the oracle's own differences of the dense loss: self-agreement and the floor, per case
@pytest.mark.parametrize("name", ALL_ELEMENT_CASES)
def test_all_element_inputs(name):
    c = CASES[name]
    for b in range(c["B"]):
        p = problem(name, b)
        check_inputs(f"{name} beam {b}", element_table(p, name, ELEMENT_COLUMNS, elements_of(c)), elements_of(c), c["zeros"])
        check_inputs(f"{name} beam {b}", scalar_table(p, name))


@pytest.mark.parametrize("name", WAVE_CASES + BC_CASES)
def test_selected_element_inputs(name):
    c = CASES[name]
    p = problem(name, 0)
    check_inputs(name, element_table(p, name, ELEMENT_COLUMNS, elements_of(c)), elements_of(c), c["zeros"])
    check_inputs(name, scalar_table(p, name))
    if name in WAVE_CASES:
        for k, xi in enumerate(directions_of(c["n"])):
            check_inputs(f"{name} direction {k}", direction_table(p, name, xi))


@pytest.mark.parametrize("name", KIND_CASES)
def test_element_kind_inputs(name):
    c = CASES[name]
    check_inputs(name, element_table(problem(name, 0), name, ("elastic_modulus", "moment_inertia"), elements_of(c)), elements_of(c))


@pytest.mark.parametrize("name", IMPULSE_CASES)
def test_impulse_inputs(name):
    c = CASES[name]
    assert T0_IMPULSE > 0 and T0_IMPULSE + 23 * DT < IMPULSE_DURATION < T0_IMPULSE + 24 * DT
    for b in range(c["B"]):
        p = problem(name, b)
        assert p.impulse_idx == 3 * 63 + 1 and p.impulse_idx != p.n - 2      # (the w of node 64: not the tip's)
        check_inputs(f"{name} beam {b}", element_table(p, name, ("elastic_modulus",), elements_of(c)), elements_of(c))
        check_inputs(f"{name} beam {b}", {"amp": p.differences("amp", AMP_STEP)})
        kept = p.amp_kept(AMP_STEP / 4)
        print(f"[param-grad-dense-cpu] {name} beam {b} | amp | keeps {np.min(kept):.2f} of its parts")
        assert np.all(kept >= AMP_KEPT), (name, b, kept)


def test_mixed_ensemble_inputs():
    for b, m in enumerate(MIXED):
        p = mixed_problem(b)
        assert p.rec_node == MIXED_REC_NODE
        el = selected(m["n"])
        cols = ELEMENT_COLUMNS if m["drag"] else ELEMENT_COLUMNS[:2]
        check_inputs(f"mixed beam {b}", element_table(p, f"mixed{b}", cols, el), el, {"drag_coef": (0,)})
        scalars = [s for s in SCALARS if (s != "fluid_density" or m["drag"]) and (not s.startswith("g_") or m["grav"])]
        check_inputs(f"mixed beam {b}", scalar_table(p, f"mixed{b}", scalars))
