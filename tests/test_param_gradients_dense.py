"""Parameter gradients of the adjoint rollout (BeamEnsemble.step_adjoint_params, crb_param_grad_kernel) where the whole rod
contributes, entry by entry.  The loss, the case table and the oracle's central differences are those of
tests/test_param_gradients_dense_cpu.py, which also shows them fit to compare against: from a warm start under a held force
on every w DOF, a seeded cotangent on every reduced DOF and recorded mid-span samples, so every element's entry is at least 1e-5
of its column's largest -- the lanes of the first waves of a multi-wave beam, the wave seams, the left-neighbour loads across
them, the left neighbour's mask at an interior pin, the per-slot tables of graded rods and the drag_coef row map all show.

Rule of every comparison (test_adjoint.py's, column-wise): err = max_e |g_e - FD_e(h/4)| / max_e |FD_e(h/4)| must be
<= min(max(1e-7, 4 self), 1e-6), self the oracle's own max_e |FD_e(h) - FD_e(h/4)| / max_e |FD_e(h/4)|.  Each comparison prints
``[param-grad-dense] case | column | err | allowed | self`` (pytest -s)."""
import numpy as np
import pytest
import torch

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams
from tests.test_param_gradients_dense_cpu import (ALL_ELEMENT_CASES, AMP_STEP, BC_CASES, CASES, DT, ELEMENT_COLUMNS, G_Y, IMPULSE_CASES,
                                                  IMPULSE_DURATION, KIND_CASES, MIXED, MIXED_REC_NODE, REC_EVERY, RHO_F, SCALARS, STEPS,
                                                  T0_IMPULSE, WAVE_CASES, allowed_error, case_columns, column_error,
                                                  direction_table, directions_of, element_table, elements_of, mixed_problem,
                                                  problem, scalar_table, selected, self_agreement)

pytestmark = pytest.mark.gpu


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def force_params(drag=True, grav=True):
    return ForceParams(fluid_density=RHO_F if drag else 0.0, enable_fluid_effects=drag, enable_gravity_effects=grav)


def layout_of(ens):
    lay = ens.plan.layout
    return (lay.n_slots, lay.beams_per_group, lay.threads)


def dense_gradients(ens, problems, rec_node):
    """step_adjoint_params for the dense loss of each beam's problem: (amp_bar [D, B] or None, the dict, each [D, B, ...])"""
    B, n, D = ens.n_beams, ens.n, problems[0].lam.shape[0]
    lam = np.stack([ens.pad_states([p.lam[d] for p in problems]) for d in range(D)])
    lam_record = np.stack([np.stack([p.lam_record[d] for p in problems]) for d in range(D)])
    x0 = ens.pad_states([p.x0 for p in problems])
    kw = dict(x0_red=x0, record=(rec_node, "w"), record_every=REC_EVERY, lam_record=lam_record)
    if problems[0].impulse_idx is None:
        held = np.zeros((B, n))
        for b, p in enumerate(problems):
            held[b, :p.n] = p.U
        kw.update(held_force=held, t0=0.0)
    else:
        kw.update(impulse_amp=np.array([p.amp for p in problems]), impulse_duration=IMPULSE_DURATION,
                  impulse_index=problems[0].impulse_idx, t0=T0_IMPULSE)
    out = ens.step_adjoint_params(STEPS, DT, lam, **kw)
    return (np_(out[1]) if out[1] is not None else None), {k: np_(v) for k, v in out[3].items()}


def case_gradients(name):
    """the ensemble of a case with its layout asserted, its problems and their gradients"""
    c = CASES[name]
    ens = BeamEnsemble(case_columns(c), c["B"], force_params=force_params(), corrected_axial=c.get("corrected", False))
    assert layout_of(ens) == c["layout"], (name, layout_of(ens))
    problems = [problem(name, b) for b in range(c["B"])]
    assert all(p.n == ens.n for p in problems)
    return problems, dense_gradients(ens, problems, problems[0].rec_node)


def compare(what, column, g, fd, elements=None, zeros=()):
    """the rule of this file on one column: g and FD [D, E] (or [D]); the named exact zeros must be exact zeros"""
    fd1, fd4 = fd
    if elements is not None:
        for i, e in enumerate(elements):
            if e in zeros:
                assert np.all(g[:, i] == 0.0) and np.all(fd4[:, i] == 0.0), (what, column, e)
    s, err = self_agreement(fd1, fd4), column_error(g, fd4)
    allowed = allowed_error(s)
    for d in range(len(err)):
        print(f"[param-grad-dense] {what}" + (f" cotangent {d}" if len(err) > 1 else "") +
              f" | {column} | {err[d]:.2e} | {allowed[d]:.1e} | {s[d]:.2e}")
    assert np.all(allowed <= 1e-6) and np.all(err <= allowed), (what, column, err, allowed)


def check_elements(what, p, grads, b, name, columns, elements, zeros, cots=slice(None)):
    el = list(elements)
    table = element_table(p, name, columns, elements)
    for col, fd in table.items():
        g = grads[col][:, b][:, el]
        if col in ELEMENT_COLUMNS:
            g = g * p.cols[col][el]
        compare(what, col, g[cots], tuple(f[cots] for f in fd), elements, zeros.get(col, ()))


def check_scalars(what, p, grads, b, name, scalars=SCALARS, cots=slice(None)):
    got = {"fluid_density": RHO_F * grads["fluid_density"][:, b], "g_x": 9.81 * grads["gravity"][:, b, 0],
           "g_y": G_Y * grads["gravity"][:, b, 1]}
    for col, fd in scalar_table(p, name, scalars).items():
        compare(what, col, got[col][cots], tuple(f[cots] for f in fd))


# ---- 1. per element, all elements, two held forces; cotangent 0 where the problem holds several
@pytest.mark.parametrize("name", ALL_ELEMENT_CASES)
def test_every_element(name):
    c = CASES[name]
    problems, (_, grads) = case_gradients(name)
    for b, p in enumerate(problems):
        check_elements(f"{name} beam {b}", p, grads, b, name, ELEMENT_COLUMNS, elements_of(c), c["zeros"], cots=slice(0, 1))
        check_scalars(f"{name} beam {b}", p, grads, b, name, cots=slice(0, 1))


# ---- 2. several waves, 3. boundary conditions: the seam elements (and those around the pin), the scalars, three directions
@pytest.mark.parametrize("name", WAVE_CASES + BC_CASES)
def test_seams_and_pins(name):
    c = CASES[name]
    (p,), (_, grads) = case_gradients(name)
    check_elements(name, p, grads, 0, name, ELEMENT_COLUMNS, elements_of(c), c["zeros"])
    check_scalars(name, p, grads, 0, name)
    if name in WAVE_CASES:
        for k, xi in enumerate(directions_of(c["n"])):
            for col, fd in direction_table(p, name, xi).items():
                compare(f"{name} direction {k}", col, np.sum(xi * p.cols[col] * grads[col][:, 0], axis=1), fd)


# ---- 4. alternating element kinds; the corrected axial strain
@pytest.mark.parametrize("name", KIND_CASES)
def test_element_kinds_and_the_axial_option(name):
    c = CASES[name]
    (p,), (_, grads) = case_gradients(name)
    check_elements(name, p, grads, 0, name, ("elastic_modulus", "moment_inertia"), elements_of(c), {})


# ---- 5. an impulse at a wave seam whose window closes inside the rollout, from a clock that does not start at 0
# (amp dL/d amp is measured against itself: the CPU file shows that it is no cancelled remainder of its parts, AMP_KEPT)
@pytest.mark.parametrize("name", IMPULSE_CASES)
def test_mid_span_impulse(name):
    c = CASES[name]
    problems, (amp_bar, grads) = case_gradients(name)
    for b, p in enumerate(problems):
        check_elements(f"{name} beam {b}", p, grads, b, name, ("elastic_modulus",), elements_of(c), {})
        compare(f"{name} beam {b}", "amp", p.amp * amp_bar[:, b], p.differences("amp", AMP_STEP))


# ---- 6. mixed ensemble: packed, two-wave (PINNED root) and four-wave members, per-beam ForceParams
def test_mixed_ensemble():
    problems = [mixed_problem(b) for b in range(len(MIXED))]
    ens = BeamEnsemble([p.cols for p in problems], len(MIXED), force_params=[force_params(m["drag"], m["grav"]) for m in MIXED])
    assert ens.mixed_topology
    _, grads = dense_gradients(ens, problems, MIXED_REC_NODE)
    for b, (m, p) in enumerate(zip(MIXED, problems)):
        what, ne = f"mixed beam {b}", m["n"]
        check_elements(what, p, grads, b, f"mixed{b}", ELEMENT_COLUMNS if m["drag"] else ELEMENT_COLUMNS[:2], selected(ne),
                       {"drag_coef": (0,)})
        check_scalars(what, p, grads, b, f"mixed{b}",
                      [s for s in SCALARS if (s != "fluid_density" or m["drag"]) and (not s.startswith("g_") or m["grav"])])
        for key in ("EA_scale", "EI_scale", "elastic_modulus", "moment_inertia", "drag_coef"):
            assert np.all(grads[key][:, b, ne:] == 0.0), (what, key)
        assert np.all(grads["drag_scale"][:, b, ne + 1:] == 0.0), what
        if not m["drag"]:
            for key in ("drag_scale", "drag_coef", "fluid_density"):
                assert np.all(grads[key][:, b] == 0.0), (what, key)
        if not m["grav"]:
            assert np.all(grads["gravity"][:, b] == 0.0), what


# ---- 7. three dense cotangents in one call, each against its own differences
def test_three_cotangents_in_one_call():
    name = "all65_mesh4_lin"
    c = CASES[name]
    assert c["n_cot"] == 3
    problems, (_, grads) = case_gradients(name)
    assert grads["elastic_modulus"].shape == (3, c["B"], c["n"])
    for b, p in enumerate(problems):
        check_elements(f"{name} beam {b}", p, grads, b, name, ELEMENT_COLUMNS, elements_of(c), c["zeros"])
        check_scalars(f"{name} beam {b}", p, grads, b, name)
