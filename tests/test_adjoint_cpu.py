"""CPU checks of the adjoint feature (crb_adjoint.h): the new entry points are declared in include/crbeam.h and exported, refuse
host-only plans, fp32 plans and bad sizes, the work-buffer size follows its documented formula, and the inverse gravity lists
reproduce the plan's forward gravity table edge for edge."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.helpers import nitinol_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_rhs_vjp", "crb_rk4_adjoint_work_bytes", "crb_step_rk4_checkpoint", "crb_step_rk4_adjoint",
         "crb_plan_get_grav_transpose")


def test_adjoint_symbols_are_declared_and_exported():
    from continuum_robot import _native as nat

    hdr = open(os.path.join(ROOT, "include", "crbeam.h")).read()
    lib = nat.load()
    for name in NAMES:
        assert re.search(rf"\b(int|size_t) {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
    assert "crb_input_cotangent" in hdr
    assert [f for f, _ in nat.InputCotangent._fields_] == ["amp_bar", "f_held_bar"]


def test_host_only_plan_has_no_adjoint_cpu_path():
    from continuum_robot import _native as nat

    plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=1, device=-1)
    lib = nat.load()
    p = C.c_void_p
    assert lib.crb_rhs_vjp(plan.h, p(8), None, p(16), 1, None, p(24), None, None) == nat.CRB_ENODEV
    assert "no CPU path" in lib.crb_last_error().decode()
    t_end = C.c_double(-1.0)
    assert lib.crb_step_rk4_checkpoint(plan.h, p(8), 0.0, 2e-5, 10, 3, None, None, p(16), C.byref(t_end), None) == nat.CRB_ENODEV
    assert t_end.value == -1.0
    assert lib.crb_step_rk4_adjoint(plan.h, p(8), p(16), 1, 0.0, 2e-5, 10, 3, None, None, None, p(24), None) == nat.CRB_ENODEV


def test_null_plan_is_invalid():
    from continuum_robot import _native as nat

    lib = nat.load()
    assert lib.crb_rhs_vjp(None, None, None, None, 1, None, None, None, None) == nat.CRB_EINVAL
    assert lib.crb_step_rk4_adjoint(None, None, None, 1, 0.0, 1.0, 1, 1, None, None, None, None, None) == nat.CRB_EINVAL
    assert lib.crb_rk4_adjoint_work_bytes(None, 4) == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_before_the_device(dtype):
    """fp32 plans: CRB_EUNSUPPORTED; bad n_cot / every / a NULL work buffer: CRB_EINVAL -- checked before the device is
    touched, so a host-only plan shows them; valid arguments on it give CRB_ENODEV"""
    from continuum_robot import _native as nat

    plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=2, device=-1, dtype=dtype)
    lib = nat.load()
    p = C.c_void_p
    adj = lambda n_cot, every, work: lib.crb_step_rk4_adjoint(plan.h, p(8), p(16), n_cot, 0.0, 2e-5, 10, every, None,   # noqa: E731
                                                              None, None, work, None)
    vjp = lambda n_cot: lib.crb_rhs_vjp(plan.h, p(8), None, p(16), n_cot, None, p(24), None, None)   # noqa: E731
    ckp = lambda every: lib.crb_step_rk4_checkpoint(plan.h, p(8), 0.0, 2e-5, 10, every, None, None, p(16), None, None)   # noqa: E731
    if dtype == "f32":
        assert adj(1, 3, p(32)) == nat.CRB_EUNSUPPORTED
        assert "fp64" in lib.crb_last_error().decode()
        assert vjp(1) == nat.CRB_EUNSUPPORTED
        assert ckp(3) == nat.CRB_EUNSUPPORTED
        return
    for n_cot in (0, -1, 65536):
        assert adj(n_cot, 3, p(32)) == nat.CRB_EINVAL
        assert "n_cot" in lib.crb_last_error().decode()
        assert vjp(n_cot) == nat.CRB_EINVAL
    for every in (0, -2):
        assert adj(1, every, p(32)) == nat.CRB_EINVAL
        assert "every" in lib.crb_last_error().decode()
        assert ckp(every) == nat.CRB_EINVAL
    assert adj(1, 3, None) == nat.CRB_EINVAL
    assert "work" in lib.crb_last_error().decode()
    assert adj(1, 3, p(16)) == nat.CRB_EINVAL   # (lam aliasing the work buffer)
    assert adj(1, 3, p(32)) == nat.CRB_ENODEV
    assert vjp(1) == nat.CRB_ENODEV
    assert ckp(3) == nat.CRB_ENODEV


def test_work_bytes_formula_on_host_only_plans():
    from continuum_robot import _native as nat

    lib = nat.load()
    for n, B in ((4, 1), (6, 3), (200, 5)):
        plan = nat.Plan(nitinol_columns(n, "nonlinear"), n_beams=B, device=-1)
        lay = None
        n_node = n + 1
        for every in (1, 7, 32):
            want = every * (4 * B * 2 * n_node * 4 + 1) * 8
            assert lib.crb_rk4_adjoint_work_bytes(plan.h, every) == want, (n, B, every, lay)
        assert lib.crb_rk4_adjoint_work_bytes(plan.h, 0) == 0
        assert lib.crb_rk4_adjoint_work_bytes(plan.h, -3) == 0


GRAV_CASES = {
    "cantilever": dict(n=6, bcs=None),
    "cantilever_long": dict(n=40, bcs=None),
    "pinned_root": dict(n=6, bcs=["PINNED"] + ["NONE"] * 5),
    "interior_pin": dict(n=8, bcs=["FIXED", "NONE", "NONE", "PINNED", "NONE", "NONE", "NONE", "NONE"]),
    "pinned_root_long": dict(n=30, bcs=["PINNED"] + ["NONE"] * 29),
}


@pytest.mark.parametrize("name", list(GRAV_CASES))
def test_inverse_gravity_lists_reproduce_the_forward_table(name):
    from continuum_robot import _native as nat

    c = GRAV_CASES[name]
    plan = nat.Plan(nitinol_columns(c["n"], "nonlinear", bcs=c["bcs"]), n_beams=1, device=-1, enable_gravity=True)
    lib = nat.load()
    lay = nat.Layout()
    nat.check(lib.crb_plan_get_layout(plan.h, C.byref(lay)))
    S = lay.n_slots
    grav = np.zeros((S, 12), dtype=np.int16)
    nat.check(lib.crb_plan_get_slot_tables(plan.h, None, None, None, grav.ctypes.data_as(C.POINTER(C.c_int16)), None))
    seg = np.zeros((S, 2, 2), dtype=np.int32)
    phi = np.zeros((S, 3, 2), dtype=np.int32)
    fan = np.zeros(2, dtype=np.int32)
    nat.check(lib.crb_plan_get_grav_transpose(plan.h, 0, seg.ctypes.data, phi.ctypes.data, fan.ctypes.data))
    # forward edges: node DOF (j, c) <- component comp[c] of segments segA[c], segB[c]; segment s <- rotations phiA, phiB
    fwd_seg, fwd_phi = [], []
    for j in range(S):
        phiA, phiB = int(grav[j, 0]), int(grav[j, 1])
        for c in range(3):
            for sg in (int(grav[j, 2 + c]), int(grav[j, 5 + c])):
                if sg >= 0:
                    fwd_seg.append((sg, int(grav[j, 8 + c]), j * 4 + c))
        for f in (phiA, phiB):
            if f >= 0:
                fwd_phi.append((f >> 2, f & 3, j, phiB >= 0))
    inv_seg = [(s, m, int(e)) for s in range(S) for m in range(2) for e in seg[s, m] if e >= 0]
    inv_phi = [(j, c, int(e) >> 1, bool(int(e) & 1)) for j in range(S) for c in range(3) for e in phi[j, c] if e >= 0]
    assert len(fwd_seg) > 0 and len(fwd_phi) > 0, name
    assert sorted(inv_seg) == sorted(fwd_seg), name           # every forward edge exactly once
    assert len(set(inv_seg)) == len(inv_seg)
    assert sorted(inv_phi) == sorted(fwd_phi), name
    assert len(set(inv_phi)) == len(inv_phi)
    assert 1 <= fan[0] <= 2 and 1 <= fan[1] <= 2
    for arr in (seg, phi):   # entries ascending, -1 only at the end of a list
        for lst in arr.reshape(-1, 2):
            real = [int(e) for e in lst if e >= 0]
            assert list(lst[:len(real)]) == real and real == sorted(real)


def test_grav_transpose_checks_its_beam_index():
    from continuum_robot import _native as nat

    plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=2, device=-1, enable_gravity=True)
    lib = nat.load()
    assert lib.crb_plan_get_grav_transpose(plan.h, 2, None, None, None) == nat.CRB_EINVAL
    assert lib.crb_plan_get_grav_transpose(plan.h, -1, None, None, None) == nat.CRB_EINVAL
    assert lib.crb_plan_get_grav_transpose(plan.h, 1, None, None, None) == nat.CRB_OK


def test_batched_api_exposes_the_adjoint_methods():
    import inspect

    from continuum_robot.batched import BeamEnsemble

    assert list(inspect.signature(BeamEnsemble.rhs_vjp).parameters)[1:] == ["lam_red", "x_red", "u_red"]
    assert list(inspect.signature(BeamEnsemble.step_adjoint).parameters)[1:] == [
        "n_steps", "dt", "lam_red", "x0_red", "impulse_amp", "impulse_duration", "impulse_index", "held_force", "t0",
        "record", "record_every", "lam_record", "checkpoint_every"]
    assert list(inspect.signature(BeamEnsemble.rollout).parameters)[1:4] == ["x0_red", "n_steps", "dt"]
