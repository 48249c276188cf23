"""CPU checks of the tangent-linear feature: both new entry points (crb_rhs_jvp, crb_step_rk4_tangent) exist, are declared
in include/crbeam.h and refuse a host-only plan; the library that loads is the one the header describes."""
import ctypes as C
import os
import re

import pytest

from tests.helpers import nitinol_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_version_matches_the_built_library_and_the_tangent_symbols_are_exported():
    from continuum_robot import _native as nat

    hdr = open(os.path.join(ROOT, "include", "crbeam.h")).read()
    declared = int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))
    lib = nat.load()
    assert lib.crb_version() == declared
    for name in ("crb_rhs_jvp", "crb_step_rk4_tangent"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
    assert "crb_input_tangent" in hdr
    assert [f for f, _ in nat.InputTangent._fields_] == ["d_amp", "df_held"]
    assert C.sizeof(nat.InputTangent) == 2 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_only_plan_has_no_tangent_cpu_path(dtype):
    from continuum_robot import _native as nat

    plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=1, device=-1, dtype=dtype)
    lib = nat.load()
    p = C.c_void_p
    rc = lib.crb_rhs_jvp(plan.h, p(8), None, p(16), None, 1, None, p(24), None)
    assert rc == nat.CRB_ENODEV
    assert "no CPU path" in lib.crb_last_error().decode()
    t_end = C.c_double(-1.0)
    rc = lib.crb_step_rk4_tangent(plan.h, p(8), p(16), 1, 0.0, 2e-5, 10, None, None, C.byref(t_end), None)
    assert rc == nat.CRB_ENODEV
    assert "no CPU path" in lib.crb_last_error().decode()
    assert t_end.value == -1.0   # (refused before anything is written)


def test_null_plan_is_invalid():
    from continuum_robot import _native as nat

    lib = nat.load()
    assert lib.crb_rhs_jvp(None, None, None, None, None, 1, None, None, None) == nat.CRB_EINVAL
    assert lib.crb_step_rk4_tangent(None, None, None, 1, 0.0, 1.0, 1, None, None, None, None) == nat.CRB_EINVAL


def test_batched_api_exposes_the_tangent_methods():
    import inspect

    from continuum_robot.batched import BeamEnsemble

    for name in ("rhs_jvp", "linearize", "step_tangent"):
        assert callable(getattr(BeamEnsemble, name, None)), name
    sig = inspect.signature(BeamEnsemble.step_tangent)
    assert list(sig.parameters)[1:] == ["n_steps", "dt", "dx0_red", "impulse_amp", "impulse_duration", "impulse_index",
                                        "held_force", "d_impulse_amp", "d_held_force", "t0"]
    assert list(inspect.signature(BeamEnsemble.rhs_jvp).parameters)[1:] == ["dx_red", "x_red", "u_red", "du_red"]
    assert list(inspect.signature(BeamEnsemble.linearize).parameters)[1:] == ["x_red", "u_red"]
