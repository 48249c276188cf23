"""CPU checks of the parameter-gradient feature (crb_paramgrad.h, crb_step_rk4_adjoint_params): the new names are declared in
include/crbeam.h and exported, the version is unchanged, host-only and fp32 plans and bad arguments are refused before the device
is touched, and the work-buffer size follows its documented formula."""
import ctypes as C
import os
import re

import pytest

from tests.helpers import nitinol_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_param_gradient_symbols_are_declared_and_exported():
    from continuum_robot import _native as nat

    hdr = open(os.path.join(ROOT, "include", "crbeam.h")).read()
    lib = nat.load()
    assert re.search(r"typedef struct crb_param_cotangent\s*\{[^}]*void\*\s*param_bar;[^}]*\}\s*crb_param_cotangent;", hdr)
    assert re.search(r"\bsize_t crb_rk4_adjoint_params_work_bytes\s*\(", hdr)
    assert re.search(r"\bint crb_step_rk4_adjoint_params\s*\(", hdr)
    for name in ("crb_rk4_adjoint_params_work_bytes", "crb_step_rk4_adjoint_params"):
        assert hasattr(lib, name), name
    assert [f for f, _ in nat.ParamCotangent._fields_] == ["param_bar"]


def test_version_is_the_headers():
    from continuum_robot import _native as nat

    hdr = open(os.path.join(ROOT, "include", "crbeam.h")).read()
    assert nat.load().crb_version() == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))


def call(lib, plan, n_cot=1, every=3, work=32, pgrad="ok", param_bar=40):
    from continuum_robot import _native as nat

    p = C.c_void_p
    pg = nat.ParamCotangent()
    pg.param_bar = param_bar
    return lib.crb_step_rk4_adjoint_params(plan.h if plan is not None else None, p(8), p(16), n_cot, 0.0, 2e-5, 10, every, None,
                                           None, None, C.byref(pg) if pgrad == "ok" else None, p(work) if work else None, None)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_before_the_device(dtype):
    """fp32 plans: CRB_EUNSUPPORTED; a NULL pgrad, param_bar or work buffer and a bad n_cot or every: CRB_EINVAL -- checked
    before the device is touched, so a host-only plan shows them; valid arguments on it give CRB_ENODEV"""
    from continuum_robot import _native as nat

    plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=2, device=-1, dtype=dtype)
    lib = nat.load()
    if dtype == "f32":
        assert call(lib, plan) == nat.CRB_EUNSUPPORTED
        assert "fp64" in lib.crb_last_error().decode()
        return
    assert call(lib, None) == nat.CRB_EINVAL
    assert call(lib, plan, pgrad=None) == nat.CRB_EINVAL
    assert "param_bar" in lib.crb_last_error().decode()
    assert call(lib, plan, param_bar=None) == nat.CRB_EINVAL
    assert "param_bar" in lib.crb_last_error().decode()
    assert call(lib, plan, work=None) == nat.CRB_EINVAL
    assert "work" in lib.crb_last_error().decode()
    for n_cot in (0, -1, 65536):
        assert call(lib, plan, n_cot=n_cot) == nat.CRB_EINVAL
        assert "n_cot" in lib.crb_last_error().decode()
    for every in (0, -2):
        assert call(lib, plan, every=every) == nat.CRB_EINVAL
        assert "every" in lib.crb_last_error().decode()
    assert call(lib, plan, param_bar=16) == nat.CRB_EINVAL   # (param_bar aliasing lam)
    assert call(lib, plan, param_bar=32) == nat.CRB_EINVAL   # (param_bar aliasing the work buffer)
    assert call(lib, plan) == nat.CRB_ENODEV
    assert "crb_step_rk4_adjoint_params" in lib.crb_last_error().decode()


def test_work_bytes_formula_on_host_only_plans():
    from continuum_robot import _native as nat

    lib = nat.load()
    for n, B in ((4, 1), (6, 3), (200, 5)):
        plan = nat.Plan(nitinol_columns(n, "nonlinear"), n_beams=B, device=-1)
        n_node = n + 1
        for every, n_cot in ((1, 1), (7, 3), (32, 2)):
            base = every * (4 * B * 2 * n_node * 4 + 1) * 8
            assert lib.crb_rk4_adjoint_work_bytes(plan.h, every) == base
            want = base + every * 4 * n_cot * B * n_node * 4 * 8
            assert lib.crb_rk4_adjoint_params_work_bytes(plan.h, every, n_cot) == want, (n, B, every, n_cot)
        for every, n_cot in ((0, 1), (-3, 1), (4, 0), (4, -1)):
            assert lib.crb_rk4_adjoint_params_work_bytes(plan.h, every, n_cot) == 0
    assert lib.crb_rk4_adjoint_params_work_bytes(None, 4, 1) == 0
