"""CPU checks of the closed-loop adjoint (crb_feedback_adjoint.h; crb_step_rk4_feedback_checkpoint / _adjoint): the entry points
are declared in include/crbeam.h, exported and bound; the work-buffer size follows its documented formula; every refusal is
made before the device is touched, so host-only plans (Plan(..., device=-1)) show them, and crb_last_error() names the
argument; the Python methods have the documented signatures and refuse lists of gains."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.helpers import nitinol_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_rk4_feedback_adjoint_work_bytes", "crb_step_rk4_feedback_checkpoint", "crb_step_rk4_feedback_adjoint")
P = C.c_void_p
X, CKPT, WORK, GAIN, REF, LAM, GBAR, RBAR = (P(64 * (i + 1)) for i in range(8))   # distinct fake device addresses


def lib_and_nat():
    from continuum_robot import _native as nat

    return nat.load(), nat


def host_plan(n=4, B=2, dtype="f64", **kw):
    from continuum_robot import _native as nat

    return nat.Plan(nitinol_columns(n, "nonlinear"), n_beams=B, device=-1, dtype=dtype, **kw)


def cotangent(nat, gain_bar=GBAR, ref_bar=RBAR):
    g = nat.FeedbackCotangent()
    g.gain_bar, g.ref_bar = gain_bar, ref_bar
    return g


def checkpoint(lib, plan, x=X, every=3, gain=GAIN, ref=REF, inp=None, rec=None, ckpt=CKPT, work=WORK, n_steps=10, dt=2e-5):
    return lib.crb_step_rk4_feedback_checkpoint(plan.h, x, 0.0, dt, n_steps, every, gain, ref, inp, rec, ckpt, work, None, None)


def adjoint(lib, nat, plan, ckpt=CKPT, lam=LAM, n_cot=1, every=3, gain=GAIN, ref=REF, inp=None, rec=None, grad="default",
            work=WORK, n_steps=10, dt=2e-5):
    g = cotangent(nat) if grad == "default" else grad
    return lib.crb_step_rk4_feedback_adjoint(plan.h, ckpt, lam, n_cot, 0.0, dt, n_steps, every, gain, ref, inp, rec,
                                             C.byref(g) if g is not None else None, work, None)


def last_error(lib):
    return lib.crb_last_error().decode()


def test_symbols_are_declared_exported_and_bound():
    lib, nat = lib_and_nat()
    hdr = open(os.path.join(ROOT, "include", "crbeam.h")).read()
    for name in NAMES:
        assert re.search(rf"\b(int|size_t) {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "typedef struct crb_feedback_cotangent" in hdr
    assert [f for f, _ in nat.FeedbackCotangent._fields_] == ["gain_bar", "ref_bar"]
    assert lib.crb_rk4_feedback_adjoint_work_bytes.restype is C.c_size_t
    # every entry cites the controller it differentiates
    for name in NAMES:
        at = hdr.index(f" {name}(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "lqr_control.py:95-125" in comment and "full_state_linear.py:81" in comment, name


def test_work_bytes_formula_and_bad_arguments():
    lib, _ = lib_and_nat()
    ceil = lambda a, b: -(-a // b)   # noqa: E731
    seen = set()
    for n, B in ((4, 1), (6, 3), (100, 5), (6, 33), (6, 100), (128, 2048)):
        plan = host_plan(n, B)
        S = B * 2 * (n + 1) * 4
        F = S // 2
        nf = plan.n_free
        Z = min(ceil(B, 32), ceil(1536, ceil(nf, 32) * ceil(2 * nf, 32)))   # slices of the gain gradient's beam reduction
        seen.add(Z)
        for every in (1, 7, 32):
            for n_cot in (1, 2, 9):
                want = ((4 * every + 2 + 3 * n_cot) * S + (1 + n_cot) * F + (n_cot * Z * nf * 2 * nf if Z > 1 else 0)) * 8
                assert lib.crb_rk4_feedback_adjoint_work_bytes(plan.h, every, n_cot) == want, (n, B, every, n_cot)
        for every, n_cot in ((0, 1), (-3, 1), (1, 0), (4, -1)):
            assert lib.crb_rk4_feedback_adjoint_work_bytes(plan.h, every, n_cot) == 0
    assert lib.crb_rk4_feedback_adjoint_work_bytes(None, 4, 1) == 0
    assert seen == {1, 2, 4, 6}


def test_valid_calls_on_host_only_plans_have_no_device():
    lib, nat = lib_and_nat()
    for kw in (dict(), dict(enable_gravity=True, enable_fluid=True, fluid_density=1000.0)):
        plan = host_plan(**kw)
        t_end = C.c_double(-1.0)
        assert lib.crb_step_rk4_feedback_checkpoint(plan.h, X, 0.0, 2e-5, 10, 3, GAIN, REF, None, None, CKPT, WORK,
                                                    C.byref(t_end), None) == nat.CRB_ENODEV
        assert "no CPU path" in last_error(lib) and t_end.value == -1.0
        assert checkpoint(lib, plan, ref=None) == nat.CRB_ENODEV
        assert adjoint(lib, nat, plan) == nat.CRB_ENODEV
        assert "no CPU path" in last_error(lib)
        assert adjoint(lib, nat, plan, ref=None, grad=cotangent(nat, None, None)) == nat.CRB_ENODEV   # (both members may be NULL)
        assert adjoint(lib, nat, plan, n_cot=65535) == nat.CRB_ENODEV


def test_null_plan_is_invalid():
    lib, nat = lib_and_nat()
    assert lib.crb_step_rk4_feedback_checkpoint(None, X, 0.0, 2e-5, 1, 1, GAIN, None, None, None, CKPT, WORK, None, None) == nat.CRB_EINVAL
    g = cotangent(nat)
    assert lib.crb_step_rk4_feedback_adjoint(None, CKPT, LAM, 1, 0.0, 2e-5, 1, 1, GAIN, None, None, None, C.byref(g), WORK,
                                             None) == nat.CRB_EINVAL


def test_fp32_and_long_beams_are_unsupported():
    lib, nat = lib_and_nat()
    f32 = host_plan(dtype="f32")
    assert checkpoint(lib, f32) == nat.CRB_EUNSUPPORTED
    assert "fp64" in last_error(lib)
    assert adjoint(lib, nat, f32) == nat.CRB_EUNSUPPORTED
    assert "fp64" in last_error(lib)
    # (mixed topology: per-beam plans have no host-only form -- crb_plan_create_ensemble refuses device -1 -- so that refusal is
    #  checked on a device plan, tests/test_feedback_adjoint.py::test_mixed_topology_and_gain_lists_are_refused)
    with pytest.raises(nat.NativeError, match="no host-only form"):
        nat.Plan([nitinol_columns(4, "nonlinear"), nitinol_columns(6, "nonlinear")], n_beams=2, device=-1)
    # more than 256 thread-carried nodes: the limit of crb_rhs_vjp
    long = host_plan(n=300, B=1)
    assert adjoint(lib, nat, long) == nat.CRB_EUNSUPPORTED
    assert "256" in last_error(lib)


def test_whole_state_snapshots_are_unsupported():
    lib, nat = lib_and_nat()
    plan = host_plan()
    rec = nat.RecordDesc(0, -1, 0, 1, P(4096))
    assert checkpoint(lib, plan, rec=C.byref(rec)) == nat.CRB_EUNSUPPORTED
    assert "CRB_RECORD_ALL" in last_error(lib)
    assert adjoint(lib, nat, plan, rec=C.byref(rec)) == nat.CRB_EUNSUPPORTED
    assert "CRB_RECORD_ALL" in last_error(lib)


@pytest.mark.parametrize("n_cot", [0, -1, 65536])
def test_bad_n_cot_is_invalid(n_cot):
    lib, nat = lib_and_nat()
    assert adjoint(lib, nat, host_plan(), n_cot=n_cot) == nat.CRB_EINVAL
    assert "n_cot" in last_error(lib)


def test_null_pointers_are_invalid_and_named():
    lib, nat = lib_and_nat()
    plan = host_plan()
    for kw, word in ((dict(gain=None), "gain"), (dict(lam=None), "lam"), (dict(ckpt=None), "ckpt"), (dict(work=None), "work"),
                     (dict(grad=None), "grad")):
        assert adjoint(lib, nat, plan, **kw) == nat.CRB_EINVAL, kw
        assert word in last_error(lib), (kw, last_error(lib))
    for kw, word in ((dict(gain=None), "gain"), (dict(x=None), "x is null"), (dict(ckpt=None), "ckpt"), (dict(work=None), "work")):
        assert checkpoint(lib, plan, **kw) == nat.CRB_EINVAL, kw
        assert word in last_error(lib), (kw, last_error(lib))


def test_bad_sizes_are_invalid_and_named():
    lib, nat = lib_and_nat()
    plan = host_plan()
    for kw, word in ((dict(every=0), "every"), (dict(every=-2), "every"), (dict(n_steps=-1), "n_steps"), (dict(dt=0.0), "dt"),
                     (dict(dt=float("nan")), "dt")):
        assert adjoint(lib, nat, plan, **kw) == nat.CRB_EINVAL, kw
        assert word in last_error(lib), (kw, last_error(lib))
        assert checkpoint(lib, plan, **kw) == nat.CRB_EINVAL, kw
        assert word in last_error(lib), (kw, last_error(lib))


def test_aliasing_outputs_are_invalid_and_named():
    lib, nat = lib_and_nat()
    plan = host_plan()
    for other in (CKPT, WORK, GAIN, REF):
        assert adjoint(lib, nat, plan, lam=other) == nat.CRB_EINVAL, other
        assert "lam" in last_error(lib)
        assert adjoint(lib, nat, plan, grad=cotangent(nat, gain_bar=other)) == nat.CRB_EINVAL, other
        assert "gain_bar" in last_error(lib)
        assert adjoint(lib, nat, plan, grad=cotangent(nat, ref_bar=other)) == nat.CRB_EINVAL, other
        assert "ref_bar" in last_error(lib)
    assert adjoint(lib, nat, plan, grad=cotangent(nat, gain_bar=LAM)) == nat.CRB_EINVAL
    assert adjoint(lib, nat, plan, grad=cotangent(nat, gain_bar=RBAR)) == nat.CRB_EINVAL
    assert adjoint(lib, nat, plan, work=CKPT) == nat.CRB_EINVAL
    assert checkpoint(lib, plan, ckpt=X) == nat.CRB_EINVAL
    assert checkpoint(lib, plan, work=X) == nat.CRB_EINVAL
    assert checkpoint(lib, plan, work=GAIN) == nat.CRB_EINVAL


def test_batched_api_signatures_and_docstrings():
    from continuum_robot.batched import BeamEnsemble

    assert list(inspect.signature(BeamEnsemble.step_feedback_adjoint).parameters)[1:16] == [
        "n_steps", "dt", "lam_red", "gain", "reference", "x0_red", "impulse_amp", "impulse_duration", "impulse_index",
        "held_force", "t0", "record", "record_every", "lam_record", "checkpoint_every"]
    sig = inspect.signature(BeamEnsemble.rollout_feedback).parameters
    assert list(sig)[1:7] == ["x0_red", "n_steps", "dt", "gain", "reference", "impulse_amp"]
    assert {"record", "record_every", "checkpoint_every"} <= set(sig)
    assert "feedback_cotangents" in inspect.signature(BeamEnsemble.checkpoint_interval).parameters
    assert "closed loop" not in BeamEnsemble.step_adjoint_params.__doc__
