"""CPU checks of the implicit stepper's adjoint (crb_implicit_adjoint.h): the entry points are declared in include/crbeam.h,
exported and bound, the work-buffer size follows its documented formula, and every refusal shows on a host-only plan in the
documented order (CRB_EINVAL, then CRB_EUNSUPPORTED, then CRB_ENODEV), naming the entry point and leaving *t_end alone."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.helpers import nitinol_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_implicit_adjoint_work_bytes", "crb_step_implicit_checkpoint", "crb_step_implicit_adjoint")
p = C.c_void_p


def test_symbols_are_declared_exported_and_bound():
    from continuum_robot import _native as nat
    from continuum_robot.batched import BeamEnsemble

    hdr = open(os.path.join(ROOT, "include", "crbeam.h")).read()
    lib = nat.load()
    for name in NAMES:
        assert re.search(rf"\b(int|size_t) {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.crb_implicit_adjoint_work_bytes.restype is C.c_size_t
    assert lib.crb_version() == int(re.search(r"#define CRB_VERSION (\d+)", hdr).group(1))
    assert list(inspect.signature(BeamEnsemble.step_implicit_adjoint).parameters)[1:] == [
        "n_steps", "h", "lam_red", "n_iter", "x0_red", "impulse_amp", "impulse_duration", "impulse_index", "held_force", "t0",
        "record", "record_every", "lam_record", "checkpoint_every"]
    assert list(inspect.signature(BeamEnsemble.rollout_implicit).parameters)[1:5] == ["x0_red", "n_steps", "h", "n_iter"]
    assert "implicit" in inspect.signature(BeamEnsemble.checkpoint_interval).parameters


def test_work_bytes_formula_on_host_only_plans():
    from continuum_robot import _native as nat

    lib = nat.load()
    for n, B in ((4, 1), (6, 3), (200, 5)):
        plan = nat.Plan(nitinol_columns(n, "nonlinear"), n_beams=B, device=-1)
        force = B * (n + 1) * 4                       # doubles of one [B][n_node][4] record
        for every in (1, 7, 32):
            for n_iter in (1, 2, 16):
                for n_cot in (1, 5, 65535):
                    want = (every * ((2 + n_iter) * force + 1) + n_cot * force) * 8
                    assert lib.crb_implicit_adjoint_work_bytes(plan.h, every, n_iter, n_cot) == want, (n, B, every, n_iter, n_cot)
        for bad in ((0, 2, 1), (-3, 2, 1), (4, 0, 1), (4, 17, 1), (4, 2, 0), (4, 2, 65536)):
            assert lib.crb_implicit_adjoint_work_bytes(plan.h, *bad) == 0, bad
    assert lib.crb_implicit_adjoint_work_bytes(None, 4, 2, 1) == 0


def _calls(lib, plan):
    h = plan.h if plan is not None else None

    def ckp(x=p(8), ckpt=p(16), h_=1e-4, n_steps=10, n_iter=2, every=3, t_end=None):
        return lib.crb_step_implicit_checkpoint(h, x, 0.0, h_, n_steps, n_iter, every, None, None, ckpt, t_end, None)

    def adj(ckpt=p(8), lam=p(16), n_cot=1, h_=1e-4, n_steps=10, n_iter=2, every=3, work=p(32), grad=None):
        return lib.crb_step_implicit_adjoint(h, ckpt, lam, n_cot, 0.0, h_, n_steps, n_iter, every, None, None, grad, work, None)

    return ckp, adj


def test_null_plan_is_invalid():
    from continuum_robot import _native as nat

    lib = nat.load()
    ckp, adj = _calls(lib, None)
    assert ckp() == nat.CRB_EINVAL
    assert "crb_step_implicit_checkpoint" in lib.crb_last_error().decode()
    assert adj() == nat.CRB_EINVAL
    assert "crb_step_implicit_adjoint" in lib.crb_last_error().decode()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_in_order_before_the_device(dtype):
    """CRB_EINVAL (NULL pointers, aliasing, n_cot, every, n_iter, h) before CRB_EUNSUPPORTED (fp32) before CRB_ENODEV: an fp32
    host-only plan shows the first two classes in that order, an fp64 one the first and the last"""
    from continuum_robot import _native as nat

    plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=2, device=-1, dtype=dtype)
    lib = nat.load()
    ckp, adj = _calls(lib, plan)
    t_end = C.c_double(-1.0)
    te = C.byref(t_end)

    def refused(rc, code, *words):
        assert rc == code, (rc, code, lib.crb_last_error().decode())
        msg = lib.crb_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)
        assert t_end.value == -1.0

    inval = nat.CRB_EINVAL
    # -- the checkpoint pass
    refused(ckp(x=None, t_end=te), inval, "crb_step_implicit_checkpoint", "null")
    refused(ckp(ckpt=None, t_end=te), inval, "crb_step_implicit_checkpoint", "null")
    refused(ckp(ckpt=p(8), t_end=te), inval, "crb_step_implicit_checkpoint", "alias")
    refused(ckp(n_steps=-1, t_end=te), inval, "crb_step_implicit_checkpoint", "n_steps")
    for every in (0, -2):
        refused(ckp(every=every, t_end=te), inval, "crb_step_implicit_checkpoint", "every")
    for n_iter in (0, -1, 17):
        refused(ckp(n_iter=n_iter, t_end=te), inval, "crb_step_implicit_checkpoint", "n_iter")
    for h_ in (0.0, -1e-4, float("nan")):
        refused(ckp(h_=h_, t_end=te), inval, "crb_step_implicit_checkpoint", "h must")
    # -- the adjoint
    refused(adj(ckpt=None), inval, "crb_step_implicit_adjoint", "null")
    refused(adj(lam=None), inval, "crb_step_implicit_adjoint", "null")
    refused(adj(work=None), inval, "crb_step_implicit_adjoint", "work")
    refused(adj(work=p(16)), inval, "crb_step_implicit_adjoint", "alias")          # lam aliasing the work buffer
    refused(adj(ckpt=p(16)), inval, "crb_step_implicit_adjoint", "alias")          # lam aliasing the checkpoints
    refused(adj(work=p(8)), inval, "crb_step_implicit_adjoint", "alias")           # the work buffer aliasing the checkpoints
    grad = nat.InputCotangent()
    grad.f_held_bar = 32
    refused(adj(grad=C.byref(grad)), inval, "crb_step_implicit_adjoint", "alias")  # f_held_bar aliasing the work buffer
    for n_cot in (0, -1, 65536):
        refused(adj(n_cot=n_cot), inval, "crb_step_implicit_adjoint", "n_cot")
    refused(adj(n_steps=-1), inval, "crb_step_implicit_adjoint", "n_steps")
    for every in (0, -2):
        refused(adj(every=every), inval, "crb_step_implicit_adjoint", "every")
    for n_iter in (0, 17):
        refused(adj(n_iter=n_iter), inval, "crb_step_implicit_adjoint", "n_iter")
    refused(adj(h_=0.0), inval, "crb_step_implicit_adjoint", "h must")
    grad = nat.InputCotangent()
    grad.amp_bar = 64
    refused(adj(grad=C.byref(grad)), inval, "crb_step_implicit_adjoint", "amp_bar")   # no impulse input
    # -- the order: several faults at once report the earliest class, and within CRB_EINVAL the earliest argument
    refused(adj(n_cot=0, every=0, n_iter=0, h_=0.0), inval, "n_cot")
    refused(adj(every=0, n_iter=0, h_=0.0), inval, "every")
    refused(adj(n_iter=0, h_=0.0), inval, "n_iter")
    refused(ckp(every=0, n_iter=0, h_=0.0, t_end=te), inval, "every")
    # -- valid arguments
    if dtype == "f32":
        refused(ckp(t_end=te), nat.CRB_EUNSUPPORTED, "crb_step_implicit_checkpoint", "fp64")
        refused(adj(), nat.CRB_EUNSUPPORTED, "crb_step_implicit_adjoint", "fp64")
    else:
        refused(ckp(t_end=te), nat.CRB_ENODEV, "crb_step_implicit_checkpoint", "host-only")
        refused(adj(), nat.CRB_ENODEV, "crb_step_implicit_adjoint", "host-only")


def test_more_than_256_thread_carried_nodes_are_unsupported_before_the_device():
    from continuum_robot import _native as nat

    plan = nat.Plan(nitinol_columns(300, "linear"), n_beams=1, device=-1)
    lib = nat.load()
    ckp, adj = _calls(lib, plan)
    assert ckp(every=0) == nat.CRB_EINVAL                       # (CRB_EINVAL still comes first)
    assert ckp() == nat.CRB_EUNSUPPORTED
    assert "crb_step_implicit_checkpoint" in lib.crb_last_error().decode() and "256" in lib.crb_last_error().decode()
    assert adj() == nat.CRB_EUNSUPPORTED
    assert "crb_step_implicit_adjoint" in lib.crb_last_error().decode() and "256" in lib.crb_last_error().decode()
