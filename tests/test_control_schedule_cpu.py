"""CPU checks of the control schedule (crb_input_schedule): the struct and the five *_sched entry points are declared in
include/crbeam.h and exported, the ctypes mirror has the header's field order, the library's version is the header's, and
every refusal comes with its code and names its argument before the device is touched -- so host-only plans show them, and
valid arguments there give CRB_ENODEV."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.helpers import nitinol_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crb_step_rk4_sched", "crb_step_rk4_tangent_sched", "crb_step_rk4_checkpoint_sched", "crb_step_rk4_adjoint_sched",
         "crb_step_rk4_adjoint_params_sched")
P = C.c_void_p
X, DX, CK, LAM, WORK, F, FBAR, PBAR, HELD = (P(64 * k) for k in range(1, 10))   # distinct fake device addresses (never read)
STEPS, K, HOLD = 33, 5, 7


def header():
    return open(os.path.join(ROOT, "include", "crbeam.h")).read()


def test_schedule_symbols_are_declared_and_exported():
    from continuum_robot import _native as nat

    hdr, lib = header(), nat.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert hasattr(lib, name), name
    # the header cites the reference interface the schedule stands in for, as the other inputs do
    doc = hdr[hdr.index("A piecewise-constant control sequence"):hdr.index("} crb_input_schedule;")]
    assert "dynamic_beam_model.py:343-362" in doc and "lqr_control.py:33-41" in doc


def test_ctypes_struct_has_the_headers_field_order():
    from continuum_robot import _native as nat

    body = re.search(r"typedef struct crb_input_schedule \{(.*?)\} crb_input_schedule;", header(), re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+);", body, re.M)
    assert [f for _, f in fields] == ["f_sched", "n_intervals", "hold"]
    assert [t for t, _ in fields] == ["void", "int32_t", "int32_t"]
    assert [f for f, _ in nat.InputSchedule._fields_] == ["f_sched", "n_intervals", "hold"]
    assert [t for _, t in nat.InputSchedule._fields_] == [C.c_void_p, C.c_int32, C.c_int32]
    assert C.sizeof(nat.InputSchedule) == 16
    s = nat.InputSchedule(0x1000, 5, 7)
    assert (s.f_sched, s.n_intervals, s.hold) == (0x1000, 5, 7)


def test_version_is_the_headers():
    from continuum_robot import _native as nat

    declared = int(re.search(r"#define CRB_VERSION (\d+)", header()).group(1))
    assert nat.load().crb_version() == declared == 106


class Calls:
    """the five entry points on one plan, with valid fake arguments unless overridden"""

    def __init__(self, dtype):
        from continuum_robot import _native as nat

        self.nat, self.lib = nat, nat.load()
        self.plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=2, device=-1, dtype=dtype)
        self.pgrad = nat.ParamCotangent(PBAR.value)

    def sched(self, f=F.value, k=K, hold=HOLD):
        return self.nat.InputSchedule(f, k, hold)

    def step(self, s, n=STEPS, desc=None):
        return self.lib.crb_step_rk4_sched(self.plan.h, X, 0.0, 2e-5, n, desc, s, None, None, None)

    def tangent(self, s, n=STEPS, desc=None, tan=None, d_sched=None):
        return self.lib.crb_step_rk4_tangent_sched(self.plan.h, X, DX, 3, 0.0, 2e-5, n, desc, tan, s, d_sched, None, None)

    def checkpoint(self, s, n=STEPS, desc=None):
        return self.lib.crb_step_rk4_checkpoint_sched(self.plan.h, X, 0.0, 2e-5, n, 4, desc, s, None, CK, None, None)

    def adjoint(self, s, n=STEPS, desc=None, grad=None, sched_bar=FBAR, lam=LAM, work=WORK, ckpt=CK):
        return self.lib.crb_step_rk4_adjoint_sched(self.plan.h, ckpt, lam, 2, 0.0, 2e-5, n, 4, desc, None, grad, s, sched_bar,
                                                   work, None)

    def params(self, s, n=STEPS, desc=None, grad=None, sched_bar=FBAR, lam=LAM, work=WORK, ckpt=CK):
        return self.lib.crb_step_rk4_adjoint_params_sched(self.plan.h, ckpt, lam, 2, 0.0, 2e-5, n, 4, desc, None, grad,
                                                          C.byref(self.pgrad), s, sched_bar, work, None)

    def all(self):
        return (self.step, self.tangent, self.checkpoint, self.adjoint, self.params)

    def error(self):
        return self.lib.crb_last_error().decode()


def test_refusals_on_a_host_only_fp64_plan():
    c = Calls("f64")
    nat = c.nat
    held = nat.InputDesc()
    held.kind, held.f_held = nat.CRB_INPUT_NONE, HELD.value
    for call in c.all():
        what = call.__name__
        for bad, word in ((c.sched(f=None), "f_sched"), (c.sched(k=0), "n_intervals"), (c.sched(k=-3), "n_intervals"),
                          (c.sched(hold=0), "hold"), (c.sched(hold=-1), "hold")):
            assert call(C.byref(bad)) == nat.CRB_EINVAL, (what, word)
            assert word in c.error(), (what, word, c.error())
        ok = c.sched()
        assert call(C.byref(ok), n=K * HOLD + 1) == nat.CRB_EINVAL, what
        assert "n_steps" in c.error(), (what, c.error())
        assert call(C.byref(ok), desc=C.byref(held)) == nat.CRB_EINVAL, what
        assert "f_held" in c.error(), (what, c.error())
        # valid arguments: the last interval cut short, every interval used in full, and the degenerate single interval
        assert call(C.byref(ok)) == nat.CRB_ENODEV, (what, c.error())
        assert call(C.byref(ok), n=K * HOLD) == nat.CRB_ENODEV, what
        one = c.sched(k=1, hold=STEPS)
        assert call(C.byref(one)) == nat.CRB_ENODEV, what
        # without a schedule each is the existing call
        no_bar = dict(sched_bar=None) if call in (c.adjoint, c.params) else {}
        assert call(None, desc=C.byref(held), **no_bar) == nat.CRB_ENODEV, what


def test_schedule_cotangent_must_not_alias():
    c = Calls("f64")
    nat = c.nat
    ok = c.sched()
    for call in (c.adjoint, c.params):
        for kw in (dict(sched_bar=LAM), dict(sched_bar=WORK), dict(sched_bar=CK), dict(sched_bar=F)):
            assert call(C.byref(ok), **kw) == nat.CRB_EINVAL, (call.__name__, kw)
            assert "sched_bar" in c.error(), c.error()
        assert call(C.byref(ok), sched_bar=None) == nat.CRB_ENODEV          # (not wanted)
        assert call(None, sched_bar=FBAR) == nat.CRB_EINVAL                  # (a cotangent of no schedule)
        assert "sched_bar" in c.error()
        grad = nat.InputCotangent(None, HELD.value)                          # f_held_bar next to a schedule: no such input
        assert call(C.byref(ok), grad=C.byref(grad)) == nat.CRB_EINVAL
        assert "f_held_bar" in c.error()
    tan = nat.InputTangent(None, HELD.value)
    assert c.tangent(C.byref(ok), tan=C.byref(tan)) == nat.CRB_EINVAL
    assert "df_held" in c.error()
    assert c.tangent(None, d_sched=DX) == nat.CRB_EINVAL
    assert "d_sched" in c.error()
    assert c.tangent(C.byref(ok), d_sched=FBAR) == nat.CRB_ENODEV


def test_refusals_on_a_host_only_fp32_plan():
    """fp32 plans run schedules in the plain stepper only: the tangent and adjoint calls are CRB_EUNSUPPORTED"""
    c = Calls("f32")
    nat = c.nat
    ok = c.sched()
    for bad, word in ((c.sched(f=None), "f_sched"), (c.sched(k=0), "n_intervals"), (c.sched(hold=0), "hold")):
        assert c.step(C.byref(bad)) == nat.CRB_EINVAL
        assert word in c.error()
    assert c.step(C.byref(ok), n=K * HOLD + 1) == nat.CRB_EINVAL
    assert "n_steps" in c.error()
    assert c.step(C.byref(ok)) == nat.CRB_ENODEV
    for call in (c.tangent, c.checkpoint, c.adjoint, c.params):
        assert call(C.byref(ok)) == nat.CRB_EUNSUPPORTED, call.__name__
        assert "fp64" in c.error()


def test_batched_api_takes_the_schedule():
    from continuum_robot.batched import BeamEnsemble, ControlSchedule

    for method in (BeamEnsemble.step, BeamEnsemble.step_adjoint_params, BeamEnsemble.rollout):
        names = list(inspect.signature(method).parameters)
        assert names[-2:] == ["control", "control_hold"], method.__name__
    assert ControlSchedule._fields == ("control", "hold")


@pytest.mark.parametrize("kw, word", [
    (dict(control=[[[0.0] * 12] * 2] * 5, control_hold=7, held_force=[[0.0] * 12] * 2), "held_force"),
    (dict(control=[[[0.0] * 12] * 2] * 5), "control_hold"),
    (dict(control=[[[0.0] * 12] * 2] * 5, control_hold=0), "control_hold"),
    (dict(control_hold=7), "control"),
    (dict(control=[[0.0] * 12] * 2, control_hold=7), "control must be"),
    (dict(control=[[[0.0] * 11] * 2] * 5, control_hold=7), "control must be"),
    (dict(control=[[[0.0] * 12] * 2] * 4, control_hold=7), "n_steps"),
])
def test_python_argument_checks_need_no_device(kw, word):
    """BeamEnsemble._control: what step / step_tangent / step_adjoint / rollout refuse, on an object that has only the fields
    the check reads (no plan, no device)"""
    import torch

    from continuum_robot.batched import BeamEnsemble

    ens = BeamEnsemble.__new__(BeamEnsemble)
    ens.dtype, ens.device, ens.n_beams, ens.n = torch.float64, torch.device("cpu"), 2, 12
    with pytest.raises(ValueError, match=word):
        ens._control(kw.get("held_force"), kw.get("control"), kw.get("control_hold"), 33, "step")
