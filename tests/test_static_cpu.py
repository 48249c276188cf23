"""CPU checks of the static-equilibrium feature: the golden equilibria against the C oracle, and the refusal of a
host-only plan by both new entry points (crb_tangent_stiffness, crb_solve_static)."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import Golden, beam_columns, oracle_beam

G = Golden()


def static_cases():
    return [str(c) for c in G["g10_static"]["cases"]]


def oracle_residual(z, name, q):
    ob = oracle_beam(beam_columns(z, name), enable_gravity=True, gravity=z[f"{name}/gravity"])
    k = ob.internal_force(q)
    gu = ob.gravity(np.concatenate([q, np.zeros_like(q)])) + z[f"{name}/u"]
    return np.max(np.abs(k - gu)) / max(np.max(np.abs(k)), np.max(np.abs(gu)))


@pytest.mark.parametrize("name", static_cases())
def test_golden_equilibria_satisfy_the_oracle(name):
    z = G["g10_static"]
    assert oracle_residual(z, name, z[f"{name}/q"]) <= 1e-10


def test_golden_covers_the_issue_cases():
    names = set(static_cases())
    for n in (6, 10):
        for kind in ("lin", "non"):
            assert {f"{kind}{n}_tip0", f"{kind}{n}_tip5", f"{kind}{n}_tip50"} <= names
    assert {"mixed6_tip5", "nl6_pinned0_pinned3_tip5", "nl40_tip5"} <= names


def test_host_only_plan_has_no_static_cpu_path():
    from continuum_robot import _native as nat
    from tests.helpers import nitinol_columns

    plan = nat.Plan(nitinol_columns(4, "nonlinear"), n_beams=1, device=-1)
    lib = nat.load()
    with pytest.raises(nat.NativeError, match="no CPU path"):
        nat.check(lib.crb_tangent_stiffness(plan.h, C.c_void_p(8), C.c_void_p(16), None))
    iters = C.c_void_p(24)
    with pytest.raises(nat.NativeError, match="no CPU path"):
        nat.check(lib.crb_solve_static(plan.h, C.c_void_p(8), None, 8, 20, 1e-9, 0.0, iters, None, None))
