#!/usr/bin/env python3
"""Generate tests/golden/g11_graded.npz: the reference's own k(q), right-hand side and a short RK4 rollout on beams whose
properties vary along the span (tests/helpers.py:graded_columns).

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_graded.py

The reference package is imported read-only from /root/reference/src.  Every golden before this one holds a beam of equal
elements, except the 7-element `hetero7`; this one pins the oracle where each element has its own constants: `taper10`
(radius 0.005 -> 0.0005, geometric) and `allcols` (radius, length, density and drag coefficient all vary, no two neighbours
equal) at 40, 100 and 256 elements, with alternating linear / nonlinear elements, with drag or gravity on.

Stored per case (vectors only): the beam columns as the reference parsed them, the force parameters, two seeded states (a
large one, where drag matters, and a small one), an
input, the reference's k(q) and dynamic_system(0, x, u) for each state, and the end state of 20 RK4 steps of 2e-5 s over the
reference's RHS from the small state under the tip impulse.  Rods of 256 elements store the small state alone.
"""
import os
import sys
import tempfile

import numpy as np

REF_SRC = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REF_SRC)

import pandas as pd  # noqa: E402
from continuum_robot.models.dynamic_beam_model import DynamicEulerBernoulliBeam  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402

from tests.helpers import COLS, graded_columns  # noqa: E402

DT, STEPS, AMP, DURATION = 2e-5, 20, 0.1, 0.01


def mixed(n):
    return ["linear", "nonlinear"] * (n // 2)


DRAG = dict(fluid_density=1000.0, enable_fluid_effects=True)
GRAV = dict(enable_gravity_effects=True)
# name -> (elements, kinds, family, ForceParams keywords)
CASES = {
    "taper10_40_nl_drag": (40, "nonlinear", "taper10", DRAG),
    "taper10_100_mixed_grav": (100, mixed(100), "taper10", GRAV),
    "taper10_256_nl_drag": (256, "nonlinear", "taper10", DRAG),
    "allcols_40_mixed_both": (40, mixed(40), "allcols", dict(DRAG, **GRAV)),
    "allcols_100_nl_drag": (100, "nonlinear", "allcols", DRAG),
    "allcols_256_lin_grav": (256, "linear", "allcols", GRAV),
}


def rk4(dyn, u_of_t, x0, dt, n_steps):
    x, t = x0.copy(), 0.0
    for _ in range(n_steps):
        th, t1 = t + 0.5 * dt, t + dt
        k1 = dyn(t, x, u_of_t(t))
        k2 = dyn(th, x + (0.5 * dt) * k1, u_of_t(th))
        k3 = dyn(th, x + (0.5 * dt) * k2, u_of_t(th))
        k4 = dyn(t1, x + dt * k3, u_of_t(t1))
        x = x + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        t = t1
    return x


def main():
    out, names = {}, []
    for name, (n_e, kinds, family, kw) in CASES.items():
        cols = graded_columns(n_e, kinds, family)
        f = tempfile.NamedTemporaryFile(mode="w", delete=False, suffix=".csv")
        pd.DataFrame({c: cols[c] for c in COLS})[COLS].to_csv(f, index=False)
        f.close()
        try:
            parsed = pd.read_csv(f.name)
            beam = DynamicEulerBernoulliBeam(f.name, force_params=ForceParams(**kw))
        finally:
            os.unlink(f.name)
        for c in COLS:   # as the reference parsed them (pandas' float parser is not round-trip exact)
            v = parsed[c].to_numpy()
            out[f"{name}/{c}"] = v.astype(str) if c in ("type", "boundary_condition") else v.astype(np.float64)
        fp = ForceParams(**kw)
        out[f"{name}/fluid_density"] = np.float64(fp.fluid_density)
        out[f"{name}/enable_fluid"] = np.int32(fp.enable_fluid_effects)
        out[f"{name}/gravity"] = fp.get_gravity_vector()
        out[f"{name}/enable_gravity"] = np.int32(fp.enable_gravity_effects)
        beam.create_system_func()
        beam.create_input_func()
        dyn = beam.get_dynamic_system()
        kfun = beam.beam_model.get_stiffness_function()
        n = beam.beam_model.M.shape[0]
        axial = np.array([beam.beam_model.dof_to_node_param[i][0] == "u" for i in range(n)])
        rng = np.random.default_rng(1100 + n_e + len(names))
        # state 0: the size of g34's states (drag matters); state 1: SURVEY 8(d)'s small start, axial DOFs at rest
        x_big = rng.normal(0.0, 1e-2, 2 * n)
        x_big[n:] *= 50.0
        q, v = rng.normal(0.0, 1e-5, n), rng.normal(0.0, 1e-3, n)
        q[axial], v[axial] = 0.0, 0.0
        # (rods of 256 elements store the small state alone: seeded vectors do not compress)
        X = np.stack([x_big, np.concatenate([q, v])]) if n_e < 256 else np.concatenate([q, v])[None]
        u = rng.normal(0.0, 1.0, n)
        out[f"{name}/x"] = X
        out[f"{name}/u"] = u
        out[f"{name}/k_q"] = np.array([np.asarray(kfun(x[:n]), dtype=np.float64) for x in X])
        out[f"{name}/xdot"] = np.array([np.asarray(dyn(0.0, x, u), dtype=np.float64) for x in X])

        def u_of_t(t, n=n):
            w = np.zeros(n)
            if t < DURATION:
                w[-2] = AMP
            return w

        xT = rk4(dyn, u_of_t, X[-1], DT, STEPS)
        assert np.all(np.isfinite(xT))
        out[f"{name}/x_end"] = xT
        names.append(name)
        print(f"{name:26s} n={n:4d} |k|={np.max(np.abs(out[f'{name}/k_q'])):.2e} |xdot|={np.max(np.abs(out[f'{name}/xdot'])):.2e} "
              f"tip w @{STEPS} = {xT[n - 2]!r}")
    out["cases"] = np.array(names)
    out["dt"], out["steps"], out["amp"], out["duration"] = np.float64(DT), np.int32(STEPS), np.float64(AMP), np.float64(DURATION)
    np.savez_compressed(os.path.join(HERE, "g11_graded.npz"), **out)


if __name__ == "__main__":
    main()
