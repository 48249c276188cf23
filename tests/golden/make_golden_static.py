#!/usr/bin/env python3
"""Generate tests/golden/g10_static.npz: static equilibria pinned by the reference's own force functions.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_static.py

The reference package is imported read-only from /root/reference/src.  An equilibrium is the q at which its dynamic
system has zero acceleration at v = 0:

    r(q) = k(q) - g([q; 0]) - u = 0

k = EulerBernoulliBeam.get_stiffness_function() (euler_bernoulli_beam.py:163-219), g = the registered GravityForce's
compute_forces (gravity_forces.py:97-146), u = a held generalised force.  The solve below is OURS (the reference has no
static solver): Newton with a central-difference Jacobian along the load path H(q, lam) = r(q) - (1 - lam) r(q0),
lam = 0 -> 1 in equal increments from q0 = 0, an increment halved when it does not converge -- the homotopy
crb_solve_static runs, so both return the equilibrium reached along the same path.  Converged to
|r|inf <= 1e-11 max(|k|inf, |g + u|inf) (RTOL; 1e-10 for the 40-element rod).

Cases: the examples' 1.5 m Nitinol rod (examples/example_utilities.py:25-34 materials) in 6 and 10 elements, linear and
nonlinear, gravity only and gravity plus 5 N / 50 N tip loads (50 N diverges from q = 0 in one step: continuation); a
mixed linear / nonlinear rod; a rod PINNED at the root and at an interior node; a 40-element rod.  Stored: the beam
columns as the reference parsed them, the load, the increments and the solution (data only).
"""
import os
import sys
import tempfile

import numpy as np

REF_SRC = "/root/reference/src"
sys.dont_write_bytecode = True
sys.path.insert(0, REF_SRC)

import pandas as pd  # noqa: E402
from continuum_robot.models.dynamic_beam_model import DynamicEulerBernoulliBeam  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ["length", "elastic_modulus", "moment_inertia", "density", "cross_area", "type", "boundary_condition",
        "wetted_area", "drag_coef"]
TOTAL_LENGTH = 1.5
LOAD_STEPS = 8
# the fp64 floor of the reference residual: 1e-12 .. 7e-12 at 10 elements (condition 4e7), above 1e-11 at 40
RTOL = 1e-11
RTOL_LONG = 1e-10   # rods of more than 10 elements


def rod(n, kinds, bcs=None):
    r = 0.005
    L = TOTAL_LENGTH / n
    kinds = [kinds] * n if isinstance(kinds, str) else list(kinds)
    return pd.DataFrame({
        "length": [L] * n, "elastic_modulus": [75e9] * n, "moment_inertia": [np.pi * r**4 / 4] * n,
        "density": [6450.0] * n, "cross_area": [np.pi * r**2] * n, "type": kinds,
        "boundary_condition": bcs or (["FIXED"] + ["NONE"] * (n - 1)),
        "wetted_area": [2 * np.pi * r * L] * n, "drag_coef": [0.82] * n,
    })


def cases():
    out = []
    for n in (6, 10):
        for kind in ("linear", "nonlinear"):
            for tip in (0.0, 5.0, 50.0):
                out.append((f"{kind[:3]}{n}_tip{int(tip)}", rod(n, kind), tip))
    out.append(("mixed6_tip5", rod(6, ["linear"] * 3 + ["nonlinear"] * 3), 5.0))
    out.append(("nl6_pinned0_pinned3_tip5", rod(6, "nonlinear", ["PINNED", "NONE", "NONE", "PINNED", "NONE", "NONE"]), 5.0))
    out.append(("nl40_tip5", rod(40, "nonlinear"), 5.0))
    return out


def newton_homotopy(res, n, rtol, load_steps=LOAD_STEPS, max_iter=40):
    """res(q) -> (r, scale); Newton with a central-difference Jacobian along H = r(q) - (1 - lam) r(0)"""
    q = np.zeros(n)
    r0, _ = res(q)
    lam, dlam, nominal, iters, halv = 0.0, 1.0 / load_steps, 1.0 / load_steps, 0, 0
    while True:
        lt = 1.0 if dlam >= 1.0 - lam else lam + dlam
        qs = q.copy()
        ok = False
        for _ in range(max_iter + 1):
            r, scale = res(q)
            H = r - (1.0 - lt) * r0
            if not np.all(np.isfinite(H)):
                break
            if np.max(np.abs(H)) <= rtol * scale:
                ok = True
                break
            J = np.empty((n, n))
            for j in range(n):
                h = 1e-7 * max(1e-3, abs(q[j]))
                e = np.zeros(n)
                e[j] = h
                J[:, j] = (res(q + e)[0] - res(q - e)[0]) / (2 * h)
            q = q - np.linalg.solve(J, H)
            iters += 1
        if ok:
            lam, halv = lt, 0
            if lam >= 1.0:
                r, scale = res(q)
                return q, iters, float(np.max(np.abs(r)) / scale)
            dlam = min(2 * dlam, nominal, 1.0 - lam)
        else:
            halv += 1
            if halv > 6:
                raise RuntimeError("no convergence")
            dlam *= 0.5
            q = qs


def main():
    out = {}
    names = []
    for name, df, tip in cases():
        f = tempfile.NamedTemporaryFile(mode="w", delete=False, suffix=".csv")
        df[COLS].to_csv(f, index=False)
        f.close()
        try:
            parsed = pd.read_csv(f.name)
            beam = DynamicEulerBernoulliBeam(f.name, force_params=ForceParams(enable_gravity_effects=True))
        finally:
            os.unlink(f.name)
        kfun = beam.beam_model.get_stiffness_function()
        grav = [g for g in beam.force_registry.get_registered_forces() if type(g).__name__ == "GravityForce"][0]
        n = beam.beam_model.M.shape[0]
        u = np.zeros(n)
        u[-2] = -tip   # tip w of the cantilever's last node (reduced ordering [.., u, w, phi])

        def res(q):
            k = np.asarray(kfun(q), dtype=np.float64)
            gu = np.asarray(grav.compute_forces(np.concatenate([q, np.zeros(n)]), 0.0), dtype=np.float64) + u
            return k - gu, max(np.max(np.abs(k)), np.max(np.abs(gu)))

        q, iters, rel = newton_homotopy(res, n, RTOL if len(parsed) <= 10 else RTOL_LONG)
        for c in COLS:
            v = parsed[c].to_numpy()
            out[f"{name}/{c}"] = v.astype(str) if c in ("type", "boundary_condition") else v.astype(np.float64)
        out[f"{name}/u"] = u
        out[f"{name}/gravity"] = ForceParams(enable_gravity_effects=True).get_gravity_vector()
        out[f"{name}/load_steps"] = np.int32(LOAD_STEPS)
        out[f"{name}/q"] = q
        out[f"{name}/iters"] = np.int32(iters)
        out[f"{name}/residual"] = np.float64(rel)
        names.append(name)
        print(f"{name:28s} n={n:3d} iters={iters:3d} residual={rel:.1e} max|w|={np.max(np.abs(q[1::3])):.3f} "
              f"max|phi|={np.max(np.abs(q[2::3])):.3f}")
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "g10_static.npz"), **out)


if __name__ == "__main__":
    main()
