"""Adjoint rollouts at scale: the checkpoint pass, the per-segment recompute and the backward sweep of
crb_step_rk4_adjoint next to crb_step_rk4_tangent on the same plan (4096 x 256-node nonlinear rods with drag, 20 steps, one
cotangent), and the full gradient of a scalar loss of 64 six-element rods over 1000 steps in one adjoint, next to the
36-direction tangent state-transition matrix.  Wall time per call with HIP events after a warm-up; the kernel times of
record come from a rocprofv3 run of the same script (crb_adj_kernel<double, 1> = checkpoint pass and recompute,
<double, 2> = backward sweep).

    timeout -k 10 600 python profiles/exp_adjoint.py [--json out.json]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/exp_adjoint.py --reps 3
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "continuum-robot_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from continuum_robot.batched import BeamEnsemble  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402
from tests.helpers import nitinol_columns  # noqa: E402

DT = 2e-5


def timed(fn, reps):
    fn()   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def large(reps, steps):
    cols = nitinol_columns(256, "nonlinear")
    B = 4096
    ens = BeamEnsemble(cols, B, force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    amps = torch.linspace(0.1, 0.5, B, dtype=torch.float64, device=ens.device)
    lam = torch.zeros((B, 2 * ens.n), dtype=torch.float64, device=ens.device)
    lam[:, ens.n - 2] = 1.0
    x0 = torch.zeros_like(lam)
    every = ens.checkpoint_interval(steps)
    plain = timed(lambda: ens.step(steps, DT, impulse_amp=amps, t0=0.0), reps)
    tangent = timed(lambda: ens.step_tangent(steps, DT, lam, impulse_amp=amps, t0=0.0), reps)
    adjoint = timed(lambda: ens.step_adjoint(steps, DT, lam, x0_red=x0, impulse_amp=amps, t0=0.0), reps)
    return dict(case="4096 x 256 nonlinear + drag, 1 cotangent", steps=steps, checkpoint_every=every,
                step_rk4_us_per_step=1e3 * plain / steps, step_tangent_us_per_step=1e3 * tangent / steps,
                step_adjoint_us_per_step=1e3 * adjoint / steps)


def small(reps, steps):
    cols = nitinol_columns(6, "nonlinear")
    B = 64
    ens = BeamEnsemble(cols, B, force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    n2 = 2 * ens.n
    seeds = torch.eye(n2, dtype=torch.float64, device=ens.device)[:, None, :].expand(n2, B, n2).contiguous()
    amps = torch.linspace(0.05, 0.5, B, dtype=torch.float64, device=ens.device)
    lam = torch.zeros((B, n2), dtype=torch.float64, device=ens.device)
    lam[:, ens.n - 2] = 1.0
    x0 = torch.zeros_like(lam)
    tangent = timed(lambda: ens.step_tangent(steps, DT, seeds, impulse_amp=amps, t0=0.0), reps)
    adjoint = timed(lambda: ens.step_adjoint(steps, DT, lam, x0_red=x0, impulse_amp=amps, t0=0.0), reps)
    return dict(case="64 x 6 nonlinear + drag, gradient of a scalar loss (x0, amplitude, held force)", steps=steps,
                checkpoint_every=ens.checkpoint_interval(steps), step_tangent_stm_ms=tangent, step_adjoint_ms=adjoint)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = [large(a.reps, 20), small(a.reps, 1000)]
    for r in out:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
