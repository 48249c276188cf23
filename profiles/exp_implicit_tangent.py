"""The tangent of the implicit stepper at scale: per case -- 4096 x 256 nonlinear rods with drag, 1 direction, 40
steps; 64 x 10 with the 2n identity directions, 1000 steps; h = 1e-4, n_iter = 2 -- the time of
  (a) step_implicit_tangent (crb_step_implicit_tangent: the base and every direction in one launch),
  (b) step_implicit on the same ensemble (the kernel it picks by default), in the same run,
  (c) what a central difference costs instead: two step_implicit rollouts per direction.
HIP events after a warm-up, median of 5, all five kept.

    timeout -k 10 600 python profiles/exp_implicit_tangent.py [--json profiles/implicit_tangent_times.json]
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

H, N_ITER, REPS = 1e-4, 2, 5


def timed(fn):
    """(median, all REPS) in ms"""
    fn()   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(m) for m in ms]


def case(B, n_elem, steps, identity):
    cols = nitinol_columns(n_elem, "nonlinear")
    ens = BeamEnsemble(cols, B, force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    n = ens.n
    amps = np.linspace(0.1, 0.5, B)
    D = 2 * n if identity else 1
    if identity:
        dx0 = torch.eye(2 * n, dtype=torch.float64, device=ens.device)[:, None, :].expand(D, B, 2 * n).contiguous()
    else:
        dx0 = torch.zeros((1, B, 2 * n), dtype=torch.float64, device=ens.device)
        dx0[:, :, n - 2] = 1.0
    out = dict(case=f"{B} x {n_elem} nonlinear + drag, h = {H}, n_iter = {N_ITER}, {steps} steps, {D} direction(s)", steps=steps,
               directions=D)

    def tangent():
        ens.zero_state()
        ens.step_implicit_tangent(steps, H, dx0, n_iter=N_ITER, impulse_amp=amps, t0=0.0)

    def plain():
        ens.zero_state()
        ens.step_implicit(steps, H, n_iter=N_ITER, impulse_amp=amps, t0=0.0)

    def differences():
        for _ in range(2 * D):
            plain()

    for key, fn in (("step_implicit_tangent", tangent), ("step_implicit", plain), ("central_difference_rollouts", differences)):
        med, ms = timed(fn)
        out[f"{key}_ms"] = med
        out[f"{key}_ms_all"] = ms
    out["tangent_over_step_implicit"] = out["step_implicit_tangent_ms"] / out["step_implicit_ms"]
    out["central_difference_over_tangent"] = out["central_difference_rollouts_ms"] / out["step_implicit_tangent_ms"]
    out["tangent_us_per_step"] = 1e3 * out["step_implicit_tangent_ms"] / steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    a = ap.parse_args()
    out = [case(4096, 256, 40, False), case(64, 10, 1000, True)]
    for r in out:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
