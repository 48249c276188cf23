"""The adjoint of the implicit stepper at scale: per case -- 4096 x 256 and 64 x 10 nonlinear rods with drag,
h = 1e-4, n_iter = 2 --
  (a) time per step of the checkpoint pass (crb_step_implicit_checkpoint) and of crb_step_implicit_adjoint (per segment: the
      recompute launch and the sweep) for 1, 4 and 8 cotangents, next to step_implicit through the general kernel
      (CRB_DISABLE_LEAN_IMPLICIT) and through the kernel it picks by default, in the same run;
  (b) wall time of one gradient (checkpoint pass + adjoint, one cotangent) per simulated second, next to step_adjoint (RK4) at
      dt = 2e-5 on the same ensemble.
Wall time per call with HIP events after a warm-up, median of --reps.  (c) the kernel-time breakdown comes from a rocprofv3 run
of the same script (crb_imp_adj_kernel<double, 0> = checkpoint pass, <double, 1> = recompute, <double, 2> = sweep).

    timeout -k 10 600 python profiles/exp_implicit_adjoint.py [--json out.json]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/exp_implicit_adjoint.py --reps 2
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

from continuum_robot.batched import _IMPLICIT, BeamEnsemble  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402
from tests.helpers import nitinol_columns  # noqa: E402

H, DT, N_ITER = 1e-4, 2e-5, 2


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


def case(B, n_elem, steps, reps):
    cols = nitinol_columns(n_elem, "nonlinear")
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True)
    dev = dict(dtype=torch.float64)
    amps = np.linspace(0.1, 0.5, B)
    out = dict(case=f"{B} x {n_elem} nonlinear + drag, h = {H}, n_iter = {N_ITER}", steps=steps)
    # step_implicit: the general kernel (a plan of its own, so that its tables of A are built under the switch), then the default
    os.environ["CRB_DISABLE_LEAN_IMPLICIT"] = "1"
    gen = BeamEnsemble(cols, B, force_params=fp)
    out["step_implicit_general_us_per_step"] = 1e3 * timed(
        lambda: (gen.zero_state(), gen.step_implicit(steps, H, n_iter=N_ITER, impulse_amp=amps, t0=0.0)), reps) / steps
    del os.environ["CRB_DISABLE_LEAN_IMPLICIT"]
    del gen
    ens = BeamEnsemble(cols, B, force_params=fp)
    out["step_implicit_default_us_per_step"] = 1e3 * timed(
        lambda: (ens.zero_state(), ens.step_implicit(steps, H, n_iter=N_ITER, impulse_amp=amps, t0=0.0)), reps) / steps
    # (a) the two calls of a gradient, separately
    desc, keep = ens._input_desc(amps, 0.01, -2, None)
    every = ens.checkpoint_interval(steps, None, implicit=(N_ITER, 8))
    out["checkpoint_every"] = every
    x0 = torch.zeros_like(ens.state)
    x = x0.clone()

    def ckpt_pass():
        x.copy_(x0)
        return ens._checkpoint_pass(_IMPLICIT, x, steps, 0.0, (H, N_ITER), desc, every, None)

    out["checkpoint_pass_us_per_step"] = 1e3 * timed(ckpt_pass, reps) / steps
    ckpt = ckpt_pass()
    for D in (1, 4, 8):
        lam0 = torch.zeros((D, B, 2 * ens.n), device=ens.device, **dev)
        lam0[:, :, ens.n - 2] = 1.0
        lamd0 = ens._pack_dirs(lam0, True)
        lamd = lamd0.clone()

        def sweep():
            lamd.copy_(lamd0)
            ens._sweep(_IMPLICIT, ckpt, lamd, steps, 0.0, (H, N_ITER), desc, every, None, True)

        out[f"adjoint_{D}_cot_us_per_step"] = 1e3 * timed(sweep, reps) / steps
    # (b) one gradient per simulated second, implicit and RK4
    lam = torch.zeros((B, 2 * ens.n), device=ens.device, **dev)
    lam[:, ens.n - 2] = 1.0
    xr = torch.zeros_like(lam)
    imp = timed(lambda: ens.step_implicit_adjoint(steps, H, lam, n_iter=N_ITER, x0_red=xr, impulse_amp=amps, t0=0.0), reps)
    rk4 = timed(lambda: ens.step_adjoint(steps, DT, lam, x0_red=xr, impulse_amp=amps, t0=0.0), reps)
    out["implicit_gradient_s_per_simulated_s"] = 1e-3 * imp / (steps * H)
    out["rk4_gradient_s_per_simulated_s"] = 1e-3 * rk4 / (steps * DT)
    out["rk4_step_adjoint_us_per_step"] = 1e3 * rk4 / steps
    out["rk4_over_implicit"] = out["rk4_gradient_s_per_simulated_s"] / out["implicit_gradient_s_per_simulated_s"]
    del keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = [case(4096, 256, 40, a.reps), case(64, 10, 1000, a.reps)]
    for r in out:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
