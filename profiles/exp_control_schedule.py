"""Control schedules in the RK4 rollout family: what the schedule costs the calls without one, and what it buys.

Non-regression rows (they also run on a tree without the feature, for a back-to-back comparison with the parent commit):
  held_step      step(held_force) at 4096 x 256 nonlinear + drag, 100 steps
  adjoint_large  step_adjoint at 4096 x 256 nonlinear + drag, 20 steps, one cotangent   (the cases of profiles/exp_adjoint.py)
  adjoint_small  step_adjoint at 64 x 6 nonlinear + drag, 1000 steps, one cotangent
Feature rows:
  sched_step     4096 x 256, 100 steps: control K = 10, hold = 10 in ONE call against 10 chained step(held_force) calls
  sched_grad     64 x 6, 1000 steps, K = 100, hold = 10: rollout(control) + backward() against 100 chained rollouts + backward()
  sweep_switch   4096 x 256, 20 steps: step_adjoint with a schedule that switches after EVERY step (hold = 1) against the held
                 force -- the difference per step is what storing, moving and reloading the interval's record costs the sweep

Medians of --reps calls (default 9) with HIP events after a warm-up call; kernel times come from a rocprofv3 run of its own:

    timeout -k 10 600 python profiles/exp_control_schedule.py [--rows regression|feature|all] [--json out.json]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/exp_control_schedule.py --reps 3
"""
import argparse
import inspect
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
HAS_SCHEDULE = "control" in inspect.signature(BeamEnsemble.step).parameters


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
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def rods(n_elem, n_beams):
    ens = BeamEnsemble(nitinol_columns(n_elem, "nonlinear"), n_beams,
                       force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    dev = dict(dtype=torch.float64, device=ens.device)
    lam = torch.zeros((n_beams, 2 * ens.n), **dev)
    lam[:, ens.n - 2] = 1.0
    return ens, dev, lam


def tip_loads(ens, dev, k, seed):
    """[k, B, n]: random transverse loads"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.zeros((k, ens.n_beams, ens.n), **dev)
    u[:, :, 1::3] = (0.05 * torch.randn((k, ens.n_beams, len(range(1, ens.n, 3))), generator=g, dtype=torch.float64)).to(ens.device)
    return u


def regression(reps):
    out = {}
    ens, dev, lam = rods(256, 4096)
    amps = torch.linspace(0.1, 0.5, 4096, **dev)
    u = tip_loads(ens, dev, 1, 1)[0]
    x0 = torch.zeros_like(lam)
    out["held_step_4096x256_100_steps"] = timed(lambda: ens.step(100, DT, impulse_amp=amps, held_force=u, t0=0.0), reps)
    out["adjoint_large_4096x256_20_steps"] = timed(lambda: ens.step_adjoint(20, DT, lam, x0_red=x0, impulse_amp=amps, t0=0.0), reps)
    del ens
    ens, dev, lam = rods(6, 64)
    amps = torch.linspace(0.05, 0.5, 64, **dev)
    x0 = torch.zeros_like(lam)
    out["adjoint_small_64x6_1000_steps"] = timed(lambda: ens.step_adjoint(1000, DT, lam, x0_red=x0, impulse_amp=amps, t0=0.0), reps)
    return out


def feature(reps):
    from continuum_robot.batched import ControlSchedule

    out = {}
    ens, dev, lam = rods(256, 4096)
    amps = torch.linspace(0.1, 0.5, 4096, **dev)
    x0 = torch.zeros_like(lam)
    u = tip_loads(ens, dev, 10, 2)

    def chained():
        ens.time = 0.0
        for k in range(10):
            ens.step(10, DT, impulse_amp=amps, held_force=u[k])

    out["sched_step_4096x256_one_call"] = timed(lambda: ens.step(100, DT, impulse_amp=amps, control=u, control_hold=10, t0=0.0), reps)
    out["sched_step_4096x256_10_chained_calls"] = timed(chained, reps)
    u20 = tip_loads(ens, dev, 20, 3)
    out["sweep_held_4096x256_20_steps"] = timed(
        lambda: ens.step_adjoint(20, DT, lam, x0_red=x0, impulse_amp=amps, held_force=u20[0], t0=0.0), reps)
    out["sweep_switch_every_step_4096x256_20_steps"] = timed(
        lambda: ens.step_adjoint(20, DT, lam, x0_red=x0, impulse_amp=amps, held_force=ControlSchedule(u20, 1), t0=0.0), reps)
    del ens
    ens, dev, lam = rods(6, 64)
    amps = torch.linspace(0.05, 0.5, 64, **dev)
    u = tip_loads(ens, dev, 100, 4).requires_grad_(True)
    x0 = torch.zeros_like(lam)

    def one_rollout():
        u.grad = None
        xT = ens.rollout(x0, 1000, DT, impulse_amp=amps, control=u, control_hold=10)
        (xT * lam).sum().backward()

    def chained_rollouts():
        u.grad = None
        x, t = x0, 0.0
        for k in range(100):
            x = ens.rollout(x, 10, DT, impulse_amp=amps, held_force=u[k], t0=t)
            for _ in range(10):
                t = t + DT
        (x * lam).sum().backward()

    out["sched_grad_64x6_one_rollout_and_backward"] = timed(one_rollout, reps)
    out["sched_grad_64x6_100_chained_rollouts_and_backward"] = timed(chained_rollouts, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", default="all", choices=["regression", "feature", "all"])
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"has_schedule": HAS_SCHEDULE}
    if a.rows in ("regression", "all"):
        out["regression"] = regression(a.reps)
    if a.rows in ("feature", "all") and HAS_SCHEDULE:
        out["feature"] = feature(a.reps)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
