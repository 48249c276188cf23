"""steer_tip.py on the implicit stepper: the same tracking task -- a piecewise-constant tip-force sequence found by gradient
descent through the simulator -- at h = 1e-4 s instead of dt = 2e-5 s, a fifth of the steps for the same simulated horizon
(BeamEnsemble.rollout_implicit(control=...)).

Four 8-element nonlinear Nitinol rods in water start at rest.  The control is K tip forces per rod, each held for HOLD
implicit midpoint steps; the recorded tip deflection is to follow the trajectory a hidden force sequence produces, so that the
best loss is known to be 0.  Every iterate is ONE differentiable rollout of the whole horizon: the forward pass switches the
force inside the kernel (every interval starts its modified-Newton iteration from 0, as a call does), and loss.backward()
returns dL/d control for all K intervals from one sweep of the stepper's discrete adjoint.  At the end the wall time per
iterate is printed next to that of steer_tip.py's RK4 formulation of the same horizon, measured in the same run.

    python examples/steer_tip_implicit.py [--iterations 80]
"""
import argparse
import time

import numpy as np
import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

H, K, HOLD, EVERY, N_ELEM, B = 1e-4, 20, 4, 1, 8, 4          # 80 steps of 1e-4 s: the 8 ms of steer_tip.py's 400 RK4 steps
RK4_DT, RK4_HOLD, RK4_EVERY = 2e-5, 20, 5                    # steer_tip.py's own discretisation of the same horizon


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=80)
    a = ap.parse_args()
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True, enable_gravity_effects=False)
    ens = BeamEnsemble.from_dataframes([rod(N_ELEM, "nonlinear")] * B, force_params=[fp] * B)
    dev = dict(dtype=torch.float64, device=ens.device)
    tip_w = ens.n - 2                                        # (reduced index n - 2: the tip's transverse DOF)
    x0 = torch.zeros((B, 2 * ens.n), **dev)

    def tip_trajectory(force, rk4=False):                    # force [K, B] -> recorded tip w [B, K * HOLD / EVERY]
        control = torch.zeros((K, B, ens.n), **dev)
        control[:, :, tip_w] = force
        if rk4:
            return ens.rollout(x0, K * RK4_HOLD, RK4_DT, control=control, control_hold=RK4_HOLD, record=(ens.n_elem, "w"),
                               record_every=RK4_EVERY)[1]
        return ens.rollout_implicit(x0, K * HOLD, H, control=control, control_hold=HOLD, record=(ens.n_elem, "w"),
                                    record_every=EVERY)[1]

    k = torch.arange(K, **dev)[:, None]
    hidden = 0.5 * torch.sin(2.0 * np.pi * (k + 0.5) / K) * torch.linspace(0.6, 1.2, B, **dev)[None]   # N, per interval and rod

    def iterate(force, opt, target, scale, rk4=False):
        opt.zero_grad()
        loss = ((tip_trajectory(force, rk4) - target) ** 2).mean() / scale
        loss.backward()
        opt.step()
        return loss

    def wall_time(rk4, n=20):                                # seconds per iterate, after a warm-up
        with torch.no_grad():
            target = tip_trajectory(hidden, rk4)
        scale = float((target ** 2).mean())
        force = torch.zeros((K, B), requires_grad=True, **dev)
        opt = torch.optim.Adam([force], lr=0.05)
        iterate(force, opt, target, scale, rk4)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            iterate(force, opt, target, scale, rk4)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n

    with torch.no_grad():
        target = tip_trajectory(hidden)
    scale = float((target ** 2).mean())
    force = torch.zeros((K, B), requires_grad=True, **dev)
    opt = torch.optim.Adam([force], lr=0.05)
    for it in range(a.iterations):
        loss = iterate(force, opt, target, scale)
        if it % 5 == 0 or it == a.iterations - 1:
            print(f"iterate {it:3d}  relative tracking loss {float(loss.detach()):.4e}  "
                  f"largest force error {float((force.detach() - hidden).abs().max()):.3f} N")
    t_imp, t_rk4 = wall_time(False), wall_time(True)
    print(f"wall time per iterate: implicit, {K * HOLD} steps of h = {H:g} s: {1e3 * t_imp:.2f} ms   "
          f"RK4 (steer_tip.py), {K * RK4_HOLD} steps of dt = {RK4_DT:g} s: {1e3 * t_rk4:.2f} ms")


if __name__ == "__main__":
    main()
