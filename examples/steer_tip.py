"""Steer the tip of a few rods along a target trajectory: optimise a piecewise-constant tip-force sequence by gradient descent
through the simulator (BeamEnsemble.rollout(control=...)).

Four 8-element nonlinear Nitinol rods in water start at rest.  The control is K tip forces per rod, each held for HOLD RK4 steps
(a zero-order hold, the `u` of the reference's dynamic_system(t, x, u)); the recorded tip deflection is to follow a target --
here the trajectory a hidden force sequence produces, so that the best loss is known to be 0.  Every iterate is ONE
differentiable rollout of the whole horizon: the forward pass switches the force inside the kernel, and loss.backward() returns
dL/d control for all K intervals from one adjoint sweep.  torch.optim.Adam does the rest.

    python examples/steer_tip.py [--iterations 80]
"""
import argparse

import numpy as np
import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

DT, K, HOLD, EVERY, N_ELEM, B = 2e-5, 20, 20, 5, 8, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=80)
    a = ap.parse_args()
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True, enable_gravity_effects=False)
    ens = BeamEnsemble.from_dataframes([rod(N_ELEM, "nonlinear")] * B, force_params=[fp] * B)
    dev = dict(dtype=torch.float64, device=ens.device)
    steps, tip_w = K * HOLD, ens.n - 2                       # (reduced index n - 2: the tip's transverse DOF)
    x0 = torch.zeros((B, 2 * ens.n), **dev)

    def tip_trajectory(force):                               # force [K, B] -> recorded tip w [B, steps / EVERY]
        control = torch.zeros((K, B, ens.n), **dev)
        control[:, :, tip_w] = force
        return ens.rollout(x0, steps, DT, control=control, control_hold=HOLD, record=(ens.n_elem, "w"), record_every=EVERY)[1]

    k = torch.arange(K, **dev)[:, None]
    hidden = 0.5 * torch.sin(2.0 * np.pi * (k + 0.5) / K) * torch.linspace(0.6, 1.2, B, **dev)[None]   # N, per interval and rod
    with torch.no_grad():
        target = tip_trajectory(hidden)
    scale = float((target ** 2).mean())

    force = torch.zeros((K, B), requires_grad=True, **dev)
    opt = torch.optim.Adam([force], lr=0.05)
    for it in range(a.iterations):
        opt.zero_grad()
        loss = ((tip_trajectory(force) - target) ** 2).mean() / scale
        loss.backward()
        opt.step()
        if it % 5 == 0 or it == a.iterations - 1:
            print(f"iterate {it:3d}  relative tracking loss {float(loss.detach()):.4e}  "
                  f"largest force error {float((force.detach() - hidden).abs().max()):.3f} N")


if __name__ == "__main__":
    main()
