"""Bring the tip of 64 rods to a target at t = 0.1 s: find the held tip force of each rod by gradient descent through the
implicit stepper (BeamEnsemble.rollout_implicit).

64 ten-element nonlinear Nitinol rods in water, under gravity, start at rest.  Each rod is held by one constant transverse tip
force; its tip deflection at t = 0.1 s -- 1000 implicit midpoint steps of h = 1e-4 s, the horizon and step of the reference's
LSODA call sites, where explicit RK4 would need 5000 steps -- is to reach a per-rod target.  The targets are the deflections a
hidden set of forces produces, so that the best loss is known to be 0.  Every iterate is ONE differentiable rollout of the
whole horizon; loss.backward() returns dL/d force for all rods from one sweep of the stepper's discrete adjoint.
torch.optim.Adam takes the descent steps.

    python examples/reach_tip_implicit.py [--iterations 60]
"""
import argparse

import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

H, STEPS, N_ELEM, B = 1e-4, 1000, 10, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=60)
    a = ap.parse_args()
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True, enable_gravity_effects=True)
    ens = BeamEnsemble.from_dataframes([rod(N_ELEM, "nonlinear")] * B, force_params=[fp] * B)
    dev = dict(dtype=torch.float64, device=ens.device)
    tip_w = ens.n - 2                                        # (reduced index n - 2: the tip's transverse DOF)
    x0 = torch.zeros((B, 2 * ens.n), **dev)

    def tip_at_end(force):                                   # force [B] -> tip w at t = STEPS * H, [B]
        held = torch.zeros((B, ens.n), **dev)
        held[:, tip_w] = force
        return ens.rollout_implicit(x0, STEPS, H, held_force=held)[:, tip_w]

    hidden = torch.linspace(-1.0, 1.0, B, **dev)             # N
    with torch.no_grad():
        target = tip_at_end(hidden)
        scale = float(((tip_at_end(torch.zeros(B, **dev)) - target) ** 2).mean())

    force = torch.zeros(B, requires_grad=True, **dev)
    opt = torch.optim.Adam([force], lr=0.05)
    for it in range(a.iterations):
        opt.zero_grad()
        loss = ((tip_at_end(force) - target) ** 2).mean() / scale
        loss.backward()
        opt.step()
        if it % 5 == 0 or it == a.iterations - 1:
            print(f"iterate {it:3d}  relative miss {float(loss.detach()):.4e}  "
                  f"largest force error {float((force.detach() - hidden).abs().max()):.3f} N")


if __name__ == "__main__":
    main()
