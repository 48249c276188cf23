"""Inverse statics for many targets at once: which tip force and moment hold each rod at its own tip pose under gravity?
(BeamEnsemble.static_jvp / equilibrium)

64 eight-element nonlinear Nitinol rods hang under gravity.  Each has its own target tip pose (u, w, phi) -- here the pose a
hidden tip load produces, so that the answer is known.  Gauss-Newton: solve the equilibrium under the current load
(solve_static), take the 3 x 3 tip compliance d(tip pose) / d(tip load) from ONE static_jvp launch with three unit load
directions, and correct the load by compliance^-1 times the pose error, all 64 rods at once.  `--adam` instead descends the
pose error through the differentiable `equilibrium`, whose backward is one static_vjp launch.

    python examples/hold_pose.py [--iterations 6] [--adam]
"""
import argparse

import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

N_ELEM, B = 8, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--adam", action="store_true")
    a = ap.parse_args()
    fp = ForceParams(enable_gravity_effects=True)
    ens = BeamEnsemble.from_dataframes([rod(N_ELEM, "nonlinear")] * B, force_params=[fp] * B)
    dev = dict(dtype=torch.float64, device=ens.device)
    tip = slice(ens.n - 3, ens.n)                            # the tip's (u, w, phi) in the reduced ordering

    def held(load):                                          # tip load [B, 3] -> held force [B, n]
        u = torch.zeros((B, ens.n), **dev)
        u[:, tip] = load
        return u

    s = torch.linspace(0.0, 1.0, B, **dev)
    hidden = torch.stack([0.5 * s - 0.2, 2.0 * s - 1.0, 0.05 * (1.0 - s)], dim=1)   # N, N, N m per rod
    target = ens.solve_static(held(hidden), rtol=1e-10).q[:, tip]
    load = torch.zeros((B, 3), **dev)
    if a.adam:
        load.requires_grad_(True)
        scale = target.abs().amax(dim=0)
        opt = torch.optim.Adam([load], lr=0.05)
        for it in range(a.iterations or 200):
            opt.zero_grad()
            q, converged = ens.equilibrium(held(load), rtol=1e-10)
            loss = (((q[:, tip] - target) / scale) ** 2).mean()
            loss.backward()
            opt.step()
            if it % 20 == 0:
                print(f"iterate {it:3d}  pose loss {float(loss.detach()):.3e}  largest load error "
                      f"{float((load.detach() - hidden).abs().max()):.4f}  converged {int(converged.sum())}/{B}")
    else:
        unit = torch.zeros((3, B, ens.n), **dev)
        for k in range(3):
            unit[k, :, ens.n - 3 + k] = 1.0
        for it in range(a.iterations or 6):
            q = ens.solve_static(held(load), rtol=1e-10).q
            err = q[:, tip] - target
            compliance = ens.static_jvp(unit, q)[:, :, tip].permute(1, 2, 0)      # [B, pose, load]
            load = load - torch.linalg.solve(compliance, err.unsqueeze(2)).squeeze(2)
            print(f"iterate {it}  largest pose error {float(err.abs().max()):.3e}  largest load error "
                  f"{float((load - hidden).abs().max()):.3e}  singular tangents {int((ens.static_status != 0).sum())}")


if __name__ == "__main__":
    main()
