"""Tune an LQR gain on the nonlinear rod by gradient descent through the closed loop (BeamEnsemble.rollout_feedback).

The reference designs a full-state LQR on the LINEAR model and then runs it on the rod (examples/lqr_control.py:46-125).  Here
that gain is the starting point: 64 copies of a 6-element NONLINEAR Nitinol rod in water are each hit by their own tip impulse,
the controller u = K (0 - x) acts in every Runge-Kutta stage, and the cost is the mean squared tip deflection over the samples
recorded after the impulse has ended -- how well the tip settles.  Every iterate is ONE differentiable closed-loop rollout of the
whole ensemble; loss.backward() returns dL/dK for all 18 x 36 gain entries from one adjoint sweep (central differences would
take 1296 rollouts), and plain gradient descent with a fixed step does the rest.

    python examples/tune_gain.py [--iterations 20]
"""
import argparse

import numpy as np
import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.control import LinearQuadraticRegulator
from continuum_robot.models.force_params import ForceParams

DT, STEPS, EVERY, N_ELEM, B = 5e-6, 1600, 20, 6, 64     # 8 ms of closed loop, a tip sample every 0.1 ms
IMPULSE_S = 2e-3                                        # the disturbance acts for the first 2 ms


def lqr_gain():
    """the gain of lqr_control.py:46-84 for the linear rod: Q = diag(100 I, 10 I), R = I"""
    lin = BeamEnsemble(rod(N_ELEM, "linear"), 1)
    K, M = lin.plan.stiffness(), lin.plan.mass()
    n = K.shape[0]
    Q = np.eye(2 * n)
    Q[:n, :n] *= 100.0
    Q[n:, n:] *= 10.0
    return LinearQuadraticRegulator(K, M, Q, np.eye(n)).compute_gain_matrix()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--step", type=float, default=0.05, help="first update as a fraction of the gain's norm")
    a = ap.parse_args()
    ens = BeamEnsemble(rod(N_ELEM, "nonlinear"), B, force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    dev = dict(dtype=torch.float64, device=ens.device)
    gain = torch.as_tensor(lqr_gain(), **dev).requires_grad_(True)
    amps = torch.linspace(0.5, 2.0, B, **dev)            # N, one disturbance amplitude per rod
    x0 = torch.zeros((B, 2 * ens.n), **dev)
    settled = torch.arange(STEPS // EVERY, device=ens.device) * EVERY * DT >= IMPULSE_S

    def settling_cost(K):
        _, tip = ens.rollout_feedback(x0, STEPS, DT, K, impulse_amp=amps, impulse_duration=IMPULSE_S, record=(ens.n_elem, "w"),
                                      record_every=EVERY)
        return (tip[:, settled] ** 2).mean()

    rate = None
    for it in range(a.iterations + 1):
        gain.grad = None
        loss = settling_cost(gain)
        if not torch.isfinite(loss):
            raise SystemExit(f"iterate {it}: the closed loop left the finite range; lower --step")
        cost = float(loss.detach())
        if it == 0:
            first = cost
        print(f"iterate {it:3d}  tip-settling cost {cost:.6e}  ({cost / first:.3f} of the LQR gain's)")
        if it == a.iterations:
            break
        loss.backward()
        if rate is None:    # a fixed step: the first update moves the gain by --step of its norm
            rate = a.step * float(gain.detach().norm() / gain.grad.norm())
        with torch.no_grad():
            gain -= rate * gain.grad


if __name__ == "__main__":
    main()
