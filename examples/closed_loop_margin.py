"""Is the 1 kHz regulator designed on the linearisation stable on the plant the stepper applies?

examples/digital_lqr.py designs a digital LQR on `linearize_implicit`'s (A_d, B_d) of the linear rod at rest.  Here the rods are
nonlinear, in water and under gravity.  The gain still comes from scipy.linalg.solve_discrete_are on (A_d, B_d), taken about the
static equilibrium `solve_static` finds, and the regulator holds that equilibrium: u_k = K (x_eq - x_k).  What the design
promises is the spectral radius of A_d - B_d K.  What the loop does is the map `step_implicit_feedback` applies, sample to
sample, and `linearize_implicit_feedback` returns its Jacobian -- the closed loop's sampled state-transition matrix -- about any
operating point, from one call of the loop's tangent with identity seeds.  About the equilibrium the two agree (the design was
made there); about a rod deflected by a tip impulse the plant has moved -- drag is quadratic in the rate, the shipped element is
nonlinear in the deflection -- and the radius of the exact matrix is the margin that is left.

    python examples/closed_loop_margin.py [--elements 6] [--beams 4] [--kick-steps 20]
"""
import argparse

import numpy as np
import scipy.linalg
import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

H = 1e-3                                   # the sample time: 1 kHz


def radius(M):
    return float(np.max(np.abs(np.linalg.eigvals(M))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=6)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--kick-steps", type=int, default=20)
    args = ap.parse_args(argv)

    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True, enable_gravity_effects=True)
    ens = BeamEnsemble(rod(args.elements, "nonlinear"), args.beams, force_params=fp)
    n, B = ens.n, args.beams
    sol = ens.solve_static()
    assert bool(sol.converged.all())
    x_eq = torch.cat([sol.q, torch.zeros_like(sol.q)], dim=1)
    A_d, B_d = (t[0].cpu().numpy() for t in ens.linearize_implicit(H, n_iter=2, x_red=x_eq))
    Q = np.eye(2 * n)
    Q[:n, :n] *= 100.0                     # Q / R of lqr_control.py:61-66
    Q[n:, n:] *= 10.0
    R = np.eye(n)
    P = scipy.linalg.solve_discrete_are(A_d, B_d, Q, R)
    K = np.linalg.solve(R + B_d.T @ P @ B_d, B_d.T @ P @ A_d)
    design = radius(A_d - B_d @ K)

    # the operating points: the equilibrium, and each rod where the open loop is `kick_steps` samples into a tip impulse
    amps = 10.0 * (1.0 + np.arange(B) / B)
    ens.set_state(x_eq, 0.0)
    ens.step_implicit(args.kick_steps, H, n_iter=2, impulse_amp=amps)
    x_kick = ens.unpack_state().clone()
    rows = []
    for label, x in (("equilibrium", x_eq), (f"{args.kick_steps} ms into the impulse", x_kick)):
        Phi, _ = ens.linearize_implicit_feedback(H, K, reference=x_eq, hold=1, n_samples=1, n_iter=2, x_red=x)
        A_x, B_x = ens.linearize_implicit(H, n_iter=2, x_red=x)
        for b in sorted({0, B - 1}):
            rows.append((label, b, float(amps[b]), float((x[b, n - 2] - x_eq[b, n - 2]).item()), radius(A_x[b].cpu().numpy()),
                         radius(Phi[b].cpu().numpy())))

    print(f"{B} rods x {args.elements} nonlinear elements in water under gravity, sample time {H:g} s, gain from "
          f"solve_discrete_are about the static equilibrium (tip w {float(x_eq[0, n - 2]):.3e} m)")
    print(f"spectral radius the design promises, A_d - B_d K about the equilibrium: {design:.6f}")
    for label, b, amp, dw, open_r, closed_r in rows:
        print(f"{label:<26} rod {b} ({amp:4.1f} N, tip w - w_eq {dw:+.3e} m): open loop {open_r:.6f}, closed loop "
              f"(linearize_implicit_feedback) {closed_r:.6f}, against the design {closed_r - design:+.2e}")
    return design, rows


if __name__ == "__main__":
    main()
