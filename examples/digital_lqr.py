"""A digital LQR at 1 kHz on the discrete linearisation of the implicit stepper, for an ensemble of disturbed rods.

The reference designs a continuous full-state LQR for the linear rod (examples/lqr_control.py:46-84, Q / R at :61-66) and
evaluates u = K (0 - x) inside the RHS of one disturbed closed loop.  A sampled controller sees another plant: the map
x_{k+1} = Phi_h(x_k, u_k) that one implicit step of h = 1e-3 s applies with u_k held.  `BeamEnsemble.linearize_implicit` returns
that map's Jacobians (A_d, B_d) -- two launches of the implicit stepper's tangent with identity seeds -- and
scipy.linalg.solve_discrete_are designs the gain on them.  The loop u_k = -K x_k then runs for B rods under different tip
impulses, one `step_implicit(1, h, n_iter=1, held_force=u_k)` per sample.  (No gravity or drag here: x = 0 is the equilibrium
the regulator holds, and the open loop of the undamped rod rings on.)  The same loop then runs in ONE call,
`step_implicit_feedback(samples, h, K, hold=1, n_iter=1)`: the controller samples and holds inside the native call, and the time
per sample of both and the largest difference between their tip traces are printed.

    python examples/digital_lqr.py [--elements 6] [--beams 64] [--t-final 1.0]
"""
import argparse
import time

import numpy as np
import scipy.linalg
import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

H = 1e-3                                   # the sample time: 1 kHz


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=6)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--t-final", type=float, default=1.0)
    args = ap.parse_args(argv)

    ens = BeamEnsemble(rod(args.elements, "linear"), args.beams, force_params=ForceParams())
    n = ens.n
    ens.zero_state()
    A_d, B_d = (t[0].cpu().numpy() for t in ens.linearize_implicit(H, n_iter=1))
    Q = np.eye(2 * n)
    Q[:n, :n] *= 100.0                     # Q / R of lqr_control.py:61-66
    Q[n:, n:] *= 10.0
    R = np.eye(n)
    P = scipy.linalg.solve_discrete_are(A_d, B_d, Q, R)
    K = np.linalg.solve(R + B_d.T @ P @ B_d, B_d.T @ P @ A_d)
    radius = lambda M: float(np.max(np.abs(np.linalg.eigvals(M))))   # noqa: E731
    K_dev = torch.as_tensor(K, dtype=torch.float64, device=ens.device)

    amps = 10.0 * (1.0 + np.arange(args.beams) / args.beams)         # the example's 10 N for 0.01 s, and up to twice that
    samples = int(round(args.t_final / H))
    tail = max(1, samples // 5)                                      # the deviation is read over the last fifth of the run
    rows = []
    for label, gain in (("open loop", None), ("digital LQR", K_dev)):
        ens.zero_state()
        tip = torch.empty((samples, args.beams), dtype=torch.float64, device=ens.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(samples):
            u = None if gain is None else -(ens.unpack_state() @ gain.T)
            ens.step_implicit(1, H, n_iter=1, impulse_amp=amps, held_force=u)
            tip[k] = ens.tip_displacement()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rows.append((label, float(tip[-tail:].abs().max()), float(tip.abs().max()), wall / samples))

    # the same digital loop in one native call: the zero-order-hold controller inside the implicit stepper
    ens.zero_state()
    ens.step_implicit_feedback(min(samples, 10), H, K_dev, hold=1, n_iter=1, impulse_amp=amps)          # (warm-up)
    ens.zero_state()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, trace = ens.step_implicit_feedback(samples, H, K_dev, hold=1, n_iter=1, impulse_amp=amps, record=(ens.n_elem, "w"))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rows.append((f"one call ({ens.implicit_feedback_path()})", float(trace[:, -tail:].abs().max()), float(trace.abs().max()),
                 wall / samples))
    differ = float((trace.T - tip).abs().max())                      # (tip: the host loop's closed-loop trace)

    print(f"{args.beams} rods x {args.elements} linear elements, {samples} samples of {H:g} s, impulses {amps[0]:.1f} .. {amps[-1]:.1f} N")
    print(f"spectral radius: A_d {radius(A_d):.6f}, A_d - B_d K {radius(A_d - B_d @ K):.6f}")
    for label, late, peak, per in rows:
        print(f"{label:<20} tip |w| over the last {tail} samples: {late:.3e} m   (peak {peak:.3e} m)   {per * 1e6:.0f} us per sample")
    print(f"largest difference between the tip traces of the host loop and the one call: {differ:.3e} m")
    return rows, radius(A_d - B_d @ K)


if __name__ == "__main__":
    main()
