"""Tune a digital LQR gain on the nonlinear rod by gradient descent through the sampled-data loop at h = 1e-3 s
(BeamEnsemble.rollout_implicit_feedback).

examples/digital_lqr.py designs the 1 kHz regulator on the discrete linearisation of the implicit stepper
(`linearize_implicit(1e-3)` and a discrete Riccati solve) and can only simulate it; examples/tune_gain.py tunes a gain on the
nonlinear rod, but through the RK4 loop, which needs dt <= 8.6e-6 s once closed.  Here the digital gain itself is the starting
point: 64 copies of a 6-element NONLINEAR Nitinol rod in water are each hit by their own tip impulse, the controller samples
the state every millisecond and holds u_k = K (0 - x_k), and the cost is the mean squared tip deflection over the samples taken
after the impulse has ended.  Every iterate is ONE differentiable rollout of the whole ensemble at the controller's own rate;
loss.backward() returns dL/dK for all 18 x 36 entries from one adjoint sweep.  The same iterate composed from
`rollout_implicit` per sample -- one autograd node, one checkpoint pass and one sweep per millisecond, the only way before --
is timed next to it.

    python examples/tune_digital_gain.py [--iterations 20]
"""
import argparse
import time

import numpy as np
import scipy.linalg
import torch

from _common import rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

H, SAMPLES, N_ELEM, B = 1e-3, 100, 6, 64               # 0.1 s of closed loop at 1 kHz
IMPULSE_S = 0.01                                        # the disturbance acts for the first 10 ms


def digital_lqr_gain():
    """the gain of examples/digital_lqr.py: Q = diag(100 I, 10 I), R = I on (A_d, B_d) of one implicit step of the linear rod"""
    lin = BeamEnsemble(rod(N_ELEM, "linear"), 1, force_params=ForceParams())
    lin.zero_state()
    A_d, B_d = (t[0].cpu().numpy() for t in lin.linearize_implicit(H, n_iter=1))
    n = B_d.shape[1]
    Q = np.eye(2 * n)
    Q[:n, :n] *= 100.0
    Q[n:, n:] *= 10.0
    R = np.eye(n)
    P = scipy.linalg.solve_discrete_are(A_d, B_d, Q, R)
    return np.linalg.solve(R + B_d.T @ P @ B_d, B_d.T @ P @ A_d)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--step", type=float, default=5e-7, help="first update as a fraction of the gain's norm")
    a = ap.parse_args(argv)
    ens = BeamEnsemble(rod(N_ELEM, "nonlinear"), B, force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    dev = dict(dtype=torch.float64, device=ens.device)
    gain = torch.as_tensor(digital_lqr_gain(), **dev).requires_grad_(True)
    amps = torch.linspace(0.5, 2.0, B, **dev)            # N, one disturbance amplitude per rod
    x0 = torch.zeros((B, 2 * ens.n), **dev)
    settled = torch.arange(1, SAMPLES + 1, device=ens.device) * H >= IMPULSE_S
    tip = ens.n - 2

    def settling_cost(K):
        _, trace = ens.rollout_implicit_feedback(x0, SAMPLES, H, K, hold=1, impulse_amp=amps, impulse_duration=IMPULSE_S,
                                                 record=(ens.n_elem, "w"), record_every=1)
        return (trace[:, settled] ** 2).mean()

    def settling_cost_composed(K):
        """the same iterate from existing calls: rollout_implicit per sample, the controller in torch"""
        x, t, trace = x0, 0.0, []
        for _ in range(SAMPLES):
            x = ens.rollout_implicit(x, 1, H, impulse_amp=amps, held_force=-(x @ K.T), impulse_duration=IMPULSE_S, t0=t)
            t = t + H
            trace.append(x[:, tip])
        return (torch.stack(trace, dim=1)[:, settled] ** 2).mean()

    def iterate_seconds(cost, reps=5):
        """median wall time of one iterate (cost and dL/dK) over ``reps`` after two warm-up iterates"""
        K = gain.detach().clone().requires_grad_(True)
        walls = []
        for r in range(reps + 2):
            K.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = cost(K)
            loss.backward()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        return float(np.median(walls[2:])), float(loss.detach())

    one, cost_one = iterate_seconds(settling_cost)
    many, cost_many = iterate_seconds(settling_cost_composed)
    print(f"{B} rods x {N_ELEM} nonlinear elements, {SAMPLES} samples of {H:g} s: one iterate (cost and dL/dK)")
    print(f"  rollout_implicit_feedback     {one * 1e3:8.2f} ms   cost {cost_one:.6e}")
    print(f"  rollout_implicit per sample   {many * 1e3:8.2f} ms   cost {cost_many:.6e}   ({many / one:.1f} x)")

    # Gradient steps with a fixed rate that is halved whenever a step does not lower the cost or leaves the finite range.
    # The first step is tiny on purpose: the LQR gain of the linear rod (entries up to 8e4) sits at the edge of what the
    # sampled loop on the nonlinear rod tolerates at h = 1e-3 -- moving it along the gradient by 1e-6 of its norm takes this
    # loop, and step_implicit_feedback with the same gain, out of the finite range within the 100 samples; half of that lowers
    # the cost by 40 %.
    rate, first, cost, best = None, None, None, None
    t0 = time.perf_counter()
    for it in range(a.iterations + 1):
        gain.grad = None
        loss = settling_cost(gain)
        cost = float(loss.detach())
        if it == 0:
            if not np.isfinite(cost):
                raise SystemExit("the digital LQR gain does not hold the nonlinear rod in the finite range")
            first = cost
        if best is not None and not cost < best[0]:       # (also a NaN): back to the best gain, half the rate
            print(f"iterate {it:3d}  tip-settling cost {cost:.6e}  not lower: step halved")
            with torch.no_grad():
                gain.copy_(best[1])
            rate *= 0.5
            loss = settling_cost(gain)
            cost = best[0]
        else:
            best = (cost, gain.detach().clone())
            print(f"iterate {it:3d}  tip-settling cost {cost:.6e}  ({cost / first:.3f} of the digital LQR gain's)")
        if it == a.iterations:
            break
        loss.backward()
        if rate is None:    # the first update moves the gain by --step of its norm
            rate = a.step * float(gain.detach().norm() / gain.grad.norm())
        with torch.no_grad():
            gain -= rate * gain.grad
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / max(a.iterations, 1)
    print(f"loss before {first:.6e}, after {cost:.6e}; {wall * 1e3:.2f} ms of wall time per iterate")
    return first, cost


if __name__ == "__main__":
    main()
