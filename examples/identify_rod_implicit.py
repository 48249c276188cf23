"""identify_rod.py's task through the implicit stepper: recover a stiffness scale and the drag coefficient of four rods from a
recorded tip trajectory, at h = 1e-4 s instead of dt = 2e-5 s -- the same simulated horizon in a fifth of the steps
(BeamEnsemble.step_implicit_adjoint_params, DESIGN.md §10 "Parameter gradients of the implicit adjoint").

The rods, the true parameters, the loss sum_k (w_tip(t_k) - measured_k)^2 over the same sample times and the Rprop descent are
identify_rod.py's.  Each formulation is measured by its own stepper at the true parameters and fitted through its own adjoint:
the implicit one differentiates the map step_implicit computes with two modified-Newton iterations per step, iteration matrix
included.  Both fits run here, one after the other, and the recovered parameters and the wall time per iterate are printed
side by side.

    python examples/identify_rod_implicit.py [--iterations 60]
"""
import argparse
import time

import numpy as np
import torch

from _common import DRAG_COEF, MODULUS
from identify_rod import AMPS, DT, EVERY, STEPS, TRUE_DRAG, TRUE_SCALE, ensemble

H, N_ITER = 1e-4, 2
RATIO = int(round(H / DT))                      # RK4 steps per implicit step
IMP_STEPS, IMP_EVERY = STEPS // RATIO, EVERY // RATIO


def rk4_samples(ens):
    ens.zero_state()
    return ens.step(STEPS, DT, impulse_amp=AMPS, record=(ens.n_elem, "w"), record_every=EVERY)[1]


def rk4_gradients(ens, lam, resid):
    return ens.step_adjoint_params(STEPS, DT, lam, x0_red=torch.zeros_like(lam), impulse_amp=AMPS, t0=0.0,
                                   record=(ens.n_elem, "w"), record_every=EVERY, lam_record=2.0 * resid)[3]


def implicit_samples(ens):
    ens.zero_state()
    return ens.step_implicit(IMP_STEPS, H, n_iter=N_ITER, impulse_amp=AMPS, record=(ens.n_elem, "w"), record_every=IMP_EVERY)[1]


def implicit_gradients(ens, lam, resid):
    return ens.step_implicit_adjoint_params(IMP_STEPS, H, lam, n_iter=N_ITER, x0_red=torch.zeros_like(lam), impulse_amp=AMPS,
                                            t0=0.0, record=(ens.n_elem, "w"), record_every=IMP_EVERY, lam_record=2.0 * resid)[3]


def fit(name, samples, gradients, iterations):
    """identify_rod.py's descent with the formulation's own rollout and adjoint: (scale, Cd, final loss, seconds per iterate)"""
    measured = samples(ensemble(TRUE_SCALE, TRUE_DRAG)).clone()
    B = len(TRUE_SCALE)
    theta = np.zeros((B, 2))                      # log(scale), log(Cd / nominal)
    delta = np.full((B, 2), 0.05)
    last_sign = np.zeros((B, 2))
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for it in range(iterations):
        scale, drag = np.exp(theta[:, 0]), DRAG_COEF * np.exp(theta[:, 1])
        ens = ensemble(scale, drag)
        resid = samples(ens) - measured
        loss = float((resid ** 2).sum())
        lam = torch.zeros((B, 2 * ens.n), dtype=torch.float64, device=ens.device)
        grads = gradients(ens, lam, resid)
        g = np.stack([(grads["elastic_modulus"].cpu().numpy() * MODULUS * scale[:, None]).sum(axis=1),
                      (grads["drag_coef"].cpu().numpy() * drag[:, None]).sum(axis=1)], axis=1)
        if it % 10 == 0 or it == iterations - 1:
            print(f"{name} iterate {it:3d}  loss {loss:.6e}  scale " + " ".join(f"{s:.4f}" for s in scale)
                  + "  Cd " + " ".join(f"{c:.4f}" for c in drag))
        sign = np.sign(g)
        delta = np.where(sign * last_sign > 0, np.minimum(1.2 * delta, 0.2), np.where(sign * last_sign < 0, 0.5 * delta, delta))
        theta -= sign * delta
        last_sign = sign
    torch.cuda.synchronize()
    per_iterate = (time.perf_counter() - t_start) / max(iterations, 1)
    return scale, drag, loss, per_iterate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=60)
    a = ap.parse_args()
    fit("warm-up ", implicit_samples, implicit_gradients, 2)          # (the first calls build tables and load kernels)
    fit("warm-up ", rk4_samples, rk4_gradients, 2)
    imp = fit("implicit", implicit_samples, implicit_gradients, a.iterations)
    rk4 = fit("rk4     ", rk4_samples, rk4_gradients, a.iterations)
    fmt = lambda v: " ".join(f"{x:.4f}" for x in v)   # noqa: E731
    print(f"true                                   scale {fmt(TRUE_SCALE)}  Cd {fmt(TRUE_DRAG)}")
    print(f"implicit h = {H:g}, {IMP_STEPS:3d} steps, n_iter {N_ITER}   scale {fmt(imp[0])}  Cd {fmt(imp[1])}  loss {imp[2]:.3e}  "
          f"{1e3 * imp[3]:.2f} ms / iterate")
    print(f"rk4      dt = {DT:g}, {STEPS:3d} steps           scale {fmt(rk4[0])}  Cd {fmt(rk4[1])}  loss {rk4[2]:.3e}  "
          f"{1e3 * rk4[3]:.2f} ms / iterate")
    print(f"wall time per iterate, rk4 / implicit: {rk4[3] / imp[3]:.2f}")


if __name__ == "__main__":
    main()
