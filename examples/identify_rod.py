"""Fit a rod to a recorded tip trajectory: recover a stiffness scale and the drag coefficient of a few rods by gradient descent
through the simulator (BeamEnsemble.step_adjoint_params).

Four 8-element nonlinear Nitinol rods in water, each with its own (unknown) modulus scale and drag coefficient, are "measured":
the tip deflection under the examples' tip impulse, sampled every 10 steps.  Starting from the nominal rod, every iterate
rebuilds the ensemble with the current parameters, rolls it out, and takes the gradient of sum_k (w_tip(t_k) - measured_k)^2
with respect to the logarithms of the two parameters from ONE adjoint sweep per iterate: d/d log s = sum_e E_e dL/dE_e,
d/d log Cd = sum_e Cd dL/dCd_e.  The descent is sign-based with one step size per parameter (Rprop: grown by 1.2 while a
gradient keeps its sign, halved when it flips), since the drag gradient is orders of magnitude below the stiffness one.

    python examples/identify_rod.py [--iterations 60]
"""
import argparse

import numpy as np
import torch

from _common import DRAG_COEF, MODULUS, rod

from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams

DT, STEPS, EVERY, N_ELEM = 2e-5, 400, 10, 8
TRUE_SCALE = np.array([0.8, 0.9, 1.1, 1.25])
TRUE_DRAG = np.array([0.5, 0.7, 1.0, 1.3])
AMPS = np.array([0.4, 0.5, 0.6, 0.7])


def ensemble(scale, drag):
    frames = []
    for s, cd in zip(scale, drag):
        f = rod(N_ELEM, "nonlinear")
        f["elastic_modulus"] = MODULUS * s
        f["drag_coef"] = cd
        frames.append(f)
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True, enable_gravity_effects=True)
    return BeamEnsemble.from_dataframes(frames, force_params=[fp] * len(frames))


def tip_samples(ens):
    ens.zero_state()
    return ens.step(STEPS, DT, impulse_amp=AMPS, record=(ens.n_elem, "w"), record_every=EVERY)[1]   # [B, STEPS / EVERY]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=60)
    a = ap.parse_args()
    measured = tip_samples(ensemble(TRUE_SCALE, TRUE_DRAG)).clone()
    B = len(TRUE_SCALE)
    theta = np.zeros((B, 2))                      # log(scale), log(Cd / nominal)
    delta = np.full((B, 2), 0.05)
    last_sign = np.zeros((B, 2))
    for it in range(a.iterations):
        scale, drag = np.exp(theta[:, 0]), DRAG_COEF * np.exp(theta[:, 1])
        ens = ensemble(scale, drag)
        resid = tip_samples(ens) - measured
        loss = (resid ** 2).sum(dim=1)
        lam = torch.zeros((B, 2 * ens.n), dtype=torch.float64, device=ens.device)
        _, _, _, grads = ens.step_adjoint_params(STEPS, DT, lam, x0_red=torch.zeros_like(lam), impulse_amp=AMPS, t0=0.0,
                                                 record=(ens.n_elem, "w"), record_every=EVERY, lam_record=2.0 * resid)
        g = np.stack([(grads["elastic_modulus"].cpu().numpy() * MODULUS * scale[:, None]).sum(axis=1),
                      (grads["drag_coef"].cpu().numpy() * drag[:, None]).sum(axis=1)], axis=1)
        print(f"iterate {it:3d}  loss {float(loss.sum()):.6e}  scale " + " ".join(f"{s:.4f}" for s in scale)
              + "  Cd " + " ".join(f"{c:.4f}" for c in drag))
        sign = np.sign(g)
        delta = np.where(sign * last_sign > 0, np.minimum(1.2 * delta, 0.2), np.where(sign * last_sign < 0, 0.5 * delta, delta))
        theta -= sign * delta
        last_sign = sign
    print("true        scale " + " ".join(f"{s:.4f}" for s in TRUE_SCALE) + "  Cd " + " ".join(f"{c:.4f}" for c in TRUE_DRAG))


if __name__ == "__main__":
    main()
