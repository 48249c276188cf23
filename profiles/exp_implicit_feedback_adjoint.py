"""The adjoint of the sampled-data implicit loop at scale ("Adjoint of the sampled-data loop"): per controller
sample, the time of the checkpoint pass and of the backward sweep of `step_implicit_feedback_adjoint`, next to the same gradient
from the composed Python loop -- `rollout_implicit` per sample with u = held + (r - x) K^T in torch and loss.backward() through
that graph, the only way before this call -- and the gain gradient's share of the sweep (want_gain True against False).
Linear rods, no drag, n_iter = 2, one cotangent:

  64 x 6, hold = 1 (h = 1e-3)    64 x 6, hold = 10 (h = 1e-4)    64 x 40, hold = 1    4096 x 256, hold = 1, 20 samples

Wall time with HIP events after a warm-up, median of --reps; all figures are kept in the JSON.

    timeout -k 10 600 python profiles/exp_implicit_feedback_adjoint.py --json profiles/implicit_feedback_adjoint_times.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "continuum-robot_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from continuum_robot.batched import _IMPLICIT_FEEDBACK, BeamEnsemble  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402
from profiles.exp_implicit_feedback import timed  # noqa: E402
from tests.helpers import nitinol_columns  # noqa: E402

N_ITER = 2
SIZES = ((64, 6, 1e-3, 1, 200), (64, 6, 1e-4, 10, 200), (64, 40, 1e-3, 1, 200), (4096, 256, 1e-3, 1, 20))   # (B, elements, h, hold, samples)


def case(B, n_elem, h, hold, samples, reps):
    ens = BeamEnsemble(nitinol_columns(n_elem, "linear"), B, force_params=ForceParams())
    n, dev = ens.n, dict(dtype=torch.float64, device=ens.device)
    rng = np.random.default_rng(B + n_elem)
    K = 1e-6 * rng.normal(0.0, 1.0, (n, 2 * n))              # (the gain of profiles/exp_implicit_feedback.py: a contraction)
    K[np.arange(n), n + np.arange(n)] += 1e-3
    K = torch.as_tensor(K, **dev)
    x0 = torch.as_tensor(1e-3 * rng.normal(0.0, 1.0, (B, 2 * n)), **dev)
    R = 0.3 * x0.roll(1, 0)
    amps = torch.as_tensor(np.linspace(0.1, 0.5, B), **dev)
    lam = torch.as_tensor(rng.normal(0.0, 1.0, (B, 2 * n)), **dev)
    steps = samples * hold
    every = ens.checkpoint_interval(steps, implicit_feedback=(N_ITER, hold, 1))
    out = dict(case=f"{B} x {n_elem} linear, h = {h}, hold = {hold}, n_iter = {N_ITER}", samples=samples, checkpoint_every=every)

    def put(key, ms):
        out[key + "_us_per_sample"] = 1e3 * float(np.median(ms)) / samples
        out[key + "_us_per_sample_runs"] = [1e3 * m / samples for m in ms]

    # the pass and the sweep apart, as _rollout_adjoint issues them
    step, _, _, _ = _IMPLICIT_FEEDBACK.prepare(ens, steps, (h, N_ITER, hold, K, R, True), None, amps, None)
    desc, keep = ens._input_desc(amps, 0.01, -2, None)
    x = ens.pack_state(x0)
    ckpt = [None]

    def the_pass():
        x.copy_(ens.pack_state(x0))
        ckpt[0] = ens._checkpoint_pass(_IMPLICIT_FEEDBACK, x, steps, 0.0, step, desc, every, None)

    def sweep(want_gain):
        lamd = ens._pack_dirs(lam[None], True)
        ens._sweep(_IMPLICIT_FEEDBACK, ckpt[0], lamd, steps, 0.0, step, desc, every, None, (want_gain, True))

    put("pass", timed(the_pass, reps))
    put("sweep", timed(lambda: sweep(True), reps))
    put("sweep_without_gain", timed(lambda: sweep(False), reps))
    out["gain_share_of_sweep"] = 1.0 - out["sweep_without_gain_us_per_sample"] / out["sweep_us_per_sample"]

    def one_call():
        ens.step_implicit_feedback_adjoint(steps, h, lam, K, reference=R, hold=hold, n_iter=N_ITER, x0_red=x0, impulse_amp=amps,
                                           t0=0.0)

    put("pass_and_sweep", timed(one_call, reps))

    def composed():
        leaf = [t.clone().requires_grad_(True) for t in (x0, K, R, amps)]
        xs, Ks, Rs, As = leaf
        xk, t = xs, 0.0
        for _ in range(samples):
            u = (Rs - xk) @ Ks.T
            xk = ens.rollout_implicit(xk, hold, h, n_iter=N_ITER, impulse_amp=As, held_force=u, t0=t)
            for _ in range(hold):
                t = t + h
        (lam * xk).sum().backward()

    put("composed_loop", timed(composed, reps))
    out["speedup_over_composed_loop"] = out["composed_loop_us_per_sample"] / out["pass_and_sweep_us_per_sample"]
    del keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--sizes", default="", help="comma-separated indices into SIZES (default: all)")
    a = ap.parse_args()
    runs = []
    for size in ([SIZES[int(i)] for i in a.sizes.split(",")] if a.sizes else SIZES):
        runs.append(case(*size, a.reps))
        print(json.dumps(runs[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
