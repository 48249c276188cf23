"""The tangent of the sampled-data implicit loop at scale ("Tangent of the sampled-data implicit loop"): the time
of `step_implicit_feedback_tangent` next to the two ways the same columns could be had before it -- linear rods, no drag,
n_iter = 2, h = 1e-3:

  one call                step_implicit_feedback_tangent: per sample one boundary launch and one launch of the implicit tangent
  host loop               per sample unpack_state(), the three torch matmuls of u_k and du_k, and
                          step_implicit_tangent(hold, h, dx, held_force=u_k, d_held_force=du_k)
  differencing            the two step_implicit_feedback rollouts of one central difference, timed once and multiplied by the
                          number of directions (each direction needs its own pair)

on 64 x 6 with 2n = 36 directions at hold = 1 and hold = 10, 64 x 40 with 2n = 240 directions, and 4096 x 256 with one
direction.  Wall time per call with HIP events after a warm-up, median of --reps; all figures are kept in the JSON.  The
boundary kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script with --only-call.

    timeout -k 10 600 python profiles/exp_implicit_feedback_tangent.py --json profiles/implicit_feedback_tangent_times.json
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

from continuum_robot.batched import BeamEnsemble  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402
from tests.helpers import nitinol_columns  # noqa: E402

N_ITER, H = 2, 1e-3
# (B, elements, directions (None: 2n identity seeds), hold, samples)
SIZES = ((64, 6, None, 1, 50), (64, 6, None, 10, 20), (64, 40, None, 1, 20), (4096, 256, 1, 1, 5))


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def case(B, n_elem, D, hold, samples, reps, only_call):
    ens = BeamEnsemble(nitinol_columns(n_elem, "linear"), B, force_params=ForceParams())
    n = ens.n
    dev = dict(dtype=torch.float64, device=ens.device)
    rng = np.random.default_rng(B + n_elem)
    # a gain that keeps the loop a contraction whatever the size: weak rate damping and a dense part far below it
    K = 1e-6 * rng.normal(0.0, 1.0, (n, 2 * n))
    K[np.arange(n), n + np.arange(n)] += 1e-3
    K = torch.as_tensor(K, **dev)
    x0 = torch.as_tensor(1e-3 * rng.normal(0.0, 1.0, (B, 2 * n)), **dev)
    R = 0.5 * x0.roll(1, 0)
    if D is None:
        D = 2 * n
        dx0 = torch.eye(2 * n, **dev)[:, None, :].expand(D, B, 2 * n).contiguous()
    else:
        dx0 = torch.as_tensor(1e-3 * rng.normal(0.0, 1.0, (D, B, 2 * n)), **dev)
    dK = torch.as_tensor(1e-6 * rng.normal(0.0, 1.0, (D, n, 2 * n)), **dev)
    amps = np.linspace(0.1, 0.5, B)
    steps = samples * hold
    out = dict(case=f"{B} x {n_elem} linear, {D} direction(s), h = {H}, hold = {hold}, n_iter = {N_ITER}", samples=samples, directions=D)

    def put(key, ms, scale=1.0):
        out[key + "_ms"] = scale * float(np.median(ms))
        out[key + "_ms_runs"] = [scale * m for m in ms]

    def one_call():
        ens.set_state(x0, 0.0)
        ens.step_implicit_feedback_tangent(steps, H, dx0, K, reference=R, hold=hold, n_iter=N_ITER, d_gain=dK, impulse_amp=amps)

    put("one_call", timed(one_call, reps))
    if only_call:
        return out

    def host_loop():
        ens.set_state(x0, 0.0)
        dx = dx0
        for _ in range(samples):
            e = R - ens.unpack_state()
            u = e @ K.T
            du = -(dx @ K.T) + torch.einsum("bj,dij->dbi", e, dK)
            dx = ens.step_implicit_tangent(hold, H, dx, n_iter=N_ITER, impulse_amp=amps, held_force=u, d_held_force=du)

    put("host_loop", timed(host_loop, reps))

    def difference_pair():
        for sign in (1.0, -1.0):
            ens.set_state(x0 + sign * 1e-6 * dx0[0], 0.0)
            ens.step_implicit_feedback(steps, H, K, reference=R, hold=hold, n_iter=N_ITER, impulse_amp=amps)

    put("differencing", timed(difference_pair, reps), scale=float(D))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--sizes", default="", help="comma-separated indices into SIZES (default: all)")
    ap.add_argument("--only-call", action="store_true", help="time the one call alone (for a kernel trace)")
    a = ap.parse_args()
    sizes = [SIZES[int(i)] for i in a.sizes.split(",")] if a.sizes else SIZES
    runs = []
    for B, n_elem, D, hold, samples in sizes:
        runs.append(case(B, n_elem, D, hold, samples, a.reps, a.only_call))
        print(json.dumps(runs[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
