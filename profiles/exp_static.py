"""crb_solve_static at scale: 4096 x 256-node nonlinear rods (1.5 m, gravity, per-beam tip loads 0 .. 5 N)
and 64 x 10-element rods.  Wall time per solve with HIP events after a warm-up, the Newton-iteration histogram, time per
iteration, the scaled residual reached (the default rtol of BeamEnsemble.solve_static comes from its distribution), and
the numpy / C-oracle Newton per beam on the host for comparison.

    timeout -k 10 600 python profiles/exp_static.py [--json out.json]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/exp_static.py --reps 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "continuum-robot_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from continuum_robot.batched import BeamEnsemble  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402
from tests.helpers import nitinol_columns, oracle_beam  # noqa: E402


def rod(n_el):
    cols = nitinol_columns(n_el, "nonlinear")
    cols["length"] = np.full(n_el, 1.5 / n_el)
    return cols


def run(n_el, B, reps, rtol):
    cols = rod(n_el)
    ens = BeamEnsemble(cols, B, force_params=ForceParams(enable_gravity_effects=True))
    U = np.zeros((B, ens.n))
    U[:, -2] = -np.linspace(0.0, 5.0, B)
    Ud = torch.as_tensor(U, device=ens.device)
    sol = ens.solve_static(held_force=Ud, rtol=rtol)   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sol = ens.solve_static(held_force=Ud, rtol=rtol)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    it = sol.iterations.cpu().numpy()
    res = sol.residual.cpu().numpy()
    conv = it >= 0
    hist = {int(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))}
    med = float(np.median(ms))
    out = dict(n_elem=n_el, beams=B, rtol=rtol, solve_ms_median=med, solve_ms_all=ms, converged=int(conv.sum()),
               iterations_hist=hist, ms_per_iteration=med / max(int(it[conv].max()) if conv.any() else 1, 1),
               residual_max=float(res[conv].max()) if conv.any() else None,
               residual_median=float(np.median(res[conv])) if conv.any() else None)
    # the host comparison: Newton with the oracle's residual and a dense solve, per beam, from q = 0 in the same increments
    ob = oracle_beam(cols, enable_gravity=True)
    q_gpu = sol.q.cpu().numpy()
    b = B - 1
    t0 = time.perf_counter()
    q = np.zeros(ens.n)
    n_newton = 0
    r0 = ob.internal_force(q) - ob.gravity(np.zeros(2 * ens.n)) - U[b]
    for s in range(1, 9):
        lt = s / 8
        for _ in range(20):
            r = ob.internal_force(q) - ob.gravity(np.concatenate([q, np.zeros_like(q)])) - U[b]
            H = r - (1 - lt) * r0
            if np.max(np.abs(H)) <= rtol * np.max(np.abs(ob.internal_force(q))):
                break
            # tangent by central differences of the oracle (2 n evaluations) -- what a host solver without the analytic
            # tangent pays per iteration
            J = np.empty((ens.n, ens.n))
            for j in range(ens.n):
                h = 1e-7 * max(1e-3, abs(q[j]))
                e = np.zeros(ens.n)
                e[j] = h
                J[:, j] = (ob.internal_force(q + e) - ob.internal_force(q - e)) / (2 * h)
            q = q - np.linalg.solve(J, H)
            n_newton += 1
    host_s = time.perf_counter() - t0
    out.update(host_newton_s_per_beam=host_s, host_newton_iterations=n_newton,
               host_vs_gpu_max_abs_diff=float(np.max(np.abs(q - q_gpu[b]))),
               host_threads=int(os.environ.get("OMP_NUM_THREADS", "1")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rtol", type=float, default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from continuum_robot.batched import STATIC_RTOL

    rtol = STATIC_RTOL if args.rtol is None else args.rtol
    res = [run(255, 4096, args.reps, rtol), run(10, 64, args.reps, rtol)]
    for r in res:
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
