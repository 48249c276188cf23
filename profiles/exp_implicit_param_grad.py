"""Parameter gradients of the implicit adjoint at scale: step_implicit_adjoint next to
step_implicit_adjoint_params (the recompute crb_imp_adj_kernel<double, 4>, the storing sweep crb_imp_adj_kernel<double, 3> and
the reduction crb_imp_param_grad_kernel per segment) on 4096 x 256-node nonlinear rods with drag over 40 steps and 64
ten-element rods over 1000 steps, one cotangent, h = 1e-4, two iterations.  Wall time per call with HIP events after a warm-up,
the median of ``--reps`` calls; the kernel times of record come from a rocprofv3 run of the same script.  ``--plain-only`` times
step_implicit_adjoint alone (the figure to hold against a build of the parent commit: CRB_LIB_PATH selects the library).

    timeout -k 10 600 python profiles/exp_implicit_param_grad.py [--json out.json]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/exp_implicit_param_grad.py --reps 3
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

H, N_ITER = 1e-4, 2


def timed(fn, reps):
    fn()   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def case(name, n_elem, B, steps, reps, plain_only):
    ens = BeamEnsemble(nitinol_columns(n_elem, "nonlinear"), B,
                       force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True))
    amps = torch.linspace(0.1, 0.5, B, dtype=torch.float64, device=ens.device)
    lam = torch.zeros((B, 2 * ens.n), dtype=torch.float64, device=ens.device)
    lam[:, ens.n - 2] = 1.0
    x0 = torch.zeros_like(lam)
    kw = dict(n_iter=N_ITER, x0_red=x0, impulse_amp=amps, t0=0.0)
    out = dict(case=name, steps=steps, checkpoint_every=ens.checkpoint_interval(steps, implicit=(N_ITER, 1)))
    med, lo, hi = timed(lambda: ens.step_implicit_adjoint(steps, H, lam, **kw), reps)
    out.update(step_implicit_adjoint_ms=med, step_implicit_adjoint_ms_min=lo, step_implicit_adjoint_ms_max=hi)
    if not plain_only:
        every = ens.checkpoint_interval(steps, implicit_params=(N_ITER, 1))
        med, lo, hi = timed(lambda: ens.step_implicit_adjoint_params(steps, H, lam, **kw), reps)
        # what the reduction reads once: per step the start state (2 planes), per iteration the iterate and gbar (1 plane each),
        # [B][n_node][4] doubles a plane; a thread's reads of its left neighbour's records hit the lines its neighbour loads
        read_bytes = steps * (2 + 2 * N_ITER) * B * ens.n_node * 4 * 8
        out.update(checkpoint_every_params=every, step_implicit_adjoint_params_ms=med, step_implicit_adjoint_params_ms_min=lo,
                   step_implicit_adjoint_params_ms_max=hi, reduction_read_bytes=read_bytes,
                   reduction_read_bytes_per_segment=read_bytes // steps * every)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = [case("4096 x 256 nonlinear + drag, 40 steps, 1 cotangent", 256, 4096, 40, a.reps, a.plain_only),
           case("64 x 10 nonlinear + drag, 1000 steps, 1 cotangent", 10, 64, 1000, a.reps, a.plain_only)]
    for r in out:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
