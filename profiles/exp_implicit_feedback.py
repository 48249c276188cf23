"""Sampled-data state feedback inside the implicit stepper at scale ("Sampled-data state feedback"): the time per
controller sample of `step_implicit_feedback` in both of its forms, next to the loops it replaces -- linear rods, no drag,
n_iter = 2, at h = 1e-3 with hold = 1 (a 1 kHz controller) and h = 1e-4 with hold = 2, 4 and 10 (1 kHz on a finer step):

  one call, in-kernel     64 x 6, 64 x 10, 4096 x 10, the largest gain in LDS (64 x 30, 512 x 30, 4096 x 30) and the ensembles
                          that place the choice between the forms (1024 x 16, 4096 x 16, 16384 x 10), under CRB_IMPLICIT_FEEDBACK=1
  one call, chain         the same sizes under CRB_IMPLICIT_FEEDBACK=0, and 64 x 40, 4096 x 256 (whose gain leaves LDS)
  host loop               unpack_state(), a torch matmul and step_implicit(hold, h, held_force=u) per sample (examples/digital_lqr.py)
  native loop             crb_feedback_force into a force buffer and crb_step_implicit with that buffer held, per sample, from
                          Python: the chain form's launches issued by the interpreter

Wall time per call with HIP events after a warm-up, median of --reps; all figures are kept in the JSON.

    timeout -k 10 900 python profiles/exp_implicit_feedback.py --json profiles/implicit_feedback_times.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "continuum-robot_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from continuum_robot import _native as nat  # noqa: E402
from continuum_robot.batched import BeamEnsemble  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402
from tests.helpers import nitinol_columns  # noqa: E402

N_ITER = 2
RATES = ((1e-3, 1), (1e-4, 2), (1e-4, 4), (1e-4, 10))            # (h, hold)
# (B, elements, samples): the sizes of the table, then what places the choice between the forms -- ensembles of one round of
# workgroups and of several (the in-kernel form's workgroup is one wave, min(4, 160 KB / LDS bytes) of them per CU)
SIZES = ((64, 6, 200), (64, 10, 200), (4096, 10, 200), (64, 30, 200), (4096, 30, 100), (64, 40, 200), (4096, 256, 20),
         (16384, 10, 100), (4096, 16, 100), (1024, 16, 100), (512, 30, 100))


def timed(fn, reps):
    for _ in range(3):   # warm-up (the first calls of a new ensemble run up to 9 % long at 4096 x 256)
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


def case(B, n_elem, samples, h, hold, reps):
    ens = BeamEnsemble(nitinol_columns(n_elem, "linear"), B, force_params=ForceParams())
    n = ens.n
    rng = np.random.default_rng(B + n_elem)
    # a gain that keeps the loop a contraction whatever the size: weak rate damping and a dense part far below it
    K = 1e-6 * rng.normal(0.0, 1.0, (n, 2 * n))
    K[np.arange(n), n + np.arange(n)] += 1e-3
    K = torch.as_tensor(K, dtype=torch.float64, device=ens.device)
    x0 = torch.as_tensor(1e-3 * rng.normal(0.0, 1.0, (B, 2 * n)), dtype=torch.float64, device=ens.device)
    amps = np.linspace(0.1, 0.5, B)
    steps = samples * hold
    out = dict(case=f"{B} x {n_elem} linear, h = {h}, hold = {hold}, n_iter = {N_ITER}", samples=samples)

    def put(key, ms):
        out[key + "_us_per_sample"] = 1e3 * float(np.median(ms)) / samples
        out[key + "_us_per_sample_runs"] = [1e3 * m / samples for m in ms]

    def one_call():
        ens.set_state(x0, 0.0)
        ens.step_implicit_feedback(steps, h, K, hold=hold, n_iter=N_ITER, impulse_amp=amps)

    os.environ.pop("CRB_IMPLICIT_FEEDBACK", None)
    out["chosen_form"] = ens.implicit_feedback_path()
    os.environ["CRB_IMPLICIT_FEEDBACK"] = "1"            # (both forms wherever the gain fits LDS, whichever is chosen)
    if ens.implicit_feedback_path() == "in-kernel":
        put("one_call_in_kernel", timed(one_call, reps))
    os.environ["CRB_IMPLICIT_FEEDBACK"] = "0"
    put("one_call_chain", timed(one_call, reps))
    os.environ.pop("CRB_IMPLICIT_FEEDBACK", None)

    def host_loop():
        ens.set_state(x0, 0.0)
        for _ in range(samples):
            u = -(ens.unpack_state() @ K.T)
            ens.step_implicit(hold, h, n_iter=N_ITER, impulse_amp=amps, held_force=u)

    put("host_loop", timed(host_loop, reps))

    lib, u = ens._lib, torch.zeros((B, ens.n_node, 4), dtype=torch.float64, device=ens.device)
    desc, keep = ens._input_desc(amps, 0.01, -2, None)
    desc.f_held = u.data_ptr()
    t_end = C.c_double(0.0)

    def native_loop():
        ens.set_state(x0, 0.0)
        t = 0.0
        for _ in range(samples):
            nat.check(lib.crb_feedback_force(ens.plan.h, ens._ptr(ens.state), ens._ptr(K), None, ens._ptr(u), ens._stream()))
            nat.check(lib.crb_step_implicit(ens.plan.h, ens._ptr(ens.state), t, h, hold, N_ITER, C.byref(desc), None,
                                            C.byref(t_end), ens._stream()))
            t = t_end.value

    put("native_loop", timed(native_loop, reps))
    del keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--sizes", default="", help="comma-separated indices into SIZES (default: all)")
    a = ap.parse_args()
    sizes = [SIZES[int(i)] for i in a.sizes.split(",")] if a.sizes else SIZES
    runs = []
    for B, n_elem, samples in sizes:
        for h, hold in RATES:
            runs.append(case(B, n_elem, samples, h, hold, a.reps))
            print(json.dumps(runs[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
