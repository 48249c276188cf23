"""Control schedules in the implicit stepper at scale ("Control schedules in the implicit stepper"): per case --
4096 x 256 (40 steps) and 64 x 10 (1000 steps) nonlinear rods with drag, h = 1e-4, n_iter = 2 -- the time per step of
  step_implicit                     without a schedule (a held force) and with one (hold = 5),
  the checkpoint pass               (crb_step_implicit_checkpoint[_sched]) likewise,
  the adjoint, one cotangent        (crb_step_implicit_adjoint[_sched]) likewise.
Wall time per call with HIP events after a warm-up, median of --reps; all --reps figures are kept, so that the run-to-run
spread can be read next to every median.  --tree names the checkout whose package and built library are timed (default: this
one); a checkout of the parent commit has no *_sched entry points for the implicit family, and the scheduled columns are then
left out: run once per checkout and merge with --merge to put the parent's unscheduled figures next to this commit's.

    timeout -k 10 600 python profiles/exp_implicit_schedule.py --label this --json profiles/implicit_schedule_times.json
    timeout -k 10 600 python profiles/exp_implicit_schedule.py --tree <built checkout of the parent> --label parent \\
        --json profiles/implicit_schedule_times.json --merge
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--tree", default=ROOT)
TREE = os.path.abspath(_pre.parse_known_args()[0].tree)
for p in (TREE, os.path.join(TREE, "continuum-robot_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from continuum_robot.batched import _IMPLICIT, BeamEnsemble  # noqa: E402
from continuum_robot.models.force_params import ForceParams  # noqa: E402
from tests.helpers import nitinol_columns  # noqa: E402

H, N_ITER, HOLD = 1e-4, 2, 5


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
    return ms


def case(B, n_elem, steps, reps, scheduled):
    cols = nitinol_columns(n_elem, "nonlinear")
    fp = ForceParams(fluid_density=1000.0, enable_fluid_effects=True)
    ens = BeamEnsemble(cols, B, force_params=fp)
    rng = np.random.default_rng(B + n_elem)
    amps = np.linspace(0.1, 0.5, B)
    K = steps // HOLD
    U = np.where((ens.free_index % 3 == 1)[None, None], rng.normal(0.0, 0.05, (K, B, ens.n)), 0.0)
    U = torch.as_tensor(U, dtype=torch.float64, device=ens.device)
    out = dict(case=f"{B} x {n_elem} nonlinear + drag, h = {H}, n_iter = {N_ITER}, hold = {HOLD}", steps=steps)

    def put(key, ms):
        out[key + "_us_per_step"] = 1e3 * float(np.median(ms)) / steps
        out[key + "_us_per_step_runs"] = [1e3 * m / steps for m in ms]

    variants = [("held", dict(held_force=U[0]), None)]
    if scheduled:
        variants.append(("sched", dict(control=U, control_hold=HOLD), (U, HOLD)))
    every = ens.checkpoint_interval(steps, None, implicit=(N_ITER, 1))
    out["checkpoint_every"] = every
    x0 = torch.zeros_like(ens.state)
    x = x0.clone()
    lam0 = torch.zeros((1, B, 2 * ens.n), dtype=torch.float64, device=ens.device)
    lam0[:, :, ens.n - 2] = 1.0
    lamd0 = ens._pack_dirs(lam0, True)
    lamd = lamd0.clone()
    for name, kw, sch in variants:
        put(f"step_implicit_{name}",
            timed(lambda: (ens.zero_state(), ens.step_implicit(steps, H, n_iter=N_ITER, impulse_amp=amps, t0=0.0, **kw)), reps))
        desc, keep = ens._input_desc(amps, 0.01, -2, None if sch is not None else U[0])
        extra = ()
        if scheduled:       # (this commit's private helpers take the schedule descriptor last; the parent's have no such argument)
            sd, packed = ens._sched_desc(sch)
            extra = (sd,)

        def ckpt_pass():
            x.copy_(x0)
            return ens._checkpoint_pass(_IMPLICIT, x, steps, 0.0, (H, N_ITER), desc, every, None, *extra)

        put(f"checkpoint_pass_{name}", timed(ckpt_pass, reps))
        ckpt = ckpt_pass()

        def sweep():
            lamd.copy_(lamd0)
            ens._sweep(_IMPLICIT, ckpt, lamd, steps, 0.0, (H, N_ITER), desc, every, None, True, *extra)

        put(f"adjoint_1_cot_{name}", timed(sweep, reps))
        del keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="this")
    ap.add_argument("--tree", default=ROOT, help="the built checkout to time")
    ap.add_argument("--json")
    ap.add_argument("--merge", action="store_true", help="add this run to the cases already in --json")
    a = ap.parse_args()
    from continuum_robot import _native as nat

    scheduled = hasattr(nat.load(), "crb_step_implicit_sched")
    runs = [case(4096, 256, 40, a.reps, scheduled), case(64, 10, 1000, a.reps, scheduled)]
    for r in runs:
        print(json.dumps(dict(library=a.label, **r)))
    if a.json:
        doc = {}
        if a.merge and os.path.exists(a.json):
            with open(a.json) as f:
                doc = json.load(f)
        doc[a.label] = runs
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
