"""Adjoint of the closed-loop rollout ("Closed loop"): what the backward pass costs next to the forward one.

Rows, each at 64 x 6 elements x 1000 steps ("small") and 2048 x 128 elements x 20 steps ("large"), nonlinear + drag + gravity,
one cotangent:
  feedback_default      step_feedback as it dispatches (fused / persistent / stage-split)
  feedback_stage_split  step_feedback forced to the stage-split launches (CRB_FUSED_FEEDBACK=0 CRB_LOOP=0) -- the forward map
                        the differentiable rollout runs
  checkpoint_pass       rollout_feedback without a graph: crb_step_rk4_feedback_checkpoint
  adjoint               step_feedback_adjoint: checkpoint pass + per-segment recompute + sweep
  adjoint_no_gain       the same with want_gain=False (the gain-gradient product skipped)
Derived (the recompute issues the checkpoint pass's launches plus one state copy per step, so it is taken as equal to it):
  sweep = adjoint - 2 checkpoint_pass;  backward / forward = (adjoint - checkpoint_pass) / feedback_stage_split;
  at the small shape, the gain entries of central differences (2 default rollouts each) one adjoint call is worth.

Medians of --reps calls (default 9) with HIP events after a warm-up call.  Kernel times (crb_feedback_ws_kernel or
crb_feedback_kernel = the forward product, crb_feedback_transpose_kernel, crb_feedback_gain_grad_kernel) come from a rocprofv3
run of its own:

    timeout -k 10 600 python profiles/exp_feedback_adjoint.py [--rows small|large|all] [--json out.json]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- \\
        python profiles/exp_feedback_adjoint.py --rows large --reps 2
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
from tests.helpers import nitinol_columns, oracle_beam  # noqa: E402
from tests.test_graded_beams_cpu import closed_loop_gain  # noqa: E402

DT = 2e-5


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
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def shape(n_elem, n_beams, steps, reps):
    cols = nitinol_columns(n_elem, "nonlinear")
    ens = BeamEnsemble(cols, n_beams, force_params=ForceParams(fluid_density=1000.0, enable_fluid_effects=True,
                                                               enable_gravity_effects=True))
    ob = oracle_beam(cols, fluid_density=1000.0, enable_fluid=True, enable_gravity=True)
    rng = np.random.default_rng(7)
    dev = dict(dtype=torch.float64, device=ens.device)
    K = torch.as_tensor(closed_loop_gain(ob, rng), **dev)
    R = torch.as_tensor(rng.normal(0.0, 1e-3, (n_beams, 2 * ens.n)), **dev)
    amps = torch.linspace(0.1, 0.2, n_beams, **dev)
    x0 = torch.zeros((n_beams, 2 * ens.n), **dev)
    lam = torch.zeros_like(x0)
    lam[:, ens.n - 2] = 1.0

    def forward():
        ens.set_state(x0)
        ens.step_feedback(steps, DT, K, R, impulse_amp=amps)

    out = {"case": f"{n_beams} x {n_elem} nonlinear + drag + gravity, {steps} steps, 1 cotangent, checkpoint_every "
                   f"{ens.checkpoint_interval(steps, feedback_cotangents=1)}", "feedback_path": ens.feedback_path()}
    out["feedback_default"] = timed(forward, reps)
    os.environ["CRB_FUSED_FEEDBACK"], os.environ["CRB_LOOP"] = "0", "0"
    out["feedback_stage_split"] = timed(forward, reps)
    del os.environ["CRB_FUSED_FEEDBACK"], os.environ["CRB_LOOP"]
    with torch.no_grad():
        out["checkpoint_pass"] = timed(lambda: ens.rollout_feedback(x0, steps, DT, K, R, impulse_amp=amps), reps)
    adj = lambda **kw: ens.step_feedback_adjoint(steps, DT, lam, K, R, x0_red=x0, impulse_amp=amps, t0=0.0, **kw)   # noqa: E731
    out["adjoint"] = timed(adj, reps)
    out["adjoint_no_gain"] = timed(lambda: adj(want_gain=False), reps)
    assert all(bool(torch.isfinite(t).all()) for t in adj())
    med = {k: v["median_ms"] for k, v in out.items() if isinstance(v, dict)}
    out["derived"] = {
        "us_per_step": {k: 1e3 * v / steps for k, v in med.items()},
        "sweep_us_per_step": 1e3 * (med["adjoint"] - 2.0 * med["checkpoint_pass"]) / steps,
        "backward_over_forward": (med["adjoint"] - med["checkpoint_pass"]) / med["feedback_stage_split"],
        "gain_entries_of_central_differences_one_adjoint_is_worth": med["adjoint"] / (2.0 * med["feedback_default"]),
        "gain_entries": ens.n * 2 * ens.n,
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", default="all", choices=["small", "large", "all"])
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {}
    if a.rows in ("small", "all"):
        out["small"] = shape(6, 64, 1000, a.reps)
    if a.rows in ("large", "all"):
        out["large"] = shape(128, 2048, 20, a.reps)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
