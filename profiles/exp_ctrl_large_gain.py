"""Experiment: the closed loop of examples/lqr_control.py:117-125 (solve_ivp(..., method="LSODA", rtol=1e-8, atol=1e-10) with
u = K (0 - x) in the RHS, tip impulse 10 N for 10 ms) for rods whose gain does not fit the LDS: the in-kernel controller
(controller="device": every beam its own step sequence, the gain streamed from global memory, one launch) against the
host loop (controller="host": the worst beam decides, one step_feedback rollout per piece and doubling, a host sync per
interval).  Times each call with HIP events after one warm-up call of the same shape; prints one JSON line per case.
usage: python profiles/exp_ctrl_large_gain.py [--elems 40,128] [--beams 1,64,2048] [--controllers device,host] [--T 0.005]
       [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "continuum-robot_amd"))
sys.path.insert(0, ROOT)
from tests.helpers import nitinol_columns      # noqa: E402


def ensemble(cols, B):
    from continuum_robot.batched import BeamEnsemble
    from continuum_robot.models.force_params import ForceParams

    return BeamEnsemble(cols, B, force_params=ForceParams(), dtype=torch.float64)


def care_gain(ens):
    from continuum_robot.control import LinearQuadraticRegulator

    K, M = ens.plan.stiffness(), ens.plan.mass()
    n = K.shape[0]
    Q = np.eye(2 * n)
    Q[:n, :n] *= 100
    Q[n:, n:] *= 10
    return LinearQuadraticRegulator(K, M, Q, np.eye(n)).compute_gain_matrix()


def timed(cols, B, K, t_eval, controller):
    ens = ensemble(cols, B)
    call = dict(method="LSODA", rtol=1e-8, atol=1e-10, impulse_amp=np.full(B, 10.0), impulse_duration=0.01, gain=K,
                controller=controller)
    ens.solve_ivp((0.0, t_eval[1]), t_eval[:2], **call)           # warm-up: code objects, tables, buffers
    ens.set_state(np.zeros((B, 2 * ens.n)))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sol = ens.solve_ivp((0.0, t_eval[-1]), t_eval, **call)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert sol.controller == controller and bool(torch.isfinite(sol.y).all())
    if controller == "device":
        per_beam = sol.substeps_per_beam.sum(axis=1)
        steps, steps_min = int(per_beam.max()), int(per_beam.min())
        doublings = int(sol.doublings.max())
    else:
        steps = steps_min = int(sum(sol.substeps))
        doublings = None
    return dict(wall_ms=round(ms, 3), steps_per_beam=steps, steps_per_beam_min=steps_min, doublings_max=doublings,
                us_per_step=round(1e3 * ms / steps, 3)), sol.y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", default="40,128")
    ap.add_argument("--beams", default="1,64,2048")
    ap.add_argument("--controllers", default="device,host")
    ap.add_argument("--T", type=float, default=0.005)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t_eval = np.arange(0.0, a.T + 0.0005, 0.001)
    rows = []
    for n_e in [int(v) for v in a.elems.split(",")]:
        cols = nitinol_columns(n_e, "linear")
        t0 = time.perf_counter()
        K = care_gain(ensemble(cols, 1))
        print(f"# {n_e} elements: CARE {time.perf_counter() - t0:.1f} s", flush=True)
        for B in [int(v) for v in a.beams.split(",")]:
            ys = {}
            for ctrl in a.controllers.split(","):
                r, ys[ctrl] = timed(cols, B, K, t_eval, ctrl)
                row = dict(elems=n_e, beams=B, controller=ctrl, span_s=float(t_eval[-1]), intervals=int(t_eval.size - 1), **r)
                if ctrl == "host" and "device" in ys:   # positions of the two controllers, in units of the default band
                    yd, yh = ys["device"].cpu().numpy(), ys["host"].cpu().numpy()
                    n = yd.shape[1] // 2
                    row["pos_diff_default_band"] = float(np.max(np.abs(yd[:, :n] - yh[:, :n]) / (1e-6 + 1e-3 * np.abs(yh[:, :n]))))
                print(json.dumps(row), flush=True)
                rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
