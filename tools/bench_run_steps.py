#!/usr/bin/env python3
"""Time ihm2mpc_run_steps at the headline shape (batch 1024, fkin6, N = 40, all steps in one launch) under a chosen integrator of the
shooting intervals, next to RK4 x 25 in the same process: the two alternate, `--reps` times each; the line reports medians and spreads
(max - min) / median, the kernels launched, the mean interior-point iterations and the fraction of status-0 solves.

  --integrator ERK_LAG --M n   RK4 x n with the actuator lags in closed form (plant: the same integrator with --M-sim sub-steps, on lane N)
  --sim-integrator ERK         ... with the RK4 x 25 plant instead (a phase of its own)

usage: tools/bench_run_steps.py [--integrator ERK_LAG] [--M 4] [--M-sim 4] [--steps 500] [--reps 3] [--batch 1024] > result.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (build_problem / sample_x0 of the headline workload)


def run(B, steps, warmup, integrator, M, sim_integrator, M_sim):
    from ihm2_amd.solver import BatchedOcpSolver

    ocp, track = bench.build_problem(B)
    o = ocp.solver_options
    o.integrator_type, o.sim_method_num_steps, o.sim_integrator_type = integrator, M, sim_integrator
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    s.set_x0(bench.sample_x0(track, B, seed=20240607))
    s.init_guess()
    s.set_lap_wrap(True)
    s.reserve_history(max(steps, warmup))
    s.step(bench.S_TARGET, model=0, M_sim=M_sim)
    s.run_steps(bench.S_TARGET, warmup, model=0, M_sim=M_sim)
    s.synchronize()
    t0 = time.perf_counter()
    h = s.run_steps(bench.S_TARGET, steps, model=0, M_sim=M_sim, status_hist=True, qp_iter_hist=True)
    elapsed = time.perf_counter() - t0
    out = dict(ms_per_step=elapsed / steps * 1e3, solves_per_s=B * steps / elapsed, launch=s.get_launch_record(),
               mean_qp_iter=float(h["qp_iter"].mean()), ok_fraction=float((h["status"] == 0).mean()))
    s.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--integrator", default="ERK_LAG", choices=("ERK", "ERK_LAG"))
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--sim-integrator", default=None, choices=("ERK", "ERK_LAG"), help="default: the integrator of the shooting intervals")
    ap.add_argument("--M-sim", type=int, default=None, help="default: --M for an ERK_LAG plant, 25 for RK4")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args()
    sim = a.sim_integrator or a.integrator
    M_sim = a.M_sim or (a.M if sim == "ERK_LAG" else bench.M_SUB)
    runs = {"base": [], "this": []}
    for _ in range(a.reps):
        runs["base"].append(run(a.batch, a.steps, a.warmup, "ERK", bench.M_SUB, "ERK", bench.M_SUB))
        runs["this"].append(run(a.batch, a.steps, a.warmup, a.integrator, a.M, sim, M_sim))
    rec = dict(batch=a.batch, steps=a.steps, integrator=a.integrator, M=a.M, sim_integrator=sim, M_sim=M_sim)
    for k, v in runs.items():
        ms = [r["ms_per_step"] for r in v]
        rec[k] = dict(ms_per_step=float(np.median(ms)), spread=float((max(ms) - min(ms)) / np.median(ms)), runs_ms=ms,
                      solves_per_s=float(np.median([r["solves_per_s"] for r in v])), steps_kernel=v[0]["launch"]["steps"],
                      steps_form=v[0]["launch"]["steps_form"], mean_qp_iter=v[0]["mean_qp_iter"], ok_fraction=v[0]["ok_fraction"])
    rec["ratio_this_over_base"] = rec["this"]["ms_per_step"] / rec["base"]["ms_per_step"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
