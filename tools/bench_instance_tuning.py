#!/usr/bin/env python3
"""Cost of per-instance tuning on the configs[1] workload (batch 1024 fkin6, N = 40, RK4 x 25, run_steps: all steps in one launch).

  (a) shared tables;  (b) per-instance mode, every instance given the shared tuning (outputs must equal (a) bit for bit);
  (c) K = 8 distinct tunings (limits and weights), solves/s and the fraction of status-0 solves per tuning.

(a) and (b) alternate, `--reps` times each, at 20 and at 500 steps; the line reports medians and spreads (max - min) / median.
usage: tools/bench_instance_tuning.py [--reps 3] [--batch 1024] > result.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (build_problem / sample_x0 of the headline workload)


def make_solver(B, mode, K=8):
    from ihm2_amd import ocp as O
    from ihm2_amd.solver import BatchedOcpSolver

    ocp, track = bench.build_problem(B)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    d = ocp.flatten()
    names = ("lbx", "ubx", "lbu", "ubu", "lg", "ug")
    assign = np.arange(B) % K
    if mode == "b":
        s.set_instance_weights(np.tile(d.W[0][None], (B, 1, 1)), np.tile(d.W_e[None], (B, 1, 1)))
        s.set_instance_bounds(**{k: np.tile(np.asarray(getattr(d, k))[None], (B,) + (1,) * np.ndim(getattr(d, k))) for k in names})
    elif mode == "c":
        Ws, Wes, tabs = [], [], []
        for j in range(K):     # a limit and weight sweep: v_x_max 10..31 m/s, T_max 300..500 N, delta_max 0.35..0.5, q_n 1..8
            f = j / (K - 1)
            m = O.get_acados_model_from_explicit_dynamics("ihm2_fkin6", O.fkin6_model, 8, 2, 3000)
            o = O.get_acados_ocp(m, bench.N_H, 2.0, 10.0 + 21.0 * f, 300.0 + 200.0 * f, 0.35 + 0.15 * f, 1e6, 0.6 + 0.4 * f)
            W, W_e = O.default_weights(q_n=1.0 + 7.0 * f)
            Ws.append(W); Wes.append(W_e)
            tabs.append(o.flatten())
        s.set_instance_weights(np.stack([Ws[j] for j in assign]), np.stack([Wes[j] for j in assign]))
        s.set_instance_bounds(**{k: np.stack([np.asarray(getattr(tabs[j], k)) for j in assign]) for k in names})
    x0 = bench.sample_x0(track, B, seed=20240607)
    return s, x0, assign


def run(B, mode, steps, warmup=50):
    s, x0, assign = make_solver(B, mode)
    s.set_x0(x0)
    s.init_guess()
    s.set_lap_wrap(True)
    n = max(steps, warmup)
    s.reserve_history(n)
    s.step(bench.S_TARGET, model=0, M_sim=bench.M_SUB)
    s.run_steps(bench.S_TARGET, warmup, model=0, M_sim=bench.M_SUB)
    s.synchronize()
    t0 = time.perf_counter()
    h = s.run_steps(bench.S_TARGET, steps, model=0, M_sim=bench.M_SUB, u0_hist=True, status_hist=True, qp_iter_hist=True)
    elapsed = time.perf_counter() - t0
    out = dict(solves_per_s=B * steps / elapsed, hist=h, x=s.get_x(), assign=assign)
    s.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    args = ap.parse_args()
    B, rec = args.batch, {"batch": args.batch}
    for steps in (20, 500):
        r = {"a": [], "b": []}
        identical = True
        for _ in range(args.reps):
            ra, rb = run(B, "a", steps), run(B, "b", steps)
            r["a"].append(ra["solves_per_s"]); r["b"].append(rb["solves_per_s"])
            identical &= all(np.array_equal(ra["hist"][k], rb["hist"][k]) for k in ra["hist"]) and np.array_equal(ra["x"], rb["x"])
        med = {k: float(np.median(v)) for k, v in r.items()}
        rec[f"steps{steps}"] = {
            "shared_solves_per_s": med["a"], "per_instance_same_tuning_solves_per_s": med["b"], "ratio_b_over_a": med["b"] / med["a"],
            "spread_a": float((max(r["a"]) - min(r["a"])) / med["a"]), "spread_b": float((max(r["b"]) - min(r["b"])) / med["b"]),
            "runs_a": r["a"], "runs_b": r["b"], "b_bit_identical_to_a": bool(identical)}
        rc = run(B, "c", steps)
        st = rc["hist"]["status"]
        rec[f"steps{steps}"]["k8_solves_per_s"] = rc["solves_per_s"]
        rec[f"steps{steps}"]["k8_ok_fraction_per_tuning"] = [float((st[:, rc["assign"] == j] == 0).mean()) for j in range(8)]
    print(json.dumps(rec))
    if not all(rec[f"steps{s}"]["b_bit_identical_to_a"] for s in (20, 500)):
        raise SystemExit("per-instance mode with the shared tuning did not reproduce the shared results bit for bit")


if __name__ == "__main__":
    main()
