#!/usr/bin/env python3
"""Cost of the x0 sensitivities (kernels_sens.hip) on the configs[1] workload (fkin6, N = 40, RK4 x 25, reference bounds).

  (a) batch B = 1024 and 8192: RTI steps (prepare_step + solve) with the mode 0, 1, 2; the handle's events time the QP phase
      (ihm2mpc_get_timings: from after the linearisation to after the last kernel of the solve), which with the mode on holds the
      sensitivity kernel as well -- its cost is the difference of the medians (the QPs are the same: every other output is bit-identical);
  (b) the one-car controller: wall-clock latency of IHM2Controller.compute_control with and without x0_sensitivities=True.
usage: tools/bench_sensitivity.py [--steps 50] [--warmup 5] > result.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (build_problem / sample_x0 of the headline workload)


def batch_timings(B, mode, steps, warmup):
    from ihm2_amd.solver import BatchedOcpSolver

    ocp, track = bench.build_problem(B)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    if mode:
        s.set_x0_sensitivities(mode)
    s.set_x0(bench.sample_x0(track, B, 20240607))
    s.init_guess()
    qp, tot = [], []
    for i in range(warmup + steps):
        s.prepare_step(40.0)
        s.solve_async()
        t = s.get_timings()
        if i >= warmup:
            qp.append(t["qp_ms"]); tot.append(t["total_ms"])
    st = s.get_status()
    s.free()
    return dict(qp_ms=float(np.median(qp)), total_ms=float(np.median(tot)), qp_ms_spread=float(np.ptp(qp) / np.median(qp)),
                status0=float((st == 0).mean()))


def one_car_latency(sens, steps, warmup):
    from ihm2_amd.controller import IHM2Controller

    ocp, track = bench.build_problem(1)
    c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=1, x0_sensitivities=sens)
    x = bench.sample_x0(track, 1, 7)
    c.warm_start(x)
    lat = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        u0 = c.compute_control(x[0])
        if sens:
            c.feedback_gain
        lat.append(time.perf_counter() - t0)
        if u0 is not None:
            x = c.solver.sim_step(x, u0[None], model=0, M_sim=25)
    c.solver.free()
    lat = np.array(lat[warmup:]) * 1e3
    return dict(p50_ms=float(np.median(lat)), p90_ms=float(np.percentile(lat, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = {"batch": {}, "one_car": {}}
    for B in (1024, 8192):
        r = {m: batch_timings(B, m, a.steps, a.warmup) for m in (0, 1, 2)}
        for m in (1, 2):
            r[m]["sens_ms"] = r[m]["qp_ms"] - r[0]["qp_ms"]
        out["batch"][str(B)] = {f"mode{m}": v for m, v in r.items()}
    for sens in (False, True):
        out["one_car"]["with_sens" if sens else "without"] = one_car_latency(sens, 4 * a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
