#!/usr/bin/env python3
"""Cost of per-instance tuning on the configs[1] workload (batch 1024 fkin6, N = 40, RK4 x 25, run_steps: all steps in one launch).

  (a) shared tables;  (b) per-instance mode, every instance given the shared tuning (outputs must equal (a) bit for bit);
  (c) K = 8 distinct tunings (limits and weights), solves/s and the fraction of status-0 solves per tuning.

(a) and (b) alternate, `--reps` times each, at 20 and at 500 steps; the line reports medians and spreads (max - min) / median.
usage: tools/bench_instance_tuning.py [--reps 3] [--batch 1024] > result.json

--penalties: the same for per-instance slack penalties, on configs[1] with the two track rows soft (100 / 100 on both sides), 500 steps:
  (a) another build of the library (--parent-lib: the parent commit's libihm2mpc.so), shared penalties;  (b) this tree, shared;
  (c) per-instance mode, every instance holding the shared values (outputs must equal (b) bit for bit);  (d) 8 distinct penalty sets.
Every measurement runs in a process of its own, the rows interleaved, `--reps` times each.
usage: tools/bench_instance_tuning.py --penalties [--reps 5] [--parent-lib PATH] > result.json"""
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


PENALTY_WIDTHS = [[1.6, 1.5]]


def make_penalty_solver(B, mode, K=8):
    """configs[1] with the two track rows soft on both sides; mode: a / b shared 100 / 100, c per-instance with those values, d K sets."""
    from ihm2_amd.solver import BatchedOcpSolver

    ocp, track = bench.build_problem(B)
    ocp.model.con_h_expr = "track"
    c = ocp.constraints
    c.lh = c.lh_e = np.array([-1e3, -1e3]); c.uh = c.uh_e = np.array([0.0, 0.0])
    c.idxsh, c.idxsh_e = np.arange(2), np.arange(2)
    ocp.cost.zl = ocp.cost.zu = ocp.cost.Zl = ocp.cost.Zu = np.full(2, 100.0)
    ocp.cost.zl_e = ocp.cost.zu_e = ocp.cost.Zl_e = ocp.cost.Zu_e = np.full(2, 100.0)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=np.array(PENALTY_WIDTHS))
    d = ocp.flatten()
    z, Z = np.tile(d.soft_z[None], (B, 1, 1)), np.tile(d.soft_Z[None], (B, 1, 1))
    if mode == "d":     # a penalty sweep: z 10 .. 1000 (geometric), Z 1000 .. 10
        f = np.geomspace(0.1, 10.0, K)[np.arange(B) % K][:, None, None]
        soft = Z >= 0.0
        z, Z = np.where(soft, z * f, z), np.where(soft, Z / f, Z)
    if mode in ("c", "d"):
        s.set_instance_soft(z, Z)
    return s, bench.sample_x0(track, B, seed=20240607)


def penalty_child(B, mode, steps, parent_lib, out_path):
    from ihm2_amd import _lib

    if mode == "a":     # the other build: its library, without the entries it does not have
        _lib.LIB_PATH = parent_lib
        for name in ("ihm2mpc_set_instance_soft", "ihm2mpc_set_instance_alat_soft"):
            _lib.SYMBOLS.pop(name, None)
    s, x0 = make_penalty_solver(B, mode)
    s.set_x0(x0)
    s.init_guess()
    s.set_lap_wrap(True)
    s.reserve_history(steps)
    s.step(bench.S_TARGET, model=0, M_sim=bench.M_SUB)
    s.run_steps(bench.S_TARGET, 50, model=0, M_sim=bench.M_SUB)
    s.synchronize()
    t0 = time.perf_counter()
    h = s.run_steps(bench.S_TARGET, steps, model=0, M_sim=bench.M_SUB, u0_hist=True, status_hist=True, qp_iter_hist=True)
    elapsed = time.perf_counter() - t0
    np.savez(out_path, solves_per_s=B * steps / elapsed, x=s.get_x(), record=str(s.get_launch_record().get("steps")),
             qp_iter_mean=float(h["qp_iter"].mean()), ok=float((h["status"] == 0).mean()), **{"h_" + k: v for k, v in h.items()})
    s.free()


def penalties_main(args):
    import subprocess
    import tempfile

    B, steps = args.batch, 500
    modes = ("a", "b", "c", "d") if args.parent_lib else ("b", "c", "d")
    runs = {m: [] for m in modes}
    identical, same_as_parent, info = True, True, {}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(args.reps):
            got = {}
            for m in modes:
                out = os.path.join(tmp, m + ".npz")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--penalties", "--child", m, "--batch", str(B), "--out", out,
                                "--parent-lib", args.parent_lib or ""], check=True, timeout=300)
                got[m] = dict(np.load(out))
                runs[m].append(float(got[m]["solves_per_s"]))
                info[m] = dict(steps_kernel=str(got[m]["record"]), qp_iter_mean=float(got[m]["qp_iter_mean"]), ok_fraction=float(got[m]["ok"]))
            same = [k for k in got["b"] if k == "x" or k.startswith("h_")]
            identical &= all(np.array_equal(got["b"][k], got["c"][k]) for k in same)
            if "a" in got:
                same_as_parent &= all(np.array_equal(got["b"][k], got["a"][k]) for k in same)
    med = {m: float(np.median(v)) for m, v in runs.items()}
    rec = {"batch": B, "steps": steps, "reps": args.reps, "runs": runs, "median": med,
           "spread": {m: float((max(v) - min(v)) / med[m]) for m, v in runs.items()}, "info": info,
           "c_over_b": med["c"] / med["b"], "d_over_b": med["d"] / med["b"], "shared_and_same_values_bit_identical": bool(identical)}
    if "a" in med:
        rec["b_over_a"] = med["b"] / med["a"]
        rec["b_bit_identical_to_a"] = bool(same_as_parent)
        rec["b_median_not_below_parents_slowest"] = bool(med["b"] >= min(runs["a"]))
    print(json.dumps(rec))
    if not identical:
        raise SystemExit("the per-instance mode with the shared values did not reproduce the shared results bit for bit")
    if "a" in med and not rec["b_median_not_below_parents_slowest"]:
        raise SystemExit("this tree with shared penalties is slower than the parent's slowest repetition")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--penalties", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="--penalties: libihm2mpc.so of the commit to compare with (row a)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.penalties and args.child:
        return penalty_child(args.batch, args.child, 500, args.parent_lib, args.out)
    if args.reps is None:
        args.reps = 5 if args.penalties else 3
    if args.penalties:
        return penalties_main(args)
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
