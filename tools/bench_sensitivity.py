#!/usr/bin/env python3
"""Cost of the x0 sensitivities (kernels_sens.hip) on the configs[1] workload (fkin6, N = 40, RK4 x 25, reference bounds).

  (a) batch B = 1024 and 8192: RTI steps (prepare_step + solve) with the mode 0, 1, 2; the handle's events time the QP phase
      (ihm2mpc_get_timings: from after the linearisation to after the last kernel of the solve), which with the mode on holds the
      sensitivity kernel as well -- its cost is the difference of the medians (the QPs are the same: every other output is bit-identical);
  (b) the one-car controller: wall-clock latency of IHM2Controller.compute_control with and without x0_sensitivities=True;
  (c) closed loops of n control steps (bench.py's persistent setup: one untimed step, a warm-up call, then the timed call): plain
      run_steps, run_steps_sens in mode 1 (the gain of every step into pinned memory) and n x step() with mode 1 and the gain read back
      in stream order; solves/s and the time each adds per step.  B = 8192 takes launches per step in both run_steps calls.
  (d) --adjoint: the adjoint sensitivities (kernels_adj.hip) after one RTI step of the same workload, B = 1024 and 8192, n_seeds = 1,
      2 (both seeds NULL: the unit seeds on u_0, nothing to upload) and 8 (seed_x and seed_u given): median of --steps calls of
      ihm2mpc_eval_adjoint_sensitivities -- wall time of the whole call with the seed upload and the three downloads, and HIP events on
      the handle's stream around the call with every output NULL (the seed upload and the kernel; for the default seeds the kernel alone).
  (e) --adjoint-weights: the same rows for ihm2mpc_eval_adjoint_sensitivities_w (k_adj<true>: the gradients in the cost weights W, W_e as
      well; the wall time holds its five downloads).
  (f) --plant: the plant step with forward sensitivities (kernels_simsens.hip) beside the plant step the handle already has, B = 1024,
      RK4 x 30, model 0 and model 2: HIP events on the handle's stream around ihm2mpc_sim_advance (the kernel of ihm2mpc_sim_step alone, on
      the handle's x0, u0, which are restored before every call) and around ihm2mpc_sim_step_sens_device on the same pairs with every
      output NULL (the kernel alone) and with all four outputs; wall time of the two blocking host calls.  --lib PATH times a library
      that lacks the new entries (the parent's build) on the plant rows alone: ihm2mpc_sim_step's kernel is not to move.
  (g) --value: the cost and its total gradient (kernels_cost.hip) after one RTI step, B = 1024 and 8192 (--batches): wall time of the
      blocking calls ihm2mpc_eval_cost and ihm2mpc_eval_cost_gradient with every output, HIP events around them with every output NULL
      (the call-local allocation and the kernels; a kernel profiler run on this mode gives k_cost alone), and in the same process the
      rows of (e), whose eight-seed call the whole gradient call is set against.
  (h) --value-soft: the rows of (g) for ihm2mpc_eval_cost_gradient_soft on a soft table -- the same workload with the two track rows soft
      100 / 100 on both sides (bench.py's track_rows="soft") -- where k_slack_fold<true> (kernels_slackseed.hip) runs between k_cost<1>
      and k_adj<true>, and in the same process the eight-seed rows of (e) on that handle's table; a kernel profiler run on this mode
      sets the fold against k_adj<true>.
  (i) --penalties: the gradients in the slack penalties (kernels_penaltygrad.hip) on the soft table of (h), B = 1024 and 8192
      (--batches), n_seeds = 1 and 8 with seeds on the stages and on the slacks: ihm2mpc_eval_adjoint_sensitivities_w (k_adj<true>),
      ihm2mpc_eval_adjoint_sensitivities_s (k_slack_fold, k_adj<true>) and ihm2mpc_eval_adjoint_sensitivities_p (k_slack_fold,
      k_adj<true, true>, k_penalty_grad) in the same process -- HIP events around each call with every output NULL (uploads, the
      call-local allocations, the kernels) and the wall time of the whole blocking call with every output -- and the extra time of _p
      over _s.  A kernel profiler run on this mode gives k_penalty_grad and k_adj<true, true> beside k_adj<true>.
  (j) --adjoint-device: the entries with device pointers beside their host twins, B = 1024 and 8192, in one process and in interleaved
      rounds (host call, device call, host call, ..): wall time of ihm2mpc_eval_adjoint_sensitivities_w (host seeds and gradients; it
      blocks) and of ihm2mpc_eval_adjoint_sensitivities_w_device followed by ihm2mpc_synchronize, with one and with eight seeds and
      all five outputs; and of ihm2mpc_set_instance_weights (host expansion and upload) against ihm2mpc_set_instance_weights_device
      with check = 0 (followed by ihm2mpc_synchronize) and check = 1 (it blocks itself).  Median and minimum of --steps rounds.
  (k) --penalties-device: the same for the penalty side, on the soft table of (h), B = 1024 and 8192, interleaved rounds:
      ihm2mpc_set_instance_soft (host images and upload) against ihm2mpc_set_instance_soft_device with check = 0 (followed by
      ihm2mpc_synchronize) and check = 1 -- the device setter once behind the host setter (it then releases the handle's host copy)
      and in rounds of its own; ihm2mpc_eval_adjoint_sensitivities_p (host seeds and outputs; it blocks) against
      ihm2mpc_eval_adjoint_sensitivities_p_device followed by ihm2mpc_synchronize, one seed on the stages and on the slacks and all
      ten outputs.
usage: tools/bench_sensitivity.py [--steps 50] [--warmup 5] [--loop-steps 20,500] [--only-loops | --adjoint | --adjoint-weights | --value [--batches 1024,8192] | --value-soft [--batches 1024,8192] | --penalties [--batches 1024,8192] | --plant [--lib PATH] | --adjoint-device | --penalties-device] > result.json"""
import argparse
import ctypes
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


def loop_throughput(B, n, warmup, how):
    """Solves/s over n control steps of configs[1]: how = "run_steps" (no sensitivities), "run_steps_sens" or "n_x_step" (mode 1)."""
    from ihm2_amd.solver import BatchedOcpSolver

    ocp, track = bench.build_problem(B)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    if how != "run_steps":
        s.set_x0_sensitivities(1)
    s.set_x0(bench.sample_x0(track, B, 20240607)); s.init_guess()
    s.set_lap_wrap(True)
    m = max(n, warmup, 1)
    u0 = s.alloc_pinned((m, B, 2))
    k = s.alloc_pinned((m, B, 2, 8)) if how != "run_steps" else None
    s.reserve_history(m)
    s.step(40.0, model=0, M_sim=25)
    if how == "n_x_step":       # the gain of every step into a device history, as run_steps_sens keeps it when it launches per step
        hip = ctypes.CDLL("libamdhip64.so")
        dk = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(dk), ctypes.c_size_t(m * B * 16 * 8)) == 0

    def run(steps):
        if how == "n_x_step":
            for i in range(steps):
                s.step(40.0, model=0, M_sim=25)
                s.get_u0_async(u0[i])
                s.get_sens_u0_device(dk.value + i * B * 16 * 8)
            return
        kw = dict(sens_u0_hist=k[:steps]) if how == "run_steps_sens" else {}
        s.run_steps(40.0, steps, model=0, M_sim=25, u0_hist=u0[:steps], wait=False, **kw)

    if warmup:
        run(warmup)
    s.synchronize()
    t0 = time.perf_counter()
    run(n)
    s.synchronize()
    el = time.perf_counter() - t0
    rec = s.get_launch_record()["steps"] if how != "n_x_step" else "per_step"
    if how == "n_x_step":
        assert hip.hipMemcpy(ctypes.c_void_p(k.ctypes.data), dk, ctypes.c_size_t(n * B * 16 * 8), 2) == 0      # hipMemcpyDeviceToHost
        hip.hipFree(dk)
    ok = float(np.isfinite(np.asarray(k[:n])).all(axis=(2, 3)).mean()) if k is not None else None
    s.free()
    return dict(solves_per_s=B * n / el, ms_per_step=el * 1e3 / n, launch=rec, finite_gain_rows=ok)


def soft_track_problem(B):
    """bench.build_problem with the track rows of bench.rti_throughput(track_rows="soft"): (ocp, track, track_widths)."""
    ocp, track = bench.build_problem(B)
    ocp.model.con_h_expr = "track"
    c = ocp.constraints
    c.lh = c.lh_e = np.array([-1e3, -1e3]); c.uh = c.uh_e = np.array([0.0, 0.0])
    c.idxsh, c.idxsh_e = np.arange(2), np.arange(2)
    ocp.cost.zl = ocp.cost.zu = ocp.cost.Zl = ocp.cost.Zu = np.full(2, 100.0)
    ocp.cost.zl_e = ocp.cost.zu_e = ocp.cost.Zl_e = ocp.cost.Zu_e = np.full(2, 100.0)
    return ocp, track, np.array([[track.right_widths.min(), track.left_widths.min()]])


def adjoint_timings(B, steps, warmup, weights=False, soft=False):
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    hip = ctypes.CDLL("libamdhip64.so")
    ocp, track, widths = soft_track_problem(B) if soft else bench.build_problem(B) + (None,)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=widths)
    s.set_x0_sensitivities(1)
    s.set_x0(bench.sample_x0(track, B, 20240607))
    s.init_guess()
    s.prepare_step(40.0)
    st = s.solve()
    stream = ctypes.c_void_p()
    _lib.check(s.lib.ihm2mpc_get_stream(s._h, ctypes.byref(stream)))
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rng = np.random.default_rng(1)
    N = s.N
    out = {"status0": float((st == 0).mean())}
    fn = s.lib.ihm2mpc_eval_adjoint_sensitivities_w if weights else s.lib.ihm2mpc_eval_adjoint_sensitivities
    for S in (1, 2, 8):
        sx = None if S == 2 else rng.standard_normal((B, S, N + 1, 8))
        su = None if S == 2 else rng.standard_normal((B, S, N, 2))
        g = [np.empty((B, S, 8)), np.empty((B, S, N, 12)), np.empty((B, S, 8))]
        if weights:
            g += [np.empty((B, S, 12, 12)), np.empty((B, S, 8, 8))]
        ptr = lambda a: None if a is None else a.ctypes.data_as(_lib.c_double_p)      # noqa: E731
        wall, dev = [], []
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            _lib.check(fn(s._h, S, ptr(sx), ptr(su), *[ptr(a) for a in g]))
            wall.append((time.perf_counter() - t0) * 1e3)
        for i in range(warmup + steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            _lib.check(fn(s._h, S, ptr(sx), ptr(su), *[None] * len(g)))
            assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0
            dev.append(ms.value)
        out[f"n_seeds_{S}"] = dict(call_wall_ms=float(np.median(wall[warmup:])), upload_and_kernel_event_ms=float(np.median(dev[warmup:])),
                                   event_ms_spread=float(np.ptp(dev[warmup:]) / np.median(dev[warmup:])),
                                   finite_rows=float(np.isfinite(g[-2]).all(axis=(1, 2, 3)).mean()))
    for e in ev:
        hip.hipEventDestroy(e)
    s.free()
    return out


def adjoint_device_timings(B, steps, warmup):
    """Row (j): the host entries and their device twins on one handle, in interleaved rounds."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    hip = ctypes.CDLL("libamdhip64.so")
    ocp, track = bench.build_problem(B)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    s.set_x0_sensitivities(1)
    s.set_x0(bench.sample_x0(track, B, 20240607))
    s.init_guess()
    rng = np.random.default_rng(1)
    N = s.N
    held = []

    def dev(nbytes, src=None):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        held.append(p)
        if src is not None:
            assert hip.hipMemcpy(p, ctypes.c_void_p(src.ctypes.data), ctypes.c_size_t(src.nbytes), 4) == 0
        return p

    ptr = lambda a: a.ctypes.data_as(_lib.c_double_p)      # noqa: E731

    def rounds(calls):
        """calls: name -> function; every round runs each once, in order; (median, min) ms per name over the rounds after the warm-up"""
        t = {k: [] for k in calls}
        for i in range(warmup + steps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                t[k].append((time.perf_counter() - t0) * 1e3)
        return {k: dict(median_ms=float(np.median(v[warmup:])), min_ms=float(np.min(v[warmup:]))) for k, v in t.items()}

    # the weight setters first (the adjoint rows then differentiate a solve with per-instance weights, as a learning loop's would)
    W = np.tile(np.asarray(s.data.W[0], dtype=np.float64)[None], (B, 1, 1)) * (1.0 + 0.001 * np.arange(B))[:, None, None]
    We = np.tile(np.asarray(s.data.W_e, dtype=np.float64)[None], (B, 1, 1))
    dW, dWe = dev(W.nbytes, W), dev(We.nbytes, We)

    def set_device(check):
        _lib.check(s.lib.ihm2mpc_set_instance_weights_device(s._h, dW, dWe, check))
        _lib.check(s.lib.ihm2mpc_synchronize(s._h))

    out = {"set_instance_weights": rounds({"host": lambda: _lib.check(s.lib.ihm2mpc_set_instance_weights(s._h, ptr(W), ptr(We))),
                                           "device_check0": lambda: set_device(0), "device_check1": lambda: set_device(1)})}
    s.prepare_step(40.0)
    st = s.solve()
    out["status0"] = float((st == 0).mean())
    for S in (1, 8):
        sx, su = rng.standard_normal((B, S, N + 1, 8)), rng.standard_normal((B, S, N, 2))
        g = [np.empty((B, S, 8)), np.empty((B, S, N, 12)), np.empty((B, S, 8)), np.empty((B, S, 12, 12)), np.empty((B, S, 8, 8))]
        dsx, dsu = dev(sx.nbytes, sx), dev(su.nbytes, su)
        dg = [dev(a.nbytes) for a in g]

        def host():
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w(s._h, S, ptr(sx), ptr(su), *[ptr(a) for a in g]))
            _lib.check(s.lib.ihm2mpc_synchronize(s._h))

        def device():
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w_device(s._h, S, dsx, dsu, *dg))
            _lib.check(s.lib.ihm2mpc_synchronize(s._h))

        out[f"adjoint_w_n_seeds_{S}"] = rounds({"host": host, "device": device})
        back = np.empty_like(g[3])
        assert hip.hipMemcpy(ctypes.c_void_p(back.ctypes.data), dg[3], ctypes.c_size_t(back.nbytes), 4) == 0
        out[f"adjoint_w_n_seeds_{S}"]["same_bits"] = bool(np.array_equal(back.view(np.uint64), g[3].view(np.uint64)))
    s.free()
    for p in held:
        hip.hipFree(p)
    return out


def penalties_device_timings(B, steps, warmup):
    """Row (k): the host entries of the penalty side and their device twins on one handle, in interleaved rounds."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    hip = ctypes.CDLL("libamdhip64.so")
    ocp, track, widths = soft_track_problem(B)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=widths)
    s.set_x0_sensitivities(1)
    s.set_x0(bench.sample_x0(track, B, 20240607))
    s.init_guess()
    rng = np.random.default_rng(1)
    N = s.N
    held = []

    def dev(nbytes, src=None):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        held.append(p)
        if src is not None:
            assert hip.hipMemcpy(p, ctypes.c_void_p(src.ctypes.data), ctypes.c_size_t(src.nbytes), 4) == 0
        return p

    ptr = lambda a: a.ctypes.data_as(_lib.c_double_p)      # noqa: E731

    def rounds(calls):
        t = {k: [] for k in calls}
        for i in range(warmup + steps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                t[k].append((time.perf_counter() - t0) * 1e3)
        return {k: dict(median_ms=float(np.median(v[warmup:])), min_ms=float(np.min(v[warmup:]))) for k, v in t.items()}

    # per-instance penalties: the shared table's on its soft sides times a factor, the shared values elsewhere
    z0, Z0 = np.asarray(s.data.soft_z, dtype=np.float64), np.asarray(s.data.soft_Z, dtype=np.float64)
    f = (1.0 + 0.0005 * np.arange(B))[:, None, None]
    z, Z = np.ascontiguousarray(np.where(Z0 >= 0.0, z0 * f, z0)), np.ascontiguousarray(np.where(Z0 >= 0.0, Z0 * f, Z0))
    dz, dZ = dev(z.nbytes, z), dev(Z.nbytes, Z)

    def set_device(check):
        _lib.check(s.lib.ihm2mpc_set_instance_soft_device(s._h, dz, dZ, check))
        _lib.check(s.lib.ihm2mpc_synchronize(s._h))

    # the device setter behind the host setter drops the handle's host copy of the pair (two arrays of B (N+1) 28 doubles that were the
    # source of uploads a moment ago: releasing them is what that call's time consists of); a loop that stays on the device setter never
    # does that, so the steady rows are timed in rounds of their own
    out = {"set_instance_soft": rounds({"host": lambda: _lib.check(s.lib.ihm2mpc_set_instance_soft(s._h, ptr(z), ptr(Z))),
                                        "device_check0_after_host": lambda: set_device(0)})}
    out["set_instance_soft"].update(rounds({"device_check0": lambda: set_device(0), "device_check1": lambda: set_device(1)}))
    tables = s.get_instance_penalty_tables()            # the device setter's (it ran last)
    _lib.check(s.lib.ihm2mpc_set_instance_soft(s._h, ptr(z), ptr(Z)))
    host_tables = s.get_instance_penalty_tables()
    out["set_instance_soft"]["same_bits"] = bool(all(np.array_equal(tables[k].view(np.uint64), host_tables[k].view(np.uint64)) for k in tables))
    set_device(0)
    s.prepare_step(40.0)
    st = s.solve()
    out["status0"] = float((st == 0).mean())
    S = 1
    seeds = [rng.standard_normal((B, S, N + 1, 8)), rng.standard_normal((B, S, N, 2)), rng.standard_normal((B, S, N + 1, 28)),
             rng.standard_normal((B, S, N + 1, 2))]
    g = [np.empty((B, S, 8)), np.empty((B, S, N, 12)), np.empty((B, S, 8)), np.empty((B, S, 12, 12)), np.empty((B, S, 8, 8)),
         np.empty((B, S, N + 1, 28)), np.empty((B, S, N + 1, 28)), np.empty((B, S, N + 1, 2)), np.empty((B, S, N + 1, 2)), np.empty((B, S, N + 1, 10))]
    dseeds = [dev(a.nbytes, a) for a in seeds]
    dg = [dev(a.nbytes) for a in g]

    def host():
        _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_p(s._h, S, *[ptr(a) for a in seeds], *[ptr(a) for a in g]))
        _lib.check(s.lib.ihm2mpc_synchronize(s._h))

    def device():
        _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_p_device(s._h, S, *dseeds, *dg))
        _lib.check(s.lib.ihm2mpc_synchronize(s._h))

    out["adjoint_p_n_seeds_1"] = rounds({"host": host, "device": device})
    same = True
    for a, p in zip(g, dg):
        back = np.empty_like(a)
        assert hip.hipMemcpy(ctypes.c_void_p(back.ctypes.data), p, ctypes.c_size_t(back.nbytes), 4) == 0
        same = same and bool(np.array_equal(back.view(np.uint64), a.view(np.uint64)))
    out["adjoint_p_n_seeds_1"]["same_bits"] = same
    out["adjoint_p_n_seeds_1"]["live_penalty_gradient"] = bool(np.nan_to_num(g[5]).any())
    s.free()
    for p in held:
        hip.hipFree(p)
    return out


def value_timings(B, steps, warmup, soft=False):
    """ihm2mpc_eval_cost and ihm2mpc_eval_cost_gradient after one RTI step: wall time of the whole blocking call with every output, and
    HIP events on the handle's stream around the call with every output NULL (no download: the call-local allocation on the host, then
    k_cost alone / k_cost<1>, k_adj<true> with one seed and k_cost_epilogue).  soft: ihm2mpc_eval_cost_gradient_soft on the soft track
    rows of soft_track_problem, with k_slack_fold<true> in front of k_adj<true>."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    hip = ctypes.CDLL("libamdhip64.so")
    ocp, track, widths = soft_track_problem(B) if soft else bench.build_problem(B) + (None,)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=widths)
    s.set_x0_sensitivities(1)
    s.set_x0(bench.sample_x0(track, B, 20240607))
    s.init_guess()
    s.prepare_step(40.0)
    st = s.solve()
    stream = ctypes.c_void_p()
    _lib.check(s.lib.ihm2mpc_get_stream(s._h, ctypes.byref(stream)))
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    N = s.N
    ptr = lambda a: a.ctypes.data_as(_lib.c_double_p)      # noqa: E731
    cost_out = [np.empty(B), np.empty((B, N + 1)), np.empty(B)]
    grad_out = [np.empty(B), np.empty((B, 8)), np.empty((B, N, 12)), np.empty((B, 8)), np.empty((B, 12, 12)), np.empty((B, 8, 8)),
                np.empty((B, N + 1, 8)), np.empty((B, N, 2))]
    out = {"status0": float((st == 0).mean())}
    if soft:
        out["status_0_or_2"] = float(np.isin(st, (0, 2)).mean())
        out["slack_cost_in_use"] = float((s.get_slack_cost() > 1e-6).mean())
    grad_fn = s.lib.ihm2mpc_eval_cost_gradient_soft if soft else s.lib.ihm2mpc_eval_cost_gradient
    for name, fn, bufs in (("cost", s.lib.ihm2mpc_eval_cost, cost_out), ("gradient", grad_fn, grad_out)):
        wall, dev = [], []
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            _lib.check(fn(s._h, *[ptr(a) for a in bufs]))
            wall.append((time.perf_counter() - t0) * 1e3)
        for i in range(warmup + steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            _lib.check(fn(s._h, *[None] * len(bufs)))
            assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0
            dev.append(ms.value)
        out[name] = dict(call_wall_ms=float(np.median(wall[warmup:])), alloc_and_kernel_event_ms=float(np.median(dev[warmup:])),
                         event_ms_spread=float(np.ptp(dev[warmup:]) / np.median(dev[warmup:])))
    out["finite_rows"] = float(np.isfinite(grad_out[4]).all(axis=(1, 2)).mean())
    for e in ev:
        hip.hipEventDestroy(e)
    s.free()
    return out


def penalty_timings(B, steps, warmup):
    """The three adjoint entries on soft_track_problem after one RTI step, the same seeds for all: see (i) above."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    hip = ctypes.CDLL("libamdhip64.so")
    ocp, track, widths = soft_track_problem(B)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=widths)
    s.set_x0_sensitivities(1)
    s.set_x0(bench.sample_x0(track, B, 20240607))
    s.init_guess()
    s.prepare_step(40.0)
    st = s.solve()
    stream = ctypes.c_void_p()
    _lib.check(s.lib.ihm2mpc_get_stream(s._h, ctypes.byref(stream)))
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rng = np.random.default_rng(1)
    N = s.N
    ptr = lambda a: a.ctypes.data_as(_lib.c_double_p)      # noqa: E731
    out = {"status_0_or_2": float(np.isin(st, (0, 2)).mean()), "slack_cost_in_use": float((s.get_slack_cost() > 1e-6).mean())}
    for S in (1, 8):
        sx, su = rng.standard_normal((B, S, N + 1, 8)), rng.standard_normal((B, S, N, 2))
        ss, sa = rng.standard_normal((B, S, N + 1, 28)), rng.standard_normal((B, S, N + 1, 2))
        g = [np.empty((B, S, 8)), np.empty((B, S, N, 12)), np.empty((B, S, 8)), np.empty((B, S, 12, 12)), np.empty((B, S, 8, 8))]
        gp = [np.empty((B, S, N + 1, 28)), np.empty((B, S, N + 1, 28)), np.empty((B, S, N + 1, 2)), np.empty((B, S, N + 1, 2)),
              np.empty((B, S, N + 1, 10))]
        entries = (("w", s.lib.ihm2mpc_eval_adjoint_sensitivities_w, [sx, su], g),
                   ("s", s.lib.ihm2mpc_eval_adjoint_sensitivities_s, [sx, su, ss, sa], g),
                   ("p", s.lib.ihm2mpc_eval_adjoint_sensitivities_p, [sx, su, ss, sa], g + gp))
        r = {}
        for name, fn, seeds, bufs in entries:
            wall, dev = [], []
            for i in range(warmup + steps):
                t0 = time.perf_counter()
                _lib.check(fn(s._h, S, *[ptr(a) for a in seeds], *[ptr(a) for a in bufs]))
                wall.append((time.perf_counter() - t0) * 1e3)
            for i in range(warmup + steps):
                assert hip.hipEventRecord(ev[0], stream) == 0
                _lib.check(fn(s._h, S, *[ptr(a) for a in seeds], *[None] * len(bufs)))
                assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
                ms = ctypes.c_float()
                assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0
                dev.append(ms.value)
            r[name] = dict(call_wall_ms=float(np.median(wall[warmup:])), upload_alloc_and_kernel_event_ms=float(np.median(dev[warmup:])),
                           event_ms_spread=float(np.ptp(dev[warmup:]) / np.median(dev[warmup:])))
        r["p_over_s_event_ms"] = r["p"]["upload_alloc_and_kernel_event_ms"] - r["s"]["upload_alloc_and_kernel_event_ms"]
        r["p_over_s_wall_ms"] = r["p"]["call_wall_ms"] - r["s"]["call_wall_ms"]
        r["live_penalty_rows"] = float(np.any(gp[0] != 0.0, axis=(1, 2, 3)).mean())
        out[f"n_seeds_{S}"] = r
    for e in ev:
        hip.hipEventDestroy(e)
    s.free()
    return out


def plant_timings(B, steps, warmup, lib_path=None):
    from ihm2_amd import _lib

    new = ("ihm2mpc_sim_step_sens", "ihm2mpc_sim_step_sens_device")
    if lib_path:
        _lib.LIB_PATH, _lib._lib = os.path.abspath(lib_path), None
        probe = ctypes.CDLL(_lib.LIB_PATH)
        if not all(hasattr(probe, n) for n in new):          # the parent's build: bind what it has
            for n in new:
                _lib.SYMBOLS.pop(n, None)
    have = all(n in _lib.SYMBOLS for n in new)
    from ihm2_amd.solver import BatchedOcpSolver

    hip = ctypes.CDLL("libamdhip64.so")
    ocp, track = bench.build_problem(B)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    s.set_x0(bench.sample_x0(track, B, 20240607))
    s.init_guess()
    s.prepare_step(40.0)
    s.solve()
    x0, u0 = s.get_x0(), s.get_u0()
    stream = ctypes.c_void_p()
    _lib.check(s.lib.ihm2mpc_get_stream(s._h, ctypes.byref(stream)))
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    sizes = dict(x=x0.nbytes, u=u0.nbytes, xn=B * 64, Sx=B * 512, Su=B * 128, mu=B * 4)
    buf = {}
    for k, n in sizes.items():
        buf[k] = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(buf[k]), ctypes.c_size_t(n)) == 0
    assert hip.hipMemcpy(buf["x"], ctypes.c_void_p(x0.ctypes.data), ctypes.c_size_t(x0.nbytes), 1) == 0
    assert hip.hipMemcpy(buf["u"], ctypes.c_void_p(u0.ctypes.data), ctypes.c_size_t(u0.nbytes), 1) == 0

    def events(call, before=None):
        ms_all = []
        for _ in range(warmup + steps):
            if before:
                before()
            assert hip.hipEventRecord(ev[0], stream) == 0
            call()
            assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0
            ms_all.append(ms.value)
        t = ms_all[warmup:]
        return dict(event_ms=float(np.median(t)), spread=float(np.ptp(t) / np.median(t)))

    def wall(call):
        t = []
        for _ in range(warmup + steps):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t[warmup:]))

    out = {}
    for model in (0, 2):
        r = {"sim_step_kernel": events(lambda: s.sim_advance(model=model, M_sim=30), before=lambda: s.set_x0(x0))}
        r["sim_step_kernel"]["kernel"] = s.get_launch_record()["sim"]
        r["sim_step_call_wall_ms"] = wall(lambda: s.sim_step(x0, u0, model=model, M_sim=30))
        if have:
            r["sim_step_sens_kernel"] = events(lambda: s.sim_step_sens_device(buf["x"].value, buf["u"].value, model=model, M_sim=30))
            r["sim_step_sens_kernel_and_stores"] = events(lambda: s.sim_step_sens_device(
                buf["x"].value, buf["u"].value, model=model, M_sim=30, x_next=buf["xn"].value, Sx=buf["Sx"].value, Su=buf["Su"].value,
                model_used=buf["mu"].value))
            r["sim_step_sens_call_wall_ms"] = wall(lambda: s.sim_step_sens(x0, u0, model=model, M_sim=30))
            r["kernel_ratio"] = r["sim_step_sens_kernel"]["event_ms"] / r["sim_step_kernel"]["event_ms"]
        out[f"model{model}"] = r
    for e in ev:
        hip.hipEventDestroy(e)
    for b in buf.values():
        hip.hipFree(b)
    s.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-steps", default="20,500")
    ap.add_argument("--only-loops", action="store_true")
    ap.add_argument("--adjoint", action="store_true")
    ap.add_argument("--adjoint-weights", action="store_true")
    ap.add_argument("--plant", action="store_true")
    ap.add_argument("--lib", default=None, help="--plant: path of another build of libihm2mpc.so (one without the new entries times ihm2mpc_sim_step alone)")
    ap.add_argument("--value", action="store_true")
    ap.add_argument("--value-soft", action="store_true")
    ap.add_argument("--penalties", action="store_true")
    ap.add_argument("--adjoint-device", action="store_true")
    ap.add_argument("--penalties-device", action="store_true")
    ap.add_argument("--batches", default="1024,8192", help="--value, --value-soft, --penalties: the batch sizes (one at a time under a kernel profiler)")
    a = ap.parse_args()
    if a.penalties_device:
        print(json.dumps({"penalties_device": {str(B): penalties_device_timings(B, a.steps, a.warmup) for B in (1024, 8192)}}))
        return
    if a.adjoint_device:
        print(json.dumps({"adjoint_device": {str(B): adjoint_device_timings(B, a.steps, a.warmup) for B in (1024, 8192)}}))
        return
    if a.penalties:
        print(json.dumps({"penalties": {str(B): penalty_timings(B, a.steps, a.warmup) for B in (int(v) for v in a.batches.split(","))}}))
        return
    if a.value or a.value_soft:
        batches = [int(v) for v in a.batches.split(",")]
        print(json.dumps({"value_soft" if a.value_soft else "value": {str(B): value_timings(B, a.steps, a.warmup, a.value_soft) for B in batches},
                          "adjoint_weights": {str(B): adjoint_timings(B, a.steps, a.warmup, True, a.value_soft) for B in batches}}))
        return
    if a.plant:
        print(json.dumps({"plant": {"1024": plant_timings(1024, a.steps, a.warmup, a.lib)}, "lib": a.lib or "product"}))
        return
    if a.adjoint or a.adjoint_weights:
        key = "adjoint_weights" if a.adjoint_weights else "adjoint"
        print(json.dumps({key: {str(B): adjoint_timings(B, a.steps, a.warmup, a.adjoint_weights) for B in (1024, 8192)}}))
        return
    out = {"batch": {}, "one_car": {}, "loops": {}}
    for B in (1024, 8192):
        for n in (int(v) for v in a.loop_steps.split(",")):
            if B == 8192 and n > 100:
                continue        # launches per step: the rate does not depend on n
            r = {how: loop_throughput(B, n, a.warmup, how) for how in ("run_steps", "run_steps_sens", "n_x_step")}
            for how in ("run_steps_sens", "n_x_step"):
                r[how]["added_ms_per_step"] = r[how]["ms_per_step"] - r["run_steps"]["ms_per_step"]
            out["loops"][f"B{B}_n{n}"] = r
            print(json.dumps({f"B{B}_n{n}": r}), file=sys.stderr, flush=True)
    if a.only_loops:
        print(json.dumps(out))
        return
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
