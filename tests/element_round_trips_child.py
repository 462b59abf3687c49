"""Child process of tests/test_gpu_element_round_trips.py (started through tests/qp_forms.py: runs(level, child=...)): the reference's OCP at
N = 40 in the form of the QP that IHM2MPC_QP_FORM chooses, at the OCP's own QP tolerance ("d") and at 1e-12 ("t"), where the followed
residuals pass the convergence test before the residuals formed from the data do -- the solve then goes on in exact_mode, the other path
through the update of the followed stationarity residual.  Written to an .npz:
  * "b<B>_<tol>_<path>_<name>", tol d | t, path step | loop: one solve() from the start, then three control steps through step() and, on a
    second handle, the same three in one run_steps launch; "b<B>_<tol>_kernels": the launch records of both;
  * "b<B>_<case>_<name>", case clean | x0: ONE solve() at 1e-12 from inputs the oracle takes unchanged; x0: instance NAN_AT has a NaN in
    x0[., 1].  "b<B>_clean_orc_<status | qp_iter | exact_went_on>": the oracle's solve of the clean inputs, traced (orc_debug): an instance
    entered exact_mode and went on when an iteration number is printed twice and is not the last one.
B = 67 first: the B = 3 batch is made of its instances 0 and the first two that the oracle saw go on in exact_mode.
usage: element_round_trips_child.py out.npz"""
import ctypes
import os
import re
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from conftest import make_ocp  # noqa: E402

import drive  # noqa: E402

SEED, STEPS, NAN_AT, TIGHT = 31, 3, 1, 1e-12
BATCHES = (67, 3)
TOLS = {"d": {}, "t": {"qp_tol": TIGHT}}


def left_behind(s):
    pi, lam = s.get_multipliers()
    return dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), qp_iter=s.get_qp_iter(), status=s.get_status(), qp_res=s.get_qp_residuals(),
                res=s.get_residuals(), u0=s.get_u0())


def traced_oracle_step(P, orc, inp):
    """the oracle's RTI step of the inputs on one thread with its interior-point trace: (out, went_on) -- went_on[b]: the followed residuals
    passed, the residuals formed from the data did not, and the solve took further iterations (exact_mode)"""
    dbg = ctypes.c_int.in_dll(orc.lib(), "orc_debug")
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        dbg.value = 1
        try:
            out = P.rti_step(inp["x"].copy(), inp["u"].copy(), inp["x0"], inp["yref"], inp["yref_e"], pi=inp["pi"].copy(), lam=inp["lam"].copy(), nthreads=1)
        finally:
            dbg.value = 0
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        its = [int(m.group(1)) for m in re.finditer(rb"ipm it +(\d+) ", f.read())]
    solves = []
    for i in its:
        if i == 0:      # a solve starts at iteration 0 (printed once: its residuals are formed from the data)
            solves.append([])
        solves[-1].append(i)
    B = inp["x"].shape[0]
    assert len(solves) == B, (len(solves), B)
    went_on = np.array([any(s[q] == s[q + 1] and q + 2 < len(s) for q in range(len(s) - 1)) for s in solves])
    return out, went_on


def main(out):
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table
    from oracle import oracle as orc

    track = track_table("fsds_competition_1")
    os.environ["IHM2MPC_BLOCK_QP"] = "0"
    res = {}

    def handle(B, tol):
        s = BatchedOcpSolver(make_ocp(**TOLS[tol]), B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        return s

    def loop(s):
        return s.run_steps(40.0, STEPS, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)

    x0_all = drive.clipped_start(track, max(BATCHES), SEED)
    P = orc.OracleProblem(make_ocp(**TOLS["t"]).flatten().as_dict(track.s_ref, track.kappa_ref))
    pick = None
    for B in BATCHES:
        x0 = x0_all[:B] if pick is None or B == max(BATCHES) else x0_all[pick[:B]]
        # ---- single solves at the tight tolerance, from inputs the oracle takes as they are ----
        s = handle(B, "t")
        s.set_x0(x0); s.init_guess()
        x, u = s.get_x(), s.get_u()
        yref, yref_e = orc.prepare_step(s.N, x0, 40.0, x, u)       # shifts x, u in place
        at = min(NAN_AT, B - 1)
        for case in ("clean", "x0"):
            inp = dict(x=x.copy(), u=u.copy(), x0=x0.copy(), yref=yref.copy(), yref_e=yref_e.copy(), pi=np.zeros((B, s.N + 1, 8)), lam=np.zeros((B, s.N + 1, 28)))
            if case == "x0":
                inp["x0"][at, 1] = np.nan
            s.set_x0(inp["x0"]); s.set_x(inp["x"]); s.set_u(inp["u"]); s.set_yref(inp["yref"]); s.set_yref_e(inp["yref_e"])
            s.set_multipliers(inp["pi"], inp["lam"])
            s.solve()
            rec = s.get_launch_record()
            res[f"b{B}_{case}_kernels"] = np.array([rec["qp"], rec["qp_form"], rec["qp_slots"]])
            res.update({f"b{B}_{case}_{k}": v for k, v in left_behind(s).items()})
            res[f"b{B}_{case}_in_x0"] = inp["x0"]
            if case == "clean":
                o, went_on = traced_oracle_step(P, orc, inp)
                res.update({f"b{B}_clean_orc_status": o["status"], f"b{B}_clean_orc_qp_iter": o["qp_iter"], f"b{B}_clean_orc_exact_went_on": went_on})
                if pick is None:      # the small batch: instance 0 and two that went on in exact_mode (the NaN lands on one of them)
                    hit = np.flatnonzero(went_on & (o["status"] == 0))
                    pick = np.array([0] + [int(i) for i in hit if i != 0][:2] + [1, 2])[:3]
        s.free()
        # ---- three steps, launch by launch and in one launch, at both tolerances ----
        for tol in TOLS:
            kernels = []
            for path in ("step", "loop"):
                s = handle(B, tol)
                s.set_x0(x0); s.init_guess()
                s.prepare_step(40.0)
                s.solve()
                h = loop(s) if path == "loop" else drive.per_step(s, 40.0, STEPS, model=0, M_sim=25)
                rec = s.get_launch_record()
                kernels += [rec["steps"], rec["steps_form"], rec["steps_slots"]] if path == "loop" else [rec["qp"], rec["qp_form"], rec["qp_slots"]]
                res.update({f"b{B}_{tol}_{path}_hist_{k}": v for k, v in h.items()})
                res.update({f"b{B}_{tol}_{path}_{k}": v for k, v in left_behind(s).items()})
                s.free()
            res[f"b{B}_{tol}_kernels"] = np.array(kernels)
    np.savez(out, **res)
    print(f"element_round_trips_child: IHM2MPC_QP_FORM={os.environ.get('IHM2MPC_QP_FORM', 'unset')} done", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
