"""Child process of tests/test_gpu_packed_reductions.py: the reference's OCP at N = 40 for every batch size named on the command line, in the
form of the QP that IHM2MPC_QP_FORM in the parent's environment chooses (the library reads it once per process).  Per batch size B, written to
an .npz under the keys "b<B>_<case>_<name>":
  * step, loop: one solve(), then three control steps through step() and, on a second handle from the same start, the same three in one
    run_steps launch (the start of tests/paired_rows_child.py);
  * clean, yref, x0, lam: ONE solve() from inputs the parent can hand to the oracle unchanged -- the shifted guess, yref, yref_e (the oracle's own
    prepare_step, pushed to the handle), x0 and the incoming multipliers -- and everything it leaves behind; the inputs are stored as "in_<name>".
    yref, x0, lam: instance NAN_AT of the batch has a NaN in that input, its neighbours are untouched.
usage: packed_reductions_child.py out.npz B [B ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from conftest import make_ocp, sample_x0  # noqa: E402

SEED, STEPS, NAN_AT = 31, 3, 1
CASES = ("clean", "yref", "x0", "lam")


def start(track, B):
    x0 = sample_x0(track, B, seed=SEED)
    x0[:, 3] = np.clip(x0[:, 3], 4.0, 12.0)
    return x0


def left_behind(s):
    pi, lam = s.get_multipliers()
    return dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, qp_iter=s.get_qp_iter(), status=s.get_status(), qp_res=s.get_qp_residuals(), res=s.get_residuals(),
                u0=s.get_u0())


def main(out, batches):
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table
    from oracle import oracle as orc

    track = track_table("fsds_competition_1")
    os.environ["IHM2MPC_BLOCK_QP"] = "0"
    res = {}
    for B in batches:
        x0 = start(track, B)
        kernels = []
        for path in ("step", "loop"):
            s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
            s.set_lap_wrap(True)
            s.set_x0(x0); s.init_guess()
            s.prepare_step(40.0)
            s.solve()
            if path == "loop":
                h = s.run_steps(40.0, STEPS, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
                rec = s.get_launch_record()
                kernels += [rec["steps"], rec["steps_form"], rec["steps_slots"]]
            else:
                h = dict(u0=[], x0=[], status=[], qp_iter=[])
                for _ in range(STEPS):
                    s.step(40.0, model=0, M_sim=25)
                    h["u0"].append(s.get_u0()); h["x0"].append(s.get_x0()); h["status"].append(s.get_status()); h["qp_iter"].append(s.get_qp_iter())
                rec = s.get_launch_record()
                kernels += [rec["qp"], rec["qp_form"], rec["qp_slots"]]
            got = dict(hist_u0=np.array(h["u0"]), hist_x0=np.array(h["x0"]), hist_status=np.array(h["status"]), hist_qp_iter=np.array(h["qp_iter"]), **left_behind(s))
            res.update({f"b{B}_{path}_{k}": v for k, v in got.items()})
            s.free()
        res[f"b{B}_kernels"] = np.array(kernels)

        # ---- single solves from inputs the oracle takes as they are ----
        s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        s.set_x0(x0); s.init_guess()
        x, u = s.get_x(), s.get_u()
        yref, yref_e = orc.prepare_step(s.N, x0, 40.0, x, u)       # shifts x, u in place
        at = min(NAN_AT, B - 1)
        for case in CASES:
            inp = dict(x=x.copy(), u=u.copy(), x0=x0.copy(), yref=yref.copy(), yref_e=yref_e.copy(), pi=np.zeros((B, s.N + 1, 8)), lam=np.zeros((B, s.N + 1, 28)))
            if case == "yref":
                inp["yref"][at, 7, 3] = np.nan
            elif case == "x0":
                inp["x0"][at, 1] = np.nan
            elif case == "lam":
                inp["lam"][at, 5, 8] = np.nan
            s.set_x0(inp["x0"]); s.set_x(inp["x"]); s.set_u(inp["u"]); s.set_yref(inp["yref"]); s.set_yref_e(inp["yref_e"])
            s.set_multipliers(inp["pi"], inp["lam"])
            s.solve()
            rec = s.get_launch_record()
            res[f"b{B}_{case}_kernels"] = np.array([rec["qp"], rec["qp_form"], rec["qp_slots"]])
            res.update({f"b{B}_{case}_{k}": v for k, v in left_behind(s).items()})
            res.update({f"b{B}_{case}_in_{k}": v for k, v in inp.items()})
        s.free()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], [int(b) for b in sys.argv[2:]])
