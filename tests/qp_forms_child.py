"""Child process of tests/qp_forms.py: the reference's OCP at N = 40 in the form of the QP that IHM2MPC_QP_FORM in the parent's environment
chooses (the library reads it once per process), everything it leaves behind written to an .npz:
  * "b<B>_<path>_<name>", B in PATH_BATCHES, path step | loop: one solve() from the clipped start, then three control steps through step()
    and, on a second handle from the same start, the same three in one run_steps launch; "b<B>_kernels": the launch records of both;
  * "sweep_a_<name>", "sweep_b_<name>", "sweep_kernels": B = 8 from the UNCLIPPED start on one handle -- after one solve(), and after three
    persistent steps behind it (the sequence of tests/test_gpu_factor_sweep_forms.py);
  * "b<B>_<case>_<name>", B in SOLVE_BATCHES, case clean | yref | x0 | lam: ONE solve() from inputs the parent can hand to the oracle
    unchanged -- the shifted guess, yref, yref_e (the oracle's own prepare_step, pushed to the handle), x0 and the incoming multipliers --
    with the inputs as "b<B>_<case>_in_<name>" and the launch record as "b<B>_<case>_kernels".  yref, x0, lam: instance NAN_AT of the batch
    has a NaN in that input, its neighbours are untouched.
usage: qp_forms_child.py out.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from conftest import make_ocp, sample_x0  # noqa: E402

import drive  # noqa: E402

SEED, STEPS, NAN_AT = 31, 3, 1
PATH_BATCHES, SOLVE_BATCHES, SWEEP_B = (3, 8, 67), (3, 67), 8
CASES = ("clean", "yref", "x0", "lam")


def left_behind(s):
    pi, lam = s.get_multipliers()
    return dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), qp_iter=s.get_qp_iter(), status=s.get_status(), qp_res=s.get_qp_residuals(),
                res=s.get_residuals(), u0=s.get_u0())


def main(out):
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table
    from oracle import oracle as orc

    track = track_table("fsds_competition_1")
    os.environ["IHM2MPC_BLOCK_QP"] = "0"
    res = {}

    def solved(B, x0):
        """a fresh handle after one solve() from x0"""
        s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        s.set_x0(x0); s.init_guess()
        s.prepare_step(40.0)
        s.solve()
        return s

    def loop(s):
        return s.run_steps(40.0, STEPS, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)

    for B in PATH_BATCHES:
        x0 = drive.clipped_start(track, B, SEED)
        kernels = []
        for path in ("step", "loop"):
            s = solved(B, x0)
            h = loop(s) if path == "loop" else drive.per_step(s, 40.0, STEPS, model=0, M_sim=25)
            rec = s.get_launch_record()
            kernels += [rec["steps"], rec["steps_form"], rec["steps_slots"]] if path == "loop" else [rec["qp"], rec["qp_form"], rec["qp_slots"]]
            res.update({f"b{B}_{path}_hist_{k}": v for k, v in h.items()})
            res.update({f"b{B}_{path}_{k}": v for k, v in left_behind(s).items()})
            s.free()
        res[f"b{B}_kernels"] = np.array(kernels)
        if B not in SOLVE_BATCHES:
            continue

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

    # ---- the factor sweep's sequence: one handle, the unclipped start ----
    s = solved(SWEEP_B, sample_x0(track, SWEEP_B, seed=SEED))
    rec = s.get_launch_record()
    pi, lam = s.get_multipliers()
    res.update(sweep_a_status=s.get_status(), sweep_a_qp_iter=s.get_qp_iter(), sweep_a_x=s.get_x(), sweep_a_u=s.get_u(), sweep_a_pi=pi, sweep_a_lam=lam)
    h = loop(s)
    rec2 = s.get_launch_record()
    pi, lam = s.get_multipliers()
    res.update(sweep_b_status=h["status"], sweep_b_qp_iter=h["qp_iter"], sweep_b_u0=h["u0"], sweep_b_x0=h["x0"], sweep_b_x=s.get_x(), sweep_b_u=s.get_u(),
               sweep_b_pi=pi, sweep_b_lam=lam)
    res["sweep_kernels"] = np.array([rec["qp"], rec["qp_form"], rec2["steps"], rec2["steps_form"]])
    s.free()
    np.savez(out, **res)
    print(f"qp_forms_child: IHM2MPC_QP_FORM={os.environ.get('IHM2MPC_QP_FORM', 'unset')} done", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
