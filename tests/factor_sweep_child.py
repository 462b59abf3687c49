"""Child process of tests/test_gpu_factor_sweep_forms.py: the reference's OCP at N = 40, B = 8, one solve() and three persistent
control steps, everything the two produce written to an .npz.  The form of the factor sweep is chosen by IHM2MPC_QP_FORM in the
environment the parent gives the child (the library reads it once per process).  usage: factor_sweep_child.py out.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from conftest import make_ocp, sample_x0  # noqa: E402


def main(out):
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table

    track = track_table("fsds_competition_1")
    B = 8
    os.environ["IHM2MPC_BLOCK_QP"] = "0"
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_lap_wrap(True)
    x0 = sample_x0(track, B, seed=31)
    s.set_x0(x0); s.init_guess()
    s.prepare_step(40.0)
    res = {}
    st = s.solve()
    rec = s.get_launch_record()
    pi, lam = s.get_multipliers()
    res.update(a_status=st, a_qp_iter=s.get_qp_iter(), a_x=s.get_x(), a_u=s.get_u(), a_pi=pi, a_lam=lam)
    h = s.run_steps(40.0, 3, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
    rec2 = s.get_launch_record()
    pi, lam = s.get_multipliers()
    res.update(b_status=h["status"], b_qp_iter=h["qp_iter"], b_u0=h["u0"], b_x0=h["x0"], b_x=s.get_x(), b_u=s.get_u(), b_pi=pi, b_lam=lam)
    res["kernels"] = np.array([rec["qp"], rec["qp_form"], rec2["steps"], rec2["steps_form"]])
    s.free()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
