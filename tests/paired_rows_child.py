"""Child process of tests/test_gpu_paired_rows.py: the reference's OCP at N = 40 for every batch size named on the command line -- one
solve(), then three control steps through step() and, on a second handle from the same start, the same three in one run_steps launch;
what the two paths leave behind written to an .npz, keys "b<B>_<path>_<name>".  The form of the QP (and with it the layout of the M_k
rows in the workspace) is chosen by IHM2MPC_QP_FORM in the environment the parent gives the child: the library reads it once per process.
usage: paired_rows_child.py out.npz B [B ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from conftest import make_ocp, sample_x0  # noqa: E402

SEED, STEPS = 31, 3      # (the seed, the plant and its sub-steps of tests/slot_forms_child.py)


def main(out, batches):
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table

    track = track_table("fsds_competition_1")
    os.environ["IHM2MPC_BLOCK_QP"] = "0"
    res = {}
    for B in batches:
        x0 = sample_x0(track, B, seed=SEED)
        x0[:, 3] = np.clip(x0[:, 3], 4.0, 12.0)
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
            pi, lam = s.get_multipliers()
            got = dict(hist_u0=np.array(h["u0"]), hist_x0=np.array(h["x0"]), hist_status=np.array(h["status"]), hist_qp_iter=np.array(h["qp_iter"]),
                       x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, qp_iter=s.get_qp_iter(), status=s.get_status())
            res.update({f"b{B}_{path}_{k}": v for k, v in got.items()})
            s.free()
        res[f"b{B}_kernels"] = np.array(kernels)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], [int(b) for b in sys.argv[2:]])
