"""Child process of tests/test_gpu_workspace_poison.py::test_qp_forms: the reference layout at N = 40, B = 5, on a poisoned and a clean
handle and replayed on each (poison_cases.run_twin) -- three solve() calls, a step and three persistent steps.  The form of the factor sweep
and of the slot phases is chosen by IHM2MPC_QP_FORM in the environment the parent gives the child (the library reads it once per
process).  usage: poison_child.py 0|1|2|unset"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import conftest  # noqa: E402,F401  (puts the repository root on the path)

import layouts as L  # noqa: E402
import poison_cases as PC  # noqa: E402
import qp_forms as QF  # noqa: E402  (the forms both launch records must report; tests/test_qp_select.py runs them on this layout without a GPU)


def main(form):
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table

    track = track_table("fsds_competition_1")
    level = QF.NAMES[form]
    lay, B = PC.MISC_LAYOUT, PC.MISC_B
    x0, yref, yref_e = PC.qp_start(track, lay, B, PC.MISC_SEED)

    def make():
        with PC.environ(IHM2MPC_BLOCK_QP="0"):
            s = BatchedOcpSolver(L.make_ocp(lay), B, track.s_ref, track.kappa_ref)
        L.apply(s.data, lay)
        s._push_bounds()
        s.set_lap_wrap(True)
        return s

    def start(s):
        s.set_x0(x0); s.init_guess()
        s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
        return yref, yref_e

    def calls(s, tag):
        out = []
        for _ in range(3):
            s.solve_async()
            rec = s.get_launch_record()
            assert (rec["qp"], rec["qp_form"], rec["qp_slots"]) == QF.qp_record(level), rec
            out.append(PC.outputs(s))
        s.step(40.0, model=0, M_sim=25)
        out.append(PC.outputs(s))
        h = s.run_steps(40.0, 3, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
        rec = s.get_launch_record()
        assert (rec["steps"], rec["steps_form"], rec["steps_slots"]) == QF.steps_record(level), rec
        out += [{"hist_" + k: v for k, v in h.items()}, PC.outputs(s)]
        return out

    PC.run_twin(make, start, calls)
    print("forms ok", form)


if __name__ == "__main__":
    main(sys.argv[1])
