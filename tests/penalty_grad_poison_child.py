"""Child process of tests/test_gpu_penalty_grad.py::test_workspace_poison: ihm2mpc_eval_adjoint_sensitivities_p and
ihm2mpc_eval_cost_gradient_penalties on a poisoned and a clean handle and replayed on each (poison_cases.run_twin), bit for bit -- their
call-local workspace "penalty_grad_work" (zeta and the four gradients, every entry of which a kernel must write before it is copied out),
"slack_seed_work" and "cost_work" are NaN instead of zero on the poisoned handle.  A soft table and the lateral-acceleration row.
usage: penalty_grad_poison_child.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import conftest  # noqa: E402,F401  (puts the repository root on the path)

import numpy as np  # noqa: E402

import layouts as L  # noqa: E402
import poison_cases as PC  # noqa: E402


def main():
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table

    track = track_table("fsds_competition_1")
    B = 5
    for lay in (L.TABLE["soft_2_per_lane"][0], L.TABLE["alat_soft"][0]):
        N = lay.N
        x0, yref, yref_e = PC.qp_start(track, lay, B, 77)
        rng = np.random.default_rng(12)
        seed_x, seed_u = rng.standard_normal((B, 3, N + 1, 8)), rng.standard_normal((B, 3, N, 2))
        seed_s, seed_sa = rng.standard_normal((B, 3, N + 1, 28)), rng.standard_normal((B, 3, N + 1, 2))

        def make():
            s = BatchedOcpSolver(L.make_ocp(lay), B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
            L.apply(s.data, lay)
            s._push_bounds()
            s.set_x0_sensitivities(1)
            return s

        def start(s):
            s.set_x0(x0); s.init_guess()
            s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
            return yref, yref_e

        def calls(s, tag):
            out = []
            for _ in range(2):
                s.solve_async()
                out.append(s.eval_adjoint_penalty_sensitivities(seed_s=seed_s))            # NULL stage seeds, NULL seed_sa
                out.append(s.eval_adjoint_penalty_sensitivities(seed_x, None, None, seed_sa))
                out.append(s.eval_cost_gradient_penalties())
                out.append(s.eval_adjoint_penalty_sensitivities())                          # the two unit seeds on u_0
                out.append(s.eval_adjoint_penalty_sensitivities(None, seed_u[:, :1], seed_s[:, :1], seed_sa[:, :1]))
                out.append(PC.outputs(s, sens=True, adjoint=True))
            return out

        first = PC.run_twin(make, start, calls, accepted=(0, 2))
        assert np.isfinite(first[2]["cost"]).all()
        for k in ("soft_z", "soft_Z"):
            assert np.abs(np.nan_to_num(first[0][k])).max() > 0.0 and np.abs(np.nan_to_num(first[2][k])).max() > 0.0, k
    print("penalty grad poison ok")


if __name__ == "__main__":
    main()
