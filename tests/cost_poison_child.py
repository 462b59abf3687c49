"""Child process of tests/test_gpu_cost.py::test_workspace_poison: ihm2mpc_eval_cost and ihm2mpc_eval_cost_gradient on a poisoned and a
clean handle and replayed on each (poison_cases.run_twin), bit for bit -- their call-local workspace ("cost_work") and the adjoint
entries' seed buffers, which the cost kernel fills, are NaN instead of zero on the poisoned handle.  The all-hard reference layout with
shared and with per-instance weights, and a soft layout (cost only).  usage: cost_poison_child.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import conftest  # noqa: E402,F401  (puts the repository root on the path)

import numpy as np  # noqa: E402

import layouts as L  # noqa: E402
import poison_cases as PC  # noqa: E402


def _all_costs(s):
    from ihm2_amd import _lib
    from ihm2_amd.solver import _ptr

    c, st, sl = np.empty(s.B), np.empty((s.B, s.N + 1)), np.empty(s.B)
    _lib.check(s.lib.ihm2mpc_eval_cost(s._h, _ptr(c), _ptr(st), _ptr(sl)))
    return dict(cost=c, stage_cost=st, slack_cost=sl)


def main():
    from ihm2_amd import ocp as O
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table

    track = track_table("fsds_competition_1")
    B = 5
    W0, We0 = O.default_weights()
    f = 1.0 + 0.25 * (np.arange(B) % 3)
    for lay, per_instance, grad in ((L.Layout("cost_poison_hard", N=10), False, True), (L.Layout("cost_poison_hard", N=10), True, True),
                                    (L.TABLE["soft_2_per_lane"][0], False, False)):
        x0, yref, yref_e = PC.qp_start(track, lay, B, 77)

        def make():
            s = BatchedOcpSolver(L.make_ocp(lay), B, track.s_ref, track.kappa_ref)
            L.apply(s.data, lay)
            s._push_bounds()
            if per_instance:
                s.set_instance_weights(f[:, None, None] * W0[None], f[:, None, None] * We0[None])
            s.set_x0_sensitivities(1)
            return s

        def start(s):
            s.set_x0(x0); s.init_guess()
            s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
            return yref, yref_e

        def calls(s, tag):
            out = [_all_costs(s)]                   # before any solve
            for _ in range(2):
                s.solve_async()
                if grad:
                    out.append(s.eval_cost_gradient())
                out.append(_all_costs(s))
                out.append(PC.outputs(s, sens=True, adjoint=True))
            return out

        first = PC.run_twin(make, start, calls)
        assert all(np.isfinite(v).all() for v in first[0].values())
    print("cost poison ok")


if __name__ == "__main__":
    main()
