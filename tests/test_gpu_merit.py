"""The device's line search (csrc/sqp_body.hpp: k_line_search and the SQP instantiations' shared body) against the independent
merit-function reference of tests/merit_ref.py: per instance the accepted step length is a member of the reference's admissible set,
m(0), m(alpha), D and the infeasibility part read back by get_sqp_merit() lie within the rounding band, and the accepted iterate is the
interpolation between the start and the QP's full step.  The cases and their inputs are those tests/test_oracle_merit.py proves on the CPU."""
import pytest

import sqp_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(SC.CASES))
def test_gpu_line_search_lands_in_the_admissible_set_with_the_reference_merit_values(track, name):
    c = SC.make_case(track, name)
    fig, refs, walks = SC.judge(c, SC.GpuDut(c))
    assert fig["worst"] <= 1.0
    # the case sees its terms through the device's (wider) band as well: the reference without one of them is rejected
    for drop in c.targets:
        assert SC.mutant_is_rejected(refs, walks, drop), (name, drop)


def test_merit_read_back_is_zero_without_a_line_search_and_refused_before_a_solve(track):
    import numpy as np
    from ihm2_amd.solver import BatchedOcpSolver

    c = SC.make_case(track, "hard_plain")
    ocp, _ = SC.case_ocp(c.model, c.variant, c.N, dict(globalization="FIXED_STEP", nlp_solver_max_iter=1))
    s = BatchedOcpSolver(ocp, c.B, c.s_ref, c.kappa_ref)
    with pytest.raises(RuntimeError, match="no SQP-mode solve"):
        s.get_sqp_merit()
    s.set_x0(c.x0); s.set_x(c.x); s.set_u(c.u); s.set_yref(c.yref); s.set_yref_e(c.yref_e)
    s.solve()
    np.testing.assert_array_equal(s.get_sqp_merit(), np.zeros((c.B, 4)))


def test_instances_that_meet_the_tolerances_are_left_alone(track):
    """Status 0, no iteration counted, step length 1, the iterate and the multipliers bit for bit, zeros in the merit read-back."""
    c = SC.make_case(track, "all_converged")
    fig, _, _ = SC.judge(c, SC.GpuDut(c), conditions=False)
    assert fig["ladder"] == 0
