"""The 128-interval switch on hardware: ``linearize()`` and ``sim_step()`` at 128 intervals (N = 64, B = 2) and at 129 (N = 43, B = 3)
leave the two kernel names of tests/launch_cases.py in the launch record.  (Every other row of the table is asserted where a GPU test
runs its shape; tests/test_launch_select.py runs the selectors on all of them without a GPU.)"""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import launch_cases as LC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,N", [(2, 64), (3, 43)])
def test_both_kernels_at_the_boundary(track, B, N):
    from ihm2_amd.solver import BatchedOcpSolver

    s = BatchedOcpSolver(make_ocp(N=N), B, track.s_ref, track.kappa_ref)
    x0 = sample_x0(track, B, seed=5)
    s.set_x0(x0); s.init_guess()
    s.linearize()
    xn = s.sim_step(x0, np.zeros((B, 2)), model=0, M_sim=25)
    rec = s.get_launch_record()
    s.free()
    assert np.all(np.isfinite(xn))
    assert (rec["linearize"], rec["sim"]) == LC.names(s)
    assert (rec["linearize"] == "k_linearize_cols") == (rec["sim"] == "k_sim_step") == LC.latency_batch(B, N)
