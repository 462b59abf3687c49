"""The reference of tests/test_gpu_sim_sens.py, certified on the CPU: ``orc.rk4_sens`` against central differences of ``orc.rk4`` on the
benign states of ``sample_x0``, models 0 and 2, RK4 x 25, Gauss-Legendre x 4 and Radau IIA x 4.  What it measures is the error of the
difference quotient that the GPU test's own central-difference check (of ``ihm2mpc_sim_step``, no oracle involved) may show:
``sim_sens_cases.FD_WORST``; both tests assert ten times that figure."""
import numpy as np
import pytest

import sim_sens_cases as SC


@pytest.mark.parametrize("integ", [i[0] for i in SC.INTEGRATORS])
@pytest.mark.parametrize("model", [0, 2])
def test_sensitivities_are_the_derivative_of_the_step(track, model, integ):
    from oracle import oracle as orc

    _, code, _, M = next(i for i in SC.INTEGRATORS if i[0] == integ)
    x, u = SC.fd_cases(track)

    def step(xs, us):
        return np.stack([orc.rk4(model, a, b, track.s_ref, track.kappa_ref, SC.DT, M, integrator=code) for a, b in zip(xs, us)])

    ref = np.empty((len(x), 8, 10))
    for i in range(len(x)):
        xn, A, Bm = orc.rk4_sens(model, x[i], u[i], track.s_ref, track.kappa_ref, SC.DT, M, integrator=code)
        ref[i] = np.hstack([A, Bm])
        np.testing.assert_allclose(xn, step(x[i:i + 1], u[i:i + 1])[0], rtol=1e-13, atol=0)          # one map, with and without sensitivities
    err = SC.column_error(SC.central_differences(step, x, u), ref)
    print(f"model {model} {integ}: central differences against rk4_sens, worst {err:.3e} (FD_WORST {SC.FD_WORST:.1e})")
    assert err <= SC.FD_WORST, "the measured figure moved: update sim_sens_cases.FD_WORST and NOTES.md"
