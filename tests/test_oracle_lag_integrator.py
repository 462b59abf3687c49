"""Pins the integrator IHM2MPC_INTEG_ERK_LAG on the CPU: the host function that evaluates the lags' stage factors against an
extended-precision evaluation, and the NumPy restatement of the map (tests/lag_ref.py, which the GPU tests compare the kernels with)
against a stiff reference, finite differences and the structure of RK4's record."""
import ctypes as C

import numpy as np
import pytest
from conftest import random_state
from scipy.integrate import solve_ivp

import lag_ref
from layouts import RATE
from oracle import models_np as mnp
from oracle import oracle as orc

DT = 0.05


def _factors(h, tau):
    from ihm2_amd import _lib

    out = np.zeros(4)
    assert _lib.load().ihm2mpc_lag_stage_factors(C.c_double(h), C.c_double(tau), out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out


def test_stage_factors_match_extended_precision():
    """1e-13 relative for r = h / tau from 1e-3 to 50 (both branches of the evaluation: the series below r = 1, the closed forms above)."""
    worst = 0.0
    for tau in (1e-3, 0.02):
        for r in np.concatenate([np.geomspace(1e-3, 50.0, 200), [0.999999, 1.0, 1.000001]]):
            got = _factors(r * tau, tau)
            ref = lag_ref.stage_factors_ld(r * tau, tau)
            worst = max(worst, float(np.max(np.abs((got - ref) / ref))))
    print(f"stage factors: max relative deviation from np.longdouble {worst:.2e}")
    assert worst < 1e-13


def test_stage_factors_check_value():
    got = _factors(12.5e-3, 1e-3)
    np.testing.assert_allclose(got[:3], (0.37708781, 0.03225617, -0.02611426), rtol=0, atol=5e-9)
    assert got[3] == pytest.approx(np.exp(-12.5), rel=1e-15)
    # the defining property: Simpson's rule with these stage values integrates the transient's first three moments exactly
    h, tau = 12.5e-3, 1e-3
    E = lag_ref.stage_factors_ld(h, tau)
    r = np.longdouble(h) / np.longdouble(tau); e = np.exp(-r); t = np.longdouble(tau)
    m = (t * (1 - e), t * t * (1 - e * (1 + r)), 2 * t ** 3 * (1 - e * (1 + r + r * r / 2)))
    for j in range(3):
        simpson = h / 6 * ((0.0 if j else 1.0) * E[0] + 4 * (h / 2) ** j * E[1] + h ** j * E[2])
        assert float(abs(simpson - m[j]) / m[j]) < 1e-15


def test_stage_factors_refuse_bad_arguments():
    from ihm2_amd import _lib

    out = np.zeros(4)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    for h, tau in ((0.0, 1e-3), (-1.0, 1e-3), (1e-3, 0.0), (float("nan"), 1e-3), (1e-3, float("inf"))):
        assert _lib.load().ihm2mpc_lag_stage_factors(C.c_double(h), C.c_double(tau), p) != 0


@pytest.fixture(scope="module")
def flows(track):
    """60 random_state draws with rate-feasible inputs (|u - x[6:8]| <= RATE): the Radau reference at rtol 1e-13 and the errors of the
    schemes against it, max over states of |err| / (1 + |ref|)."""
    rng = np.random.default_rng(2024)
    err = {"lag4": [], "lag8": [], "point4": []}
    for _ in range(60):
        x, _ = random_state(rng)
        u = x[6:8] + np.array([rng.uniform(*RATE[0]), rng.uniform(*RATE[1])])
        sol = solve_ivp(lambda t, y: mnp.fkin6(y, u, track.s_ref, track.kappa_ref), (0.0, DT), x, method="Radau", rtol=1e-13, atol=1e-14)
        ref = sol.y[:, -1]
        rel = lambda xn: float(np.max(np.abs(xn - ref) / (1 + np.abs(ref))))        # noqa: E731
        err["lag4"].append(rel(lag_ref.lag_step(x, u, track.s_ref, track.kappa_ref, DT, 4)))
        err["lag8"].append(rel(lag_ref.lag_step(x, u, track.s_ref, track.kappa_ref, DT, 8)))
        err["point4"].append(rel(lag_ref.lag_step(x, u, track.s_ref, track.kappa_ref, DT, 4, pointwise=True)))
    out = {k: max(v) for k, v in err.items()}
    print("ERK_LAG against Radau, rate-feasible inputs: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()))
    return out


def test_converges_to_stiff_reference(flows):
    """M = 4 below 1e-5 at rate-feasible inputs (measured 2.2e-6 when the scheme was proposed; this seed: see NOTES.md), and no worse at M = 8."""
    assert flows["lag4"] < 1e-5
    assert flows["lag8"] <= flows["lag4"]


def test_fitted_stage_values_beat_the_pointwise_closed_form(flows):
    """At the same M = 4 the moment-fitted stage values are at least 5x closer to the reference than the closed form sampled at the
    stage times (measured 15x)."""
    assert flows["point4"] >= 5.0 * flows["lag4"]


@pytest.mark.parametrize("M", [1, 4, 7])
def test_sensitivities_match_finite_differences(track, M):
    """The column-scaled 1e-5 rule of test_oracle_integrator.py::test_sensitivities_match_finite_differences."""
    rng = np.random.default_rng(11)
    for _ in range(3):
        x, u = random_state(rng)
        x[3] = rng.uniform(4, 15)
        xn, A, Bm = lag_ref.lag_step(x, u, track.s_ref, track.kappa_ref, DT, M, sens=True)
        S = np.hstack([A, Bm])
        Sfd = np.zeros((8, 10))
        for j in range(10):
            h = (1e-5, 1e-5, 1e-5, 1e-5, 1e-5, 1e-5, 1e-1, 1e-5, 1e-1, 1e-5)[j]
            xp, up, xm, um = x.copy(), u.copy(), x.copy(), u.copy()
            if j < 8:
                xp[j] += h; xm[j] -= h
            else:
                up[j - 8] += h; um[j - 8] -= h
            fp = lag_ref.lag_step(xp, up, track.s_ref, track.kappa_ref, DT, M)
            fm = lag_ref.lag_step(xm, um, track.s_ref, track.kappa_ref, DT, M)
            Sfd[:, j] = (fp - fm) / (2 * h)
        err = np.abs(S - Sfd) / (1e-6 + np.abs(Sfd).max(axis=0, keepdims=True))
        assert err.max() < 1e-5, err.max()
        np.testing.assert_allclose(xn, lag_ref.lag_step(x, u, track.s_ref, track.kappa_ref, DT, M), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("M", [1, 4, 25])
def test_lag_rows_are_exact(track, M):
    x, u = random_state(np.random.default_rng(5))
    _, A, Bm = lag_ref.lag_step(x, u, track.s_ref, track.kappa_ref, DT, M, sens=True)
    eT, ed = np.exp(-DT / 1e-3), np.exp(-DT / 0.02)
    assert abs(A[6, 6] - eT) < 1e-14 and abs(Bm[6, 0] - (1 - eT)) < 1e-14
    assert abs(A[7, 7] - ed) < 1e-14 and abs(Bm[7, 1] - (1 - ed)) < 1e-14


def test_zero_pattern_is_that_of_rk4(track):
    rng = np.random.default_rng(12)
    mask = lag_ref.structural_mask()
    for M in (1, 4):
        x, u = random_state(rng)
        _, A, Bm = lag_ref.lag_step(x, u, track.s_ref, track.kappa_ref, DT, M, sens=True)
        _, Ar, Br = orc.rk4_sens(orc.MODEL_FKIN6, x, u, track.s_ref, track.kappa_ref, DT, 25)
        S, Sr = np.hstack([A, Bm]), np.hstack([Ar, Br])
        assert np.array_equal(S != 0, Sr != 0)
        assert np.all(S[~mask] == 0) and np.all(S[mask] != 0)
        # test_oracle_integrator.py::test_block_triangular_structure_of_A
        assert np.all(A[3:, :3] == 0) and np.all(A[6:, :6] == 0)
        assert A[6, 7] == 0 and A[7, 6] == 0
        assert np.all(Bm[6:, :] == np.diag(np.diag(Bm[6:, :])))
