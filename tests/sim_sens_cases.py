"""Shared by tests/test_oracle_sim_sens.py (no GPU) and tests/test_gpu_sim_sens.py: the benign pairs (x, u) the central-difference checks
run on, the difference quotient itself, and its measured error.

``FD_WORST`` is the worst error of the central difference of ``orc.rk4`` against ``orc.rk4_sens`` over ``fd_cases`` (models 0 and 2, the three
integrators), per-component step 1e-6 (1 + |z_j|), relative to the column scale -- measured by test_oracle_sim_sens.py, which prints it
and fails if it moves above this figure.  It is the truncation and cancellation of the difference quotient (a state with s of a few
hundred metres differenced over 1e-4 loses seven digits), not an error of either integrator; both tests assert 10 x this figure.

The collocation integrators take four steps here.  With ONE step over 0.05 s the three Newton iterations from K = 0 do not converge for
the dynamic model at two of these states, and the implicit-function sensitivities -- the derivative of the collocation solution, which
is what acados returns as well -- are then not the derivative of the truncated iteration that a difference quotient of the step sees
(measured: O(10) relative in the columns of v_y and r).  That is a property of the method, shared by the reference, not of a kernel;
the comparison of the kernels with ``orc.rk4_sens`` covers one step as well.
"""
import numpy as np

FD_WORST = 1.8e-4       # measured 1.72e-4 (fkin6, RK4 x 25, the column of T: its scale is exp(-h / t_T) small), see NOTES.md
FD_BOUND = 10 * FD_WORST
DT = 0.05
# (name, oracle integrator code, plant options of the handle, M_sim)
INTEGRATORS = (("ERK", 0, {}, 25),
               ("IRK_GL4", 1, dict(sim_integrator_type="IRK", sim_collocation_type="GAUSS_LEGENDRE"), 4),
               ("IRK_RADAU4", 2, dict(sim_integrator_type="IRK", sim_collocation_type="GAUSS_RADAU_IIA"), 4))


def fd_cases(track, B=12, seed=11):
    """x (B, 8) of conftest.sample_x0 and controls near them: u_T within the torque range, u_delta near the steering angle."""
    from conftest import sample_x0

    x = sample_x0(track, B, seed=seed)
    rng = np.random.default_rng(seed + 1)
    u = np.stack([rng.uniform(-100, 300, B), x[:, 7] + rng.uniform(-0.05, 0.05, B)], 1)
    return x, u


def central_differences(step, x, u):
    """[S_x S_u] (B, 8, 10) of ``step(x (B,8), u (B,2)) -> (B,8)`` by central differences with the step 1e-6 (1 + |z_j|) per component."""
    z = np.hstack([x, u])
    S = np.empty((len(x), 8, 10))
    for j in range(10):
        e = 1e-6 * (1.0 + np.abs(z[:, j]))
        zp, zm = z.copy(), z.copy()
        zp[:, j] += e
        zm[:, j] -= e
        S[:, :, j] = (step(zp[:, :8], zp[:, 8:]) - step(zm[:, :8], zm[:, 8:])) / (zp[:, j] - zm[:, j])[:, None]
    return S


def column_error(S, ref):
    """max over instances, rows and columns of |S - ref| relative to the column's largest entry in ref."""
    scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-30)
    return float((np.abs(S - ref) / scale).max())
