"""CPU: the float64 reference of the Stanley warm start and of the recovery rollout (tests/rollout_ref.py) pinned down without a GPU --
against the oracle's own Stanley guess, the exact solution of the actuator lags, a plain RK4 rollout on a fine grid, and the clamp
tables it must honour."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import rollout_ref as R

N = 40


def _rel(a, b):
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))


def _problem(track, B, ocp=None, inst_bounds=None, track_id=None):
    ocp = make_ocp() if ocp is None else ocp
    tid = np.zeros(B, dtype=np.int32) if track_id is None else track_id
    return R.RolloutProblem.from_data(ocp.flatten(), track.s_ref, track.kappa_ref, tid, inst_bounds), ocp


def test_substep_rules_and_models():
    P, _ = _problem(type("T", (), dict(s_ref=np.arange(3.0), kappa_ref=np.zeros(3)))(), 1)
    assert (R.substeps(P, False), R.substeps(P, True)) == (25, 4)
    P.integrator, P.dt = 1, 0.05
    assert R.substeps(P, False) == 25
    P.dt = 0.1
    assert (R.substeps(P, False), R.substeps(P, True)) == (50, 8)
    for model in (R.MODEL_FKIN6, R.MODEL_FDYN6, R.MODEL_FDYN6U):
        P.model = model
        assert R.rollout_model(P, True) == R.MODEL_FKIN6
        assert R.rollout_model(P, False) == (R.MODEL_FDYN6U if model == R.MODEL_FDYN6U else R.MODEL_FKIN6)


def test_normal_mode_equals_the_oracle_stanley_guess(track):
    """fkin6, M = 25, the reference's bounds, one track: where the two statements coincide they agree to rounding."""
    from oracle import oracle as orc

    B = 48
    P, ocp = _problem(track, B)
    O = orc.OracleProblem(ocp.flatten().as_dict(track.s_ref, track.kappa_ref))
    x0 = sample_x0(track, B, seed=5)
    x, u = R.rollout(P, x0, oracle=O)
    xs, us = orc.stanley_guess(O, track.s_ref, track.kappa_ref, x0, N, M=25)
    assert _rel(u, us) < 1e-13 and _rel(x, xs) < 1e-13
    assert np.array_equal(x[:, 0], x0)
    # the steering-rate row binds somewhere (otherwise this compares less than it claims)
    assert np.any(np.abs(np.abs(u[:, :, 1] - x[:, :-1, 7]) - 0.02) < 1e-12)


def test_closed_form_lag_step_is_the_exact_solution():
    """The recovery sub-steps compose to the exact solution of T' = (u_T - T) / t_T, delta' = (u_delta - delta) / t_delta over an
    interval, whatever the sub-step."""
    rng = np.random.default_rng(3)
    B = 64
    a0 = np.stack([rng.uniform(-500, 500, B), rng.uniform(-0.5, 0.5, B)], 1)
    u = np.stack([rng.uniform(-500, 500, B), rng.uniform(-0.5, 0.5, B)], 1)
    for dt, M in ((0.05, 4), (0.1, 8), (0.05, 1), (0.003, 7)):
        a = a0.copy()
        for _ in range(M):
            a = R.lag_exact(a, u, dt / M)
        exact = np.stack([u[:, i] + (a0[:, i] - u[:, i]) * np.exp(-dt / tau) for i, tau in enumerate((1e-3, 0.02))], 1)
        assert np.max(np.abs(a - exact) / np.maximum(np.abs(a0), np.abs(u))) < 1e-14
        # the lag states a full recovery sub-step leaves (the rest of the state plays no part in them)
        x = np.zeros((B, 8)); x[:, 3] = 5.0; x[:, 6:8] = a0
        s = np.linspace(0, 100, 11)
        for _ in range(M):
            x = R.rk4_substep(x, u, dt / M, s, np.zeros(11), True)
        assert np.max(np.abs(x[:, 6:8] - exact) / np.maximum(np.abs(a0), np.abs(u))) < 1e-14


def test_recovery_rollout_converges_to_plain_rk4(track):
    """On a fine grid (M = 2000) the closed-form-lag RK4 and classical RK4 of all eight states integrate the same ODE: they agree to
    1e-8.  At the recovery's own 4 sub-steps classical RK4 is unstable on the 1 ms torque lag; the closed form is not."""
    B, n = 16, 4
    P, _ = _problem(track, B)
    P.N = n
    x0 = sample_x0(track, B, seed=11)
    _, u = R.rollout(P, x0, recovery=True)
    idx = np.arange(B)
    fine = R.rk4_rollout_plain(P, x0, u, 2000)
    x = np.zeros_like(fine); x[:, 0] = x0
    for k in range(n):
        xm = x[:, k]
        for _ in range(2000):
            xm = R.rk4_substep(xm, u[:, k], P.dt / 2000, track.s_ref, track.kappa_ref, True)
        x[:, k + 1] = xm
    assert _rel(x, fine) < 1e-8
    # the recovery's own grid: close to the fine solution; classical RK4 on the same grid is not
    coarse = np.zeros_like(fine); coarse[:, 0] = x0
    for k in range(n):
        coarse[:, k + 1] = R.interval(P, coarse[:, k], u[:, k], True, idx)
    assert _rel(coarse[:, :, :6], fine[:, :, :6]) < 1e-2
    with np.errstate(all="ignore"):
        plain = R.rk4_rollout_plain(P, x0, u, R.substeps(P, True))
    assert not np.all(np.isfinite(plain)) or _rel(plain, fine) > 1.0


@pytest.mark.parametrize("recovery", [False, True])
def test_clamp_tables_are_honoured(track, recovery):
    """Every u_k lies in its own instance's box and rate row around x_k; the clamps bind; instance b's rollout is what a batch whose
    shared tables are b's gives."""
    from oracle import oracle as orc

    B = 12
    ocp = make_ocp()
    data = ocp.flatten()
    ib = R.tight_bounds(data, B, seed=21)
    P, _ = _problem(track, B, ocp, ib)
    O = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref))
    x0 = sample_x0(track, B, seed=8)
    x0[:, 6:8] = np.clip(x0[:, 6:8], 0.9 * ib["lbu"][:, 0], 0.9 * ib["ubu"][:, 0])     # actuators inside the box: box and rate row intersect
    x, u = R.rollout(P, x0, recovery=recovery, oracle=O)
    act = x[:, :-1, 6:8]
    tol = 1e-12
    assert np.all(u >= ib["lbu"] - tol) and np.all(u <= ib["ubu"] + tol)
    assert np.all(u - act >= ib["lg"] - tol) and np.all(u - act <= ib["ug"] + tol)
    for j, name in ((0, "torque"), (1, "steering")):
        on_box = np.isclose(u[:, :, j], ib["lbu"][:, :, j], rtol=0, atol=1e-12) | np.isclose(u[:, :, j], ib["ubu"][:, :, j], rtol=0, atol=1e-12)
        on_rate = (np.isclose(u[:, :, j] - act[:, :, j], ib["lg"][:, :, j], rtol=0, atol=1e-9)
                   | np.isclose(u[:, :, j] - act[:, :, j], ib["ug"][:, :, j], rtol=0, atol=1e-9))
        assert on_box.sum() >= 5 and on_rate.sum() >= 5, name
    for b in (0, 7):
        Pb = R.RolloutProblem(**{**P.__dict__, "track_id": P.track_id[b:b + 1],
                                  **{k: ib[k][b] for k in ("lbu", "ubu", "lg", "ug")}})
        xb, ub = R.rollout(Pb, x0[b:b + 1], recovery=recovery, oracle=O)
        assert np.array_equal(xb[0], x[b]) and np.array_equal(ub[0], u[b])


def test_several_tracks_and_the_recovery_contract(track):
    """Instances on three tracks roll out on their own tables; expected_after_recovery keeps the statuses 0 and 2 and clears the rest."""
    from ihm2_amd.track import track_table

    plans = [track] + [track_table(t) for t in ("fsds_competition_2", "fsds_default")]
    s_ref = np.stack([p.s_ref for p in plans]); k_ref = np.stack([p.kappa_ref for p in plans])
    B = 9
    tid = (np.arange(B) % 3).astype(np.int32)
    ocp = make_ocp(N=6)
    data = ocp.flatten()
    P = R.RolloutProblem.from_data(data, s_ref, k_ref, tid)
    x0 = np.zeros((B, 8))
    for t in range(3):
        x0[tid == t] = sample_x0(plans[t], 3, seed=30 + t)
    x, u = R.rollout(P, x0, recovery=True)
    for t in range(3):
        m = tid == t
        Pt = R.RolloutProblem.from_data(data, s_ref[t], k_ref[t], np.zeros(m.sum(), dtype=np.int32))
        xt, ut = R.rollout(Pt, x0[m], recovery=True)
        assert np.array_equal(xt, x[m]) and np.array_equal(ut, u[m])
    assert np.max(np.abs(x[tid == 1] - R.rollout(R.RolloutProblem.from_data(data, s_ref[0], k_ref[0], np.zeros(3, np.int32)),
                                                   x0[tid == 1], recovery=True)[0])) > 1e-6
    rng = np.random.default_rng(0)
    shapes = dict(x=(B, 7, 8), u=(B, 6, 2), pi=(B, 7, 8), lam=(B, 7, 28), slk=(B, 7, 28), lam_a=(B, 7, 2), slk_a=(B, 7, 2))
    before = {f: rng.standard_normal(sh) for f, sh in shapes.items()}
    status = np.array([0, 1, 2, 4, 3, 0, 2, 1, 0], dtype=np.int32)
    exp, sel = R.expected_after_recovery(P, before, status, x0)
    assert list(sel) == [False, True, False, True, True, False, False, True, False]
    for f in R.STATE_FIELDS:
        assert np.array_equal(exp[f][~sel], before[f][~sel])
    for f in R.CLEARED_FIELDS:
        assert np.all(exp[f][sel] == 0.0)
    assert np.array_equal(exp["x"][sel], x[sel]) and np.array_equal(exp["u"][sel], u[sel])
