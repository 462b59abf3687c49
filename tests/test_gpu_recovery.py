"""GPU: the Stanley warm start (``ihm2mpc_init_guess``) and the recovery of failed instances (``ihm2mpc_reinit_failed``) -- both
``kernels_misc.hip::k_init_guess`` -- against the float64 reference of tests/rollout_ref.py, and the state a recovery hands to the
next solve: a handle that runs ``solve -> reinit_failed -> solve`` must give, bit for bit, what a handle given the recovered warm start
with zero multipliers and slacks gives."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import rollout_ref as R

pytestmark = pytest.mark.gpu

N = 40
TRACKS = ("fsds_competition_1", "fsds_competition_2", "fsds_default")


def _rel(a, b):
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))


def _tracks(ntracks):
    from ihm2_amd.track import track_table

    plans = [track_table(t) for t in TRACKS[:ntracks]]
    return plans, np.stack([p.s_ref for p in plans]), np.stack([p.kappa_ref for p in plans])


def _x0(plans, tid, seed):
    x0 = np.zeros((len(tid), 8))
    for t, p in enumerate(plans):
        m = tid == t
        if m.any():
            x0[m] = sample_x0(p, int(m.sum()), seed=seed + t)
    return x0


# pairwise over model x integrator (ERK M=25, IRK GL4 with dt 0.05 / 0.1) x bounds (shared / per-instance, binding) x tracks (1 / 3)
# x v_ref_scale (1 / 0.7), on batches with a ragged last wavefront (63, 65, 200) and a batch of one
INIT_CASES = [
    ("fkin6", "ERK", 0.05, False, 1, 1.0, 63),
    ("fkin6", "IRK", 0.1, True, 3, 0.7, 65),
    ("fkin6", "IRK", 0.05, False, 3, 0.7, 1),
    ("fkin6", "ERK", 0.05, True, 1, 0.7, 200),
    ("fdyn6", "ERK", 0.05, True, 3, 1.0, 200),
    ("fdyn6", "IRK", 0.1, False, 1, 0.7, 63),
    ("fdyn6", "IRK", 0.05, True, 1, 1.0, 65),
    ("fdyn6u", "ERK", 0.05, False, 3, 0.7, 200),
    ("fdyn6u", "IRK", 0.05, True, 1, 0.7, 1),
    ("fdyn6u", "IRK", 0.1, True, 3, 1.0, 65),
    ("fdyn6u", "ERK", 0.05, True, 1, 1.0, 63),
]


def _ocp(model, integ, dt, **kw):
    if integ == "IRK":
        return make_ocp(model=model, M=1, integrator_type="IRK", tf=N * dt, **kw)
    return make_ocp(model=model, M=25, tf=N * dt, **kw)


@pytest.mark.parametrize("model,integ,dt,inst,ntracks,v_scale,B", INIT_CASES)
def test_init_guess_matches_the_reference_rollout(model, integ, dt, inst, ntracks, v_scale, B):
    from ihm2_amd.solver import BatchedOcpSolver
    from oracle import oracle as orc

    plans, s_ref, k_ref = _tracks(ntracks)
    tid = (np.arange(B) % ntracks).astype(np.int32)
    ocp = _ocp(model, integ, dt)
    data = ocp.flatten()
    s = BatchedOcpSolver(ocp, B, s_ref, k_ref, track_id=tid)
    x0 = _x0(plans, tid, 100 + B)
    ib = None
    if inst:
        ib = R.tight_bounds(data, B, seed=B)
        s.set_instance_bounds(**ib)
        x0[:, 6:8] = np.clip(x0[:, 6:8], 0.9 * ib["lbu"][:, 0], 0.9 * ib["ubu"][:, 0])
    s.set_x0(x0)
    s.init_guess(v_scale)
    x, u = s.get_x(), s.get_u()
    P = R.RolloutProblem.from_data(data, s_ref, k_ref, tid, ib)
    O = orc.OracleProblem(data.as_dict(s_ref, k_ref))
    assert np.array_equal(x[:, 0], x0)
    # the whole horizon from x0 alone; compared where the reference rollout is well posed (R.well_posed)
    xr, ur = R.rollout(P, x0, v_scale, oracle=O)
    ok = R.well_posed(P, x0, xr, v_scale, oracle=O)
    assert ok.mean() >= 0.8
    eh = max(_rel(x[ok], xr[ok]), _rel(u[ok], ur[ok]))
    # per interval, from the GPU's own x_k
    eu = ex = 0.0
    for k in range(N):
        eu = max(eu, _rel(u[ok, k], R.stanley_input(P, x[ok, k], x0[ok], v_scale, idx=np.flatnonzero(ok), k=k)))
        ex = max(ex, _rel(x[ok, k + 1], R.interval(P, x[ok, k], u[ok, k], False, idx=np.flatnonzero(ok), oracle=O)))
    print(f"\nINIT {model} {integ} dt={dt} inst={inst} tracks={ntracks} v_scale={v_scale} B={B}: {int(ok.sum())}/{B} compared, "
          f"u_k {eu:.2e}  x_k+1 {ex:.2e}  horizon {eh:.2e}")
    assert eu <= 1e-12 and ex <= 1e-11
    assert eh <= 1e-8
    if inst:        # the per-instance clamps bind (otherwise the case tests the shared path twice)
        act = x[:, :-1, 6:8]
        binds = (np.isclose(u, ib["lbu"], rtol=0, atol=1e-12) | np.isclose(u, ib["ubu"], rtol=0, atol=1e-12)
                 | np.isclose(u - act, ib["lg"], rtol=0, atol=1e-9) | np.isclose(u - act, ib["ug"], rtol=0, atol=1e-9))
        assert binds.mean() > 0.05


# ---- recovery ----

def _track_rows(ocp, soft, alat=False):
    """Nonlinear track rows (``lh = -1e3, uh = 0``), with ``alat`` the a_lat row |a_lat| <= 8 at the stages; ``soft``: every row soft,
    100/100 (bench.py configs[2])."""
    c = ocp.constraints
    nh = 3 if alat else 2
    ocp.model.con_h_expr = "track+a_lat" if alat else "track"
    c.lh = np.array([-1e3, -1e3, -A_MAX][:nh]); c.uh = np.array([0.0, 0.0, A_MAX][:nh])
    c.lh_e = np.array([-1e3, -1e3]); c.uh_e = np.array([0.0, 0.0])
    if soft:
        c.idxsh, c.idxsh_e = np.arange(nh), np.arange(2)
        ocp.cost.zl = ocp.cost.zu = ocp.cost.Zl = ocp.cost.Zu = np.full(nh, 100.0)
        ocp.cost.zl_e = ocp.cost.zu_e = ocp.cost.Zl_e = ocp.cost.Zu_e = np.full(2, 100.0)
    return ocp


A_MAX = 8.0


def _recovery_ocp(case):
    if case in ("hard", "block"):
        return make_ocp()
    if case == "track_soft":
        return _track_rows(make_ocp(), True)
    if case == "alat_hard":
        return _track_rows(make_ocp(), False, True)
    if case == "alat_soft":
        return _track_rows(make_ocp(), True, True)
    if case == "sqp_soft":        # soft n box and steering-rate row (test_gpu_sqp.py), one SQP iteration: status 2 where it does not converge
        ocp = make_ocp(n_max=0.6, nlp_solver_type="SQP", globalization="MERIT_BACKTRACKING", nlp_solver_max_iter=1, nlp_tol=1e-3,
                       nlp_solver_tol_eq=1e-8, nlp_solver_tol_ineq=1e-8)
        c = ocp.constraints
        c.idxsbx = np.array([0]); c.idxsg = np.array([1])
        ocp.cost.zl = np.array([50.0, 5.0]); ocp.cost.zu = np.array([50.0, 5.0])
        ocp.cost.Zl = np.array([200.0, 20.0]); ocp.cost.Zu = np.array([200.0, 20.0])
        return ocp
    if case == "fdyn6u_cfg2":     # bench.py configs[2] fdyn6u: stage terminal box, soft track rows
        ocp = make_ocp(model="fdyn6u")
        c = ocp.constraints
        c.idxbx_e, c.lbx_e, c.ubx_e = c.idxbx.copy(), c.lbx.copy(), c.ubx.copy()
        return _track_rows(ocp, True)
    raise ValueError(case)


# (table, B, the statuses the batch must show after the failing solve, the QP kernel it runs)
RECOVERY_CASES = [
    ("hard", 65, (0, 1, 4), None),
    ("block", 3, (0, 1, 4), "k_qp_block"),
    ("track_soft", 63, (0, 1, 4), None),
    ("alat_hard", 66, (0, 1, 4), "k_qp_wave<8,0,2,1>"),
    ("alat_soft", 66, (0, 1, 4), "k_qp_wave<10,4,2,1>"),
    ("sqp_soft", 65, (0, 1, 2, 4), None),
    ("fdyn6u_cfg2", 200, (0, 1, 4), None),
]
FIELDS = R.STATE_FIELDS


def _state(s):
    pi, lam = s.get_multipliers()
    lam_a, slk_a = s.get_alat_multipliers()
    return dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), lam_a=lam_a, slk_a=slk_a)


def _handle(case, B, track, x0, yref, yref_e):
    from ihm2_amd.solver import BatchedOcpSolver

    ocp = _recovery_ocp(case)
    data = ocp.flatten()
    widths = np.array([[1.6, 1.5]]) if data.path_on else None
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=widths)
    if data.soft_Z is not None:
        s.set_soft(data.soft_z, data.soft_Z)
    s.set_x0(x0); s.init_guess()
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None); s.set_slacks(None)
    return s, data


def _inputs(track, B, case):
    x0 = sample_x0(track, B, seed=900 + B)
    x0[:, 3] = np.linspace(5.0, 12.0, B)
    x0[:, 5] = x0[:, 3] * np.interp(x0[:, 0], track.s_ref, track.kappa_ref)
    x0[:, 1] = np.clip(x0[:, 1], -0.3, 0.3)
    if case == "alat_hard":       # a hard row needs a start inside it
        from test_gpu_alat import _alat_np

        for _ in range(60):
            x0[:, 3] = np.where(np.abs(_alat_np(x0)) > 0.5 * A_MAX, 0.95 * x0[:, 3], x0[:, 3])
        x0[:, 5] = x0[:, 3] * np.interp(x0[:, 0], track.s_ref, track.kappa_ref)
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + 40.0 * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = x0[:, 0] + 40.0
    return x0, yref, yref_e


def _fail(B):
    """Instances given NaN data (status 1) and a steering angle the hard delta box cannot hold from stage 1 on (status 4)."""
    if B <= 3:
        return np.array([1]), np.array([2])
    return np.array([3, B - 1]), np.array([7, B // 2 + 1])


def _failed_batch(track, case, B, statuses, kernel, build):
    """Handle A after clean solves, a solve in which some instances fail, and reinit_failed; handle B of the same configuration,
    untouched.  Returns both handles, the rollout problem, x0, yref and the NaN yref of the failing solve, its statuses and A's state before / after."""
    from test_gpu_configs import _build

    x0, yref, yref_e = _inputs(track, B, case)
    with _build(build):
        A, data = _handle(case, B, track, x0, yref, yref_e)
        Bh, _ = _handle(case, B, track, x0, yref, yref_e)
    # clean solves first: every instance then carries multipliers and slacks a failed solve may leave behind (and in the SQP mode
    # some have converged: status 0 beside 2)
    for _ in range(3):
        A.solve()
    if data.nlp_solver_type == "SQP":       # a stationarity tolerance some instances meet: status 0 beside 2 (both handles)
        tol = (float(np.median(A.get_residuals()[:, 0])), 1e3, 1e3, 1e6)
        for h in (A, Bh):
            h.set_sqp_options("MERIT_BACKTRACKING", tol=tol)
    nan_rows, far_rows = _fail(B)
    # delta_0 = 1.2: with the 20 ms lag and |u_delta| <= 0.5, delta_1 >= 0.55 -- outside the hard box [-0.5, 0.5] of stage 1
    x0f = x0.copy(); x0f[far_rows, 7] = 1.2
    yref_bad = yref.copy(); yref_bad[nan_rows, 5, 1] = np.nan
    A.set_x0(x0f); A.set_yref(yref_bad)
    status = A.solve()
    if kernel is not None:
        assert A.get_launch_record()["qp"].startswith(kernel)
    seen = sorted(set(int(v) for v in status))
    print(f"\nRECOVERY {case} {build} B={B}: statuses {seen}, counts {np.bincount(status).tolist()}")
    for st in statuses:
        assert st in seen, f"status {st} does not occur: {seen}"
    before = _state(A)
    A.reinit_failed()
    after = _state(A)
    P = R.RolloutProblem.from_data(data, track.s_ref, track.kappa_ref, np.zeros(B, dtype=np.int32))
    return A, Bh, P, x0f, yref, yref_bad, status, before, after


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("case,B,statuses,kernel", RECOVERY_CASES)
def test_reinit_failed_matches_the_recovery_contract(track, case, B, statuses, kernel, build):
    """Selection (statuses 0 and 2 keep everything, bit for bit), cleared multipliers and slacks, and the recovery rollout."""
    A, Bh, P, x0f, _, _, status, before, after = _failed_batch(track, case, B, statuses, kernel, build)
    exp, sel = R.expected_after_recovery(P, before, status, x0f)
    assert sel.any() and (~sel).any()
    # selection: every kept instance is untouched, bit for bit
    for f in FIELDS:
        np.testing.assert_array_equal(after[f][~sel], before[f][~sel], err_msg=f)
    # cleared state
    for f in R.CLEARED_FIELDS:
        assert np.all(after[f][sel] == 0.0), f
    # rollout: per interval from the GPU's own x_k, and over the whole horizon
    assert np.array_equal(after["x"][sel, 0], x0f[sel])
    idx = np.flatnonzero(sel)
    idx = idx[R.well_posed(P, x0f[idx], exp["x"][idx], recovery=True, idx=idx)]
    assert len(idx) >= 0.8 * sel.sum()
    xg, ug = after["x"][idx], after["u"][idx]
    eu = ex = 0.0
    for k in range(N):
        eu = max(eu, _rel(ug[:, k], R.stanley_input(P, xg[:, k], x0f[idx], idx=idx, k=k)))
        ex = max(ex, _rel(xg[:, k + 1], R.interval(P, xg[:, k], ug[:, k], True, idx)))
    eh = max(_rel(xg, exp["x"][idx]), _rel(ug, exp["u"][idx]))
    print(f"RECOVERY {case} {build}: {int(sel.sum())} re-initialised, {len(idx)} compared, u_k {eu:.2e}  x_k+1 {ex:.2e}  horizon {eh:.2e}")
    assert eu <= 1e-12 and ex <= 1e-11 and eh <= 1e-8
    A.free(); Bh.free()


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("case,B,statuses,kernel", RECOVERY_CASES)
def test_step_after_reinit_failed_equals_a_clean_warm_start(track, case, B, statuses, kernel, build):
    """The next solve after a recovery is, bit for bit, that of a handle given the recovered warm start with zero multipliers and
    slacks where A recovered and A's own elsewhere: nothing of the failed iterate leaks into the next step."""
    A, Bh, P, x0f, yref, _, status, before, after = _failed_batch(track, case, B, statuses, kernel, build)
    sel = R.recovered(status)
    # next step, differential: handle B starts from A's recovered warm start with zero multipliers and slacks where A recovered
    give = {f: after[f].copy() for f in FIELDS}
    for f in R.CLEARED_FIELDS:
        give[f][sel] = 0.0
    Bh.set_x0(x0f); Bh.set_yref(yref); Bh.set_x(give["x"]); Bh.set_u(give["u"])
    Bh.set_multipliers(give["pi"], give["lam"]); Bh.set_slacks(give["slk"]); Bh.set_alat_multipliers(give["lam_a"], give["slk_a"])
    A.set_yref(yref)
    st_a, st_b = A.solve(), Bh.solve()
    np.testing.assert_array_equal(st_a, st_b)
    np.testing.assert_array_equal(A.get_qp_iter(), Bh.get_qp_iter())
    sa, sb = _state(A), _state(Bh)
    for f in FIELDS:
        np.testing.assert_array_equal(sa[f], sb[f], err_msg=f)
    np.testing.assert_array_equal(A.get_residuals(), Bh.get_residuals())
    A.free(); Bh.free()


def test_controller_recovery_keeps_the_rows_that_never_failed(track):
    """IHM2Controller(recover_failed=True) against recover_failed=False: rows that never failed give bit-identical u0 at every step,
    failed rows are NaN in both at the step they fail."""
    from ihm2_amd.controller import IHM2Controller

    B = 65
    x0, _, _ = _inputs(track, B, "hard")
    ctl = {r: IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, recover_failed=r) for r in (False, True)}
    for c in ctl.values():
        c.warm_start(x0)
    bad = np.array([4, 40])
    failed = np.zeros(B, dtype=bool)
    for step in range(4):
        x = x0.copy()
        if step == 1:
            x[bad, 3] = 36.0
        out = {r: c.compute_control(x) for r, c in ctl.items()}
        st = {r: c.last_status for r, c in ctl.items()}
        for r in (False, True):
            assert np.all(np.isnan(out[r][~np.isin(st[r], (0, 2))]))
        failed |= ~np.isin(st[False], (0, 2)) | ~np.isin(st[True], (0, 2))
        if step == 1:
            assert np.all(failed[bad])
        np.testing.assert_array_equal(out[False][~failed], out[True][~failed])
    assert (~failed).sum() >= B - 4
