"""The integrator IHM2MPC_INTEG_ERK_LAG on the GPU (RK4 on the vehicle states, the actuator lags in closed form): linearisation records
and the plant against the NumPy restatement tests/lag_ref.py, one RTI step end to end against the oracle's QP on those records, the
persistent loop against launches per step, the x0 sensitivities, the init guess and the refusals."""
import ctypes as C

import numpy as np
import pytest
from conftest import make_ocp, random_state, sample_x0

import drive
import lag_ref

pytestmark = pytest.mark.gpu

DT = 0.05
LAG = dict(integrator_type="ERK_LAG", sim_integrator_type="ERK_LAG")
# du_0/dx0 by k_sens against the adjoint's grad_x0 for the unit seeds: the bound of tests/test_gpu_adjoint.py (IDENTITY_TOL)
IDENTITY_TOL = 1.7e-10


def _rel(a, b, floor=1.0):
    return np.max(np.abs(a - b) / (floor + np.abs(b)))


def _record(s):
    rec = np.zeros(16, dtype=np.int32)
    assert s.lib.ihm2mpc_get_launch_record(s._h, rec.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    return [int(v) for v in rec]


def _two_tracks():
    from ihm2_amd.track import track_table

    plans = [track_table(t) for t in ("fsds_competition_1", "fsds_competition_2")]
    return plans, np.stack([p.s_ref for p in plans]), np.stack([p.kappa_ref for p in plans])


def _iterate(plans, tid, B, N, seed):
    """random_state draws for every (instance, stage), with the edge states of the issue spread over them: v_x = 0.5, s on a knot of the
    instance's table, s just past the lap seam."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, N + 1, 8)); u = np.zeros((B, N, 2))
    for b in range(B):
        for k in range(N + 1):
            x[b, k], uk = random_state(rng)
            if k < N:
                u[b, k] = uk
    flat = x[:, :N].reshape(-1, 8)
    owner = np.repeat(tid, N)
    flat[0::7, 3] = 0.5
    for j in range(1, len(flat), 5):
        p = plans[owner[j]]
        flat[j, 0] = p.s_ref[int(rng.integers(len(p.s_ref) // 3 + 2, 2 * len(p.s_ref) // 3 - 2))]
    for j in range(2, len(flat), 9):
        flat[j, 0] = plans[owner[j]].lap_length + 1e-3
    x[:, :N] = flat.reshape(B, N, 8)
    return x, u


@pytest.fixture(scope="module", params=[(3, 1), (3, 4), (3, 7), (67, 1), (67, 4), (67, 7)], ids=lambda p: f"B{p[0]}-M{p[1]}")
def case(request):
    """One handle per (B, M): its records and plant steps, and lag_ref's (computed once, shared by the tests below)."""
    from ihm2_amd.solver import BatchedOcpSolver

    B, M = request.param
    N = 5
    plans, s_ref, k_ref = _two_tracks()
    tid = (np.arange(B) % 2).astype(np.int32)
    x, u = _iterate(plans, tid, B, N, seed=100 + B)
    s = BatchedOcpSolver(make_ocp(N=N, M=M, **LAG), B, s_ref, k_ref, track_id=tid)
    s.set_x(x); s.set_u(u); s.linearize()
    A, Bm, b = s.get_linearization()
    rec = _record(s)
    xn = s.sim_step(x[:, 0].copy(), u[:, 0].copy(), model=0, M_sim=M)
    rec_sim = _record(s)
    # the defect against x_1 = 0 is Phi(x_0, u_0) itself
    x1 = x.copy(); x1[:, 1:] = 0.0
    s.set_x(x1); s.linearize()
    phi0 = s.get_linearization()[2][:, 0].copy()
    s.free()
    Ar, Br, br = lag_ref.linearize(x, u, s_ref, k_ref, DT, M, track_id=tid)
    return dict(B=B, M=M, x=x, u=u, A=A, Bm=Bm, b=b, rec=rec, rec_sim=rec_sim, xn=xn, phi0=phi0, Ar=Ar, Br=Br, br=br)


def test_records_match_lag_ref(case):
    """The tolerances of tests/test_gpu_parity.py::test_linearize_matches_oracle for RK4: 1e-10 relative to the column scale, 1e-11 on b."""
    A, Bm, b, Ar, Br, br = (case[k] for k in ("A", "Bm", "b", "Ar", "Br", "br"))
    assert case["rec"][15] & 15 == 5
    eA = np.max(np.abs(A - Ar) / np.maximum(np.abs(Ar).max(axis=2, keepdims=True), 1e-30))
    eB = np.max(np.abs(Bm - Br) / np.maximum(np.abs(Br).max(axis=2, keepdims=True), 1e-30))
    eb = np.max(np.abs(b - br))
    print(f"ERK_LAG records B={case['B']} M={case['M']}: A {eA:.2e} B {eB:.2e} b {eb:.2e}")
    assert eA < 1e-10 and eB < 1e-10
    assert eb < 1e-11
    mask = lag_ref.structural_mask()
    S = np.concatenate([A, Bm], axis=3)
    assert np.all(S[:, :, ~mask] == 0)          # structural zeros are exact
    assert np.all(np.isfinite(S))
    eT, ed = np.exp(-DT / 1e-3), np.exp(-DT / 0.02)
    assert np.max(np.abs(A[:, :, 6, 6] - eT)) < 1e-14 and np.max(np.abs(Bm[:, :, 6, 0] - (1 - eT))) < 1e-14
    assert np.max(np.abs(A[:, :, 7, 7] - ed)) < 1e-14 and np.max(np.abs(Bm[:, :, 7, 1] - (1 - ed))) < 1e-14


def test_plant_matches_lag_ref_and_the_record(case):
    """ihm2mpc_sim_step(model 0) under sim type 3 is lag_ref's map, and the bits of x_1 + b of the record (taken against x_1 = 0)."""
    assert (case["rec_sim"][15] >> 4) & 15 == 4
    want = case["br"][:, 0] + case["x"][:, 1]
    e = _rel(case["xn"], want)
    print(f"ERK_LAG plant B={case['B']} M={case['M']}: {e:.2e}")
    assert e < 1e-11
    np.testing.assert_array_equal(case["xn"], case["phi0"])


@pytest.fixture(scope="module")
def rti(track):
    """B = 8, N = 10, M = 4: one solve with x0 sensitivities on, and what the tests below read from it."""
    from ihm2_amd.solver import BatchedOcpSolver

    B, N = 8, 10
    ocp = make_ocp(N=N, M=4, **LAG)
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    x0 = sample_x0(track, B, seed=5)
    s.set_x0(x0); s.init_guess()
    x, u = s.get_x(), s.get_u()
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + 10.0 * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = x0[:, 0] + 10.0
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
    s.set_x0_sensitivities(1)
    status = s.solve()
    out = dict(ocp=ocp, B=B, N=N, x0=x0, x=x, u=u, yref=yref, yref_e=yref_e, status=status, qp_iter=s.get_qp_iter(), xg=s.get_x(), ug=s.get_u(),
               K0=s.get_x0_sensitivities()[1], adj=s.eval_adjoint_sensitivities())
    s.free()
    return out


def test_rti_step_matches_the_oracle_qp_on_lag_ref_records(rti, track):
    """OracleProblem.build_qp at the iterate, its A, Bm, b replaced by lag_ref's, orc.qp_solve, the step applied: x, u to 1e-7 as in the
    GPU-oracle tests of tests/test_gpu_parity.py, status and interior-point iteration count equal."""
    from oracle import oracle as orc
    from steps_cases import rti_status_of_qp

    B, N, x, u = rti["B"], rti["N"], rti["x"], rti["u"]
    desc = dict(rti["ocp"].flatten().as_dict(track.s_ref, track.kappa_ref))
    desc["integrator"], desc["M"] = orc.INTEG_RK4, 25          # (the oracle's own records are replaced below)
    P = orc.OracleProblem(desc)
    A, Bm, b = lag_ref.linearize(x, u, track.s_ref, track.kappa_ref, DT, 4)
    xo, uo = x.copy(), u.copy()
    status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    for i in range(B):
        qp = P.build_qp(x[i], u[i], rti["x0"][i], rti["yref"][i], rti["yref_e"][i])
        r = orc.qp_solve(qp["H"], qp["g"], A[i], Bm[i], b[i], qp["dx0"], qp["R"], qp["dl"], qp["du"], iter_max=P.p.ipm_iter_max, tol=P.p.ipm_tol,
                         mu0=P.p.ipm_mu0, tau0=P.p.ipm_tau0)
        iters[i] = r["iters"]
        status[i] = rti_status_of_qp(r)
        if status[i] == 0:
            xo[i] += r["dz"][:, :8]; uo[i] += r["dz"][:N, 8:]
    np.testing.assert_array_equal(rti["status"], status)
    np.testing.assert_array_equal(rti["qp_iter"], iters)
    ok = status == 0
    assert ok.sum() >= 6
    ex, eu = _rel(rti["xg"][ok], xo[ok]), _rel(rti["ug"][ok], uo[ok])
    print(f"ERK_LAG RTI step against the oracle QP: x {ex:.2e} u {eu:.2e}")
    assert ex < 1e-7 and eu < 1e-7
    assert np.abs(rti["xg"][ok] - x[ok]).max() > 1e-3          # a step was taken


def test_x0_sensitivities_equal_the_adjoint(rti):
    ok = (rti["status"] == 0) | (rti["status"] == 2)
    K0, g = rti["K0"], rti["adj"]["x0"]
    assert ok.any() and np.isfinite(K0[ok]).all() and np.isfinite(g[ok]).all()
    assert np.abs(K0[ok]).max() > 0
    e = float((np.abs(g[ok] - K0[ok]).max((1, 2)) / np.abs(K0[ok]).max((1, 2))).max())
    print(f"ERK_LAG du_0/dx0 against the adjoint's grad_x0: {e:.2e}")
    assert e <= IDENTITY_TOL


def _soften(ocp):
    c = ocp.constraints
    c.idxsbx = np.array([0]); c.idxsg = np.array([1])
    ocp.cost.zl = np.array([50.0, 5.0]); ocp.cost.zu = np.array([50.0, 5.0])
    ocp.cost.Zl = np.array([200.0, 20.0]); ocp.cost.Zu = np.array([200.0, 20.0])


@pytest.mark.parametrize("name,sim,M_sim,soft", [("lag_plant_on_lane_N", "ERK_LAG", 4, False), ("rk4_plant_own_phase", "ERK", 25, False),
                                                ("soft_table_per_step", "ERK_LAG", 4, True)])
def test_persistent_loop_equals_step_by_step(track, name, sim, M_sim, soft, monkeypatch):
    """B = 300, N = 10, M = 4, 5 steps: run_steps gives the bits of 5 x step.  The all-hard table takes k_steps<..., IRK = 2> (launch
    record [5] = 1, [11] = 2) with the plant on lane N (sim type 3) or in a phase of its own (RK4 x 25); a soft table has no such
    instantiation and goes per step ([13] = 1)."""
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    B, N, steps = 300, 10, 5
    x0 = sample_x0(track, B, seed=31)
    res = []
    for persistent in (False, True):
        ocp = make_ocp(N=N, M=4, n_max=0.6 if soft else 2.0, integrator_type="ERK_LAG", sim_integrator_type=sim)
        if soft:
            _soften(ocp)
        s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
        if soft:
            s.set_soft(s.data.soft_z, s.data.soft_Z)
        s.set_lap_wrap(True)
        s.set_x0(x0); s.init_guess()
        s.step(10.0, model=0, M_sim=M_sim)
        if persistent:
            h = s.run_steps(10.0, steps, model=0, M_sim=M_sim, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
            rec = _record(s)
            if soft:
                assert rec[5] == 2 and rec[13] == 1
            else:
                assert rec[5] == 1 and rec[11] == 2 and rec[13] == 0 and rec[10] == 0 and rec[12] == 0
        else:
            h = drive.per_step(s, 10.0, steps, model=0, M_sim=M_sim)
            rec = _record(s)
            assert rec[15] & 15 == 5 and (rec[15] >> 4) & 15 == (4 if sim == "ERK_LAG" else 2)
        res.append((h, s.get_x(), s.get_u(), s.get_multipliers()))
        s.free()
    (ha, xa, ua, ma), (hb, xb, ub, mb) = res
    for k in ("status", "qp_iter", "x0", "u0"):
        np.testing.assert_array_equal(ha[k], hb[k])
    np.testing.assert_array_equal(xa, xb); np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(ma[0], mb[0]); np.testing.assert_array_equal(ma[1], mb[1])
    assert np.isfinite(ha["x0"]).all() and (ha["status"] == 0).mean() > 0.8
    assert np.all(ha["x0"][-1, :, 0] != x0[:, 0])          # the cars moved


def test_init_guess_is_that_of_an_irk_handle(track):
    """ihm2mpc_init_guess on a type-3 handle with M = 4 does not roll out plain RK4 with 4 sub-steps (unstable on the torque lag): it
    takes the rule of the IRK handles, and gives their iterates."""
    from ihm2_amd.solver import BatchedOcpSolver

    B, N = 70, 10
    x0 = sample_x0(track, B, seed=9)
    out = []
    for opts in (dict(M=4, **LAG), dict(M=1, integrator_type="IRK")):
        s = BatchedOcpSolver(make_ocp(N=N, **opts), B, track.s_ref, track.kappa_ref)
        s.set_x0(x0); s.init_guess()
        out.append((s.get_x(), s.get_u()))
        s.free()
    (xa, ua), (xb, ub) = out
    assert np.isfinite(xa).all() and np.isfinite(ua).all()
    np.testing.assert_array_equal(xa, xb); np.testing.assert_array_equal(ua, ub)


def test_refusals(track):
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    for model in ("fdyn6", "fdyn6u"):
        with pytest.raises(_lib.Ihm2mpcError, match="ERK_LAG.*kinematic OCP model.*not for the dynamic models"):
            BatchedOcpSolver(make_ocp(N=10, M=4, model=model, integrator_type="ERK_LAG"), 4, track.s_ref, track.kappa_ref)
    with pytest.raises(_lib.Ihm2mpcError, match="ERK_LAG.*IHM2MPC_SQP_RTI only"):
        BatchedOcpSolver(make_ocp(N=10, M=4, integrator_type="ERK_LAG", nlp_solver_type="SQP", nlp_solver_max_iter=2), 4, track.s_ref, track.kappa_ref)
    # a dynamic plant under sim type 3, at every call that takes a plant model
    B = 4
    s = BatchedOcpSolver(make_ocp(N=10, M=4, **LAG), B, track.s_ref, track.kappa_ref)
    x0 = sample_x0(track, B, seed=2)
    s.set_x0(x0); s.init_guess()
    u = np.zeros((B, 2))
    msg = "plant integrator ERK_LAG.*kinematic plant \\(model 0\\) only"
    for model in (1, 2, -1, -2):
        with pytest.raises(_lib.Ihm2mpcError, match=msg):
            s.sim_step(x0, u, model=model, M_sim=4)
        with pytest.raises(_lib.Ihm2mpcError, match=msg):
            s.sim_advance(model=model, M_sim=4)
        with pytest.raises(_lib.Ihm2mpcError, match=msg):
            s.step(10.0, model=model, M_sim=4)
        with pytest.raises(_lib.Ihm2mpcError, match=msg):
            s.run_steps(10.0, 2, model=model, M_sim=4)
    with pytest.raises(_lib.Ihm2mpcError, match=msg):
        s.sim_step_dyn10(np.zeros((B, 15)), np.zeros((B, 5)), M_sim=4)
    assert np.isfinite(s.sim_step(x0, u, model=0, M_sim=1)).all()          # any M_sim >= 1 is accepted: no RK4 stability refusal
    s.free()
    # integrator type 4 does not exist
    d = make_ocp(N=10).flatten()
    for integ, sim in ((4, 0), (0, 4)):
        cfg = _lib.Config(batch=1, N=d.N, M=d.M, model=d.model, ntracks=1, nknots=len(track.s_ref), device=0, nlp_solver_type=0,
                          nlp_solver_max_iter=d.nlp_solver_max_iter, ipm_iter_max=d.ipm_iter_max, dt=d.dt, cost_scale_stage=d.cost_scale_stage,
                          ipm_tol=d.ipm_tol, ipm_mu0=d.ipm_mu0, ipm_tau0=d.ipm_tau0, nlp_tol=d.nlp_tol, integrator_type=integ, sim_integrator_type=sim)
        h = C.c_void_p()
        assert _lib.load().ihm2mpc_create(C.byref(cfg), C.byref(h)) != 0
        assert "unknown integrator type" in _lib.load().ihm2mpc_last_error().decode()


def test_python_layers_pass_the_integrator_through(track):
    """ocp.integrator_code, the IHM2Controller pass-through and AcadosSimOpts.integrator_type = "ERK_LAG" for the fkin6 sim model."""
    from ihm2_amd import ocp as O
    from ihm2_amd.controller import IHM2Controller
    from ihm2_amd.sim import AcadosSim, AcadosSimSolver

    assert O.integrator_code("ERK_LAG") == 3
    B = 3
    x0 = sample_x0(track, B, seed=4)
    ctrl = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, Nf=10, integrator_type="ERK_LAG", sim_integrator_type="ERK_LAG",
                          sim_method_num_steps=4)
    ctrl.solver.set_x0(x0); ctrl.solver.init_guess(); ctrl.solver.linearize()
    assert _record(ctrl.solver)[15] & 15 == 5
    u = np.tile([50.0, 0.01], (B, 1))
    want = lag_ref.sim_step(x0, u, track.s_ref, track.kappa_ref, ctrl.dt, 4)
    assert _rel(ctrl.solver.sim_step(x0, u, model=0, M_sim=4), want) < 1e-11
    ctrl.solver.free()
    sim = AcadosSim()
    sim.model = O.get_acados_model_from_explicit_dynamics("plant", O.fkin6_model, 8, 2, 2 * len(track.s_ref))
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.integrator_type = ctrl.dt, 4, "ERK_LAG"
    sim.parameter_values = np.concatenate([track.s_ref, track.kappa_ref])
    ss = AcadosSimSolver(sim, batch_size=B)
    ss.set("x", x0); ss.set("u", u)
    assert ss.solve() == 0
    assert _rel(ss.get("x"), want) < 1e-11
    sim.model = O.get_acados_model_from_explicit_dynamics("plant", O.fdyn6_model, 8, 2, 2 * len(track.s_ref))
    with pytest.raises(ValueError, match="ERK_LAG"):
        AcadosSimSolver(sim, batch_size=B)
