"""GPU: per-instance weights and bound values in one batch (ihm2mpc_set_instance_weights / _bounds).  A mixed batch must give, for every
instance, bit for bit what a handle gives whose batch-shared tables hold that instance's tuning; the oracle agrees per tuning; the limits
are honoured; NULL restores the shared tables; bad input is refused."""
import numpy as np
import pytest
from conftest import sample_x0

pytestmark = pytest.mark.gpu
N = 40
K = 4

# four tunings: different limits; tuning 2 has a non-diagonal symmetric W (its stage Hessian has a row with four non-zeros: the dense
# H path of the QP runs beside the sparse one in the same launch)
TUNINGS = [
    dict(n_max=2.0, v_x_max=31.0, T_max=500.0, delta_max=0.5, delta_dot_max=1.0, q={}),
    dict(n_max=1.5, v_x_max=12.0, T_max=300.0, delta_max=0.4, delta_dot_max=0.8, q=dict(q_n=10.0, q_s_f=500.0)),
    dict(n_max=1.8, v_x_max=10.0, T_max=200.0, delta_max=0.35, delta_dot_max=0.6, q=dict(q_delta=50.0), offdiag=0.1),
    dict(n_max=2.2, v_x_max=14.0, T_max=400.0, delta_max=0.45, delta_dot_max=1.2, q=dict(q_v_x=3.0, q_delta_dot=200.0)),
]

CASES = {
    "fkin6_erk": dict(),
    "soft_state": dict(terminal_bounds="stage", soft_state_bounds=(1000.0, 1000.0)),
    "track_rows": dict(track_rows=True),
    "alat": dict(track_rows=True, lateral_acceleration_row=True),
    "fdyn6u": dict(model="fdyn6u"),
    "irk_gl4": dict(opts=dict(integrator_type="IRK", sim_method_num_steps=1)),
    "live": dict(opts=dict(nlp_solver_type="SQP", nlp_solver_max_iter=2, globalization="MERIT_BACKTRACKING", integrator_type="IRK",
                           sim_method_num_steps=1)),
}


def _weights(t):
    from ihm2_amd import ocp as O

    W, W_e = O.default_weights(**t["q"])
    if t.get("offdiag"):
        for j in (1, 2, 3):
            W[0, j] = W[j, 0] = t["offdiag"]
    return W, W_e


def _ocp(t, case, nknots):
    """The OCP of tuning t (weights, limits) for a test case."""
    from ihm2_amd import ocp as O
    from ihm2_amd.controller import controller_ocp

    c = CASES[case]
    lim = dict(n_max=t["n_max"], v_x_max=t["v_x_max"], T_max=t["T_max"], delta_max=t["delta_max"], T_dot_max=1e6,
               delta_dot_max=t["delta_dot_max"])
    if c.get("model", "fkin6") == "fkin6":
        _, ocp = controller_ocp(nknots, N, lim, terminal_bounds=c.get("terminal_bounds", "reference"), soft_state_bounds=c.get("soft_state_bounds"),
                                track_rows=c.get("track_rows", False),
                                lateral_acceleration_row=c.get("lateral_acceleration_row", False))
    else:
        mdl = O.get_acados_model_from_explicit_dynamics("ihm2_" + c["model"], O.fdyn6u_model, 8, 2, 2 * nknots)
        ocp = O.get_acados_ocp(mdl, N, *lim.values())
    ocp.cost.W, ocp.cost.W_e = _weights(t)
    ocp.solver_options.tf = N * 0.05
    ocp.solver_options.sim_method_num_steps = 25
    for k, v in c.get("opts", {}).items():
        setattr(ocp.solver_options, k, v)
    return ocp


def _widths(case):
    return np.array([[1.6, 1.5]]) if CASES[case].get("track_rows") else None


def _solver(track, ocp, B, case):
    from ihm2_amd.solver import BatchedOcpSolver

    return BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=_widths(case))


def _set_mixed(s, ocps, assign):
    W = np.stack([np.asarray(ocps[j].cost.W, dtype=float) for j in assign])
    W_e = np.stack([np.asarray(ocps[j].cost.W_e, dtype=float) for j in assign])
    s.set_instance_weights(W, W_e)
    flat = [o.flatten() for o in ocps]
    s.set_instance_bounds(**{k: np.stack([getattr(flat[j], k) for j in assign]) for k in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")})


def _x0(track, B, seed=7):
    x0 = sample_x0(track, B, seed=seed)
    x0[:, 3] = np.minimum(x0[:, 3], 9.0)        # inside every tuning's v_x_max
    x0[:, 6] = np.clip(x0[:, 6], -150.0, 150.0)
    return x0


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)), initial=0.0))


def _run(s, x0, steps=5):
    s.set_x0(x0)
    s.init_guess()
    out = []
    for _ in range(steps):
        s.prepare_step(40.0)
        st = s.solve()
        pi, lam = s.get_multipliers()
        out.append(dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), status=st, qp_iter=s.get_qp_iter(),
                        res=s.get_residuals()))
    return out


def _assert_rows_equal(mixed, homo, rows):
    for m, h in zip(mixed, homo):
        for k in m:
            np.testing.assert_array_equal(m[k][rows], h[k], err_msg=k)


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("B", [512, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_mixed_batch_equals_homogeneous_handles(track, case, B, build):
    from test_gpu_configs import _build

    nk = track.s_ref.shape[-1]
    ocps = [_ocp(t, case, nk) for t in TUNINGS]
    assign = np.arange(B) % K
    x0 = _x0(track, B)
    with _build(build):
        s = _solver(track, ocps[0], B, case)
        _set_mixed(s, ocps, assign)
        mixed = _run(s, x0)
        s.free()
        for j in range(K):
            rows = np.flatnonzero(assign == j)
            if rows.size == 0:
                continue
            h = _solver(track, ocps[j], rows.size, case)
            homo = _run(h, x0[rows])
            h.free()
            _assert_rows_equal(mixed, homo, rows)
    assert np.isin(mixed[-1]["status"], (0, 2)).mean() > 0.5       # (2: the SQP mode's iteration limit, accepted as python/main.py:326 does)


@pytest.mark.parametrize("plant", ["ERK", "IRK"])
def test_persistent_loop_mixed_equals_homogeneous(track, plant):
    nk = track.s_ref.shape[-1]
    ocps = [_ocp(t, "fkin6_erk", nk) for t in TUNINGS]
    for o in ocps:
        o.solver_options.sim_integrator_type = plant
        o.solver_options.sim_collocation_type = "GAUSS_RADAU_IIA"
    B = 256
    assign = np.arange(B) % K
    x0 = _x0(track, B, seed=11)

    def loop(s, x):
        s.set_x0(x)
        s.init_guess()
        h = s.run_steps(40.0, 50, M_sim=25 if plant == "ERK" else 1, freeze=True, u0_hist=True, x0_hist=True, status_hist=True,
                        qp_iter_hist=True)
        return h, s.get_x0()

    s = _solver(track, ocps[0], B, "fkin6_erk")
    _set_mixed(s, ocps, assign)
    hm, xm = loop(s, x0)
    s.free()
    for j in range(K):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, ocps[j], rows.size, "fkin6_erk")
        hh, xh = loop(h, x0[rows])
        h.free()
        for k in hm:
            np.testing.assert_array_equal(hm[k][:, rows], hh[k], err_msg=k)
        np.testing.assert_array_equal(xm[rows], xh)


def test_oracle_parity_and_limits_per_tuning(track):
    from oracle import oracle as orc

    nk = track.s_ref.shape[-1]
    ocps = [_ocp(t, "fkin6_erk", nk) for t in TUNINGS]
    B = 1024
    assign = np.arange(B) % K
    x0 = _x0(track, B, seed=3)
    s = _solver(track, ocps[0], B, "fkin6_erk")
    _set_mixed(s, ocps, assign)
    s.set_x0(x0)
    s.init_guess()
    x, u = s.get_x(), s.get_u()
    s.prepare_step(40.0)
    st = s.solve()
    xg, ug, it = s.get_x(), s.get_u(), s.get_qp_iter()
    yref, yref_e = orc.prepare_step(N, x0, 40.0, x, u)
    n_ok = n_same = 0
    for j, t in enumerate(TUNINGS):
        rows = np.flatnonzero(assign == j)
        P = orc.OracleProblem(ocps[j].flatten().as_dict(track.s_ref, track.kappa_ref))
        xo, uo = x[rows].copy(), u[rows].copy()
        out = P.rti_step(xo, uo, x0[rows], yref[rows], yref_e[rows])
        np.testing.assert_array_equal(st[rows], out["status"])
        ok = st[rows] == 0
        assert ok.mean() > 0.8
        d = np.abs(it[rows][ok] - out["qp_iter"][ok])
        assert d.max() <= 1
        same = d == 0
        n_ok += ok.sum(); n_same += same.sum()
        assert _rel(xg[rows][ok][same], xo[ok][same]) <= 1e-7
        assert _rel(ug[rows][ok][same], uo[ok][same]) <= 1e-7
        # the limits of each tuning are the ones in force
        uu = ug[rows][ok]
        assert np.all(uu[..., 0] <= t["T_max"] + 1e-8) and np.all(np.abs(uu[..., 1]) <= t["delta_max"] + 1e-8)
    assert n_same >= 0.999 * n_ok
    s.free()


def test_null_restores_shared_and_rebuilds_keep_instance_bounds(track):
    nk = track.s_ref.shape[-1]
    ocps = [_ocp(t, "fkin6_erk", nk) for t in TUNINGS]
    B = 128
    assign = np.arange(B) % K
    x0 = _x0(track, B, seed=5)
    # set, then NULL: the handle's results are those of one that never had per-instance data
    s = _solver(track, ocps[0], B, "fkin6_erk")
    _set_mixed(s, ocps, assign)
    s.set_instance_weights(None, None)
    s.set_instance_bounds()
    a = _run(s, x0, steps=3)
    s.free()
    r = _solver(track, ocps[0], B, "fkin6_erk")
    b = _run(r, x0, steps=3)
    r.free()
    _assert_rows_equal(a, b, np.arange(B))
    # per-instance bounds set BEFORE set_soft survive the slot table's rebuild
    soft_z = np.zeros((N + 1, 28)); soft_Z = np.full((N + 1, 28), -1.0)
    soft_Z[1:, [1, 15]] = 50.0; soft_z[1:, [1, 15]] = 10.0           # the n box soft on both sides
    s = _solver(track, ocps[0], B, "fkin6_erk")
    _set_mixed(s, ocps, assign)
    s.set_soft(soft_z, soft_Z)
    mixed = _run(s, x0, steps=3)
    s.free()
    for j in range(K):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, ocps[j], rows.size, "fkin6_erk")
        h.set_soft(soft_z, soft_Z)
        _assert_rows_equal(mixed, _run(h, x0[rows], steps=3), rows)
        h.free()


def test_refusals(track):
    from ihm2_amd._lib import Ihm2mpcError

    nk = track.s_ref.shape[-1]
    ocps = [_ocp(t, "fkin6_erk", nk) for t in TUNINGS]
    B = 8
    assign = np.arange(B) % K
    s = _solver(track, ocps[0], B, "fkin6_erk")
    flat = [o.flatten() for o in ocps]
    good = {k: np.stack([getattr(flat[j], k) for j in assign]) for k in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")}

    def bounds_with(name, idx, v):
        d = {k: a.copy() for k, a in good.items()}
        d[name][idx] = v
        return d

    with pytest.raises(Ihm2mpcError, match=r"instance 3, stage 5, row 8 .*finite sides"):
        s.set_instance_bounds(**bounds_with("ubu", (3, 5, 0), 1e20))        # pattern: an absent side where the table has one
    with pytest.raises(Ihm2mpcError, match=r"instance 2, stage 7, row 3 .*NaN"):
        s.set_instance_bounds(**bounds_with("lbx", (2, 7, 3), np.nan))
    with pytest.raises(Ihm2mpcError, match=r"instance 1, stage 4, row 9 .*lower bound"):
        s.set_instance_bounds(**bounds_with("lbu", (1, 4, 1), 0.9))
    W = np.stack([np.asarray(ocps[j].cost.W, dtype=float) for j in assign])
    W_e = np.stack([np.asarray(ocps[j].cost.W_e, dtype=float) for j in assign])
    Wb = W.copy(); Wb[6, 0, 1] = 1.0
    with pytest.raises(Ihm2mpcError, match=r"instance 6: .*not symmetric"):
        s.set_instance_weights(Wb, W_e)
    Wn = W.copy(); Wn[5, 2, 2] = np.nan
    with pytest.raises(Ihm2mpcError, match=r"instance 5: W\[2\]\[2\] is NaN"):
        s.set_instance_weights(Wn, W_e)
    with pytest.raises(ValueError):
        s.set_instance_weights(W[:-1], W_e)
    with pytest.raises(ValueError):
        s.set_instance_bounds(**{**good, "lbu": good["lbu"][:, :-1]})
    # nothing was taken over: the handle still solves with its shared tables
    s.set_x0(_x0(track, B))
    s.init_guess()
    s.prepare_step(40.0)
    s.solve()
    s.free()


def test_controller_arrays_equal_to_defaults_are_bit_identical(track):
    from ihm2_amd.closed_loop_sim import SimModelVariant, Simulator, SimulatorConfig, run_closed_loop_device
    from ihm2_amd.controller import LIMIT_NAMES, WEIGHT_NAMES, IHM2Controller

    B = 64
    x0 = _x0(track, B, seed=9)
    defaults = dict(n_max=2.0, v_x_max=31.0, T_max=500.0, delta_max=0.5, T_dot_max=1e6, delta_dot_max=1.0, q_s=1.0, q_n=1.0, q_psi=1.0,
                    q_v_x=1.0, q_v_y=1.0, q_r=1.0, q_T=1.0, q_delta=100.0, q_s_f=1000.0, q_n_f=100.0, q_psi_f=100.0, q_v_x_f=1.0,
                    q_v_y_f=1.0, q_r_f=1.0, q_T_f=1.0, q_delta_f=100.0, q_T_dot=0.0, q_delta_dot=500.0)
    assert set(defaults) == set(LIMIT_NAMES) | set(WEIGHT_NAMES)
    arrays = {k: np.full(B, v) for k, v in defaults.items()}
    res = []
    for kw in ({}, arrays):
        c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, **kw)
        c.warm_start(x0)
        us = [c.compute_control(x0) for _ in range(3)]
        res.append((np.array(us), c.last_status.copy(), c.x_pred))
        c.solver.free()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    loops = []
    for kw in ({}, arrays):
        c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, **kw)
        c.warm_start(x0)
        sim = Simulator(c, SimulatorConfig(sampling_time=c.dt, num_steps=25), SimModelVariant.KIN6)
        r = run_closed_loop_device(c, sim, x0, 20)
        loops.append((r.x, r.u, r.status))
        c.solver.free()
    for a, b in zip(*loops):
        np.testing.assert_array_equal(a, b)
