"""GPU: per-instance slack penalties in one batch (ihm2mpc_set_instance_soft / _alat_soft).  A mixed batch must give, for every
instance, bit for bit what a handle gives whose batch-shared penalties are that instance's -- the QP per step and in the persistent
loop, the SQP mode's merit, the cost and every gradient; the oracle agrees per tuning; NULL restores the shared table; a rebuilt slot
table keeps the values or makes the next solve refuse; bad input is refused with the instance, stage and side.
tests/test_oracle_instance_penalties.py shows on the CPU that these inputs tell the tunings apart."""
import numpy as np
import pytest

import instance_penalty_cases as IP
from test_gpu_instance_tuning import _rel

pytestmark = pytest.mark.gpu
K = IP.K


def _ocps(track, case, Nf=IP.N):
    nk = track.s_ref.shape[-1]
    return [IP.ocp_of(case, pen, nk, Nf) for pen in IP.PENALTIES]


def _solver(track, ocp, B, case):
    from ihm2_amd.solver import BatchedOcpSolver

    return BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=IP.widths(case))


def _set_mixed(s, ocps, assign):
    soft, alat = IP.instance_tables([o.flatten() for o in ocps], assign)
    s.set_instance_soft(*soft)
    if alat is not None:
        s.set_instance_alat_soft(*alat)


def _mixed(track, case, ocps, assign):
    """The handle of tuning 0's OCP with every instance's own penalties."""
    s = _solver(track, ocps[0], len(assign), case)
    _set_mixed(s, ocps, assign)
    return s


def _state(s, status, sqp):
    pi, lam = s.get_multipliers()
    lam_a, slk_a = s.get_alat_multipliers()
    out = dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), lam_a=lam_a, slk_a=slk_a, status=status,
               qp_iter=s.get_qp_iter(), res=s.get_residuals())
    if sqp:
        out["merit"] = s.get_sqp_merit()
    return out


def _run(s, x0, steps=5, sqp=False):
    s.set_x0(x0)
    s.init_guess()
    out = []
    for _ in range(steps):
        s.prepare_step(40.0)
        out.append(_state(s, s.solve(), sqp))
    return out


def _assert_rows_equal(mixed, homo, rows):
    """Both handles hold the whole batch: the linearisation and the plant kernel are chosen by B N (csrc/qp_select.hpp: latency_batch),
    and the two linearisation kernels agree to rounding only -- a homogeneous handle of a group's two or three instances would take
    the other one.  Compared: the rows of the group."""
    for m, h in zip(mixed, homo):
        for k in m:
            np.testing.assert_array_equal(m[k][rows], h[k][rows], err_msg=k)


MIXED = ([(case, 40, build) for case in ("track_rows_soft", "alat_soft") for build in ("default", "ilp")]
         + [(case, 40, "default") for case in ("soft_state", "fdyn6u", "live")] + [("track_rows_soft", 10, "default")])


@pytest.mark.parametrize("B", [9, 3])
@pytest.mark.parametrize("case,Nf,build", MIXED)
def test_mixed_batch_equals_homogeneous_handles(track, case, Nf, build, B):
    from test_gpu_configs import _build

    sqp = case == "live"
    ocps = _ocps(track, case, Nf)
    assign = np.arange(B) % K
    x0 = IP.x0_of(track, case, B)
    with _build(build):
        s = _mixed(track, case, ocps, assign)
        mixed = _run(s, x0, sqp=sqp)
        assert s.get_launch_record()["qp"].startswith("k_qp_wave<"), s.get_launch_record()       # never the four-wave kernel in this mode
        s.free()
        homo = {}
        for j in range(K):
            rows = np.flatnonzero(assign == j)
            if rows.size == 0:
                continue
            h = _solver(track, ocps[j], B, case)
            homo[j] = _run(h, x0, sqp=sqp)
            h.free()
            _assert_rows_equal(mixed, homo[j], rows)
    # the tunings differ on the same inputs: a kernel that ignored the per-instance values could not have passed
    for i, j in ((0, 1), (1, 2)):
        assert _rel(homo[i][0]["u"], homo[j][0]["u"]) > 1e-6 and _rel(homo[i][-1]["slk"], homo[j][-1]["slk"]) > 1e-6
    assert max(m["slk"].max() for m in mixed) > 1e-6                  # slacks are in use
    if case == "alat_soft":
        assert max(m["slk_a"].max() for m in mixed) > 1e-6           # ... the a_lat row's as well
    if sqp:
        assert np.any(mixed[-1]["merit"] != 0.0)                     # a line search ran: the merit read the penalties
    assert np.isin(mixed[-1]["status"], (0, 2)).mean() > 0.5


def test_persistent_loop_mixed_equals_homogeneous(track):
    """run_steps with freeze on the soft track rows, plant ERK.  The homogeneous handles hold the whole batch and the group's rows are
    compared, for the reason _assert_rows_equal gives: a group of two or three instances is a latency batch, which takes the other
    linearisation and plant kernels."""
    case, B = "track_rows_soft", 9
    ocps = _ocps(track, case)
    for o in ocps:
        o.solver_options.sim_integrator_type = "ERK"
    assign = np.arange(B) % K
    x0 = IP.x0_of(track, case, B, seed=11)

    def loop(s, x):
        s.set_x0(x)
        s.init_guess()
        h = s.run_steps(40.0, 6, M_sim=25, freeze=True, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
        return h, s.get_x0()

    s = _mixed(track, case, ocps, assign)
    hm, xm = loop(s, x0)
    s.free()
    for j in range(K):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, ocps[j], B, case)
        hh, xh = loop(h, x0)
        h.free()
        for k in hm:
            np.testing.assert_array_equal(hm[k][:, rows], hh[k][:, rows], err_msg=k)
        np.testing.assert_array_equal(xm[rows], xh[rows])


def _gradients(s, x0, seeds):
    """Everything the issue lists, after one solve with x0 sensitivity mode 2."""
    s.set_x0_sensitivities(2)
    s.set_x0(x0)
    s.init_guess()
    s.prepare_step(40.0)
    st = s.solve()
    sx, su = s.get_x0_sensitivities()
    out = dict(status=st, cost=s.get_cost(), stage_cost=s.get_cost(stagewise=True), slack_cost=s.get_slack_cost(), sens_x=sx, sens_u=su)
    for name, fn in (("slack", s.eval_adjoint_slack_sensitivities), ("penalty", s.eval_adjoint_penalty_sensitivities)):
        for k, v in fn(**seeds).items():
            out[name + "_" + k] = v
    for k, v in s.eval_cost_gradient_penalties().items():
        out["costgrad_" + k] = v
    return out


@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("case", ["track_rows_soft", "alat_soft"])
def test_gradients_are_each_instances_own(track, case, S):
    B, Nf = 9, IP.N
    ocps = _ocps(track, case)
    assign = np.arange(B) % K
    x0 = IP.x0_of(track, case, B, seed=13)
    rng = np.random.default_rng(5)
    seeds = dict(seed_x=rng.standard_normal((B, S, Nf + 1, 8)), seed_u=rng.standard_normal((B, S, Nf, 2)),
                 seed_s=rng.standard_normal((B, S, Nf + 1, 28)), seed_sa=rng.standard_normal((B, S, Nf + 1, 2)))
    s = _mixed(track, case, ocps, assign)
    gm = _gradients(s, x0, seeds)
    s.free()
    assert np.isin(gm["status"], (0, 2)).mean() > 0.5
    assert np.abs(gm["penalty_soft_z"]).max() > 0.0 and np.abs(gm["costgrad_soft_Z"]).max() > 0.0
    if case == "alat_soft":
        assert np.abs(gm["penalty_alat_soft_z"]).max() > 0.0
    for j in range(K):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, ocps[j], B, case)
        gh = _gradients(h, x0, seeds)
        h.free()
        for k in gm:
            np.testing.assert_array_equal(gm[k][rows], gh[k][rows], err_msg=k)


def test_oracle_parity_per_tuning(track):
    """Every instance against an oracle problem holding its penalties, three iterations on the frozen problem with the multipliers
    carried along.  Tolerances: those of tests/test_gpu_parity.py::test_track_rows_rti_steps_match_oracle for the soft track rows."""
    from oracle import oracle as orc

    case, B, Nf = "track_rows_soft", 8, IP.N
    ocps = _ocps(track, case)
    assign = np.arange(B) % K
    x0 = IP.x0_of(track, case, B, seed=3)
    Ps = [orc.OracleProblem(o.flatten().as_dict(track.s_ref, track.kappa_ref, track_widths=IP.widths(case))) for o in ocps]
    s = _mixed(track, case, ocps, assign)
    s.set_x0(x0)
    s.init_guess()
    x, u = s.get_x(), s.get_u()
    s.prepare_step(40.0)
    yref, yref_e = orc.prepare_step(Nf, x0, 40.0, x, u)
    s.set_multipliers(None, None)
    pi, lam = np.zeros((B, Nf + 1, 8)), np.zeros((B, Nf + 1, 28))
    for _ in range(3):
        status = s.solve()
        st_o, it_o, res_o = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros((B, 4))
        for j in range(K):
            rows = np.flatnonzero(assign == j)
            xo, uo = x[rows].copy(), u[rows].copy()
            out = Ps[j].rti_step(xo, uo, x0[rows], yref[rows], yref_e[rows], pi=pi[rows].copy(), lam=lam[rows].copy())
            x[rows], u[rows], pi[rows], lam[rows] = xo, uo, out["pi"], out["lam"]
            st_o[rows], it_o[rows], res_o[rows] = out["status"], out["qp_iter"], out["res"]
        np.testing.assert_array_equal(status, st_o)
        ok = status == 0
        assert ok.sum() >= 0.9 * B
        np.testing.assert_array_equal(s.get_qp_iter()[ok], it_o[ok])
        assert _rel(s.get_x()[ok], x[ok]) < 1e-6       # tolerance 1e-6 relative, as there
        assert _rel(s.get_u()[ok], u[ok]) < 1e-6
        assert _rel(s.get_residuals(), res_o) < 1e-7
        _, lam_g = s.get_multipliers()
        assert np.max(np.abs(lam_g[ok] - lam[ok])) / (1.0 + np.abs(lam).max()) < 1e-5
        s.set_x(x); s.set_u(u); s.set_multipliers(pi, lam)      # both sides on the same iterate
    assert s.get_slacks()[:, 1:, 14 + 12:].max() > 1e-3             # some footprint is outside the narrow track and pays for it
    s.free()


def test_null_restores_shared_and_rebuilds_keep_instance_penalties(track):
    from ihm2_amd._lib import Ihm2mpcError

    case, B = "track_rows_soft", 9
    ocps = _ocps(track, case)
    flats = [o.flatten() for o in ocps]
    assign = np.arange(B) % K
    x0 = IP.x0_of(track, case, B, seed=5)
    # set, then NULL: the handle's results are those of one that never had per-instance penalties
    s = _mixed(track, case, ocps, assign)
    s.set_instance_soft(None, None)
    a = _run(s, x0, steps=3)
    s.free()
    r = _solver(track, ocps[0], B, case)
    b = _run(r, x0, steps=3)
    r.free()
    _assert_rows_equal(a, b, np.arange(B))
    # a later set_soft with the same pattern (other shared values) keeps the per-instance values: compare with a fresh handle
    fresh = _mixed(track, case, ocps, assign)
    want = _run(fresh, x0, steps=3)
    fresh.free()
    s = _mixed(track, case, ocps, assign)
    s.set_soft(flats[2].soft_z, flats[2].soft_Z)
    _assert_rows_equal(_run(s, x0, steps=3), want, np.arange(B))
    # ... with another pattern (the lower sides of the track rows hard) the next solve refuses, until the values are set again or dropped
    Z = flats[0].soft_Z.copy(); Z[:, 12:14] = -1.0
    s.set_soft(flats[0].soft_z, Z)
    s.set_x0(x0)
    with pytest.raises(Ihm2mpcError, match=r"per-instance penalties do not fit the batch-shared constraint pattern any more: set them again, or pass NULL"):
        s.solve()
    s.set_instance_soft(None, None)
    s.solve()
    s.free()


def _instance_bounds(track, case, assign):
    """Bound values per instance inside the shared pattern, as tests/test_gpu_instance_tuning.py builds them: the bound arrays of the
    case's OCP under that file's limit tunings (tuning 0 is the shared table's own)."""
    from ihm2_amd.controller import controller_ocp
    from test_gpu_instance_tuning import TUNINGS

    assert IP.CASES[case]["kind"] == "track"
    flats = []
    for t in TUNINGS:
        lim = dict(n_max=t["n_max"], v_x_max=t["v_x_max"], T_max=t["T_max"], delta_max=t["delta_max"], T_dot_max=1e6, delta_dot_max=t["delta_dot_max"])
        flats.append(controller_ocp(track.s_ref.shape[-1], IP.N, lim, a_lat_max=5.0, track_rows=True, track_rows_penalty=IP.PENALTIES[0])[1].flatten())
    return {k: np.stack([getattr(flats[j], k) for j in assign]) for k in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")}


def _restart_and_run(s, x0):
    """Three steps from a cold start of everything a solve starts from (a handle that has run before keeps its multipliers and slacks
    through init_guess), then the cost and its slack part at the last solution."""
    s.set_multipliers(None, None)
    s.set_slacks(None)
    s.set_alat_multipliers(None, None)
    out = _run(s, x0, steps=3)
    out.append(dict(cost=s.get_cost(), slack_cost=s.get_slack_cost()))
    return out


def test_both_instance_modes_on_one_handle_through_the_cross_transitions(track):
    """Per-instance bounds and per-instance penalties share the device tables (csrc/api.hip: tables_to_device): one handle goes through
    the transitions in which one mode comes or goes while the other stays, and in every state gives, bit for bit, what a fresh handle
    built directly in that state gives -- the solves, the cost and its slack part.  In the bounds-only state the cost reads the
    batch-shared penalties from the per-instance tables."""
    case, B = "track_rows_soft", 3
    ocps = _ocps(track, case)
    flats = [o.flatten() for o in ocps]
    assign = np.arange(B)                       # three distinct tunings, of the penalties and of the bounds
    soft, _ = IP.instance_tables(flats, assign)
    bounds = _instance_bounds(track, case, assign)
    x0 = IP.x0_of(track, case, B, seed=5)
    rows = np.arange(B)

    # the target states on fresh handles (where both modes are on: in the other order than the handle under test sets them)
    want = {}
    for state in ("both", "penalties", "bounds"):
        f = _solver(track, ocps[0], B, case)
        if state != "bounds":
            f.set_instance_soft(*soft)
        if state != "penalties":
            f.set_instance_bounds(**bounds)
        want[state] = _restart_and_run(f, x0)
        f.free()
    # each mode reaches the kernels: the states differ from one another on the instances whose tuning is not the shared one
    for a, b in (("both", "penalties"), ("both", "bounds")):
        assert not np.array_equal(want[a][0]["u"][1:], want[b][0]["u"][1:]), (a, b)
    assert want["bounds"][-1]["slack_cost"].max() > 1e-6            # slacks are in use, and paid for

    s = _solver(track, ocps[0], B, case)
    s.set_instance_bounds(**bounds)             # 1. bounds on, then penalties on
    s.set_instance_soft(*soft)
    _assert_rows_equal(_restart_and_run(s, x0), want["both"], rows)
    s.set_instance_bounds()                     # 2. bounds dropped while penalties stay
    _assert_rows_equal(_restart_and_run(s, x0), want["penalties"], rows)
    s.set_instance_bounds(**bounds)             # 3. bounds on again, then penalties dropped while bounds stay
    s.set_instance_soft(None, None)
    _assert_rows_equal(_restart_and_run(s, x0), want["bounds"], rows)
    s.set_instance_soft(*soft)                  # 4. both on, then a shared set_soft with the same pattern (other shared values)
    s.set_soft(flats[2].soft_z, flats[2].soft_Z)
    _assert_rows_equal(_restart_and_run(s, x0), want["both"], rows)
    s.free()


def test_refusals(track):
    from ihm2_amd._lib import Ihm2mpcError

    B = 8
    assign = np.arange(B) % K
    ocps = _ocps(track, "alat_soft")
    (z, Z), (az, aZ) = IP.instance_tables([o.flatten() for o in ocps], assign)
    # before set_soft / without a soft a_lat row: an all-hard handle with the track rows and the a_lat row
    nk = track.s_ref.shape[-1]
    from ihm2_amd.controller import controller_ocp

    _, hard = controller_ocp(nk, IP.N, IP.LIMITS, track_rows=True, track_rows_penalty=None, lateral_acceleration_row=True)
    hard.cost.W, hard.cost.W_e = ocps[0].cost.W, ocps[0].cost.W_e
    hard.solver_options.tf, hard.solver_options.sim_method_num_steps = ocps[0].solver_options.tf, 25
    h = _solver(track, hard, B, "alat_soft")
    with pytest.raises(Ihm2mpcError, match=r"ihm2mpc_set_soft has not been called"):
        h.set_instance_soft(z, Z)
    with pytest.raises(Ihm2mpcError, match=r"ihm2mpc_set_alat_constraint has not been called with a soft side"):
        h.set_instance_alat_soft(az, aZ)
    h.free()
    s = _solver(track, ocps[0], B, "alat_soft")
    lib = s.lib
    from ihm2_amd.solver import _ptr

    for entry, arr in ((lib.ihm2mpc_set_instance_soft, z), (lib.ihm2mpc_set_instance_alat_soft, az)):
        assert entry(s._h, _ptr(arr), None) != 0 and b"both be given, or both be NULL" in lib.ihm2mpc_last_error()
        assert entry(s._h, None, _ptr(arr)) != 0 and b"both be given, or both be NULL" in lib.ihm2mpc_last_error()
    with pytest.raises(ValueError):
        s.set_instance_soft(z, None)

    def with_(arr, idx, v):
        a = arr.copy(); a[idx] = v
        return a

    # row 13 (the left track row), upper side: column 14 + 13 = 27
    with pytest.raises(Ihm2mpcError, match=r"instance 3, stage 5, side 27 \(uh\[1\]\): the side is hard .*batch-shared table holds it soft"):
        s.set_instance_soft(z, with_(Z, (3, 5, 27), -1.0))
    with pytest.raises(Ihm2mpcError, match=r"instance 2, stage 7, side 3 \(lbx\[3\]\): the side is soft .*batch-shared table holds it hard"):
        s.set_instance_soft(z, with_(Z, (2, 7, 3), 10.0))
    with pytest.raises(Ihm2mpcError, match=r"instance 1, stage 4, side 12 \(lh\[0\]\): soft_z < 0"):
        s.set_instance_soft(with_(z, (1, 4, 12), -1.0), Z)
    with pytest.raises(Ihm2mpcError, match=r"instance 6, stage 40, side 26 \(uh\[0\]\): slack penalty is NaN"):
        s.set_instance_soft(with_(z, (6, 40, 26), np.nan), Z)
    with pytest.raises(Ihm2mpcError, match=r"instance 5, stage 0, side 29 \(a_lat upper\): the side is hard"):
        s.set_instance_alat_soft(az, with_(aZ, (5, 1), -1.0))
    with pytest.raises(Ihm2mpcError, match=r"instance 4, stage 0, side 28 \(a_lat lower\): soft_z < 0"):
        s.set_instance_alat_soft(with_(az, (4, 0), -0.5), aZ)
    with pytest.raises(Ihm2mpcError, match=r"instance 7, stage 0, side 28 \(a_lat lower\): slack penalty is NaN"):
        s.set_instance_alat_soft(az, with_(aZ, (7, 0), np.nan))
    with pytest.raises(ValueError):
        s.set_instance_soft(z[:-1], Z[:-1])
    # nothing was taken over: the handle still solves with its shared table, as a fresh one
    x0 = IP.x0_of(track, "alat_soft", B)
    a = _run(s, x0, steps=2)
    s.free()
    r = _solver(track, ocps[0], B, "alat_soft")
    _assert_rows_equal(a, _run(r, x0, steps=2), np.arange(B))
    r.free()


@pytest.mark.parametrize("kind", ["soft_state", "track_alat"])
def test_controller_arrays_equal_to_defaults_are_bit_identical(track, kind):
    from ihm2_amd.controller import IHM2Controller

    B = 16
    x0 = IP.x0_of(track, "track_rows_soft", B, seed=9)
    if kind == "soft_state":
        scalar = dict(terminal_bounds="stage", soft_state_bounds=(1000.0, 1000.0), n_max=0.5)
        arrays = dict(scalar, soft_state_bounds=(np.full(B, 1000.0), np.full(B, 1000.0)))
    else:
        scalar = dict(track_widths=IP.WIDTHS, lateral_acceleration_row=True, a_lat_max=2.0)
        arrays = dict(scalar, track_rows_penalty=(np.full(B, 100.0), 100.0))
    res = []
    for kw in (scalar, arrays):
        c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, **kw)
        c.warm_start(x0)
        us = [c.compute_control(x0) for _ in range(3)]
        res.append((np.array(us), c.last_status.copy(), c.x_pred, c.solver.get_slacks(), c.solver.get_alat_multipliers()[1]))
        c.solver.free()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    assert res[0][3].max() > 1e-6
    # distinct penalties per instance reach the solver: the controls differ from the scalar controller's
    even = np.arange(B) % 2 == 0
    if kind == "soft_state":
        kw = dict(scalar, soft_state_bounds=(np.where(even, 1000.0, 10.0), 1000.0))
    else:
        kw = dict(scalar, track_rows_penalty=(np.where(even, 100.0, 10.0), 100.0))
    c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, **kw)
    c.warm_start(x0)
    u = np.array([c.compute_control(x0) for _ in range(3)])
    c.solver.free()
    np.testing.assert_array_equal(u[:, even], res[0][0][:, even])       # the instances that kept the scalar's penalties
    assert _rel(u[:, ~even], res[0][0][:, ~even]) > 1e-6
