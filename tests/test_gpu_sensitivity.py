"""x0 sensitivities on the GPU (kernels_sens.hip): parity with the numpy reference (tests/sens_ref.py) on every layout of the QP-layout
suite in both scheduler builds, finite differences of whole solves, bit-identity of every other output with the mode on, the refusals,
and the Python paths (BatchedOcpSolver, the AcadosOcpSolver shim, IHM2Controller.feedback_gain)."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import drive
import layouts as L
import sens_ref as S
from test_gpu_qp_layouts import TABLE, _solver, _start, _widen

pytestmark = pytest.mark.gpu

# _check_against_reference: of the reference's largest entry, on stage 0 and over the horizon
TOL_STAGE0, TOL_HORIZON = 1e-7, 1e-6


def _outputs(s, alat=False):
    pi, lam = s.get_multipliers()
    out = dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), status=s.get_status(), qp_iter=s.get_qp_iter())
    if alat:
        out["lam_a"], out["slk_a"] = s.get_alat_multipliers()
    return out


def _check_against_reference(s, P, data, x0, yref, yref_e, xbar, ubar, sx, su, nc, z, Z, path, idx, track_id=None):
    """GPU sensitivities of the instances idx against the dense reference at the GPU's own iterate and linearisation (track_id: the
    instances' tracks where the handle holds several; the track rows are then each instance's own)."""
    A, Bm, b = s.get_linearization()
    o = _outputs(s, alat=nc == 15)
    lam, slk = (_widen(o["lam"], o["lam_a"]), _widen(o["slk"], o["slk_a"])) if nc == 15 else (o["lam"], o["slk"])
    worst0 = worst = 0.0
    for i in idx:
        ref = P.build_qp(xbar[i], ubar[i], x0[i], yref[i], yref_e[i], track_id=0 if track_id is None else int(track_id[i])) if path else None
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref)
        dz = np.zeros((s.N + 1, 10)); dz[:, :8] = o["x"][i] - xbar[i]; dz[:s.N, 8:] = o["u"][i] - ubar[i]
        rx, ru = S.sensitivities(qp, dz, lam[i], slk[i], z, Z)
        scale = max(np.abs(rx).max(), np.abs(ru).max())
        worst0 = max(worst0, np.abs(su[i, 0] - ru[0]).max() / scale)
        worst = max(worst, np.abs(su[i] - ru).max() / scale, np.abs(sx[i] - rx).max() / scale)
    # (the Riccati recursion and the dense solve of the reference differ by the conditioning of Ht, with barrier weights up to ~1e15:
    # measured 2.3e-8 at worst on stage 0 and 4.6e-8 over the horizon, NOTES.md)
    assert worst0 <= TOL_STAGE0 and worst <= TOL_HORIZON, (worst0, worst)
    return worst0, worst


def _subset(ok):
    idx = np.flatnonzero(ok)
    return np.unique(np.concatenate([idx[:5], idx[-2:]])) if idx.size else idx


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("name", list(TABLE))
def test_layout_parity_with_reference(track, name, build):
    from oracle import oracle as orc

    lay, B, block = TABLE[name]
    s = _solver(track, lay, B, build, block)
    data = s.data
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    x0, yref, yref_e = _start(s, track, B, 900 + lay.seed)
    nc = 15 if lay.alat else L.NC
    z, Z = L.soft_arrays(data, nc, (data.alat_soft_z, data.alat_soft_Z) if lay.alat and data.alat_soft_Z is not None else None)
    s.set_x0_sensitivities(2)
    for it in range(1 if name == "empty_table" else 2):
        xbar, ubar = s.get_x(), s.get_u()
        st = s.solve()
        sx, su = s.get_x0_sensitivities()
        ok = (st == 0) | (st == 2)
        assert np.isnan(su[~ok]).all() and np.isnan(sx[~ok]).all()
        assert np.isfinite(su[ok]).all() and np.isfinite(sx[ok]).all()
        np.testing.assert_array_equal(sx[ok][:, 0], np.broadcast_to(np.eye(8), (int(ok.sum()), 8, 8)))
        _check_against_reference(s, P, data, x0, yref, yref_e, xbar, ubar, sx, su, nc, z, Z, lay.path, _subset(ok))
    s.free()


@pytest.mark.parametrize("B", [1, 96, 4096])
def test_batch_sizes_and_modes_agree(track, B):
    """B = 1 takes k_qp_block, 96 and 4096 k_qp_wave; mode 1's du_0/dx_0 is mode 2's bit for bit; the device getter gives the same."""
    import ctypes as C

    from oracle import oracle as orc

    hip = C.CDLL("libamdhip64.so")       # the HIP runtime the product library is linked against

    lay = TABLE["hard_5_per_lane"][0]
    res = {}
    for mode in (1, 2):
        s = _solver(track, lay, B, "default", "1")
        x0, yref, yref_e = _start(s, track, B, 31)
        s.set_x0_sensitivities(mode)
        xbar, ubar = s.get_x(), s.get_u()
        st = s.solve()
        sx, su = s.get_x0_sensitivities()
        if mode == 1:
            assert sx is None and su.shape == (B, 2, 8)
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), C.c_size_t(su.nbytes)) == 0
            s.get_sens_u0_device(d.value)
            s.synchronize()
            back = np.empty_like(su)
            assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), d, C.c_size_t(su.nbytes), 2) == 0      # hipMemcpyDeviceToHost
            assert hip.hipFree(d) == 0
            np.testing.assert_array_equal(back, su)
            res[1] = su
        else:
            assert sx.shape == (B, s.N + 1, 8, 8) and su.shape == (B, s.N, 2, 8)
            res[2] = su[:, 0]
            data = s.data
            P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref))
            z, Z = L.soft_arrays(data)
            ok = st == 0
            assert ok.mean() > 0.5
            _check_against_reference(s, P, data, x0, yref, yref_e, xbar, ubar, sx, su, L.NC, z, Z, False, _subset(ok))
        if B == 1:
            assert s.get_launch_record()["qp"].startswith("k_qp_block")
        s.free()
    np.testing.assert_array_equal(res[1], res[2])


def test_fdyn6u_irk(track):
    from ihm2_amd.solver import BatchedOcpSolver
    from oracle import oracle as orc

    B = 64
    ocp = make_ocp(model="fdyn6u", M=1, integrator_type="IRK")
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    x0, yref, yref_e = _start(s, track, B, 77)
    s.set_x0_sensitivities(2)
    xbar, ubar = s.get_x(), s.get_u()
    st = s.solve()
    sx, su = s.get_x0_sensitivities()
    data = s.data
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref))
    z, Z = L.soft_arrays(data)
    ok = st == 0
    assert ok.mean() > 0.5
    _check_against_reference(s, P, data, x0, yref, yref_e, xbar, ubar, sx, su, L.NC, z, Z, False, _subset(ok))
    s.free()


def test_per_instance_weights_and_bounds(track):
    """Instance b of a batch with per-instance weights and bounds has the sensitivities of a handle whose shared tables hold b's, bit for bit."""
    from ihm2_amd import ocp as O

    lay = TABLE["soft_2_per_lane_split_rows"][0]
    B, facs = 30, (1.0, 0.9, 0.8)
    assign = np.arange(B) % 3
    arr = L.make_arrays(lay)
    W0, We0 = O.default_weights()
    var = []
    for j, f in enumerate(facs):
        v = {n: np.where(np.abs(arr[n]) < L.BIG, arr[n] * f, arr[n]) for n in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")}
        var.append((v, W0 * (1.0 + 0.5 * j), We0 * (1.0 + 0.25 * j)))
    x0 = drive.clipped_start(track, B, 4343)

    def run(s, x0s):
        s.set_x0_sensitivities(2)
        s.set_x0(x0s); s.init_guess()
        out = []
        for _ in range(2):
            s.prepare_step(40.0)
            st = s.solve()
            sx, su = s.get_x0_sensitivities()
            out.append((st, sx, su))
        return out

    s = _solver(track, lay, B, "default", "0")
    s.set_instance_weights(np.stack([var[a][1] for a in assign]), np.stack([var[a][2] for a in assign]))
    s.set_instance_bounds(**{n: np.stack([var[a][0][n] for a in assign]) for n in var[0][0]})
    mixed = run(s, x0)
    s.free()
    for j in range(3):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, lay, rows.size, "default", "0")
        for n, a in var[j][0].items():
            setattr(h.data, n, a)
        h.data.W = np.broadcast_to(var[j][1], h.data.W.shape).copy(); h.data.W_e = var[j][2]
        h._push_weights(); h._push_bounds()
        homo = run(h, x0[rows])
        h.free()
        for m, hh in zip(mixed, homo):
            for a, bb in zip(m, hh):
                np.testing.assert_array_equal(a[rows], bb)
    assert (mixed[-1][0] == 0).mean() > 0.5


@pytest.mark.parametrize("name", ["hard_5_per_lane", "soft_4_per_lane_mixed", "path_soft_both_sides", "alat_soft"])
def test_finite_differences_of_whole_solves(track, name):
    """du_0/dx0 against central differences of solve() in x0 at qp_tol 1e-9, the iterate, multipliers and slacks restored each time."""
    lay, B, _ = TABLE[name]
    B = 64
    from ihm2_amd.solver import BatchedOcpSolver

    ocp = L.make_ocp(lay)
    ocp.solver_options.qp_tol = 1e-9
    ocp.solver_options.qp_solver_iter_max = 200
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
    L.apply(s.data, lay)
    s._push_weights(); s._push_bounds()
    x0, yref, yref_e = _start(s, track, B, 1234)
    s.set_x0_sensitivities(1)
    x, u = s.get_x(), s.get_u()
    pi, lam = s.get_multipliers(); slk = s.get_slacks()
    la = s.get_alat_multipliers() if lay.alat else None

    def restore(x0v):
        s.set_x(x); s.set_u(u); s.set_multipliers(pi, lam); s.set_slacks(slk)
        if la is not None:
            s.set_alat_multipliers(*la)
        s.set_x0(x0v)

    restore(x0)
    st = s.solve()
    _, K = s.get_x0_sensitivities()
    # the weakly active instances (a side with multiplier and gap both below 1e-4) have no derivative: skipped, as in the CPU test
    o = _outputs(s, alat=lay.alat)
    lamw, slkw = (_widen(o["lam"], o["lam_a"]), _widen(o["slk"], o["slk_a"])) if lay.alat else (o["lam"], o["slk"])
    nc = 15 if lay.alat else L.NC
    z, Z = L.soft_arrays(s.data, nc, (s.data.alat_soft_z, s.data.alat_soft_Z) if lay.alat_soft else None)
    from oracle import oracle as orc

    P = orc.OracleProblem(s.data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    A, Bm, b = s.get_linearization()
    keep = []
    for i in np.flatnonzero(st == 0):
        ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i]) if lay.path else None
        qp = L.assemble_qp(s.data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref)
        dz = np.zeros((s.N + 1, 10)); dz[:, :8] = o["x"][i] - x[i]; dz[:s.N, 8:] = o["u"][i] - u[i]
        if not S.weakly_active(qp, dz, lamw[i], sl=slkw[i], soft_z=z, soft_Z=Z):
            keep.append(i)
    eps = 1e-5
    fd = np.zeros((B, 2, 8))
    sts = []
    for j in range(8):
        for sgn in (1, -1):
            xp = x0.copy(); xp[:, j] += sgn * eps
            restore(xp)
            sts.append(s.solve())
            fd[:, :, j] += sgn * s.get_u0() / (2 * eps)
    keep = [i for i in keep if all(t[i] == 0 for t in sts)]
    assert len(keep) >= 0.5 * B, len(keep)
    errs = np.array([np.abs(K[i] - fd[i]).max() / max(np.abs(fd[i]).max(), 1e-12) for i in keep])
    # (at qp_tol 1e-9 the interior point's smoothing shows near the active-set boundary, as in the CPU test; measured 81 % <= 1e-5 at worst)
    assert np.median(errs) <= 1e-6 and np.mean(errs <= 1e-5) >= 0.75 and np.mean(errs <= 1e-3) >= 0.95, \
        (np.median(errs), np.mean(errs <= 1e-5), np.sort(errs)[-4:])
    s.free()


@pytest.mark.parametrize("mode", [1, 2])
def test_other_outputs_are_bit_identical(track, mode):
    lay, _, _ = TABLE["path_soft_4_per_lane"]
    B = 96
    outs = []
    for on in (False, True):
        s = _solver(track, lay, B, "default", "1")
        if on:
            s.set_x0_sensitivities(mode)
        x0, _, _ = _start(s, track, B, 55)
        o = []
        s.solve(); o.append(_outputs(s))
        u0, st = s.compute_control(x0, 40.0); o.append(dict(_outputs(s), u0=u0, st=st))
        s.step(40.0, model=0, M_sim=25); o.append(dict(_outputs(s), u0=s.get_u0(), x0=s.get_x0()))
        if on:
            _, su = s.get_x0_sensitivities()
            assert np.isfinite(su[s.get_status() == 0]).all()
        outs.append(o)
        s.free()
    for a, b in zip(*outs):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_refusals(track):
    from ihm2_amd._lib import Ihm2mpcError
    from ihm2_amd.solver import BatchedOcpSolver

    B = 8
    sq = BatchedOcpSolver(make_ocp(nlp_solver_type="SQP", nlp_solver_max_iter=2), B, track.s_ref, track.kappa_ref)
    with pytest.raises(Ihm2mpcError, match="SQP"):
        sq.set_x0_sensitivities(1)
    sq.free()
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    with pytest.raises(Ihm2mpcError, match="off"):
        s.get_x0_sensitivities()
    with pytest.raises(Ihm2mpcError, match="mode 3"):
        s.set_x0_sensitivities(3)
    s.set_x0_sensitivities(1)
    with pytest.raises(Ihm2mpcError, match="no solve"):
        s.get_x0_sensitivities()
    x0 = sample_x0(track, B, seed=9)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    _, K = s.get_x0_sensitivities()
    assert K.shape == (B, 2, 8) and np.isfinite(K[st == 0]).all()
    from ihm2_amd import _lib

    sx_buf = np.empty((B, s.N + 1, 8, 8))
    with pytest.raises(Ihm2mpcError, match="mode 2"):
        _lib.check(s.lib.ihm2mpc_get_x0_sensitivities(s._h, sx_buf.ctypes.data_as(_lib.c_double_p), None))
    s.run_steps(40.0, 2, model=0, M_sim=25)
    with pytest.raises(Ihm2mpcError, match="run_steps"):
        s.get_x0_sensitivities()
    s.prepare_step(40.0)
    s.solve()
    s.get_x0_sensitivities()            # readable again after a solve
    s.set_x0_sensitivities(2)           # a new mode needs a new solve
    with pytest.raises(Ihm2mpcError, match="no solve"):
        s.get_x0_sensitivities()
    s.free()


def test_shim_and_controller(track):
    from ihm2_amd.controller import IHM2Controller
    from ihm2_amd.solver import BatchedOcpSolver

    B = 16
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_x0_sensitivities(2)
    x0 = sample_x0(track, B, seed=3)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    s.solve()
    sx, su = s.get_x0_sensitivities()
    v = s[5]
    with pytest.raises(Exception, match="only 'ex'"):
        v.eval_param_sens(0, field="p_global")
    for j in (0, 3, 7):
        v.eval_param_sens(j)
        for k in (0, 1, s.N):
            np.testing.assert_array_equal(v.get(k, "sens_x"), sx[5, k, :, j])
        for k in (0, 7, s.N - 1):
            np.testing.assert_array_equal(v.get(k, "sens_u"), su[5, k, :, j])
    assert v.get(0, "sens_x").shape == (8,) and v.get(0, "sens_u").shape == (2,)
    s.free()

    for Bc in (1, 8):
        c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=Bc, x0_sensitivities=True)
        xs = sample_x0(track, Bc, seed=21)
        c.warm_start(xs)
        u0 = c.compute_control(xs[0] if Bc == 1 else xs)
        K = c.feedback_gain
        assert K.shape == ((2, 8) if Bc == 1 else (Bc, 2, 8))
        _, Kb = c.solver.get_x0_sensitivities()
        np.testing.assert_array_equal(K, Kb[0] if Bc == 1 else Kb)
        assert u0 is not None
        c.solver.free()


def test_feedback_gain_predicts_a_re_solve(track):
    """Closed loop: u0 + K0 dx0 predicts the u0 of a re-solve from x0 + dx0 (same warm start) better than u0 alone."""
    from ihm2_amd.controller import IHM2Controller

    B = 64
    c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, x0_sensitivities=True)
    xs = sample_x0(track, B, seed=11)
    c.warm_start(xs)
    x = xs.copy()
    for _ in range(5):          # a few closed-loop steps of the kinematic plant
        u0 = c.compute_control(x)
        ok = c.last_status == 0
        x[ok] = c.solver.sim_step(np.where(ok[:, None], x, xs), np.nan_to_num(u0), model=0, M_sim=25)[ok]
    xw, uw = c.solver.get_x(), c.solver.get_u()
    u0 = c.compute_control(x)
    K = c.feedback_gain
    ok0 = c.last_status == 0
    rng = np.random.default_rng(5)
    dx = np.zeros((B, 8))
    dx[:, 1] = rng.uniform(-0.02, 0.02, B); dx[:, 2] = rng.uniform(-0.005, 0.005, B); dx[:, 3] = rng.uniform(-0.05, 0.05, B)
    c.solver.set_x(xw); c.solver.set_u(uw)
    u1 = c.compute_control(x + dx)
    ok = ok0 & (c.last_status == 0)
    assert ok.mean() > 0.8
    pred = u0 + np.einsum("bij,bj->bi", K, dx)
    e_pred = np.abs(pred - u1)[ok] / (1 + np.abs(u1[ok]))
    e_zero = np.abs(u0 - u1)[ok] / (1 + np.abs(u1[ok]))
    assert np.median(e_pred.max(1)) < 0.2 * np.median(e_zero.max(1)), (np.median(e_pred.max(1)), np.median(e_zero.max(1)))
    assert (e_pred.max(1) <= e_zero.max(1)).mean() >= 0.8
    c.solver.free()
