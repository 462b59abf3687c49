"""x0 sensitivities inside the persistent control-step loop (ihm2mpc_run_steps_sens, k_steps<..., SENS = 1>): the gain history against
ihm2mpc_step + ihm2mpc_get_x0_sensitivities step by step, bit for bit; every other output against plain ihm2mpc_run_steps; the layouts of
the QP-layout suite in both scheduler builds; the freezing closed loop's feedback_gain; the refusals and the Python bindings."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import drive
import launch_cases as LC

from test_gpu_qp_layouts import TABLE, _solver, _start

pytestmark = pytest.mark.gpu

IRK = dict(integrator_type="IRK", sim_method_num_steps=1)                                              # python/main.py:234-236


def _final(s, mode):
    pi, lam = s.get_multipliers()
    out = dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks())
    if mode == 2:
        out["sens_x"], out["sens_u"] = s.get_x0_sensitivities()
    else:
        out["sens_u0"] = drive.gain(s)
    return out


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("plant,n_max,B,opts", [(0, 2.0, 150, {}), (-1, 0.9, 150, {}), (0, 2.0, 1100, {}), (0, 2.0, 150, IRK), (-1, 0.9, 70, IRK)])
def test_gain_history_equals_step_by_step(track, plant, n_max, B, opts, mode, monkeypatch):
    """The RTI cases of test_gpu_closed_loop.py::test_persistent_loop_equals_step_by_step with x0 sensitivities on: the history of
    run_steps_sens is what step() + get_x0_sensitivities() gives at every step, bit for bit, and so is the last step's read-back (mode 2:
    the whole horizon).  B = 1100 is not resident: launches per step with k_sens behind every QP."""
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    steps = 12
    x0 = sample_x0(track, B, seed=31)
    res = []
    for persistent in (False, True):
        s = BatchedOcpSolver(make_ocp(n_max=n_max, **opts), B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        s.set_x0_sensitivities(mode)
        s.set_x0(x0); s.init_guess()
        s.step(40.0, model=plant, M_sim=30)
        if persistent:
            h = s.run_steps(40.0, steps, model=plant, M_sim=30, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True, sens_u0_hist=True)
            rec = s.get_launch_record()["steps"]
            if B == 1100:
                assert rec == "per_step"
            else:
                assert rec.startswith("k_steps<") and rec.endswith(",1>") and rec.count(",") == 7, rec
        else:
            h = drive.per_step(s, 40.0, steps, model=plant, M_sim=30, sens=True)
        res.append((h, _final(s, mode)))
        s.free()
    (ha, fa), (hb, fb) = res
    for k in ("status", "qp_iter", "x0", "u0", "sens_u0"):
        np.testing.assert_array_equal(hb[k], ha[k], err_msg=k)
    for k in fa:
        np.testing.assert_array_equal(fb[k], fa[k], err_msg=k)
    np.testing.assert_array_equal(hb["sens_u0"][-1], _gain_of(fb, mode))
    ok = np.isin(ha["status"], (0, 2))
    assert np.isnan(hb["sens_u0"][~ok]).all() and np.isfinite(hb["sens_u0"][ok]).all()
    assert (ha["status"] == 0).mean() > (0.9 if plant == 0 else 0.7)


def _gain_of(f, mode):
    return f["sens_u"][:, 0] if mode == 2 else f["sens_u0"]


@pytest.mark.parametrize("plant,n_max,B,opts", [(0, 2.0, 150, {}), (-1, 0.9, 150, IRK), (0, 2.0, 1100, {})])
def test_nothing_else_moves(track, plant, n_max, B, opts, monkeypatch):
    """run_steps and run_steps_sens from the same start: the u0 / x0 / status / qp_iter histories and the final iterate, multipliers and
    slacks are bit-identical (the sensitivities only read them)."""
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    steps = 10
    x0 = sample_x0(track, B, seed=77)
    res = []
    for sens in (False, True):
        s = BatchedOcpSolver(make_ocp(n_max=n_max, **opts), B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        s.set_x0_sensitivities(1)
        s.set_x0(x0); s.init_guess()
        s.step(40.0, model=plant, M_sim=30)
        h = s.run_steps(40.0, steps, model=plant, M_sim=30, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True,
                        sens_u0_hist=True if sens else None)
        assert ("sens_u0" in h) == sens
        h.pop("sens_u0", None)
        pi, lam = s.get_multipliers()
        res.append((h, dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), res=s.get_residuals())))
        s.free()
    (ha, fa), (hb, fb) = res
    for k in ha:
        np.testing.assert_array_equal(hb[k], ha[k], err_msg=k)
    for k in fa:
        np.testing.assert_array_equal(fb[k], fa[k], err_msg=k)


# The table (NSLOT, NSOFT, PATH, UNI) of the loop each layout of the QP-layout suite takes (kinematic model, RK4, RTI), None where
# csrc/qp_select.hpp: select_steps finds none and run_steps launches per step: stage-varying weights or rows (UNI = 0) on anything but the all-hard
# tables of 5 and 8 slots, and the lateral-acceleration row.  The catalogue has every such loop with and without SENS.
LOOP_ON = {
    "hard_5_per_lane": "5,0,0,1", "hard_5_per_lane_stage_W": "5,0,0,0", "hard_6_per_lane": "8,0,0,1", "hard_8_per_lane_stage_rows": "8,0,0,0",
    "hard_9_per_lane": "10,0,0,1", "hard_10_per_lane_all_boxes": "10,0,0,1", "hard_10_per_lane_stage_W": None,
    "hard_random_one_sided": "5,0,0,1", "hard_narrow_rate_row": "5,0,0,1", "empty_table": "5,0,0,1",
    "block_hard": "5,0,0,1", "block_hard_B1": "5,0,0,1", "block_hard_stage_W": "5,0,0,0",
    "soft_2_per_lane": "8,2,0,1", "soft_2_per_lane_stage_W": None, "soft_2_per_lane_split_rows": "8,2,0,1", "soft_3_per_lane_asym": "10,4,0,1",
    "soft_4_per_lane_mixed": "10,4,0,1", "soft_4_per_lane_stage_rows": None, "soft_one_sided_rows_padding": "8,2,0,1",
    "path_hard": "8,0,1,1", "path_hard_stage_W": None, "path_soft_3_per_lane": "8,3,1,1", "path_soft_3_per_lane_stage_W": None,
    "path_soft_both_sides": "10,4,1,1", "path_soft_4_per_lane": "10,4,1,1", "path_soft_4_per_lane_stage_W": None,
    "alat_hard": None, "alat_soft": None,
}


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("name", list(TABLE))
def test_gain_history_on_layout(track, name, build):
    """Every layout of the QP-layout suite in both scheduler builds (the a_lat layouts and the per-instance-free tables without an
    instantiation go per step): the gain history of run_steps_sens (mode 2) against step() step by step, and the last step's horizon."""
    lay, B, _ = TABLE[name]
    steps = 3
    res, recs = [], []
    for persistent in (False, True):
        s = _solver(track, lay, B, build, "0")
        s.set_lap_wrap(True)
        s.set_x0_sensitivities(2)
        _start(s, track, B, 700 + lay.seed)
        s.step(40.0, model=0, M_sim=25)
        if persistent:
            h = s.run_steps(40.0, steps, model=0, M_sim=25, status_hist=True, sens_u0_hist=True)
        else:
            h = drive.per_step(s, 40.0, steps, model=0, M_sim=25, sens=True)
        sx, su = s.get_x0_sensitivities()
        res.append((h["status"], h["sens_u0"], sx, su))
        if not persistent:
            s.run_steps(40.0, 1, model=0, M_sim=25)            # (what plain run_steps launches for the table, after the readings)
        rec = s.get_launch_record()
        recs.append(rec["steps"])
        s.free()
    # plain run_steps' instantiation and its SENS twin, or both per step
    loop = LOOP_ON[name]
    assert recs == (["per_step", "per_step"] if loop is None else [f"k_steps<{loop},0,0,0>", f"k_steps<{loop},0,0,0,1>"]), recs
    (sta, ka, sxa, sua), (stb, kb, sxb, sub) = res
    np.testing.assert_array_equal(stb, sta)
    ok = np.isin(sta, (0, 2))
    assert np.isnan(kb[~ok]).all() and np.isfinite(kb[ok]).all()
    if LC.latency_batch(B, lay.N):
        # KNOWN DIFFERENCE (test_gpu_qp_layouts.py::test_persistent_loop_equals_step_by_step_on_layout): ihm2mpc_step's state-only plant
        # rounds differently from the loop's on a latency batch, and the iterate follows it at 1e-9 relative
        for a, b, k in [(ka, kb, "sens_u0"), (sxa, sxb, "sens_x"), (sua, sub, "sens_u")]:
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=k)
            f = np.isfinite(b)
            assert np.max(np.abs(a[f] - b[f]) / (1 + np.abs(b[f]))) < 1e-9, k
        return
    np.testing.assert_array_equal(kb, ka)
    np.testing.assert_array_equal(sxb, sxa); np.testing.assert_array_equal(sub, sua)


def test_freezing_closed_loop_feedback_gain(track, monkeypatch):
    """run_closed_loop_persistent (freezing on the device, one launch of the loop with sensitivities) against run_closed_loop_device
    (step + get_x0_sensitivities per period): feedback_gain agrees bit for bit on the live entries, is NaN on the dead ones (where u is
    zeroed) and finite wherever the status is 0; run_closed_loop fills it the same way; without the mode it stays None."""
    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    from ihm2_amd.closed_loop_sim import SimModelVariant, Simulator, SimulatorConfig, run_closed_loop, run_closed_loop_device, run_closed_loop_persistent
    from ihm2_amd.controller import IHM2Controller

    B, steps = 40, 30
    x0 = sample_x0(track, B, seed=17)
    out = []
    for runner in (run_closed_loop_device, run_closed_loop_persistent, run_closed_loop):
        ctrl = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B, x0_sensitivities=True)
        sim = Simulator(ctrl, SimulatorConfig(sampling_time=ctrl.dt, num_steps=40), SimModelVariant.KIN6_DYN6)
        ctrl.warm_start(x0)
        out.append(runner(ctrl, sim, x0, steps, lap_length=track.lap_length))
        ctrl.solver.free()
    d, p, hst = out
    n = min(d.u.shape[0], p.u.shape[0])
    assert n >= 10
    for r in (d, p, hst):
        m = r.u.shape[0]
        assert r.feedback_gain is not None and r.feedback_gain.shape == (m, B, 2, 8)
        live = r.alive_history[:m] & np.isin(r.status[:m], (0, 2))          # the rows whose u is not zeroed
        assert np.isnan(r.feedback_gain[~live]).all()
        assert np.isfinite(r.feedback_gain[live & (r.status[:m] == 0)]).all()
        assert (~live).any() and live.any()
    np.testing.assert_array_equal(d.alive_history[:n], p.alive_history[:n])
    live = d.alive_history[:n]
    np.testing.assert_array_equal(p.u[:n][live], d.u[:n][live])
    np.testing.assert_array_equal(p.feedback_gain[:n], d.feedback_gain[:n])
    ctrl = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=8)
    sim = Simulator(ctrl, SimulatorConfig(sampling_time=ctrl.dt, num_steps=40), SimModelVariant.KIN6)
    ctrl.warm_start(x0[:8])
    assert run_closed_loop_persistent(ctrl, sim, x0[:8], 3).feedback_gain is None
    ctrl.solver.free()


def test_refusals_and_read_back(track):
    from ihm2_amd import _lib
    from ihm2_amd._lib import Ihm2mpcError
    from ihm2_amd.solver import BatchedOcpSolver

    B, steps = 8, 4
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_x0(sample_x0(track, B, seed=9)); s.init_guess()
    s.step(40.0, model=0, M_sim=25)
    with pytest.raises(Ihm2mpcError, match="off"):
        s.run_steps(40.0, steps, sens_u0_hist=True)
    s.set_x0_sensitivities(1)
    h = s.run_steps(40.0, steps, status_hist=True, sens_u0_hist=True)
    rec_sens = s.get_launch_record()["steps"]
    _, K = s.get_x0_sensitivities()                     # readable: the last step's
    np.testing.assert_array_equal(K, h["sens_u0"][-1])
    assert np.isfinite(K[h["status"][-1] == 0]).all()
    s.run_steps(40.0, 2)
    rec = s.get_launch_record()["steps"]
    assert rec.startswith("k_steps<") and rec_sens == rec[:-1] + ",1>", (rec, rec_sens)
    with pytest.raises(Ihm2mpcError, match="run_steps"):
        s.get_x0_sensitivities()
    # the C entry point without a history: the last step's values are still read back
    st = np.empty((steps, B), dtype=np.int32)
    _lib.check(s.lib.ihm2mpc_run_steps_sens(s._h, 0, 25, 40.0, steps, 0, float("inf"), None, None, st.ctypes.data_as(_lib.c_int32_p), None, None))
    s.synchronize()
    _, K = s.get_x0_sensitivities()
    assert np.isfinite(K[st[-1] == 0]).all() and np.isnan(K[~np.isin(st[-1], (0, 2))]).all()
    s.free()
    # the per-step path keeps refusing freeze
    Bb = 1100
    s = BatchedOcpSolver(make_ocp(), Bb, track.s_ref, track.kappa_ref)
    s.set_x0_sensitivities(1)
    s.set_x0(sample_x0(track, Bb, seed=10)); s.init_guess()
    with pytest.raises(Ihm2mpcError, match="no persistent loop"):
        s.run_steps(40.0, 2, freeze=True, sens_u0_hist=True)
    s.free()


def test_gain_history_without_waiting_and_in_pieces(track):
    """Two run_steps_sens calls that do not wait (gain histories into pinned memory), then one synchronize(), give what one call over
    all the steps gives."""
    from ihm2_amd.solver import BatchedOcpSolver

    B, n1, n2 = 96, 5, 7
    x0 = sample_x0(track, B, seed=41)
    out = []
    for pieces in (False, True):
        s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
        s.set_x0_sensitivities(1)
        s.set_x0(x0); s.init_guess()
        s.step(40.0, model=0, M_sim=25)
        k = s.alloc_pinned((n1 + n2, B, 2, 8))
        if pieces:
            s.reserve_history(max(n1, n2))
            s.run_steps(40.0, n1, sens_u0_hist=k[:n1], wait=False)
            s.run_steps(40.0, n2, sens_u0_hist=k[n1:], wait=False)
            s.synchronize()
        else:
            s.run_steps(40.0, n1 + n2, sens_u0_hist=k)
        out.append((np.array(k), drive.gain(s)))
        s.free()
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)
    assert np.isfinite(out[0][0]).mean() > 0.9
