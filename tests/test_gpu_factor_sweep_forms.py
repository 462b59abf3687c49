"""The forms of the interior-point QP's factor sweep (ihm2_amd/csrc/riccati_mfma.hpp): the general stage -- with the symmetrising tile and
the p_k stores behind wave-uniform flags -- and the straight-line stage (PLAIN) of k_qp_wave<5,0,0,1> / k_steps<5,0,0,1,0,0,0,0>, with the
run-time horizon and with the horizon 40 compiled in.  The straight-line stage fetches its records through a clamped running offset and
stores through running addresses, D = 4 stages to a pass: the horizons below are under the ring depth, equal to it and no multiple of it.

The general stage without active rows (m_act == 0: the p_k stores) is what tests/test_gpu_qp_layouts.py runs on its layout "empty_table"
(test_layout_matches_oracle_and_kkt and test_persistent_loop_equals_step_by_step_on_layout, both builds)."""
import numpy as np
import pytest
from conftest import make_ocp

import drive
import launch_cases as LC
import qp_forms as QF

pytestmark = pytest.mark.gpu

B = 8
# seeds of sample_x0 for which the oracle alone returns status 0 on all 8 instances (found on the CPU, tools/find_factor_sweep_seeds.py)
SEEDS = {1: 8, 2: 4, 3: 1, 4: 1, 5: 0, 7: 0, 9: 0}
SEED_FDYN6 = 7


def _x0(track, seed):
    return drive.clipped_start(track, B, seed)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


def _oracle_step(track, ocp, x0, x, u):
    """the oracle's rti_step from the guess (x, u) of init_guess; x, u are updated in place"""
    from oracle import oracle as orc

    P = orc.OracleProblem(ocp.flatten().as_dict(track.s_ref, track.kappa_ref))
    yref, yref_e = orc.prepare_step(ocp.dims.N, x0, 40.0, x, u)
    out = P.rti_step(x, u, x0, yref, yref_e)
    assert np.all(out["status"] == 0), "the seed is chosen so that the oracle solves all instances"
    return out


def _solve(track, ocp, x0, ref=None):
    """one prepare_step + solve() on a fresh handle -> (handle, (out, x, u) of the oracle: computed here unless given)"""
    from ihm2_amd.solver import BatchedOcpSolver

    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    s.set_lap_wrap(True)
    s.set_x0(x0); s.init_guess()
    if ref is None:
        x, u = s.get_x(), s.get_u()
        ref = (_oracle_step(track, ocp, x0, x, u), x, u)
    s.prepare_step(40.0)
    st = s.solve()
    out, x, u = ref
    np.testing.assert_array_equal(st, out["status"])
    np.testing.assert_array_equal(s.get_qp_iter(), out["qp_iter"])
    ex, eu = _rel(s.get_x(), x), _rel(s.get_u(), u)
    print(f"N={s.N}: GPU vs oracle x {ex:.2e} u {eu:.2e}, qp_iter {out['qp_iter'].tolist()}")
    assert ex < 1e-9 and eu < 1e-9
    return s, ref


@pytest.mark.parametrize("N", sorted(SEEDS))
def test_horizons_around_the_ring_depth(track, N, monkeypatch):
    """k_qp_wave against the oracle (status, iteration count, x and u to 1e-9), then two control steps per step (k_qp_wave) and in one
    launch (k_steps).  (The kin/dyn switch plant, model -1: k_sim_step on both sides; on a latency batch the per-step path integrates the
    kinematic plant with another kernel than the loop, tests/test_gpu_qp_layouts.py: KNOWN DIFFERENCE.)"""
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    x0 = _x0(track, SEEDS[N])
    ocp = make_ocp(N=N)
    if N < 2:
        # the library takes horizons from 2 (ihm2mpc_create): the one-interval sweep cannot be reached through the API, and the case
        # says so instead of leaving the list of horizons
        from ihm2_amd._lib import Ihm2mpcError

        with pytest.raises(Ihm2mpcError, match=r"N must be in \[2, "):
            BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
        return
    s, _ = _solve(track, ocp, x0)
    rec = s.get_launch_record()
    assert rec["qp"] == "k_qp_wave<5,0,0,1>" and rec["qp_form"] == "plain"
    s.free()
    # The two GPU paths.  ihm2mpc_step linearises a latency batch (launch_cases.latency_batch) with the kernel k_linearize_cols, whose
    # records agree with the loop's to 1e-15 and not bit for bit (include/ihm2mpc.h, ihm2mpc_run_steps): at B = 8 the two paths are compared
    # as tests/test_gpu_qp_layouts.py compares them there (status and iteration counts equal, the rest to 1e-9), and bit for bit on a
    # batch just past the switch, which takes the batch linearisation on both sides.
    for Bp in (B, LC.PAST_THE_SWITCH[N]):
        xp = drive.clipped_start(track, Bp, SEEDS[N])
        res = []
        for persistent in (False, True):
            s = BatchedOcpSolver(ocp, Bp, track.s_ref, track.kappa_ref)
            s.set_lap_wrap(True)
            s.set_x0(xp); s.init_guess()
            s.prepare_step(40.0)
            s.solve()
            if persistent:
                h = s.run_steps(40.0, 2, model=-1, M_sim=30, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
                rec = s.get_launch_record()
                assert rec["steps"] == "k_steps<5,0,0,1,0,0,0>" and rec["steps_form"] == "plain"
            else:
                h = drive.per_step(s, 40.0, 2, model=-1, M_sim=30)
                rec = s.get_launch_record()
                assert rec["qp"] == "k_qp_wave<5,0,0,1>" and rec["qp_form"] == "plain"
                assert (rec["linearize"], rec["sim"]) == LC.names(s, plant=-1)
            res.append((h, s.get_x(), s.get_u(), s.get_multipliers()))
            s.free()
        (ha, xa, ua, ma), (hb, xb, ub, mb) = res
        np.testing.assert_array_equal(ha["status"], hb["status"]); np.testing.assert_array_equal(ha["qp_iter"], hb["qp_iter"])
        pairs = [(ha["x0"], hb["x0"], "x0"), (ha["u0"], hb["u0"], "u0"), (xa, xb, "x"), (ua, ub, "u"), (ma[0], mb[0], "pi"), (ma[1], mb[1], "lam")]
        for a, b, k in pairs:
            if not LC.latency_batch(Bp, N):
                np.testing.assert_array_equal(a, b, err_msg=f"B={Bp}: {k}")
            else:
                d = _rel(a, b)
                print(f"N={N} B={Bp}: per step vs k_steps {k} {d:.2e}")
                assert d < 1e-9, (Bp, k)


@pytest.mark.parametrize("N,loop", [(3, False), (4, True)])
def test_sqp_loop_is_refused_where_its_sweeps_leave_the_lds(track, N, loop, monkeypatch):
    """The SQP instantiations of the persistent loop keep the sweeps' earlier form (kernels_qp.hip: stream_rows_v1), whose unclamped prefetch
    of LDS operands starts in front of the block's LDS at N = 2, 3 (csrc/qp_lds.hpp: qp_reach_v1_vector; 60 / 24 words): run_steps launches
    those horizons per step and says so, and runs the loop from N = 4.  Three control steps, bit for bit against three calls of step().
    (The collocation integrator: on a latency batch it is the one configuration in which step() and the loop linearise and simulate with the
    same code -- see test_horizons_around_the_ring_depth.)"""
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    ocp = make_ocp(N=N, nlp_solver_type="SQP", nlp_solver_max_iter=2, globalization="MERIT_BACKTRACKING", integrator_type="IRK", sim_method_num_steps=1)
    x0 = _x0(track, SEEDS[N])
    res = []
    for persistent in (False, True):
        s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        s.set_x0(x0); s.init_guess()
        s.step(40.0, model=-1, M_sim=30)
        if persistent:
            h = s.run_steps(40.0, 3, model=-1, M_sim=30, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
            rec = s.get_launch_record()
            if loop:
                assert rec["steps"] == "k_steps<5,0,0,1,1,1,0>"
            else:
                assert rec["steps"] == "per_step" and rec["steps_fallback"] == "no_instantiation"
        else:
            h = drive.per_step(s, 40.0, 3, model=-1, M_sim=30)
        res.append((h, s.get_x(), s.get_u(), s.get_multipliers(), s.get_sqp_stats()))
        s.free()
    (ha, xa, ua, ma, sa), (hb, xb, ub, mb, sb) = res
    for k in ("status", "qp_iter", "x0", "u0"):
        np.testing.assert_array_equal(ha[k], hb[k], err_msg=k)
    np.testing.assert_array_equal(xa, xb); np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(ma[0], mb[0]); np.testing.assert_array_equal(ma[1], mb[1])
    np.testing.assert_array_equal(sa["sqp_iter"], sb["sqp_iter"]); np.testing.assert_array_equal(sa["alpha"], sb["alpha"])
    assert np.isin(ha["status"], (0, 2)).mean() > 0.5


def test_general_form_with_the_symmetrising_tile(track, monkeypatch):
    """fdyn6 as written keeps the general stage and its tile: one per-step solve at N = 5 against the oracle, on the same terms."""
    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    s, _ = _solve(track, make_ocp(N=5, model="fdyn6"), _x0(track, SEED_FDYN6))
    rec = s.get_launch_record()
    assert rec["qp"].startswith("k_qp_wave<") and rec["qp_form"] == "general"
    s.free()


def test_three_forms_give_the_same_bits_at_n40():
    """N = 40: the general stage, the straight-line stage and the straight-line stage with the horizon compiled in -- one process each
    (IHM2MPC_QP_FORM is read once; tests/qp_forms.py) -- after one solve and after three persistent steps, B = 8 from the unclipped start."""
    for level in ("0", "1", None):
        sweep = QF.FORMS[level][0]
        assert QF.runs(level)["sweep_kernels"].tolist() == [QF.QP, sweep, QF.STEPS, sweep]
    ref = QF.runs("0")
    keys = [k for k in ref if k.startswith(("sweep_a_", "sweep_b_"))]
    assert len(keys) == 14
    assert np.all(ref["sweep_a_status"] == 0) and (ref["sweep_b_status"] == 0).mean() > 0.9
    for level in ("1", None):
        QF.compare(QF.runs(level), ref, keys, what=f"{QF.FORMS[level][0]} against general")
