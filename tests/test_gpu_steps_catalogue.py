"""Every instantiation of the persistent control-step loop, by name, against launches per step.

tests/steps_cases.py holds one configuration per k_steps<NSLOT, NSOFT, PATH, UNI, SQP, IRK, DYN[, SENS]> of csrc/qp_catalogue.hpp (read
from csrc/qp_select.hpp: select_steps, which tests/test_steps_catalogue.py runs on every case without a GPU; that test also checks the table against the catalogue, the layouts' slot tables and the
oracle's first step on the CPU), and the configurations that must fall back.  Each instantiation is a register allocation of its own
of the same loop body, inlined next to another integrator, line search or sensitivity guest; here each is launched, the launch record
is compared with the name, and the results with those of ihm2mpc_step call by call, bit for bit.  That equality is worth what step()
is worth for the same configuration: the classes of configurations are also compared with the oracle, one per-step solve each.

All handles take the single-wave QP kernel (IHM2MPC_BLOCK_QP=0), as in tests/test_gpu_closed_loop.py: the four-wave kernel of small
batches sums in another order."""
import numpy as np
import pytest

import drive
import layouts as L
import steps_cases as S
from test_gpu_configs import _build

pytestmark = pytest.mark.gpu

STEPS = 4               # the shift, the carried multipliers and slacks, and the SQP merit restart all matter from the second step on
RECORDS = set()         # (build, record) of every run_steps of test_loop_equals_step_by_step


@pytest.fixture(autouse=True)
def _single_wave_qp(monkeypatch):
    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")          # read when a handle is created


def _solver(track, case, build="default", **more):
    from ihm2_amd.solver import BatchedOcpSolver

    lay = S.LAYOUTS[case.layout]
    tables, tracks = (track.s_ref, track.kappa_ref), dict(track_widths=L.track_widths(lay))
    if case.tracks > 1:         # a case of steps_cases.TWO_TRACK: both tables, per-instance ids and widths per track
        import multi_track_cases as MT

        tables, tracks = MT.tables(), dict(track_id=S.track_ids(case), track_widths=MT.widths(lay))
    with _build(build):
        s = BatchedOcpSolver(L.make_ocp(lay, **{**case.ocp_opts(), **more}), case.B, *tables, **tracks)
    arr = L.apply(s.data, lay)
    if arr["W"] is not None:
        s._push_weights()
    s._push_bounds()
    return s


def _start(s, track, case):
    x0, yref, yref_e = S.start(track, case)
    s.set_x0(x0); s.init_guess()
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
    return x0, yref, yref_e


def _sens(s, case):
    sx, su = s.get_x0_sensitivities()
    return {"sens_u": su} if sx is None else {"sens_x": sx, "sens_u": su}


def _closed_loop(track, case, build, persistent, **more):
    """One step(), then STEPS control steps in one run_steps call or in STEPS step() calls: (histories, final state, launch record)."""
    lay = S.LAYOUTS[case.layout]
    s = _solver(track, case, build, **more)
    s.set_lap_wrap(True)
    if case.sens:
        s.set_x0_sensitivities(case.sens)
    _start(s, track, case)
    tgt = S.s_target(lay)
    s.step(tgt, model=case.plant, M_sim=case.M_sim)
    rec = None
    if persistent:
        h = s.run_steps(tgt, STEPS, model=case.plant, M_sim=case.M_sim, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True,
                        sens_u0_hist=True if case.sens else None)
        rec = s.get_launch_record()
    else:
        h = drive.per_step(s, tgt, STEPS, model=case.plant, M_sim=case.M_sim, sens=bool(case.sens))
    pi, lam = s.get_multipliers()
    f = dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks())
    if lay.alat:
        f["lam_a"], f["slk_a"] = s.get_alat_multipliers()
    if case.sqp:
        f.update(s.get_sqp_stats())
    if case.sens:
        f.update(_sens(s, case))
    s.free()
    return h, f, rec


def _assert_loop_equals_steps(track, case, build, expect, **more):
    ha, fa, _ = _closed_loop(track, case, build, False, **more)
    hb, fb, rec = _closed_loop(track, case, build, True, **more)
    got = rec["steps"] if rec["steps"] != "per_step" else "per_step:" + str(rec["steps_fallback"])
    assert got == expect, (got, expect)
    if rec["steps"] != "per_step":          # which object of the name ran (steps_cases.FORMS)
        assert (rec["steps_form"], rec["steps_slots"]) == case.form, rec
    assert set(ha) == set(hb) and set(fa) == set(fb)
    for k in ha:
        np.testing.assert_array_equal(hb[k], ha[k], err_msg=k)
    for k in fa:
        np.testing.assert_array_equal(fb[k], fa[k], err_msg=k)
    if case.sens:           # the last step's read-back is the history's last entry; NaN rows exactly where the step was not accepted
        np.testing.assert_array_equal(hb["sens_u0"][-1], fb["sens_u"] if fb["sens_u"].ndim == 3 else fb["sens_u"][:, 0])
        ok = np.isin(hb["status"], (0, 2))
        assert np.isnan(hb["sens_u0"][~ok]).all() and np.isfinite(hb["sens_u0"][ok]).all()
    accepted = np.isin(ha["status"], case.accepted).mean()
    print(f"{expect} [{build}]: accepted {accepted:.2f}, status {ha['status'].tolist()}")
    assert np.isfinite(ha["x0"]).all() and accepted >= 0.5
    return got, fa


LOOPS = [(c.name, "default") for c in S.CASES] + [(c.name, "ilp") for c in S.CASES if c.qp_set in S.ILP_SETS]


@pytest.mark.parametrize("name,build", LOOPS)
def test_loop_equals_step_by_step(track, name, build):
    """run_steps / run_steps_sens launches the instantiation the case is named for, and gives what the same number of step() calls gives:
    the histories of status, qp_iter, x0, u0 (and du_0/dx_0), the final x, u, pi, lam and slacks, the SQP statistics and the last step's
    sensitivities, bit for bit; at least half of the instance-steps end accepted."""
    case = S.ILP_CASES.get(name, S.BY_NAME[name]) if build == "ilp" else S.BY_NAME[name]
    RECORDS.add((build, _assert_loop_equals_steps(track, case, build, name)[0]))


@pytest.mark.parametrize("key", list(S.FALLBACK))
def test_fallback_goes_per_step_with_the_stated_reason(track, key):
    case = S.FALLBACK[key]
    RECORDS.add(("default", _assert_loop_equals_steps(track, case, "default", "per_step:" + case.reason)[0]))


# ---- step() itself against the oracle, per class of configuration ----
# One case per (layout, model, integrator, RTI / SQP).  Left out: the kinematic model with RK4 in the RTI mode on the layouts of
# layouts.TABLE, which tests/test_gpu_qp_layouts.py::test_layout_matches_oracle_and_kkt compares with the oracle (and an independent
# KKT check) over three iterations in both builds.  The classes of the layouts of steps_cases.EXTRA are kept: the same tables at other horizons.
def _classes():
    out = {}
    for c in S.CASES:
        if c.model == "fkin6" and c.irk == 0 and not c.sqp and c.layout in L.TABLE:
            continue
        out.setdefault("%s-%s-%s-%s" % (c.layout, c.model, S.INTEG[c.irk][0], "SQP" if c.sqp else "RTI"), c)
    return out


CLASSES = _classes()


def _rel(a, b):
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if a.size else 0.0


def _oracle(track, s, case):
    if case.tracks > 1:
        import multi_track_cases as MT

        return S.oracle_problem(track, s.data, S.LAYOUTS[case.layout], tables=MT.tables(), widths=MT.widths(S.LAYOUTS[case.layout]))
    return S.oracle_problem(track, s.data, S.LAYOUTS[case.layout])


def _assert_rti_matches_oracle(track, case):
    """The assertions and tolerances of test_gpu_qp_layouts.py::test_layout_matches_oracle_and_kkt for one iteration: statuses equal,
    iteration counts equal in 99.9 % (else +-1), x / u to 1e-7, pi / lam to 1e-6 of their scale, slacks to 1e-7 against the oracle's QP."""
    from oracle import oracle as orc

    s = _solver(track, case)
    data = s.data
    P = _oracle(track, s, case)
    x0, yref, yref_e = _start(s, track, case)
    x, u = s.get_x(), s.get_u()
    x_lin, u_lin = x.copy(), u.copy()
    st = s.solve()
    tid = S.track_ids(case)         # None on one track
    out = S.oracle_rti_step(P, data, track, x, u, x0, yref, yref_e, track_id=tid)
    pi, lam = out["pi"], out["lam"]
    itg = s.get_qp_iter()
    xg, ug = s.get_x(), s.get_u()
    pig, lamg = s.get_multipliers()
    slg = s.get_slacks()
    ok = st == 0
    eq = ok & (itg == out["qp_iter"])
    ex, eu = _rel(xg[eq], x[eq]), _rel(ug[eq], u[eq])
    print(f"status {st.tolist()} oracle {out['status'].tolist()} qp_iter {itg.tolist()} oracle {out['qp_iter'].tolist()} x {ex:.2e} u {eu:.2e}")
    np.testing.assert_array_equal(st, out["status"])
    assert ok.mean() >= 0.6
    same = itg[ok] == out["qp_iter"][ok]
    assert same.mean() >= 0.999 and np.abs(itg[ok] - out["qp_iter"][ok]).max() <= 1
    assert ex < 1e-7 and eu < 1e-7
    if eq.any():
        sp = max(1.0, float(np.abs(pi[eq][:, 1:]).max())); sl_ = max(1.0, float(np.abs(lam[eq]).max()))
        assert np.abs(pig[eq][:, 1:] - pi[eq][:, 1:]).max() <= 1e-6 * sp          # (pi_0 is not defined: x_0 is eliminated)
        assert np.abs(lamg[eq] - lam[eq]).max() <= 1e-6 * sl_
    if data.soft_Z is not None:
        z, Z = L.soft_arrays(data)
        for i in np.flatnonzero(ok):
            ref = P.build_qp(x_lin[i], u_lin[i], x0[i], yref[i], yref_e[i], track_id=0 if tid is None else int(tid[i]))
            sol = orc.qp_solve(**ref, iter_max=data.ipm_iter_max, tol=data.ipm_tol, mu0=data.ipm_mu0, tau0=data.ipm_tau0, soft_z=z, soft_Z=Z)
            if sol["iters"] == itg[i]:
                assert np.max(np.abs(slg[i] - sol["sl"]) / (1 + np.abs(sol["sl"]))) < 1e-7
    s.free()


def _assert_sqp_matches_oracle(track, case, iters=1, perturb=0.0, **more):
    """SQP iterations, one per call with both sides re-synchronised in between (tests/test_gpu_sqp.py), against
    OracleProblem.sqp_solve(max_iter=1) with the handle's options, to the tolerances of that module: statuses, SQP and QP iteration
    counts equal, the step length equal to 1e-12 in 95 % of the accepted instances, x / u to 1e-6 there.  Returns, per iteration, what
    the option tests compare further."""
    s = _solver(track, case, nlp_solver_max_iter=1, **more)
    data = s.data
    P = _oracle(track, s, case)
    x0, yref, yref_e = _start(s, track, case)
    N = s.N
    if perturb:         # a poor steering guess: full steps overshoot (tests/test_gpu_sqp.py::_setup)
        u = s.get_u()
        u[:, :, 1] = np.clip(u[:, :, 1] + perturb * np.sin(np.arange(N))[None], -0.5, 0.5)
        s.set_u(u)
    x, u = s.get_x(), s.get_u()
    pi = np.zeros((case.B, N + 1, 8)); lam = np.zeros((case.B, N + 1, 28)); sl = np.zeros((case.B, N + 1, 28))
    hist = []
    for it in range(iters):
        st = s.solve()
        out = P.sqp_solve(x, u, x0, yref, yref_e, pi=pi, lam=lam, sl=sl, **{**S.sqp_kwargs(data), "max_iter": 1})
        stats = s.get_sqp_stats()
        xg, ug = s.get_x(), s.get_u()
        pig, lamg = s.get_multipliers()
        ok = np.isin(st, (0, 2))
        same = ok & (np.abs(stats["alpha"] - out["alpha"]) < 1e-12)
        ex, eu = _rel(xg[same], x[same]), _rel(ug[same], u[same])
        print(f"iteration {it}: status {st.tolist()} oracle {out['status'].tolist()} alpha {stats['alpha'].tolist()} oracle {out['alpha'].tolist()} "
              f"x {ex:.2e} u {eu:.2e}")
        np.testing.assert_array_equal(st, out["status"])
        np.testing.assert_array_equal(stats["sqp_iter"], out["sqp_iter"])
        np.testing.assert_array_equal(s.get_qp_iter()[ok], out["qp_iter"][ok])
        assert ok.mean() >= 0.6
        assert same.sum() >= 0.95 * ok.sum()
        assert ex < 1e-6 and eu < 1e-6
        hist.append(dict(ok=ok, same=same, alpha=stats["alpha"], alpha_oracle=out["alpha"].copy(), pi=pig, lam=lamg, pi_oracle=pi.copy(),
                         lam_oracle=lam.copy()))
        s.set_x(x); s.set_u(u); s.set_multipliers(pi, lam); s.set_slacks(sl)
    s.free()
    return hist


@pytest.mark.parametrize("cls", list(CLASSES))
def test_first_step_matches_oracle(track, cls):
    case = CLASSES[cls]
    if case.sqp:
        _assert_sqp_matches_oracle(track, case)
    else:
        _assert_rti_matches_oracle(track, case)


# ---- the SQP options through the loop ----
# On the 5-slot hard table with RK4 and with collocation (where the loop rolls the line search's trial points out itself, one step
# length at a time -- LsArgs.phase = 3 -- instead of k_rollout_irk launches).  Against the oracle: three iterations from a steering guess
# perturbed by 0.2 sin(k); the first iteration takes full steps (the merit weights are set from its own QP), and from this start (sample_x0
# seed 701) the ORACLE's line search shortens steps in the second and third, so that full_step_dual and the sufficient-descent test act.
SQP_OPTIONS = {
    "full_step_dual": dict(full_step_dual=1),
    "fixed_step": dict(globalization="FIXED_STEP"),
    "sufficient_descent": dict(line_search_use_sufficient_descent=1),
}
OPTION_SEED, OPTION_ITERS, OPTION_PERTURB = 701, 3, 0.2


def _option_case(irk):
    import dataclasses

    return dataclasses.replace(S.BY_NAME[S.steps_name((5, 0, 0, 1), 1, irk, 0)], seed=OPTION_SEED, plant=(0, -2)[irk])


@pytest.mark.parametrize("irk", [0, 1])
@pytest.mark.parametrize("option", list(SQP_OPTIONS))
def test_sqp_option_in_the_loop_equals_step_by_step(track, option, irk):
    case = _option_case(irk)
    _, final = _assert_loop_equals_steps(track, case, "default", case.name, **SQP_OPTIONS[option])
    # the last solve's step lengths: the line search acted inside the loop (in the oracle's closed loop from this start the second SQP
    # iteration of every step is shortened for most instances), or never with FIXED_STEP -- a loop that ignored the flag would differ
    if option == "fixed_step":
        assert np.all(final["alpha"] == 1.0)
    else:
        assert (final["alpha"] < 1.0).any(), final["alpha"]


@pytest.mark.parametrize("irk", [0, 1])
@pytest.mark.parametrize("option", list(SQP_OPTIONS))
def test_sqp_option_matches_oracle(track, option, irk):
    case = _option_case(irk)
    h = _assert_sqp_matches_oracle(track, case, OPTION_ITERS, OPTION_PERTURB, **SQP_OPTIONS[option])
    if option == "fixed_step":
        assert all(np.all(r["alpha"][r["ok"]] == 1.0) for r in h)
        return
    assert any((r["alpha_oracle"][r["ok"]] < 1.0).any() for r in h)          # the line search shortened a step
    if option != "full_step_dual":
        return
    # The multipliers follow the oracle's (tests/test_gpu_sqp.py's bound) ...
    for r in h:
        m = r["same"]
        assert np.max(np.abs(r["pi"][m] - r["pi_oracle"][m])) / (1.0 + np.abs(r["pi_oracle"]).max()) < 1e-5
        assert np.max(np.abs(r["lam"][m] - r["lam_oracle"][m])) / (1.0 + np.abs(r["lam_oracle"]).max()) < 1e-5
    # ... and are not those of full_step_dual = 0 where a step was shortened.  Up to an instance's first short step both runs take
    # full steps from the same point (alpha = 1 gives the QP's multipliers either way); there the run without the flag moves
    # pi by alpha times the step instead of the whole step, so the two differ by (1 - alpha) >= 0.3 of it.  A flag the GPU ignored gives equality.
    h0 = _assert_sqp_matches_oracle(track, case, OPTION_ITERS, OPTION_PERTURB)
    clean = np.ones(case.B, dtype=bool)
    checked = 0
    for r, r0 in zip(h, h0):
        short = clean & r["ok"] & r0["ok"] & (r["alpha"] < 1.0) & (np.abs(r["alpha"] - r0["alpha"]) < 1e-12)
        for i in np.flatnonzero(short):
            d = np.abs(r["pi"][i][1:] - r0["pi"][i][1:]).max()
            assert d > 1e-3 * np.abs(r["pi"][i][1:]).max() > 0.0, (i, d)
            checked += 1
        clean &= (r["alpha"] == 1.0) & (r0["alpha"] == 1.0)
    assert checked >= 1


def test_every_steps_instantiation_was_launched():
    """The records of this module against the case table: every name in the default build, those of the sets 0, 1 and 3 in the ILP build
    (where it exists), the fallbacks with their reasons."""
    import os

    from test_gpu_configs import ILP_LIB

    expected = S.expected_records()
    if not os.path.exists(ILP_LIB):
        expected = {r for r in expected if r[0] != "ilp"}
    assert RECORDS == expected, (sorted(expected - RECORDS), sorted(RECORDS - expected))
