"""The oracle's RTI step on seeded constraint layouts (tests/layouts.py) against an independent KKT check: one-sided rows and absent
sides written as +-1e20, narrow boxes, stage-varying rows and weights, soft sides that are one-sided, L1 or L2 only, asymmetric, or
soft on one side and hard on the other -- layouts the parity tests never build, so GPU == oracle on them needs this first.

The QP is assembled here in numpy (layouts.assemble_qp) and checked against OracleProblem.build_qp; the track rows are nonlinear and
are taken from build_qp.  The solution checked is the oracle's: rti_step moves the iterate by the step of orc_qp_solve_soft on that
QP (checked bit for bit), whose slacks the KKT report includes.  No GPU."""
import numpy as np
import pytest
from conftest import sample_x0

import layouts as L
from oracle import oracle as orc

N = 40
B = 3


def oracle_layouts():
    """About 30 seeded layouts: the knobs drawn per seed, plus a few named edge layouts."""
    out = [
        L.Layout("empty", xbox="none", ubox=False, grows="none"),
        L.Layout("all_boxes_one_sided", xbox="all", one_sided=0.5, seed=1),
        L.Layout("narrow_rate_row", grows="narrow", seed=2),
        L.Layout("stage_varying_rows_and_W", grows="stagevary", stage_W=True, xbox="random", seed=3),
        L.Layout("soft_lower_hard_upper", soft=1.0, soft_rows=(1, 3, 5, 11), soft_kind="lower", seed=4),
        L.Layout("soft_upper_hard_lower", soft=1.0, soft_rows=(1, 3, 5, 11), soft_kind="upper", seed=5),
        L.Layout("soft_l1_only", soft=1.0, soft_rows=(1, 3, 11), soft_kind="l1", seed=6),
        L.Layout("soft_l2_only", soft=1.0, soft_rows=(1, 3, 11), soft_kind="l2", seed=7),
        L.Layout("soft_asymmetric", soft=1.0, soft_rows=(1, 2, 3, 10, 11), soft_kind="asym", seed=8),
        L.Layout("soft_mixed_l1_lower_l2_upper", soft=1.0, soft_rows=(1, 3, 11), soft_kind="mixed", seed=9),
        L.Layout("soft_one_sided_rows", soft=0.7, soft_rows=(1, 3, 4, 11), one_sided=0.5, xbox="all", seed=10),
        L.Layout("track_rows_hard", path=True, xbox="random", one_sided=0.3, seed=11),
        L.Layout("track_rows_soft_with_soft_boxes", path=True, path_soft=True, soft=0.5, soft_rows=(1, 3), seed=12),
        L.Layout("track_rows_soft_state_boxes_lower", path=True, soft=1.0, soft_rows=(1, 3), soft_kind="lower", seed=13),
    ]
    for seed in range(100, 116):
        rng = np.random.default_rng(seed)
        out.append(L.Layout(
            f"random_{seed}", seed=seed, xbox=("ref", "all", "random", "none")[rng.integers(4)], ubox=bool(rng.random() < 0.8),
            grows=("ref", "none", "stagevary", "narrow")[rng.integers(4)], one_sided=float(rng.choice([0.0, 0.3, 0.7])),
            soft=float(rng.choice([0.0, 0.3, 1.0])), soft_rows=tuple(int(c) for c in rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 10, 11], 3, replace=False)),
            stage_W=bool(rng.random() < 0.4), path=bool(rng.random() < 0.3)))
    return out


LAYOUTS = oracle_layouts()


def _setup(lay, track):
    ocp = L.make_ocp(lay)
    data = ocp.flatten()
    L.apply(data, lay)
    w = L.track_widths(lay)
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=w))
    x0 = sample_x0(track, B, seed=5000 + lay.seed)
    x, u = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
    yref, yref_e = orc.prepare_step(N, x0, 40.0, x, u)
    return data, P, x0, x, u, yref, yref_e


def test_layouts_are_what_they_say(track):
    """The generator writes what the layout names: absent sides as |v| >= 1e20, one-sided rows, soft sides of every kind, a 1e-6 box."""
    a = L.make_arrays(L.Layout("x", xbox="all", one_sided=0.5, seed=1))
    lo_abs, up_abs = np.abs(a["lbx"][1:]) >= L.BIG, np.abs(a["ubx"][1:]) >= L.BIG
    assert (lo_abs & ~up_abs).any() and (up_abs & ~lo_abs).any() and not (lo_abs & up_abs).any()
    assert np.isinf(a["lbx"]).any() or np.isinf(a["ubx"]).any()
    a = L.make_arrays(L.Layout("x", grows="narrow"))
    assert np.allclose(a["ug"][:, 0] - a["lg"][:, 0], 1e-6)
    a = L.make_arrays(L.Layout("x", soft=1.0, soft_rows=(1,), soft_kind="lower"))
    assert (a["soft_Z"][1:, 1] >= 0).all() and (a["soft_Z"][1:, L.NC + 1] < 0).all()
    a = L.make_arrays(L.Layout("x", soft=1.0, soft_rows=(1,), soft_kind="mixed"))
    assert (a["soft_Z"][1:, 1] == 0).all() and (a["soft_z"][1:, 1] > 0).all() and (a["soft_z"][1:, L.NC + 1] == 0).all()
    a = L.make_arrays(L.Layout("x", grows="stagevary", stage_W=True))
    assert not np.array_equal(a["C"][0], a["C"][1]) and not np.array_equal(a["W"][0], a["W"][1])
    a = L.make_arrays(L.Layout("x", xbox="none", ubox=False, grows="none"))
    assert all((np.abs(a[n]) >= L.BIG).all() for n in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")) and a["soft_Z"] is None


@pytest.mark.parametrize("lay", LAYOUTS, ids=[lay.name for lay in LAYOUTS])
def test_numpy_assembly_matches_build_qp(lay, track):
    data, P, x0, x, u, yref, yref_e = _setup(lay, track)
    A, Bm, b = P.linearize(x, u)
    for i in range(B):
        ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i])
        qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
        for name in ("H", "g", "A", "Bm", "b", "dx0", "R"):
            np.testing.assert_allclose(qp[name], ref[name], rtol=1e-12, atol=1e-12 * max(1.0, np.abs(ref[name]).max()), err_msg=name)
        for name in ("dl", "du"):
            fin = np.isfinite(ref[name])
            np.testing.assert_array_equal(np.isfinite(qp[name]), fin, err_msg=name)
            np.testing.assert_allclose(qp[name][fin], ref[name][fin], rtol=1e-12, atol=1e-9, err_msg=name)


@pytest.mark.parametrize("lay", LAYOUTS, ids=[lay.name for lay in LAYOUTS])
def test_rti_step_satisfies_the_kkt_conditions_with_slacks(lay, track):
    data, P, x0, x, u, yref, yref_e = _setup(lay, track)
    x_lin, u_lin = x.copy(), u.copy()
    A, Bm, b = P.linearize(x_lin, u_lin)
    out = P.rti_step(x, u, x0, yref, yref_e)
    z, Z = L.soft_arrays(data)
    tol = data.ipm_tol
    solved = converged = 0
    for i in range(B):
        qp_o = P.build_qp(x_lin[i], u_lin[i], x0[i], yref[i], yref_e[i])
        sol = orc.qp_solve(**qp_o, iter_max=data.ipm_iter_max, tol=tol, mu0=data.ipm_mu0, tau0=data.ipm_tau0,
                           soft_z=None if data.soft_Z is None else z, soft_Z=None if data.soft_Z is None else Z)
        assert sol["iters"] == out["qp_iter"][i]
        if out["status"][i] != 0:
            continue
        solved += 1
        # rti_step took exactly this step
        np.testing.assert_array_equal(x[i], x_lin[i] + sol["dz"][:, :8])
        np.testing.assert_array_equal(u[i], u_lin[i] + sol["dz"][:N, 8:])
        np.testing.assert_array_equal(out["lam"][i], sol["lam"])
        qp = L.assemble_qp(data, x_lin[i], u_lin[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=qp_o if lay.path else None)
        r = L.kkt_report(qp, sol["dz"], sol["pi"], sol["lam"], sol["sl"], z, Z)
        sg, sb = L.scales(qp)
        assert r["absent"] == 0.0, r                     # multipliers of absent sides are exactly zero
        assert np.all(sol["sl"][Z < 0] == 0.0)           # hard sides carry no slack
        if sol["status"] != 0:
            continue        # (status 1: stopped loosely converged at the iteration limit, accepted by the RTI step as acados does)
        converged += 1
        assert r["stat"] <= 1.01 * tol * sg and r["comp"] <= 1.01 * tol * sg, (r, sg)
        assert r["eq"] <= 1.01 * tol * sb and r["ineq"] <= 1.01 * tol * sb, (r, sb)
        assert r["dual"] <= 1.01 * tol * sg and r["lam_min"] >= 0.0, r
        if lay.name == "empty":
            assert sol["iters"] == 1 and r["stat"] < 1e-10
    assert solved >= B - 1 and converged >= 1, (lay.name, out["status"])
