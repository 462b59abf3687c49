"""The starts of tests/test_gpu_workspace_poison.py, on the oracle alone: from each of them the oracle ends the compared calls with at least
60 % of the instances accepted, which is the condition the GPU cases assert on their clean handle (a comparison of two handles that both
failed would mean little).  The per-step QP cases run three RTI iterations at B = 5 (B = 1 and 3 as well for the four-wave kernel's
layouts, B = 8 at the shortest horizons); the starts of the persistent-loop cases are those of tests/steps_cases.py, which
tests/test_steps_catalogue.py checks in the same way.  The other cases that solve -- the reference start, the control sequence of one
instance, the two-track start, per-instance tuning, the SQP line search -- follow, each with the calls its GPU case makes."""
import numpy as np
import pytest

import layouts as L
import poison_cases as PC
import rollout_ref as R


def _oracle(track, lay, **opts):
    from oracle import oracle as orc

    data = L.make_ocp(lay, **opts).flatten()
    L.apply(data, lay)
    return data, orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))


def _guess(track, data, P, x0):
    RP = R.RolloutProblem.from_data(data, track.s_ref, track.kappa_ref, np.zeros(len(x0), dtype=np.int32))
    x, u = R.rollout(RP, x0, oracle=P)
    return np.ascontiguousarray(x), np.ascontiguousarray(u)


@pytest.mark.parametrize("cid", list(PC.QP_CASES))
def test_oracle_solves_the_qp_case(track, cid):
    _, lay, B, _, seed, _ = PC.QP_CASES[cid]
    data, P = _oracle(track, lay)
    x0, yref, yref_e = PC.qp_start(track, lay, B, seed)
    x, u = _guess(track, data, P, x0)
    pi = lam = None
    for _ in range(PC.QP_SOLVES):
        out = P.rti_step(x, u, x0, yref, yref_e, pi=pi, lam=lam)
        pi, lam = out["pi"], out["lam"]
    st = out["status"]
    print(f"{cid}: seed {seed} status {st.tolist()}")
    assert (st == 0).mean() >= 0.6, (cid, st.tolist())


def test_oracle_solves_the_start_of_the_other_cases(track):
    """The reference layout at B = 5 from the seed of PC.MISC_SEED: every RTI iteration of three."""
    lay, B = PC.MISC_LAYOUT, PC.MISC_B
    data, P = _oracle(track, lay)
    x0, yref, yref_e = PC.qp_start(track, lay, B, PC.MISC_SEED)
    x, u = _guess(track, data, P, x0)
    pi = lam = None
    for _ in range(3):
        out = P.rti_step(x, u, x0, yref, yref_e, pi=pi, lam=lam)
        pi, lam = out["pi"], out["lam"]
        assert (out["status"] == 0).mean() >= 0.6, out["status"].tolist()


def test_oracle_walks_the_ladder_past_the_third_rung_in_the_sqp_case(track):
    """SQP mode, collocation, alpha_reduction 0.9 (29 step lengths) at B = 16 from the perturbed steering guess: two solves of two
    iterations each end 0 or 2, and among the accepted instances some step lengths lie past the third rung and some within it -- so the
    second pair of launches has work, and not for everybody."""
    import steps_cases as S

    lay, B = PC.MISC_LAYOUT, PC.SQP_B
    data, P = _oracle(track, lay, integrator_type="IRK", sim_method_num_steps=1, **S.LIVE)
    x0, yref, yref_e = PC.qp_start(track, lay, B, PC.SQP_SEED)
    x, u = _guess(track, data, P, x0)
    u = np.ascontiguousarray(PC.perturb_steering(u))
    N = lay.N
    pi = np.zeros((B, N + 1, 8)); lam = np.zeros((B, N + 1, 28)); sl = np.zeros((B, N + 1, 28))
    deep = early = 0
    for _ in range(2):
        out = P.sqp_solve(x, u, x0, yref, yref_e, pi=pi, lam=lam, sl=sl, **{**S.sqp_kwargs(data), "alpha_reduction": PC.SQP_ALPHA_RED, "max_iter": 2})
        ok = np.isin(out["status"], (0, 2))
        assert ok.mean() >= 0.6, out["status"].tolist()
        deep += int((out["alpha"][ok] < PC.SQP_DEEP).sum()); early += int((out["alpha"][ok] >= PC.SQP_DEEP).sum())
    assert deep >= 1 and early >= 1, (deep, early)


def test_oracle_solves_the_single_instance_case(track):
    """compute_control at B = 1, three times with the kinematic plant (RK4 x 20) in between: shift + ramp + RTI, status 0 every time."""
    from oracle import oracle as orc

    lay = PC.MISC_LAYOUT
    data, P = _oracle(track, lay)
    x0, _, _ = PC.qp_start(track, lay, 1, PC.MISC_SEED)
    x, u = _guess(track, data, P, x0)
    xc = x0.copy()
    pi = lam = None
    for _ in range(3):
        yref, yref_e = orc.prepare_step(lay.N, xc, 40.0, x, u)
        out = P.rti_step(x, u, xc, yref, yref_e, pi=pi, lam=lam)
        pi, lam = out["pi"], out["lam"]
        assert out["status"].tolist() == [0]
        xc = P.sim_step(xc, u[:, 0].copy(), 0, 20)


def test_oracle_solves_the_two_track_case():
    """The start of the Cartesian / track-kernel case: one RTI iteration per instance on its own track."""
    from ihm2_amd import track as T
    from oracle import oracle as orc

    lay = PC.MISC_LAYOUT
    plans = [T.track_table(n) for n in PC.TWO_TRACKS]
    tid, xf, yref, yref_e = PC.two_track_start(plans)
    st = np.zeros(len(tid), dtype=np.int32)
    for t, p in enumerate(plans):
        sel = tid == t
        data, P = _oracle(p, lay)
        x0 = np.ascontiguousarray(xf[sel])
        x, u = _guess(p, data, P, x0)
        st[sel] = P.rti_step(x, u, x0, np.ascontiguousarray(yref[sel]), np.ascontiguousarray(yref_e[sel]))["status"]
    assert (st == 0).mean() >= 0.6, st.tolist()


def test_oracle_solves_the_instance_tuning_case(track):
    """Two RTI iterations of every instance under its own weights and bounds (a problem of its own on the oracle)."""
    from oracle import oracle as orc

    lay, B = L.TABLE[PC.TUNING_LAYOUT][0], PC.MISC_B
    x0, yref, yref_e = PC.qp_start(track, lay, B, 900 + lay.seed)
    st = []
    for b in range(B):
        data = L.make_ocp(lay).flatten()
        L.apply(data, lay)
        for n, a in PC.tuning_bounds(lay, b).items():
            setattr(data, n, a)
        f = PC.tuning_weight_factor(b)
        data.W, data.W_e = f * np.asarray(data.W), f * np.asarray(data.W_e)
        P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
        xb = np.ascontiguousarray(x0[b:b + 1])
        x, u = _guess(track, data, P, xb)
        pi = lam = None
        for _ in range(2):
            out = P.rti_step(x, u, xb, np.ascontiguousarray(yref[b:b + 1]), np.ascontiguousarray(yref_e[b:b + 1]), pi=pi, lam=lam)
            pi, lam = out["pi"], out["lam"]
        st.append(int(out["status"][0]))
    assert np.mean(np.array(st) == 0) >= 0.6, st
