"""The conditions on the inputs of tests/test_gpu_multi_track.py, with the oracle alone: the two-track cases of tests/multi_track_cases.py
leave solved instances on both tracks, their track rows are alive on both tracks, the dense sensitivity reference tells the instance's own
widths from track 0's, and the lap-wrap starts sit where the test needs them.  These are conditions, not measurements: where a case misses
one, its seed or batch size changes, not the condition.  The figures are printed (pytest -s) and kept in NOTES.md."""
import functools

import numpy as np
import pytest

import multi_track_cases as M
import sens_ref as S
import slack_seed_cases as SSC
import steps_cases as SC


@functools.lru_cache(maxsize=None)
def _run(layout, B, swapped=False):
    """Two oracle RTI steps of the layout on two tracks from the per-track Stanley guess; with ``swapped`` the two rows of the widths
    change places."""
    lay = M.L.TABLE[layout][0]
    data = M.flat_data(lay)
    w = M.widths(lay)
    P = M.oracle_problem(data, lay, None if w is None or not swapped else w[::-1].copy())
    tid = M.track_ids(B)
    x0, yref, yref_e = M.start_arrays(lay, B, 900 + lay.seed)
    x, u = M.stanley_guess(data, lay, x0, tid)
    guess = (x.copy(), u.copy())
    pi = lam = None
    first = None
    for _ in range(2):
        out = P.rti_step(x, u, x0, yref, yref_e, track_id=tid, pi=pi, lam=lam)
        pi, lam = out["pi"], out["lam"]
        first = out["status"].copy() if first is None else first
    return dict(lay=lay, data=data, P=P, tid=tid, x0=x0, yref=yref, yref_e=yref_e, guess=guess, x=x, u=u, status=out["status"], first=first)


@pytest.mark.parametrize("name", list(M.CASES))
def test_half_of_each_track_solves(name):
    c = M.CASES[name]
    r = _run(c.layout, c.B)
    per_track = [(int(((r["status"] == 0) & (r["tid"] == t)).sum()), int((r["tid"] == t).sum())) for t in range(2)]
    print(f"MULTI-TRACK {name} B {c.B}: solved per track {per_track}")
    for ok, n in per_track:
        assert ok >= 0.5 * n, per_track


@pytest.mark.parametrize("name", M.TRACK_ROW_CASES)
def test_track_rows_are_alive_on_both_tracks(name):
    """u of every instance that solves with the widths as they are and with their rows swapped differs by more than 1e-4: a hundred times
    the 1e-6 to which GPU and oracle are compared."""
    c = M.CASES[name]
    a, b = _run(c.layout, c.B), _run(c.layout, c.B, True)
    both = (a["status"] == 0) & (b["status"] == 0)
    moved = np.abs(a["u"] - b["u"]).max((1, 2))
    print(f"MULTI-TRACK {name} B {c.B}: {int(both.sum())} solve both ways, smallest move of u {moved[both].min():.2e}")
    for t in range(2):
        assert (both & (a["tid"] == t)).any(), t
    assert (moved[both] > 1e-4).all(), moved


@pytest.mark.parametrize("name", M.TRACK_ROW_CASES)
def test_sensitivity_reference_tells_the_tracks_apart(name):
    """sens_ref.sensitivities on the oracle's QP solution of solved track-1 instances (at most four), with the track rows of the blind
    track_id = 0 QP in place of the instance's own: at least ten tolerances away on stage 0 and over the horizon, on at least one."""
    c = M.CASES[name]
    r = _run(c.layout, c.B)
    lay, data, P = r["lay"], r["data"], r["P"]
    _, z, Z = SSC.soft_arrays(data, lay)
    xg, ug = r["guess"]
    found = []
    for i in np.flatnonzero((r["first"] == 0) & (r["tid"] == 1))[:4]:
        args = (xg[i], ug[i], r["x0"][i], r["yref"][i], r["yref_e"][i])
        qp = P.build_qp(*args, track_id=1)
        sol = SSC.qp_solve(qp, data, z, Z, data.ipm_tol, data.ipm_iter_max)
        assert SC.rti_status_of_qp(sol) == 0
        rx, ru = S.sensitivities(qp, sol["dz"], sol["lam"], sol["sl"], z, Z)
        blind = M.blind_rows(qp, P, *args)
        found.append(M.sens_distance(rx, ru, *S.sensitivities(blind, sol["dz"], sol["lam"], sol["sl"], z, Z), rx, ru))
    assert found
    print(f"MULTI-TRACK {name} B {c.B}: blind reference away by (stage 0, horizon) {[(f'{a:.1e}', f'{b:.1e}') for a, b in found]}")
    assert any(M.discriminates(d0, d) for d0, d in found), found


@pytest.mark.parametrize("key", list(SC.TWO_TRACK))
def test_oracle_solves_the_first_step_of_the_two_track_loops(key):
    """The two-track variants of the persistent-loop cases (steps_cases.TWO_TRACK), as tests/test_steps_catalogue.py asks of the cases
    on one track: at least 60 % of the instances end the oracle's first step with status 0 -- and here on each of the two tracks."""
    import rollout_ref as R

    case, _ = SC.TWO_TRACK[key]
    lay = SC.LAYOUTS[case.layout]
    data = M.L.make_ocp(lay, **case.ocp_opts()).flatten()
    M.L.apply(data, lay)
    P = SC.oracle_problem(None, data, lay, tables=M.tables(), widths=M.widths(lay))
    tid = SC.track_ids(case)
    x0, yref, yref_e = SC.start(None, case)
    x, u = R.rollout(R.RolloutProblem.from_data(data, *M.tables(), tid), x0, oracle=P)
    st = SC.oracle_rti_step(P, data, None, np.ascontiguousarray(x), np.ascontiguousarray(u), x0, yref, yref_e, track_id=tid)["status"]
    print(f"MULTI-TRACK loop {key}: seed {case.seed} status {st.tolist()}")
    assert (st == 0).mean() >= 0.6, st
    for t in range(2):
        assert (st[tid == t] == 0).mean() >= 0.5, (t, st)


def test_lap_wrap_starts():
    Ls = M.lap_lengths()
    assert Ls[1] - Ls[0] > 100.0
    x0, tid = M.wrap_start()
    np.testing.assert_array_equal(tid, [0, 0, 1, 1, 1, 1, 0, 0])
    np.testing.assert_allclose(Ls[tid[:4]] - x0[:4, 0], [4.0, 9.0, 4.0, 9.0], atol=1e-9)
    between = x0[4:6, 0]
    assert (between - Ls[0] >= 20.0).all() and (Ls[1] - between >= 20.0).all()
    # the cars that must not wrap stay between the two lap lengths for the whole run even at the speed limit of the layouts (31 m/s)
    assert (between + M.WRAP_STEPS * 0.05 * 31.0 < Ls[1]).all()
    assert (x0[6:, 0] + M.WRAP_STEPS * 0.05 * 31.0 < Ls[0]).all()
    s_ref, _ = M.tables()
    np.testing.assert_allclose(-s_ref[:, 0], Ls, rtol=0, atol=1e-9)       # the kernels read L = -s_ref[track_id * nknots]
