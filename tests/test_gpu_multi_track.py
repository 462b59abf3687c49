"""Every kernel that reads track_id, on handles that hold two tracks (tests/multi_track_cases.py: instance b on track b mod 2, two
circuits of different lap length, corridor widths that differ per track and per side).  On one track track_id[b] is 0 everywhere, and
an index written as b, 0 or trk without its * 2, a widths pointer left unset in one launch or the lap length of the wrong track gives
the right answer; the rest of the suite runs the derivative kernels, the persistent loop on track rows and the lap wrap on one track only.

* the forward QP against the oracle with per-instance track ids and an independent KKT check, on hard and soft track rows, the a_lat
  row, a ragged last wave, and k_qp_block behind a linearisation on two tables;
* the five includers of csrc/sens_rows_body.hpp and the entries composed of them against their dense references with every
  instance's own track rows -- and, for the sensitivities, a guard that the reference with track 0's rows for everybody is far from
  the GPU's result, so the comparison cannot pass for lack of signal;
* the persistent loop on track rows against launches per step, bit for bit, and its first step against the oracle;
* the lap wrap per track: cars on the longer track that sit between the two lap lengths must not be thrown back;
* set_track_id after a solve: the next solve, its sensitivities and the lap wrap are those of a handle created with the new ids.

tests/test_oracle_multi_track.py holds the conditions on the inputs without a GPU.  Tolerances are those of the module that owns the
entry, imported from it.  The handles of the derivative tests are solved once per case and shared (read only)."""
import numpy as np
import pytest
from conftest import make_ocp

import adjw_ref as RW
import cost_ref as CR
import drive
import layouts as L
import multi_track_cases as M
import penalty_grad_ref as PR
import sens_ref as SENS
import slack_seed_cases as SSC
import slack_seed_ref as SR
import steps_cases as S
import test_gpu_adjoint as TA
import test_gpu_adjoint_weights as TW
import test_gpu_cost as TC
import test_gpu_penalty_grad as TP
import test_gpu_sensitivity as TS
import test_gpu_slack_seeds as TSS
import test_gpu_steps_catalogue as TSC
from test_gpu_qp_layouts import _widen

pytestmark = pytest.mark.gpu


def _subset(ok, tid, per=4):
    """At most ``per`` solved instances of each track: the first and the last ones (the ragged last wave's)."""
    out = []
    for t in range(2):
        idx = np.flatnonzero(ok & (tid == t))
        out.append(np.unique(np.concatenate([idx[:per // 2], idx[-(per - per // 2):]])) if idx.size else idx)
    assert all(o.size for o in out), "the compared subset must hold instances of both tracks"
    return np.sort(np.concatenate(out))


# ---- 1. the forward QP against the oracle ----

@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_qp_matches_oracle_and_kkt(name):
    """Two RTI solves against OracleProblem.rti_step with the same track ids, with the assertions and tolerances of
    tests/test_gpu_qp_layouts.py::test_layout_matches_oracle_and_kkt; the KKT check runs on at most four converged instances per track."""
    from oracle import oracle as orc

    case = M.CASES[name]
    lay, B, tid = case.lay, case.B, case.track_id
    s = M.solver(case)
    data = s.data
    P = M.oracle_problem(data, lay)
    x0, yref, yref_e = M.start(s, case)
    _, z, Z = SSC.soft_arrays(data, lay)
    tol = data.ipm_tol
    x, u = s.get_x(), s.get_u()            # the oracle's iterate
    pi = lam = None
    for it in range(2):
        xg_lin, ug_lin = s.get_x(), s.get_u()
        st = s.solve()
        assert s.get_launch_record()["qp"] == case.kernel
        out = P.rti_step(x, u, x0, yref, yref_e, track_id=tid, pi=pi, lam=lam)
        pi, lam = out["pi"], out["lam"]
        itg = s.get_qp_iter()
        print(f"MULTI-TRACK forward {name} it{it}: status {st.tolist()} oracle {out['status'].tolist()}")
        np.testing.assert_array_equal(st, out["status"])
        ok = st == 0
        for t in range(2):
            assert (ok & (tid == t)).sum() >= 0.5 * (tid == t).sum(), (t, st)
        assert ok.sum() >= 0.6 * B, st
        same = itg[ok] == out["qp_iter"][ok]
        assert same.mean() >= 0.999 and np.abs(itg[ok] - out["qp_iter"][ok]).max() <= 1
        eq = ok & (itg == out["qp_iter"])
        xg, ug = s.get_x(), s.get_u()
        pig, lamg = s.get_multipliers()
        slg = s.get_slacks()
        if lay.alat:
            lam_a, slk_a = s.get_alat_multipliers()
            lamg, slg = _widen(lamg, lam_a), _widen(slg, slk_a)
        for t in range(2):
            assert (eq & (tid == t)).any(), t
        ex = np.max(np.abs(xg[eq] - x[eq]) / (1 + np.abs(x[eq]))); eu = np.max(np.abs(ug[eq] - u[eq]) / (1 + np.abs(u[eq])))
        sp = max(1.0, float(np.abs(pi[eq][:, 1:]).max())); sl_ = max(1.0, float(np.abs(lam[eq]).max()))
        epi = np.abs(pig[eq][:, 1:] - pi[eq][:, 1:]).max() / sp; elam = np.abs(lamg[eq] - lam[eq]).max() / sl_
        print(f"MULTI-TRACK forward {name} it{it}: x {ex:.2e} u {eu:.2e} pi {epi:.2e} lam {elam:.2e}")
        assert ex < 1e-7 and eu < 1e-7
        assert epi <= 1e-6 and elam <= 1e-6          # (pi_0 is not defined: x_0 is eliminated)
        conv = ok & np.all(s.get_qp_residuals() <= tol, axis=1)
        assert conv.sum() >= 0.5 * ok.sum()
        sub = _subset(conv, tid)
        A, Bm, b = P.linearize(np.ascontiguousarray(xg_lin[sub]), np.ascontiguousarray(ug_lin[sub]), track_id=tid[sub])
        for j, i in enumerate(sub):
            ref = P.build_qp(xg_lin[i], ug_lin[i], x0[i], yref[i], yref_e[i], track_id=int(tid[i]))
            qp = L.assemble_qp(data, xg_lin[i], ug_lin[i], x0[i], yref[i], yref_e[i], A[j], Bm[j], b[j], nonlinear=ref if lay.path else None)
            dz = np.zeros((s.N + 1, L.NZ)); dz[:, :8] = xg[i] - xg_lin[i]; dz[:s.N, 8:] = ug[i] - ug_lin[i]
            r = L.kkt_report(qp, dz, pig[i], lamg[i], slg[i], z, Z)
            sg, sb = L.scales(qp)
            assert r["absent"] == 0.0, (i, r)
            comp_tol = 1.01 * tol * (sg + float(np.abs(lamg[i]).max()) * sb + float(np.abs(slg[i]).max()) * sg)
            assert r["stat"] <= 1.01 * tol * sg and r["comp"] <= comp_tol and r["dual"] <= 1.01 * tol * sg, (i, r, sg, comp_tol)
            assert r["eq"] <= 1.01 * tol * sb and r["ineq"] <= 1.01 * tol * sb and r["lam_min"] >= 0.0, (i, r, sb)
            if (data.soft_Z is not None or lay.alat_soft) and not lay.alat:
                sol = orc.qp_solve(**ref, iter_max=data.ipm_iter_max, tol=tol, mu0=data.ipm_mu0, tau0=data.ipm_tau0, soft_z=z, soft_Z=Z)
                if sol["iters"] == itg[i]:
                    assert np.max(np.abs(slg[i] - sol["sl"]) / (1 + np.abs(sol["sl"]))) < 1e-7
    s.free()


# ---- 2., 3. the kernels that include sens_rows_body.hpp, after one solve per case ----

_SOLVED = {}


def _solved(name):
    """One solve of the case in the sensitivity mode 2 and the host's view of every instance's QP with its own track's rows
    (test_gpu_slack_seeds._Solved), shared by the tests below."""
    if name not in _SOLVED:
        case = M.CASES[name]
        c = TSS._Solved(None, case.lay, case.B, case.seed, "default", tracks=case, sens_mode=2)
        for t in range(2):
            assert (c.ok & (c.track_id == t)).sum() >= 0.5 * (c.track_id == t).sum(), (t, c.st)
        c.sub = _subset(c.ok, c.track_id)
        assert set(c.track_id[c.sub]) == {0, 1}
        c.seed_x, c.seed_u = TA._seeds(case.B, 2, c.N, 40 + case.lay.seed)
        rng = np.random.default_rng(41 + case.lay.seed)
        c.seed_s, c.seed_sa = rng.standard_normal((case.B, 2, c.N + 1, 28)), rng.standard_normal((case.B, 2, c.N + 1, 2))
        _SOLVED[name] = c
    return _SOLVED[name]


@pytest.fixture(scope="module", autouse=True)
def _free_shared_handles():
    yield
    for c in _SOLVED.values():
        c.s.free()
    _SOLVED.clear()


def _nan_rows(g, ok, keys=None):
    for k in (g if keys is None else keys):
        assert np.isnan(g[k][~ok]).all() and np.isfinite(g[k][ok]).all(), k


@pytest.mark.parametrize("name", M.TRACK_ROW_CASES)
def test_x0_sensitivities_take_each_instances_track_rows(name):
    """k_sens: get_x0_sensitivities (mode 2) against sens_ref at the GPU's own iterate, 1e-7 on stage 0 and 1e-6 over the horizon -- and
    not against the reference that gives every instance track 0's rows: on the compared track-1 instances the GPU's result is at least
    ten tolerances away from that one, on at least one of them."""
    c = _solved(name)
    sx, su = c.s.get_x0_sensitivities()
    assert np.isnan(su[~c.ok]).all() and np.isnan(sx[~c.ok]).all() and np.isfinite(su[c.ok]).all() and np.isfinite(sx[c.ok]).all()
    far = []
    for i in c.sub[c.track_id[c.sub] == 1]:
        qp, dz, lam, sl = c.qp(i)
        blind = M.blind_rows(qp, c.P, c.xbar[i], c.ubar[i], c.x0[i], c.yref[i], c.yref_e[i])
        bx, bu = SENS.sensitivities(blind, dz, lam, sl, c.z, c.Z)
        far.append(M.sens_distance(sx[i], su[i], bx, bu, *SENS.sensitivities(qp, dz, lam, sl, c.z, c.Z)))
    print(f"MULTI-TRACK sens {name}: the GPU's result from the blind reference (stage 0, horizon) {[(f'{a:.1e}', f'{b:.1e}') for a, b in far]}")
    missed = None
    try:        # (both findings are reported: a kernel that takes track 0's rows misses the reference and sits on the blind one)
        w0, w = TS._check_against_reference(c.s, c.P, c.data, c.x0, c.yref, c.yref_e, c.xbar, c.ubar, sx, su, c.nc, c.z, c.Z, True, c.sub,
                                            track_id=c.track_id)
        print(f"MULTI-TRACK sens {name}: against sens_ref {w0:.2e} on stage 0, {w:.2e} over the horizon")
    except AssertionError as e:
        missed = e
    assert any(M.discriminates(d0, d) for d0, d in far), ("inputs do not discriminate", far, "against sens_ref:", missed)
    if missed is not None:
        raise missed


@pytest.mark.parametrize("name", M.TRACK_ROW_CASES)
def test_adjoint_takes_each_instances_track_rows(name):
    """k_adj<false>: eval_adjoint_sensitivities against adj_ref (both seeds), and the identity against the forward sweep."""
    c = _solved(name)
    g = c.s.eval_adjoint_sensitivities(c.seed_x, c.seed_u)
    TA._finite_where_solved(g, c.ok)
    sx, su = c.s.get_x0_sensitivities()
    e_id = TA._identity_error(g["x0"], sx, su, c.seed_x, c.seed_u, c.ok)
    e_y, e_x = TA._reference_errors(c.s, c.P, c.data, c.x0, c.yref, c.yref_e, c.xbar, c.ubar, g, c.seed_x, c.seed_u, c.nc, c.z, c.Z, True,
                                    c.sub, seeds=(0, 1), track_id=c.track_id)
    print(f"MULTI-TRACK adjoint {name}: identity {e_id:.2e} ref yref {e_y:.2e} ref x0 {e_x:.2e}")
    assert e_id <= TA.IDENTITY_TOL, e_id
    assert e_y <= TA.REF_TOL_Y and e_x <= TA.REF_TOL_X, (e_y, e_x)


# The two sides form a side's gap from the same terms -- the raw bound, up to four terms of the row's value at xbar and the row times the
# step -- in different orders and contractions: they may differ by the rounding of each of these, GAP_ROUNDINGS units of 2^-52 of the
# sum of the absolute terms (test_gpu_slack_seeds._Solved.bound_mag, the magnitude that module's fold tolerance is relative to).
GAP_ROUNDINGS = 8


def _weight_entry_excess(c, g, seeds=(0, 1)):
    """Every entry of grad_W / grad_W_e of the compared instances against the refined dense reference, relative to the entry's own
    magnitude (the second measure of tests/test_gpu_adjoint_weights.py::_reference_errors), with the bound

        REF_TOL + GAP_ROUNDINGS * v,    v = how far the reference's own entry moves, relative to the same magnitude, when every gap of its
                                            QP is shifted by one unit of 2^-52 of the sum of its absolute terms.

    An entry is a product of a component of zeta and a residual.  A component of zeta that a strongly active row pins is the seed
    divided by the barrier weight lam / t of that row, so it inherits the relative error of the gap t, which is formed by cancellation: such
    an entry is not determined by the data to REF_TOL, in the reference no more than in the kernel.  v measures that on the reference
    alone, without the kernel's result.  Measured: v <= 8.3e-8, under a tenth of REF_TOL, on every entry of every case but ten entries of instance 7 of alat_soft
    (track 1; condition number of the dense system 5e24), where it reaches 2.1e-6 on grad_W_e[1, 1] -- an entry of 6.2e-16 beside a
    largest entry of 2.0e-3 -- and the kernel stands 4.7e-6 from the reference.  Returns (the worst deviation in units of its bound, the
    largest v, the number of entries with v > REF_TOL / 10, the number of entries)."""
    import adj_ref as R

    N = c.N
    nz_ = N * 10 + 8
    zp = TW._zplus(c.o["x"], c.o["u"])
    excess = own = 0.0
    loose = total = 0
    for i in c.sub:
        qp, dz, lam, sl = c.qp(i)
        shift = 2.0 ** -52 * c.bound_mag(i)
        moved = dict(qp, dl=qp["dl"] + shift[:, :c.nc], du=qp["du"] - shift[:, c.nc:])
        refs = []
        for q in (qp, moved):
            Mx = R.kkt_matrix(q, dz, lam, sl, c.z, c.Z)
            rhs = np.zeros((Mx.shape[0], len(seeds)))
            for n, j in enumerate(seeds):
                sd = np.zeros((N + 1, 10)); sd[:, :8] = c.seed_x[i, j]; sd[:N, 8:] = c.seed_u[i, j]
                rhs[:nz_, n] = sd.reshape(-1)[:nz_]
            refs.append(TW._solve_refined(Mx, rhs))
        for n, j in enumerate(seeds):
            zeta = np.zeros((2, N + 1, 10))
            for r in range(2):
                zeta[r].reshape(-1)[:nz_] = refs[r][:nz_, n]
            want = [RW.weight_gradients(c.data, zeta[r], zp[i], c.yref[i], c.yref_e[i]) for r in range(2)]
            _, mags = RW.stage_terms(c.data, zeta[0], zp[i], c.yref[i])
            mag = (TW._sym(mags.sum(0)), TW._sym(np.outer(np.abs(zeta[0, N, :8]), np.abs(zp[i, N, :8] - c.yref_e[i]))))
            for w, got in enumerate((g["W"][i, j], g["W_e"][i, j])):
                nz = mag[w] > 0.0
                v = np.abs(want[1][w] - want[0][w])[nz] / mag[w][nz]
                d = np.abs(got - want[0][w])[nz] / mag[w][nz]
                excess = max(excess, float((d / (TW.REF_TOL + GAP_ROUNDINGS * v)).max()))
                own = max(own, float(v.max()))
                loose += int((v > 0.1 * TW.REF_TOL).sum()); total += int(nz.sum())
    return excess, own, loose, total


@pytest.mark.parametrize("name", M.TRACK_ROW_CASES)
def test_adjoint_in_the_weights_takes_each_instances_track_rows(name):
    """k_adj<true>: eval_adjoint_weight_sensitivities against adj_ref + adjw_ref on the refined dense solve, to REF_TOL of the largest
    entry of the magnitude per instance and seed -- the error model of k_adj (tests/test_gpu_adjoint_weights.py: "relative to the largest
    entry of zeta and not entry by entry"); rows of the wrong track move this figure to the order of 1 -- and, the owning module's second
    measure, every entry to REF_TOL of its own magnitude plus what the reference itself is uncertain by (_weight_entry_excess)."""
    c = _solved(name)
    g = c.s.eval_adjoint_weight_sensitivities(c.seed_x, c.seed_u)
    TA._finite_where_solved(g, c.ok)
    e, e_entry = TW._reference_errors(c.s, c.P, c.data, c.x0, c.yref, c.yref_e, c.xbar, c.ubar, g, c.seed_x, c.seed_u, c.nc, c.z, c.Z, True,
                                      c.sub, track_id=c.track_id)
    excess, own, loose, total = _weight_entry_excess(c, g)
    print(f"MULTI-TRACK adjoint weights {name}: ref {e:.2e} (entry by entry {e_entry:.2e}; the reference's own uncertainty {own:.2e} at worst, "
          f"above a tenth of the tolerance on {loose} of {total} entries; worst entry at {excess:.2f} of its bound)")
    assert e <= TW.REF_TOL, (e, e_entry)
    assert excess <= 1.0, (excess, e_entry, own)
    assert loose <= 0.01 * total, (loose, total)          # the bound is the owning module's own on all but a handful of entries


@pytest.mark.parametrize("name", M.SOFT_CASES)
def test_slack_fold_takes_each_instances_track_rows(name):
    """k_slack_fold: eval_adjoint_slack_sensitivities on zero stage seeds against the _w entry fed slack_seed_ref.fold of every solved
    instance's own QP, to FOLD_TOL of the largest entry of each output, instance and seed; the fold is live on both tracks."""
    c = _solved(name)
    B, N, lay = c.B, c.N, c.lay
    fx, fu = np.zeros((B, 2, N + 1, 8)), np.zeros((B, 2, N, 2))
    for i in np.flatnonzero(c.ok):
        qp, dz, lam, sl = c.qp(i)
        for q in range(2):
            sd = _widen(c.seed_s[i, q], c.seed_sa[i, q]) if lay.alat else c.seed_s[i, q]
            f = SR.fold(qp, dz, lam, sl, c.z, c.Z, sd)
            fx[i, q], fu[i, q] = f[:, :8], f[:N, 8:]
    for t in range(2):
        assert np.abs(fx[c.track_id == t]).max() > 0.0, "the fold was not exercised on track %d" % t
    got = c.s.eval_adjoint_slack_sensitivities(None, None, c.seed_s, c.seed_sa)
    want = c.s.eval_adjoint_weight_sensitivities(fx, fu)
    worst = 0.0
    for k in want:
        assert got[k].shape == want[k].shape
        _nan_rows(got, c.ok, [k])
        ax = tuple(range(2, want[k].ndim))
        worst = max(worst, float((np.abs(got[k][c.ok] - want[k][c.ok]).max(ax) / np.abs(want[k][c.ok]).max(ax)).max()))
    print(f"MULTI-TRACK fold {name}: worst {worst:.2e} of the largest entry")
    assert worst <= TSS.FOLD_TOL, worst


@pytest.mark.parametrize("name", M.SOFT_CASES)
def test_penalty_gradients_take_each_instances_track_rows(name):
    """k_penalty_grad behind k_adj<true, true>: eval_adjoint_penalty_sensitivities against penalty_grad_ref on the refined dense system,
    with the measures of tests/test_gpu_penalty_grad.py::test_kernel_against_the_host."""
    c = _solved(name)
    N = c.N
    got = c.s.eval_adjoint_penalty_sensitivities(c.seed_x, c.seed_u, c.seed_s, c.seed_sa)
    _nan_rows(got, c.ok, TP.PEN + ("zeta",))
    worst_zeta = worst_g = 0.0
    for i in c.sub:
        qp, dz, lam, sl = c.qp(i)
        for q in range(2):
            seed_z = np.zeros((N + 1, 10)); seed_z[:, :8] = c.seed_x[i, q]; seed_z[:N, 8:] = c.seed_u[i, q]
            seed_s = TP._wide(c, c.seed_s[i, q], c.seed_sa[i, q])
            zs, zeta, _ = PR.zeta_s(qp, dz, lam, sl, c.z, c.Z, seed_z, seed_s, solve=TP._refined)
            _, mag = PR.closed_form(qp, dz, lam, sl, c.z, c.Z, zeta, seed_s)
            wz, wZ = PR.gradients(zs, sl)
            gz, gZ = TP._got_wide(c, got, i, q)
            worst_zeta = max(worst_zeta, float(np.abs(got["zeta"][i, q] - zeta).max() / np.abs(zeta).max()))
            scale = float(mag.max())
            worst_g = max(worst_g, float(np.abs(gz - wz).max() / scale), float(np.abs(gZ - wZ).max() / (scale * min(1.0, sl.max()))))
    print(f"MULTI-TRACK penalty gradients {name}: zeta {worst_zeta:.2e}, gradients {worst_g:.2e}")
    assert worst_zeta <= TP.REF_TOL and worst_g <= TP.REF_TOL, (worst_zeta, worst_g)


def _total_errors(c, g, i, adjoint, kept=None):
    """The five totals of a cost-gradient entry of instance i against cost_ref.total_gradient, relative to the largest entry of the
    magnitude (tests/test_gpu_cost.py::test_composition, tests/test_gpu_slack_seeds.py::test_cost_seeds_and_totals)."""
    N, o, data = c.N, c.o, c.data
    qp, dz, lam, sl = c.qp(i)
    Gy, Gye = c.gy(i)
    t = CR.total_gradient(data, qp, dz, lam, sl, c.z, c.Z, Gy, Gye, o["x"][i], o["u"][i], c.yref[i], c.yref_e[i], adjoint=adjoint)
    if kept is None:
        sd, _ = CR.seeds(data, o["x"][i], o["u"][i], c.yref[i], c.yref_e[i])
        zeta, _ = adjoint(qp, dz, lam, sl, c.z, c.Z, sd)
    else:
        zeta = kept["zeta"]
    zp = np.zeros((N + 1, 10)); zp[:, :8] = o["x"][i]; zp[:N, 8:] = o["u"][i]
    _, mags = RW.stage_terms(data, zeta, zp, c.yref[i])
    eN = np.abs(zp[N, :8] - c.yref_e[i])
    mag = dict(W=0.5 * (mags.sum(0) + mags.sum(0).T) + t["explicit"]["mag"]["W"],
               W_e=0.5 * (np.outer(np.abs(zeta[N, :8]), eN) + np.outer(eN, np.abs(zeta[N, :8]))) + t["explicit"]["mag"]["W_e"],
               x0=np.abs(t["x0"]), yref=np.abs(t["adj"]["yref"]) + t["explicit"]["mag"]["yref"],
               yref_e=np.abs(t["adj"]["yref_e"]) + t["explicit"]["mag"]["yref_e"])
    worst = max(float(np.abs(g[k][i] - t[k]).max() / mag[k].max()) for k in TC.GRADS)
    entry = max(float((np.abs(g[k][i] - t[k])[mag[k] > 0.0] / mag[k][mag[k] > 0.0]).max()) for k in ("W", "W_e"))
    return worst, entry


@pytest.mark.parametrize("name", M.TRACK_ROW_CASES)
def test_cost_gradient_totals_take_each_instances_track_rows(name):
    """eval_cost_gradient on the hard tables, eval_cost_gradient_soft on the soft ones: the five totals against cost_ref.total_gradient
    on the refined dense system (with every slack kept as a variable on the soft tables), REF_TOL of the owning module -- of the largest
    entry of the magnitude and, on the hard tables as tests/test_gpu_cost.py::test_composition asks, the weights entry by entry (the
    soft tables' owner, tests/test_gpu_slack_seeds.py::test_cost_seeds_and_totals, has the first measure alone; the second is printed)."""
    c = _solved(name)
    soft = name in M.SOFT_CASES
    g = c.s.eval_cost_gradient_soft() if soft else c.s.eval_cost_gradient()
    _nan_rows(g, c.ok, TC.GRADS)
    worst = worst_entry = 0.0
    for i in c.sub:
        if soft:
            kept = {}

            def adjoint(qp_, dz_, lam_, sl_, z_, Z_, sd, kept=kept):
                kept["zeta"], nu0 = SR.adjoint_with_slacks(qp_, dz_, lam_, sl_, z_, Z_, sd, SR.cost_slack_seed(sl_, z_, Z_), solve=TSS._refined)
                return kept["zeta"], nu0

            w, e = _total_errors(c, g, i, adjoint, kept)
        else:
            w, e = _total_errors(c, g, i, TC._adjoint_refined)
        worst, worst_entry = max(worst, w), max(worst_entry, e)
    print(f"MULTI-TRACK cost totals {name}: against the dense reference {worst:.2e} (weights entry by entry {worst_entry:.2e})")
    assert worst <= (TSS.REF_TOL if soft else TC.REF_TOL), worst
    if not soft:
        assert worst_entry <= TC.REF_TOL, worst_entry


@pytest.mark.parametrize("name", M.SOFT_CASES)
def test_cost_gradient_in_the_penalties_takes_each_instances_track_rows(name):
    """eval_cost_gradient_penalties: dJ/dz, dJ/dZ against the dense system with the cost's seeds, the measure and REF_TOL of
    tests/test_gpu_penalty_grad.py::test_cost_totals."""
    c = _solved(name)
    g = c.s.eval_cost_gradient_penalties()
    _nan_rows(g, c.ok, TP.PEN)
    gw = {k: v[:, None] for k, v in g.items() if k in TP.PEN}
    worst = largest = 0.0
    for i in c.sub:
        qp, dz, lam, sl = c.qp(i)
        sd, _ = CR.seeds(c.data, c.o["x"][i], c.o["u"][i], c.yref[i], c.yref_e[i])
        cs = SR.cost_slack_seed(sl, c.z, c.Z)
        zs, zeta, _ = PR.zeta_s(qp, dz, lam, sl, c.z, c.Z, sd, cs, solve=TP._refined)
        _, mag = PR.closed_form(qp, dz, lam, sl, c.z, c.Z, zeta, cs)
        wz, wZ = PR.gradients(zs, sl)
        present = np.concatenate([np.isfinite(qp["dl"]), np.isfinite(qp["du"])], 1)
        ez, eZ = PR.cost_partials(np.where(present, sl, 0.0), c.Z)
        gz, gZ = TP._got_wide(c, gw, i, 0)
        scale = float(mag.max() + sl.max())
        worst = max(worst, float(np.abs(gz - (wz + ez)).max() / scale), float(np.abs(gZ - (wZ + eZ)).max() / (scale * min(1.0, sl.max()))))
        largest = max(largest, float(np.abs(gz).max()))
    print(f"MULTI-TRACK cost in the penalties {name}: against the dense reference {worst:.2e}, largest dJ/dz {largest:.2e}")
    assert largest > 0.0
    assert worst <= TP.REF_TOL, worst


# ---- 4. the persistent loop on track rows ----

@pytest.fixture
def single_wave_qp(monkeypatch):
    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")          # read when a handle is created: the four-wave kernel of small batches sums in another order


@pytest.mark.parametrize("key", list(S.TWO_TRACK))
def test_persistent_loop_equals_step_by_step_on_two_tracks(track, key, single_wave_qp):
    """steps_cases.TWO_TRACK through tests/test_gpu_steps_catalogue.py::_assert_loop_equals_steps: the launch record is the case's, and
    STEPS control steps in one launch give what as many step() calls give, bit for bit."""
    case, expect = S.TWO_TRACK[key]
    assert TSC.STEPS == 4
    TSC._assert_loop_equals_steps(track, case, "default", expect)


@pytest.mark.parametrize("key", [k for k in S.TWO_TRACK if not S.LAYOUTS[S.TWO_TRACK[k][0].layout].alat])
def test_first_step_of_the_two_track_loops_matches_oracle(track, key, single_wave_qp):
    """step()'s solve of the same configurations against the oracle with track ids (the loop-equals-step identity would not see a mistake
    both sides share).  The a_lat row on two tracks against the oracle: test_forward_qp_matches_oracle_and_kkt[alat_soft]."""
    TSC._assert_rti_matches_oracle(track, S.TWO_TRACK[key][0])


# ---- 5. the lap wrap per track ----

def _wrap_handle(tid, wrap, created_with=None, x0=None):
    """created_with: the handle is created with these ids, takes one step() from x0 under them (every start lies inside both tables'
    three laps) and is then given tid."""
    from ihm2_amd.solver import BatchedOcpSolver

    s = BatchedOcpSolver(make_ocp(), M.WRAP_B, *M.tables(), track_id=tid if created_with is None else created_with)
    s.set_lap_wrap(wrap)
    if created_with is not None:
        s.set_x0(x0); s.init_guess()
        s.step(40.0, model=0, M_sim=25)
        assert (s.get_status() == 0).any()
        s.set_track_id(tid)
    return s


def _wrap_run(s, x0, persistent=False):
    """From x0, the device's guess and zero multipliers: one solve without the plant (the loop starts from a control: the plant applies
    the last solve's u0, which a handle that has stepped before would otherwise carry over), then WRAP_STEPS control steps: (u0 history,
    s history, status history, final x, final u)."""
    s.set_x0(x0); s.init_guess(); s.set_multipliers(None, None)
    s.prepare_step(40.0); s.solve()
    if persistent:
        h = s.run_steps(40.0, M.WRAP_STEPS, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
        assert s.get_launch_record()["steps"].startswith("k_steps<")
    else:
        h = drive.per_step(s, 40.0, M.WRAP_STEPS, model=0, M_sim=25)
    out = (h["u0"], h["x0"][:, :, 0], h["status"], s.get_x(), s.get_u())
    s.free()
    return out


def test_lap_wrap_takes_each_cars_own_lap_length(single_wave_qp):
    """The existing lap-wrap test's assertions on two tables: the cars near the end of their own lap cross L_t and are moved back by
    L_t; the cars on the longer track between the two lap lengths are never touched (with track 0's L they would be thrown back at
    once); the persistent loop does the same as the step() calls, bit for bit."""
    Ls = M.lap_lengths()
    x0, tid = M.wrap_start()
    (u0, s0, st0, _, _), (u1, s1, st1, xs1, us1) = _wrap_run(_wrap_handle(tid, False), x0), _wrap_run(_wrap_handle(tid, True), x0)
    np.testing.assert_array_equal(st0, st1)
    assert (st0 == 0).all(), st0
    Lc = Ls[tid[:4]]
    print(f"MULTI-TRACK lap wrap: last s without the wrap {s0[-1].tolist()}, with it {s1[-1].tolist()}")
    assert (s0[:, :4].max(0) > Lc).all()                  # the first four cross their own line
    assert (s1[:, :4].max(0) < Lc + 1.0).all()            # wrapped: back by one lap at the next step
    d =np.abs(np.mod(s0[-1, :4], Lc) - np.mod(s1[-1, :4], Lc))
    assert (np.minimum(d, Lc - d) < 1e-6).all(), d
    assert np.max(np.abs(u0 - u1) / (1.0 + np.abs(u0))) < 1e-6          # same controls up to the rounding of s - L
    np.testing.assert_array_equal(s1[:, 4:], s0[:, 4:])   # the cars that never reach their lap length: the same bits
    np.testing.assert_array_equal(u1[:, 4:], u0[:, 4:])
    assert (s1[:, 4:6].min(0) > Ls[0] + 20.0).all()
    assert np.all(np.abs(xs1[:, 0, 0] - s1[-1]) < 2.0)    # the iterate moved with x0
    u2, s2, st2, xs2, us2 = _wrap_run(_wrap_handle(tid, True), x0, persistent=True)
    for a, b, k in ((u2, u1, "u0"), (s2, s1, "s"), (st2, st1, "status"), (xs2, xs1, "x"), (us2, us1, "u")):
        np.testing.assert_array_equal(a, b, err_msg=k)


# ---- 6. set_track_id after a solve ----

@pytest.mark.parametrize("name", ["path_hard", "path_soft_both_sides", "alat_soft"])
def test_set_track_id_after_a_solve(name):
    """A handle that has solved with tid and is then given 1 - tid (x0, guess, references, zero multipliers and slacks set again for the
    new assignment) solves, and differentiates, as a handle created with 1 - tid does: bit for bit."""
    case = M.CASES[name]
    lay, B, tid = case.lay, case.B, case.track_id
    new = (1 - tid).astype(np.int32)
    x0, yref, yref_e = M.start_arrays(lay, B, case.seed + 10, tid=new)

    def run(s):
        s.set_x0_sensitivities(2)
        M.start(s, case, x0, yref, yref_e)
        s.set_slacks(np.zeros((B, lay.N + 1, 28)))
        if lay.alat:
            s.set_alat_multipliers(np.zeros((B, lay.N + 1, 2)), np.zeros((B, lay.N + 1, 2)))
        st = s.solve()
        out = dict(TS._outputs(s, alat=lay.alat), status=st)
        out["sens_x"], out["sens_u"] = s.get_x0_sensitivities()
        return out

    s = M.solver(case)
    s.set_x0_sensitivities(2)
    M.start(s, case)
    s.solve()
    s.set_track_id(new)
    moved = run(s)
    s.free()
    fresh_handle = M.solver(case, track_id=new)
    fresh = run(fresh_handle)
    fresh_handle.free()
    ok = np.isin(fresh["status"], (0, 2))
    for t in range(2):
        assert (ok & (new == t)).any(), fresh["status"]
    for k in fresh:
        np.testing.assert_array_equal(moved[k], fresh[k], err_msg=k)


def test_lap_wrap_follows_set_track_id(single_wave_qp):
    """A handle created with the other assignment, which has taken a step() under it (lap wrap on) and is then given the ids: the closed
    loop with the lap wrap, through step() and through run_steps, is that of a handle created with them."""
    x0, tid = M.wrap_start()
    other = (1 - tid).astype(np.int32)
    for persistent in (False, True):
        a = _wrap_run(_wrap_handle(tid, True), x0, persistent)
        b = _wrap_run(_wrap_handle(tid, True, created_with=other, x0=x0), x0, persistent)
        for p, q in zip(a, b):
            np.testing.assert_array_equal(q, p)
