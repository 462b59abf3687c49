"""Adjoint seeds on the soft slacks, the NumPy references alone (tests/slack_seed_ref.py; no GPU): (1) adj_ref.adjoint on the seed plus the
fold against the dense system that keeps every soft slack as a variable, on soft tables and on the lateral-acceleration row; (2) the total
gradient of the cost with the fold against central differences of the cost over whole QP solves (the oracle's interior point at qp_tol
1e-9, which returns the slacks), and the same prediction without the fold failing -- on the cases tests/test_gpu_slack_seeds.py takes
for the same check of the kernel."""
import copy

import numpy as np
import pytest

import adj_ref as R
import cost_cases as C
import cost_ref as CR
import layouts as L
import sens_ref as S
import slack_seed_cases as SC
import slack_seed_ref as SR
from oracle import oracle as orc
from test_gpu_adjoint import REF_TOL_X, REF_TOL_Y
from test_gpu_adjoint_weights import _solve_refined
from test_gpu_cost import _adjoint_refined


def _problem(lay, track, W=None, W_e=None):
    ocp = L.make_ocp(lay)
    ocp.solver_options.qp_tol = C.QP_TOL
    ocp.solver_options.qp_solver_iter_max = 200
    data = ocp.flatten()
    L.apply(data, lay)
    if W is not None:
        data.W, data.W_e = W, W_e
    return data, orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))


def _refined(M, rhs):
    return _solve_refined(M, rhs[:, None])[:, 0]


@pytest.mark.parametrize("name", SC.REF_LAYOUTS)
def test_fold_against_the_system_that_keeps_the_slacks(track, name):
    """Random seed_z and seed_s on B = 3 solved instances: nu_0 and Gy' zeta of adj_ref.adjoint(seed_z + fold) against those of
    adjoint_with_slacks(seed_z, seed_s), both dense solves refined in extended precision, to REF_TOL_X / REF_TOL_Y of the instance's
    largest entry.  The slack seeds must matter: without the fold the same comparison is off by more than a hundred tolerances."""
    lay = L.TABLE[name][0]
    N, B = lay.N, 3
    data, P = _problem(lay, track)
    nc, z, Z = SC.soft_arrays(data, lay)
    x0, yref, yref_e = C.start(track, B, 77, N)
    xbar, ubar = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
    A, Bm, b = P.linearize(xbar, ubar)
    rng = np.random.default_rng(21)
    worst_x = worst_y = without = 0.0
    used = 0
    for i in range(B):
        ref = P.build_qp(xbar[i], ubar[i], x0[i], yref[i], yref_e[i])
        sol = SC.qp_solve(ref, data, z, Z, C.QP_TOL)
        assert sol["status"] == 0
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
        dz, lam, sl = sol["dz"], sol["lam"], sol["sl"]
        seed_z = rng.standard_normal((N + 1, 10)); seed_z[N, 8:] = 0.0
        seed_s = rng.standard_normal((N + 1, 2 * nc))
        f = SR.fold(qp, dz, lam, sl, z, Z, seed_s)
        used += int(np.count_nonzero(np.abs(f).sum(1)))
        Gy, Gye = R.gy_tables(lambda yr, yre, i=i: P.build_qp(xbar[i], ubar[i], x0[i], yr, yre)["g"], yref[i], yref_e[i])
        zeta, nu0 = _adjoint_refined(qp, dz, lam, sl, z, Z, seed_z + f)
        zeta_w, nu0_w = SR.adjoint_with_slacks(qp, dz, lam, sl, z, Z, seed_z, seed_s, solve=_refined)
        zeta_0, nu0_0 = _adjoint_refined(qp, dz, lam, sl, z, Z, seed_z)
        gy, gye = R.gradients(zeta, Gy, Gye)
        gy_w, gye_w = R.gradients(zeta_w, Gy, Gye)
        sy = max(np.abs(gy_w).max(), np.abs(gye_w).max())
        worst_x = max(worst_x, np.abs(nu0 - nu0_w).max() / np.abs(nu0_w).max())
        worst_y = max(worst_y, np.abs(gy - gy_w).max() / sy, np.abs(gye - gye_w).max() / sy)
        without = max(without, np.abs(nu0_0 - nu0_w).max() / np.abs(nu0_w).max())
    print(f"SLACK-SEED reference {name}: x0 {worst_x:.2e} yref {worst_y:.2e}; without the fold x0 {without:.2e}; stages folded {used}")
    assert used > 0, "no soft side is active: the fold was not exercised"
    assert worst_x <= REF_TOL_X and worst_y <= REF_TOL_Y, (worst_x, worst_y)
    assert without > 100 * REF_TOL_X, without


def whole_solve_errors(track, name, fold=True, only=None):
    """The whole-solve check of case `name`: per direction the errors |pred - fd| / max(|fd|, |pred_free|) of the instances, the mask of
    the instances kept (every solve converged, not weakly active) and their slack costs.  pred: cost_ref.total_gradient with the
    adjoint on the seed plus the fold (fold = False: on the seed alone); only: a subset of the directions."""
    lay, B, seed = SC.CASES[name]
    N = lay.N
    data, P = _problem(lay, track)
    nc, z, Z = SC.soft_arrays(data, lay)
    x0, yref, yref_e = C.start(track, B, seed, N)
    xbar, ubar = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
    W0, We0 = np.asarray(data.W, dtype=np.float64), np.asarray(data.W_e, dtype=np.float64)
    assert all(np.array_equal(W0[k], W0[0]) for k in range(N))
    dirs = C.directions(name, B, N, W0[0], We0)

    def solve(prob, d_, i, x0_, yref_, yref_e_):
        ref = prob.build_qp(xbar[i], ubar[i], x0_, yref_, yref_e_)
        sol = SC.qp_solve(ref, d_, z, Z, C.QP_TOL)
        xp, up = xbar[i] + sol["dz"][:, :8], ubar[i] + sol["dz"][:N, 8:]
        slk, slk_a = SC.split_slacks(sol["sl"], nc)
        return ref, sol, xp, up, CR.cost(d_, xp, up, yref_, yref_e_, slk=slk, slk_a=slk_a)

    def adjoint(qp, dz, lam, sl, z_, Z_, sd):
        if fold:
            sd = sd + SR.fold(qp, dz, lam, sl, z_, Z_, SR.cost_slack_seed(sl, z_, Z_))
        return R.adjoint(qp, dz, lam, sl, z_, Z_, sd)

    A, Bm, b = P.linearize(xbar, ubar)
    ok = np.ones(B, dtype=bool)
    slack_cost = np.zeros(B)
    grad = {k: np.zeros(s) for k, s in (("x0", (B, 8)), ("yref", (B, N, 12)), ("yref_e", (B, 8)), ("W", (B, 12, 12)), ("W_e", (B, 8, 8)))}
    free = copy.deepcopy(grad)
    for i in range(B):
        ref, sol, xp, up, c = solve(P, data, i, x0[i], yref[i], yref_e[i])
        slack_cost[i] = c["slack_cost"]
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
        if sol["status"] != 0 or S.weakly_active(qp, sol["dz"], sol["lam"], sl=sol["sl"], soft_z=z, soft_Z=Z):
            ok[i] = False
            continue
        Gy, Gye = R.gy_tables(lambda yr, yre, i=i: P.build_qp(xbar[i], ubar[i], x0[i], yr, yre)["g"], yref[i], yref_e[i])
        for dst, lm in ((grad, sol["lam"]), (free, 0.0 * sol["lam"])):
            g = CR.total_gradient(data, qp, sol["dz"], lm, sol["sl"], z, Z, Gy, Gye, xp, up, yref[i], yref_e[i], adjoint=adjoint)
            for k in dst:
                dst[k][i] = g[k]
    errs = {}
    for dname in only or C.DIRECTIONS:
        d, eps = dirs[dname], C.EPS[dname]
        J = []
        for sign in (1.0, -1.0):
            dp, Pp = (_problem(lay, track, W0 + sign * eps * d["W"][None], We0 + sign * eps * d["W_e"]) if dname.startswith("W") else (data, P))
            Js = np.zeros(B)
            for i in np.flatnonzero(ok):
                _, sol, _, _, c = solve(Pp, dp, i, x0[i] + sign * eps * d["x0"][i], yref[i] + sign * eps * d["yref"][i],
                                        yref_e[i] + sign * eps * d["yref_e"][i])
                ok[i] &= sol["status"] == 0
                Js[i] = c["cost"]
            J.append(Js)
        fd = (J[0] - J[1]) / (2 * eps)
        with np.errstate(invalid="ignore", divide="ignore"):
            errs[dname] = np.abs(C.contract(grad, d) - fd) / np.maximum(np.abs(fd), np.abs(C.contract(free, d)))
    return errs, ok, slack_cost


@pytest.mark.parametrize("name", list(SC.CASES))
def test_cost_gradient_with_the_fold_against_whole_solves(track, name):
    """The six directions of cost_cases.DIRECTIONS: cost_cases.profile is met over all of them, at least 75 % of the instances are kept
    and at least half of those carry a slack cost above 1e-6.  Without the fold the same prediction fails the profile on the x0
    direction: the check can see the feature."""
    lay, B, seed = SC.CASES[name]
    errs, ok, slack_cost = whole_solve_errors(track, name)
    keep = np.flatnonzero(ok)
    assert keep.size >= 0.75 * B, (keep.size, B)
    for dname, e in errs.items():
        (med, s5, s3), _ = C.profile(e[keep])
        print(f"SLACK-SEED-FD reference {name} {dname}: median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {e[keep].max():.2e}")
    allerr = np.concatenate([e[keep] for e in errs.values()])
    (med, s5, s3), met = C.profile(allerr)
    used = float(np.mean(slack_cost[keep] > SC.SLACK_COST_MIN))
    print(f"SLACK-SEED-FD reference {name}: kept {keep.size} of {B}, slack cost in use {used:.2f}, median {med:.2e} share<=1e-5 {s5:.3f} "
          f"share<=1e-3 {s3:.3f} max {allerr.max():.2e}")
    assert met, (med, s5, s3)
    assert used >= 0.5, used
    e0, ok0, _ = whole_solve_errors(track, name, fold=False, only=("x0",))
    (med, s5, s3), met0 = C.profile(e0["x0"][np.flatnonzero(ok0)])
    print(f"SLACK-SEED-FD reference {name} x0 without the fold: median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f}")
    assert not met0, (med, s5, s3)
