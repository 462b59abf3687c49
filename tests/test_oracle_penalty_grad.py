"""Gradients in the slack penalties z, Z, the NumPy references alone (tests/penalty_grad_ref.py; no GPU): (1) the closed form
zeta_s = (c t - lam sgn r zeta_k) / (t rho + lam) against the slack unknowns of the dense system that keeps every slack as a variable;
(2) <gradient, direction> against central differences of L = <seed, z+> over whole QP solves with the penalties moved (the oracle's
interior point at qp_tol 1e-9), with the cases, seeds, direction, measure and condition of tests/penalty_grad_cases.py, which
tests/test_gpu_penalty_grad.py takes for the same check of the kernel -- and the zero prediction failing it."""
import numpy as np
import pytest

import cost_cases as C
import layouts as L
import penalty_grad_cases as PC
import penalty_grad_ref as PR
import sens_ref as S
import slack_seed_cases as SC
from oracle import oracle as orc
from test_gpu_adjoint_weights import ROUND_TOL, _solve_refined
from test_oracle_slack_seeds import _problem


def _refined(M, rhs):
    return _solve_refined(M, rhs[:, None])[:, 0]


@pytest.mark.parametrize("name", SC.REF_LAYOUTS)
def test_closed_form_against_the_system_that_keeps_the_slacks(track, name):
    """Random seed_z and seed_s on B = 3 solved instances: the closed form on the dense system's own zeta_z against that system's slack
    unknowns (refined in extended precision), to ROUND_TOL of the instance's largest |zeta_s|.  Some slack must be live."""
    lay = L.TABLE[name][0]
    N, B = lay.N, 3
    data, P = _problem(lay, track)
    nc, z, Z = SC.soft_arrays(data, lay)
    x0, yref, yref_e = C.start(track, B, 77, N)
    xbar, ubar = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
    A, Bm, b = P.linearize(xbar, ubar)
    rng = np.random.default_rng(21)
    worst, worst_entry, live = 0.0, 0.0, 0
    for i in range(B):
        ref = P.build_qp(xbar[i], ubar[i], x0[i], yref[i], yref_e[i])
        sol = SC.qp_solve(ref, data, z, Z, C.QP_TOL)
        assert sol["status"] == 0
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
        dz, lam, sl = sol["dz"], sol["lam"], sol["sl"]
        seed_z = rng.standard_normal((N + 1, 10)); seed_z[N, 8:] = 0.0
        seed_s = rng.standard_normal((N + 1, 2 * nc))
        zs, zeta, _ = PR.zeta_s(qp, dz, lam, sl, z, Z, seed_z, seed_s, solve=_refined)
        cf, _ = PR.closed_form(qp, dz, lam, sl, z, Z, zeta, seed_s)
        assert np.array_equal(zs != 0.0, cf != 0.0)
        live += int(np.count_nonzero(zs))
        worst = max(worst, float(np.abs(cf - zs).max() / np.abs(zs).max()))
        worst_entry = max(worst_entry, float((np.abs(cf - zs) / np.maximum(np.abs(zs), 1e-12)).max()))
    print(f"PENALTY-GRAD reference {name}: closed form against the dense system {worst:.2e} of the largest |zeta_s|, {worst_entry:.2e} of "
          f"the entry (floored at 1e-12); live sides {live}")
    assert live > 0, "no soft side carries a slack"
    assert worst <= ROUND_TOL, worst


@pytest.mark.parametrize("name", PC.CASES)
def test_gradient_against_whole_solves(track, name):
    """The condition of tests/penalty_grad_cases.py on the directions "z" and "both" (the direction "Z" is printed), with at least 75 %
    of the batch kept; the zero prediction does not meet it."""
    lay, B, seed = SC.CASES[name]
    N = lay.N
    data, P = _problem(lay, track)
    nc, z, Z = SC.soft_arrays(data, lay)
    x0, yref, yref_e = C.start(track, B, seed, N)
    xbar, ubar = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
    A, Bm, b = P.linearize(xbar, ubar)
    ddz, ddZ = PC.direction(z, Z)
    ok = np.ones(B, dtype=bool)
    slack_live = np.zeros(B, dtype=bool)
    pred = {d: np.zeros((B, PC.N_SEEDS)) for d in PC.DIRECTIONS}
    fd = {d: np.zeros((B, PC.N_SEEDS)) for d in PC.DIRECTIONS}
    free = {d: np.zeros((B, PC.N_SEEDS)) for d in PC.DIRECTIONS}
    for i in range(B):
        ref = P.build_qp(xbar[i], ubar[i], x0[i], yref[i], yref_e[i])
        sol = SC.qp_solve(ref, data, z, Z, C.QP_TOL)
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
        if sol["status"] != 0 or S.weakly_active(qp, sol["dz"], sol["lam"], sl=sol["sl"], soft_z=z, soft_Z=Z):
            ok[i] = False
            continue
        dz, lam, sl = sol["dz"], sol["lam"], sol["sl"]
        slack_live[i] = sl[Z >= 0.0].max() > 1e-6
        sd = PC.seeds(i, N)
        gz, gZ = np.zeros((PC.N_SEEDS,) + z.shape), np.zeros((PC.N_SEEDS,) + z.shape)
        for m in range(PC.N_SEEDS):
            zs, _, _ = PR.zeta_s(qp, dz, lam, sl, z, Z, sd[m], np.zeros_like(z), solve=_refined)
            gz[m], gZ[m] = PR.gradients(zs, sl)
        for d in PC.DIRECTIONS:
            dzd, dZd = PC.pick(d, ddz, ddZ)
            pred[d][i] = PC.predict(gz, gZ, dzd, dZd)
            free[d][i] = PC.free_scale(qp, dz, lam, sl, z, Z, sd, dzd, dZd)
            Lv = []
            for sign in (1.0, -1.0):
                s2 = SC.qp_solve(ref, data, z + sign * PC.EPS * dzd, Z + sign * PC.EPS * dZd, C.QP_TOL)
                ok[i] &= s2["status"] == 0
                zp = s2["dz"].copy(); zp[N, 8:] = 0.0
                Lv.append(np.einsum("skj,kj->s", sd, zp))
            fd[d][i] = (Lv[0] - Lv[1]) / (2 * PC.EPS)
    keep = np.flatnonzero(ok)
    print(f"PENALTY-GRAD-FD reference {name}: instances with a slack above 1e-6: {int(slack_live[keep].sum())} of {keep.size}")
    errs = {d: PC.measure(pred[d], fd[d], free[d]) for d in PC.DIRECTIONS}
    zero = {d: PC.measure(0.0 * pred[d], fd[d], free[d]) for d in PC.DIRECTIONS}
    PC.verdict("PENALTY-GRAD-FD reference", name, errs, zero, keep, B)
