"""The NumPy reference of the OCP's cost and of its total gradient (tests/cost_ref.py composed with tests/adj_ref.py and
tests/adjw_ref.py): (a) against central differences of the cost over whole oracle solves (OracleProblem.rti_step at qp_tol 1e-9) in
x0, yref, yref_e, W and W_e, on the layouts, instances and directions of tests/cost_cases.py -- the ones tests/test_gpu_cost.py takes
for the same check of the kernel; (b) the cost against an independent evaluation in np.longdouble.  No GPU."""
import copy

import numpy as np
import pytest

import adj_ref as R
import cost_cases as C
import cost_ref as CR
import layouts as L
import sens_ref as S
from oracle import oracle as orc


def _problem(lay, track, W=None, W_e=None):
    ocp = L.make_ocp(lay)
    ocp.solver_options.qp_tol = C.QP_TOL
    ocp.solver_options.qp_solver_iter_max = 200
    data = ocp.flatten()
    L.apply(data, lay)
    if W is not None:
        data.W, data.W_e = W, W_e
    return data, orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))


@pytest.mark.parametrize("name", list(C.CASES))
def test_reference_against_central_differences_of_whole_solves(track, name):
    """<dJ/d., direction> of cost_ref.total_gradient against (J(+eps) - J(-eps)) / (2 eps) with J = cost_ref.cost at the solution of a
    whole RTI step from the same start, for the six directions of cost_cases.directions.  The error is |pred - fd| / max(|fd|, |pred_free|),
    pred_free the same prediction with all multipliers zero; weakly active instances and instances a solve of which failed are left out
    (tests/test_gpu_adjoint_weights.py::test_du0_dW_against_whole_solves, whose acceptance profile this is).  The GPU test inherits
    these inputs: the profile is asserted for the reference alone, so they are known to be fair."""
    lay, B, seed = C.CASES[name]
    N = lay.N
    data, P = _problem(lay, track)
    x0, yref, yref_e = C.start(track, B, seed, N)
    xbar, ubar = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
    W0, We0 = np.asarray(data.W, dtype=np.float64), np.asarray(data.W_e, dtype=np.float64)
    assert all(np.array_equal(W0[k], W0[0]) for k in range(N))
    dirs = C.directions(name, B, N, W0[0], We0)

    def solve(prob, x0_, yref_, yref_e_):
        x, u = xbar.copy(), ubar.copy()
        out = prob.rti_step(x, u, x0_, yref_, yref_e_)
        return x, u, out

    def costs(d_, x, u, yref_, yref_e_):
        return np.array([CR.cost(d_, x[i], u[i], yref_[i], yref_e_[i])["cost"] for i in range(B)])

    xp, up, out = solve(P, x0, yref, yref_e)
    ok = out["status"] == 0
    A, Bm, b = P.linearize(xbar, ubar)
    z, Z = L.soft_arrays(data)
    grad = {k: np.zeros(s) for k, s in (("x0", (B, 8)), ("yref", (B, N, 12)), ("yref_e", (B, 8)), ("W", (B, 12, 12)), ("W_e", (B, 8, 8)))}
    free = copy.deepcopy(grad)
    for i in np.flatnonzero(ok):
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i])
        dz = np.zeros((N + 1, 10)); dz[:, :8] = xp[i] - xbar[i]; dz[:N, 8:] = up[i] - ubar[i]
        lam, sl = out["lam"][i], np.zeros((N + 1, 2 * L.NC))
        if S.weakly_active(qp, dz, lam, sl=sl, soft_z=z, soft_Z=Z):
            ok[i] = False
            continue
        Gy, Gye = R.gy_tables(lambda yr, yre, i=i: P.build_qp(xbar[i], ubar[i], x0[i], yr, yre)["g"], yref[i], yref_e[i])
        for dst, lm in ((grad, lam), (free, 0.0 * lam)):
            g = CR.total_gradient(data, qp, dz, lm, sl, z, Z, Gy, Gye, xp[i], up[i], yref[i], yref_e[i])
            for k in dst:
                dst[k][i] = g[k]
    errs = []
    for dname in C.DIRECTIONS:
        d, eps = dirs[dname], C.EPS[dname]
        J = []
        for sign in (1.0, -1.0):
            if dname.startswith("W"):
                dp, Pp = _problem(lay, track, W0 + sign * eps * d["W"][None], We0 + sign * eps * d["W_e"])
            else:
                dp, Pp = data, P
            yr, yre = yref + sign * eps * d["yref"], yref_e + sign * eps * d["yref_e"]
            x, u, o = solve(Pp, x0 + sign * eps * d["x0"], yr, yre)
            ok &= o["status"] == 0
            J.append(costs(dp, x, u, yr, yre))
        fd = (J[0] - J[1]) / (2 * eps)
        pred, fr = C.contract(grad, d), C.contract(free, d)
        with np.errstate(invalid="ignore"):         # instances left out have no prediction
            e = np.abs(pred - fd) / np.maximum(np.abs(fd), np.abs(fr))
        errs.append(e)
        (med, s5, s3), _ = C.profile(e[ok])
        print(f"COST-FD reference {name} {dname}: median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {e[ok].max():.2e}")
    keep = np.flatnonzero(ok)
    assert keep.size >= 0.75 * B, (keep.size, B)
    allerr = np.concatenate([e[keep] for e in errs])
    (med, s5, s3), met = C.profile(allerr)
    print(f"COST-FD reference {name}: kept {keep.size} of {B}, median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {allerr.max():.2e}")
    assert met, (med, s5, s3)


@pytest.mark.parametrize("name", ["soft_4_per_lane_mixed", "hard_5_per_lane_stage_W", "alat_soft"])
def test_cost_against_longdouble(track, name):
    """cost_ref.cost (einsum on the selector matrix, fp64) against the term-by-term evaluation in np.longdouble, at a solved iterate
    with slack values drawn at random on every side (the reference must pick the soft ones with a finite bound): 1e-14 of the
    cancellation-free magnitude.  The stage costs add up to the cost, the slack cost is their slack part."""
    assert np.finfo(np.longdouble).eps < 1e-18
    lay = L.TABLE[name][0]
    N, B = lay.N, 3
    data, P = _problem(lay, track)
    x0, yref, yref_e = C.start(track, B, 77, N)
    x, u = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
    P.rti_step(x, u, x0, yref, yref_e)
    rng = np.random.default_rng(3)
    for i in range(B):
        slk, slk_a = rng.uniform(0.0, 0.5, (N + 1, 28)), rng.uniform(0.0, 0.5, (N + 1, 2))
        c = CR.cost(data, x[i], u[i], yref[i], yref_e[i], slk=slk, slk_a=slk_a)
        want = CR.cost_longdouble(data, x[i], u[i], yref[i], yref_e[i], slk=slk, slk_a=slk_a)
        assert abs(c["cost"] - want) <= 1e-14 * c["mag"]["cost"], (c["cost"], float(want))
        assert (c["slack_cost"] > 0.0) == (data.soft_Z is not None) and abs(c["stage_cost"].sum() - c["cost"]) <= 1e-14 * c["mag"]["cost"]
        hard = CR.cost(data, x[i], u[i], yref[i], yref_e[i])
        assert abs(hard["cost"] + c["slack_cost"] - c["cost"]) <= 1e-14 * c["mag"]["cost"] and hard["slack_cost"] == 0.0
