"""Adjoint sensitivities of the RTI QP's solution (tests/adj_ref.py): the identity against the forward sensitivities of
tests/sens_ref.py, and central differences of the oracle's QP solver in the reference yref.  No GPU."""
import numpy as np

import adj_ref as R
import layouts as L
import sens_ref as S
from oracle import oracle as orc
from test_oracle_layouts import LAYOUTS, _setup

EPS = 1e-5
QP_TOL = 1e-9


def _instances(track):
    """Every instance of the 30 layouts: (data, P, solve, ref, qp, z, Z, (x, u, x0, yref, yref_e) of the instance)."""
    for lay in LAYOUTS:
        data, P, x0, x, u, yref, yref_e = _setup(lay, track)
        A, Bm, b = P.linearize(x, u)
        z, Z = L.soft_arrays(data)
        soft = data.soft_Z is not None

        def solve(qp, tol, data=data, z=z, Z=Z, soft=soft):
            return orc.qp_solve(**qp, iter_max=200, tol=tol, mu0=data.ipm_mu0, tau0=data.ipm_tau0,
                                soft_z=z if soft else None, soft_Z=Z if soft else None)

        for i in range(x.shape[0]):
            ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i])
            qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
            yield data, P, solve, ref, qp, z, Z, (x[i], u[i], x0[i], yref[i], yref_e[i])


def test_identity_against_the_forward_sensitivities(track):
    """nu_0 = sum_k sens_x[k]' seed_x[k] + sum_k sens_u[k]' seed_u[k]: two dense solves of one matrix, assembled twice (sens_ref keeps the
    soft slacks as variables, adj_ref eliminates them).  Measured: median 1.4e-12, max 6.0e-7 of the largest entry (with sens_ref's own
    matrix and a seed as right-hand side: 1.1e-7)."""
    rng = np.random.default_rng(11)
    errs = []
    for data, P, solve, ref, qp, z, Z, _ in _instances(track):
        sol = solve(ref, QP_TOL)
        if sol["status"] != 0:
            continue
        N = data.N
        seed = rng.standard_normal((N + 1, 10))
        seed[N, 8:] = 0.0
        sx, su = S.sensitivities(qp, sol["dz"], sol["lam"], sol["sl"], z, Z)
        _, nu0 = R.adjoint(qp, sol["dz"], sol["lam"], sol["sl"], z, Z, seed)
        gx0 = np.einsum("kij,ki->j", sx, seed[:, :8]) + np.einsum("kij,ki->j", su, seed[:N, 8:])
        errs.append(np.max(np.abs(gx0 - nu0)) / max(np.max(np.abs(gx0)), 1e-12))
    errs = np.array(errs)
    print("identity: n %d median %.2e max %.2e" % (errs.size, np.median(errs), errs.max()))
    assert errs.size >= 80, errs.size
    assert errs.max() <= 1e-6, errs.max()


def test_du0_dyref_against_central_differences_on_the_layouts(track):
    """d u_0,T / d yref in a random direction (d, d_e): Gy' zeta of the seed e_{u_0,T} against central differences of the oracle's QP
    solution with g rebuilt at yref +- EPS d.  The error is taken relative to max(|fd|, |pred_free|), pred_free the same prediction with
    all multipliers zero: where the constraints pin u_0 the derivative is about 0 and a plain relative error means nothing.
    Measured (89 of 90 instances): qp_tol 1e-9 median 7.9e-10, 96.6 % <= 1e-5, max 3.6e-3; 1e-11 median 1.2e-10, 98.9 % <= 1e-5, max 4.9e-5."""
    rng = np.random.default_rng(5)
    errs = {QP_TOL: [], 1e-11: []}
    total = 0
    for data, P, solve, ref, qp, z, Z, (x, u, x0, yref, yref_e) in _instances(track):
        total += 1
        sol = solve(ref, QP_TOL)
        if sol["status"] != 0 or S.weakly_active(qp, sol["dz"], sol["lam"], sl=sol["sl"], soft_z=z, soft_Z=Z):
            continue
        N = data.N
        d, de = rng.standard_normal(yref.shape), rng.standard_normal(yref_e.shape)
        gp = P.build_qp(x, u, x0, yref + EPS * d, yref_e + EPS * de)["g"]
        gm = P.build_qp(x, u, x0, yref - EPS * d, yref_e - EPS * de)["g"]
        p, m = solve(dict(ref, g=gp), 1e-11), solve(dict(ref, g=gm), 1e-11)
        assert p["status"] == 0 and m["status"] == 0
        fd = (p["dz"][0, 8] - m["dz"][0, 8]) / (2 * EPS)
        Gy, Gye = R.gy_tables(lambda yr, yre: P.build_qp(x, u, x0, yr, yre)["g"], yref, yref_e)
        seed = np.zeros((N + 1, 10))
        seed[0, 8] = 1.0

        def predict(lam, dz, sl):
            zeta, _ = R.adjoint(qp, dz, lam, sl, z, Z, seed)
            gy, gye = R.gradients(zeta, Gy, Gye)
            return float(np.sum(gy * d) + gye @ de)

        for tol in errs:
            so = sol if tol == QP_TOL else solve(ref, tol)
            pred, free = predict(so["lam"], so["dz"], so["sl"]), predict(0.0 * so["lam"], so["dz"], so["sl"])
            errs[tol].append(abs(pred - fd) / max(abs(fd), abs(free)))
    e9, e11 = np.array(errs[QP_TOL]), np.array(errs[1e-11])
    for name, e in (("1e-9", e9), ("1e-11", e11)):
        print("qp_tol %s: n %d of %d median %.2e share<=1e-5 %.3f max %.2e" % (name, e.size, total, np.median(e), np.mean(e <= 1e-5), e.max()))
    assert total == 90 and e9.size >= 80, (total, e9.size)
    assert np.median(e9) <= 1e-7 and np.mean(e9 <= 1e-5) >= 0.90, (np.median(e9), np.mean(e9 <= 1e-5))
    assert np.median(e11) <= 1e-7 and np.mean(e11 <= 1e-5) >= 0.95 and e11.max() <= 1e-3, (np.median(e11), np.mean(e11 <= 1e-5), e11.max())
