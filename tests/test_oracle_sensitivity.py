"""x0 sensitivities of the RTI QP's solution (tests/sens_ref.py) against central differences of the oracle's QP solver, against a
separately written LQR recursion, through the fifteen-row QP of the lateral-acceleration row, and the C ABI's new symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import sample_x0

import layouts as L
import sens_ref as S
from oracle import oracle as orc
from test_oracle_layouts import LAYOUTS, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
QP_TOL = 1e-9


def _fd(solve, qp, dz_shape):
    """du_0/dx0 (2,8) by central differences of the QP's solution in dx0 = x0 - xbar_0 (the linearisation stays at xbar)."""
    out = np.zeros((2, 8))
    for j in range(8):
        d = np.zeros(8); d[j] = EPS
        p = solve(dict(qp, dx0=qp["dx0"] + d), 1e-11)
        m = solve(dict(qp, dx0=qp["dx0"] - d), 1e-11)
        assert p["status"] == 0 and m["status"] == 0
        out[:, j] = (p["dz"][0, 8:] - m["dz"][0, 8:]) / (2 * EPS)
    return out


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-12))


def test_tau_is_the_headers():
    assert S._hdr_tau() == S.TAU


def test_reference_against_central_differences_on_the_layouts(track):
    """At qp_tol 1e-9 the interior point's own smoothing shows on the instances with sides near the active-set boundary (NOTES.md:
    at qp_tol 1e-11 those agree to 5e-4 or better): the median and the bulk are held at 1e-9, every instance at 1e-11."""
    errs = {QP_TOL: [], 1e-11: []}
    for lay in LAYOUTS:
        data, P, x0, x, u, yref, yref_e = _setup(lay, track)
        A, Bm, b = P.linearize(x, u)
        z, Z = L.soft_arrays(data)
        soft = data.soft_Z is not None

        def solve(qp, tol):
            return orc.qp_solve(**qp, iter_max=200, tol=tol, mu0=data.ipm_mu0, tau0=data.ipm_tau0,
                                soft_z=z if soft else None, soft_Z=Z if soft else None)

        for i in range(x.shape[0]):
            ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i])
            qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
            sol = solve(ref, QP_TOL)
            if sol["status"] != 0 or S.weakly_active(qp, sol["dz"], sol["lam"], sl=sol["sl"], soft_z=z, soft_Z=Z):
                continue
            fd = _fd(solve, ref, sol["dz"].shape)
            for tol in errs:
                so = sol if tol == QP_TOL else solve(ref, tol)
                _, su = S.sensitivities(qp, so["dz"], so["lam"], so["sl"], z, Z)
                errs[tol].append(_rel(su[0], fd))
    e9, e11 = np.array(errs[QP_TOL]), np.array(errs[1e-11])
    assert e9.size >= 60, e9.size
    assert np.median(e9) <= 1e-6 and np.mean(e9 <= 1e-5) >= 0.85, (np.median(e9), np.mean(e9 <= 1e-5))
    assert np.median(e11) <= 1e-7 and np.mean(e11 <= 1e-5) >= 0.95 and e11.max() <= 1e-3, (np.median(e11), np.mean(e11 <= 1e-5), e11.max())


def test_without_constraints_it_is_the_lqr_gain(track):
    lay = L.Layout("empty", xbox="none", ubox=False, grows="none")
    data, P, x0, x, u, yref, yref_e = _setup(lay, track)
    A, Bm, b = P.linearize(x, u)
    z, Z = L.soft_arrays(data)
    for i in range(x.shape[0]):
        qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i])
        nc = qp["R"].shape[1]
        sx, su = S.sensitivities(qp, np.zeros((data.N + 1, 10)), np.zeros((data.N + 1, 2 * nc)), np.zeros((data.N + 1, 2 * nc)), z, Z)
        K0 = S.lqr_gain0(qp["H"], qp["A"], qp["Bm"])
        assert np.max(np.abs(su[0] + K0)) <= 1e-10 * max(1.0, np.abs(K0).max())
        np.testing.assert_allclose(sx[0], np.eye(8), rtol=0, atol=1e-12)
        # the forward sweep: x_1 = A_0 + B_0 du_0/dx0
        np.testing.assert_allclose(sx[1], A[i][0] + Bm[i][0] @ su[0], rtol=0, atol=1e-10 * max(1.0, np.abs(sx[1]).max()))


def _qp_solve15(qp, tol, iter_max, mu0, tau0, soft_z, soft_Z):
    """orc_qp_solve_soft of the fifteen-row build (arrays 15 / 30 wide), called directly: oracle.qp_solve is the fourteen-row one's."""
    lib = orc.lib15()
    N = qp["A"].shape[0]
    nc = qp["R"].shape[1]
    dp = C.POINTER(C.c_double)
    arrs = {k: np.ascontiguousarray(qp[k], dtype=np.float64) for k in ("H", "g", "A", "Bm", "b", "dx0", "R", "dl", "du")}
    sz, sZ = np.ascontiguousarray(soft_z, dtype=np.float64), np.ascontiguousarray(soft_Z, dtype=np.float64)
    dz = np.zeros((N + 1, 10)); pi = np.zeros((N + 1, 8)); lam = np.zeros((N + 1, 2 * nc)); t = np.zeros((N + 1, 2 * nc))
    sl = np.zeros((N + 1, 2 * nc)); stats = np.zeros(8); iters = C.c_int(0)
    fn = lib.orc_qp_solve_soft
    fn.restype = C.c_int
    st = fn(C.c_int(N), *[arrs[k].ctypes.data_as(dp) for k in ("H", "g", "A", "Bm", "b", "dx0", "R", "dl", "du")],
            sz.ctypes.data_as(dp), sZ.ctypes.data_as(dp), C.c_int(iter_max), C.c_double(tol), C.c_double(mu0), C.c_double(tau0),
            dz.ctypes.data_as(dp), pi.ctypes.data_as(dp), lam.ctypes.data_as(dp), t.ctypes.data_as(dp), sl.ctypes.data_as(dp),
            stats.ctypes.data_as(dp), C.byref(iters))
    return dict(status=st, dz=dz, lam=lam, sl=sl)


@pytest.mark.parametrize("soft", [False, True])
def test_lateral_acceleration_row_against_central_differences(track, soft):
    lay = L.Layout("alat", path=True, alat=True, alat_max=2.5 if soft else 4.5, alat_soft=soft, path_soft=soft, width=1.2 if soft else 1.6)
    ocp = L.make_ocp(lay)
    data = ocp.flatten()
    L.apply(data, lay)
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    assert P.alat_on
    B = 4
    x0 = sample_x0(track, B, seed=777 + soft)
    x, u = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, lay.N)
    yref, yref_e = orc.prepare_step(lay.N, x0, 40.0, x, u)
    A, Bm, b = P.linearize(x, u)
    z, Z = L.soft_arrays(data, 15, (data.alat_soft_z, data.alat_soft_Z) if soft else None)

    def solve(qp, tol):
        return _qp_solve15(qp, tol, 200, data.ipm_mu0, data.ipm_tau0, z, Z)

    errs, active = [], 0
    for i in range(B):
        ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i])
        assert ref["R"].shape[1] == 15
        qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref)
        sol = solve(ref, QP_TOL)
        if sol["status"] != 0 or S.weakly_active(qp, sol["dz"], sol["lam"], sl=sol["sl"], soft_z=z, soft_Z=Z):
            continue
        active += int(np.any(sol["lam"][:, [14, 29]] > 1e-3))
        _, su = S.sensitivities(qp, sol["dz"], sol["lam"], sol["sl"], z, Z)
        errs.append(_rel(su[0], _fd(solve, ref, sol["dz"].shape)))
    assert len(errs) >= 2, errs
    assert max(errs) <= 1e-3 and np.median(errs) <= 1e-5, errs


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()
    for name in ("ihm2mpc_set_x0_sensitivities", "ihm2mpc_get_x0_sensitivities", "ihm2mpc_get_sens_u0_device"):
        assert re.search(r"\bint %s\(" % name, hdr), name
    from ihm2_amd import _lib

    lib = _lib.load()
    for name in ("ihm2mpc_set_x0_sensitivities", "ihm2mpc_get_x0_sensitivities", "ihm2mpc_get_sens_u0_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
