"""Independent numpy reference of the adjoint sensitivities of an RTI QP's solution ("adjoint sensitivities").

The differentiated system is that of sens_ref.py -- the interior point's KKT system at the returned iterate with the primal gaps
t = max(gap, TAU) in place of its own slacks -- assembled here a second time, with the soft slacks eliminated into the stage Hessians
(sens_ref.py keeps every slack as a variable): Ht_k = H_k + sum_i sigma_i r_i r_i' with sigma_i = lam_i / t_i on a hard side and
1 / (t_i / lam_i + 1 / rho_i), rho_i = Z_i + nu_i / max(s_i, TAU), on a soft one.  M = [[Ht, E'], [E, 0]] with E the rows x_0 = . ,
x_{k+1} - A_k x_k - B_k u_k = . ; a seed s = dL/dz goes in as the right-hand side, M [zeta; nu] = [s; 0], and
dL/dx0 = nu_0, dL/dyref_k = Gy_k' zeta_k, dL/dyref_e = Gy_N' zeta_N[:8], where -Gy_k = dg_k / dyref_k.  No code is shared with the kernel."""
from __future__ import annotations

import numpy as np

from sens_ref import NX, NZ, TAU


def kkt_matrix(qp, dz, lam, sl, soft_z, soft_Z, tau=TAU):
    """The matrix M (dense) for an assemble_qp / build_qp dict and the QP's solution; arguments as sens_ref.sensitivities.
    Variables: z_0 .. z_{N-1} (10 each), x_N (8); then the N + 1 multiplier blocks of 8."""
    H, A, Bm, R, dl, du = (np.asarray(qp[k], dtype=np.float64) for k in ("H", "A", "Bm", "R", "dl", "du"))
    N, nc = A.shape[0], R.shape[1]
    nz, ne = N * NZ + NX, NX * (N + 1)
    M = np.zeros((nz + ne, nz + ne))
    for k in range(N + 1):
        m = NZ if k < N else NX
        Ht = H[k][:m, :m].copy()
        for c in range(nc):
            r = R[k, c, :m]
            rz = float(r @ dz[k, :m])
            for up, bound in ((0, dl[k, c]), (1, du[k, c])):
                col = up * nc + c
                lm = float(lam[k, col])
                if not np.isfinite(bound) or not lm > 0.0:
                    continue
                soft = soft_Z[k, col] >= 0.0
                s = float(sl[k, col]) if soft else 0.0
                t = max((rz - bound if up == 0 else bound - rz) + s, tau)
                if soft:
                    rho = soft_Z[k, col] + max(soft_z[k, col] + soft_Z[k, col] * s - lm, 0.0) / max(s, tau)
                    sigma = lm * rho / (t * rho + lm)
                else:
                    sigma = lm / t
                Ht += sigma * np.outer(r, r)
        M[k * NZ:k * NZ + m, k * NZ:k * NZ + m] = Ht
    E = M[nz:, :nz]
    E[:NX, :NX] = np.eye(NX)
    for k in range(N):
        rows = slice(NX * (k + 1), NX * (k + 2))
        E[rows, (k + 1) * NZ:(k + 1) * NZ + NX] = np.eye(NX)
        E[rows, k * NZ:k * NZ + NX] = -A[k]
        E[rows, k * NZ + NX:(k + 1) * NZ] = -Bm[k]
    M[:nz, nz:] = E.T
    return M


def adjoint(qp, dz, lam, sl, soft_z, soft_Z, seed, tau=TAU):
    """seed (N+1,10) = dL/dz_k (the input part of row N is ignored).  Returns zeta (N+1,10) (zeros there) and nu_0 (8) = dL/dx0."""
    N = np.asarray(qp["A"]).shape[0]
    nz = N * NZ + NX
    M = kkt_matrix(qp, dz, lam, sl, soft_z, soft_Z, tau)
    rhs = np.zeros(M.shape[0])
    rhs[:nz] = np.asarray(seed, dtype=np.float64).reshape(-1)[:nz]
    sol = np.linalg.solve(M, rhs)
    zeta = np.zeros((N + 1, NZ))
    zeta.reshape(-1)[:nz] = sol[:nz]
    return zeta, sol[nz:nz + NX]


def gy_tables(build_g, yref, yref_e):
    """Gy (N,10,12) and Gy_e (8,8) with g_k = H_k z_k - Gy_k yref_k, from the QP's own gradient: g is affine in the reference, so column
    l of -Gy_k is g_k(yref + e_l) - g_k(yref), exact to rounding.  build_g(yref, yref_e) -> g (N+1,10)."""
    N = yref.shape[0]
    g0 = build_g(yref, yref_e)
    Gy, Gye = np.zeros((N, NZ, yref.shape[1])), np.zeros((NX, yref_e.shape[0]))
    for l in range(yref.shape[1]):
        d = np.zeros_like(yref)
        d[:, l] = 1.0
        Gy[:, :, l] = -(build_g(yref + d, yref_e) - g0)[:N]
    for l in range(yref_e.shape[0]):
        d = np.zeros_like(yref_e)
        d[l] = 1.0
        Gye[:, l] = -(build_g(yref, yref_e + d) - g0)[N, :NX]
    return Gy, Gye


def gradients(zeta, Gy, Gye):
    """dL/dyref (N,12) and dL/dyref_e (8) from zeta."""
    N = Gy.shape[0]
    return np.einsum("kjl,kj->kl", Gy, zeta[:N]), Gye.T @ zeta[N, :NX]
