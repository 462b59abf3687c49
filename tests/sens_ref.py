"""Independent numpy reference of the x0 sensitivities of an RTI QP's solution ("x0 sensitivities").

The QP (layouts.assemble_qp) returned dz with multipliers lam and soft slacks sl.  Its interior-point KKT system linearised at that
iterate, with the primal gaps t = max(gap, TAU) in place of the interior point's own slacks, is solved here as ONE dense KKT system in
which every soft slack is a variable of its own (the kernel eliminates them in series and runs a Riccati recursion):

    min  1/2 sum_k z_k' H_k z_k + sum_i lam_i / t_i (s_i + sgn_i r_i z_k)^2 / 2 + sum_soft (Z_i + nu_i / max(s_i, TAU)) s_i^2 / 2
    s.t. x_0 = e_j,  x_{k+1} = A_k x_k + B_k u_k

with s_i only on soft sides, sgn_i = +1 on a lower and -1 on an upper side, nu_i = max(z_i + Z_i s_i - lam_i, 0) the slack's own
multiplier (from the slack's stationarity).  No code is shared with the kernel or the oracle."""
from __future__ import annotations

import numpy as np

NX, NU, NZ = 8, 2, 10
TAU = 1e-9          # include/ihm2mpc.h: IHM2MPC_SENS_TAU


def _hdr_tau():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define\s+IHM2MPC_SENS_TAU\s+([0-9.eE+-]+)", open(os.path.join(root, "include", "ihm2mpc.h")).read())
    return float(m.group(1))


def sensitivities(qp, dz, lam, sl, soft_z, soft_Z, tau=TAU):
    """qp: an assemble_qp / build_qp dict (H, A, Bm, R (N+1,nc,10), dl, du); dz (N+1,10) the QP's solution, lam and sl (N+1, 2 nc)
    (nc lower sides, then nc upper sides), soft_z / soft_Z (N+1, 2 nc) with soft_Z < 0 on a hard side.
    Returns sens_x (N+1,8,8) = d x_k / d x0 and sens_u (N,2,8) = d u_k / d x0."""
    H, A, Bm, R, dl, du = (np.asarray(qp[k], dtype=np.float64) for k in ("H", "A", "Bm", "R", "dl", "du"))
    N = A.shape[0]
    nc = R.shape[1]
    nzv = N * NZ + NX

    def zi(k):          # indices of z_k in the variable vector (x_N alone at k = N)
        return np.arange(k * NZ, k * NZ + (NZ if k < N else NX))

    sides = []          # (k, vector over z_k, weight lam / t, soft slack weight or None)
    for k in range(N + 1):
        m = NZ if k < N else NX
        for c in range(nc):
            r = R[k, c, :m]
            for up, bound in ((0, dl[k, c]), (1, du[k, c])):
                if not np.isfinite(bound):
                    continue
                col = up * nc + c
                lm = float(lam[k, col])
                if not lm > 0.0:
                    continue
                soft = soft_Z[k, col] >= 0.0
                s = float(sl[k, col]) if soft else 0.0
                rz = float(r @ dz[k, :m])
                gap = (rz - bound if up == 0 else bound - rz) + s
                t = max(gap, tau)
                sgn = 1.0 if up == 0 else -1.0
                ws = None
                if soft:
                    nu = max(soft_z[k, col] + soft_Z[k, col] * s - lm, 0.0)
                    ws = soft_Z[k, col] + nu / max(s, tau)
                sides.append((k, sgn * r, lm / t, ws))
    nsoft = sum(1 for sd in sides if sd[3] is not None)
    n = nzv + nsoft
    Hd = np.zeros((n, n))
    for k in range(N + 1):
        idx = zi(k)
        Hd[np.ix_(idx, idx)] += H[k][:len(idx), :len(idx)]
    q = nzv
    for k, v, g, ws in sides:
        idx = zi(k)
        if ws is None:
            Hd[np.ix_(idx, idx)] += g * np.outer(v, v)
        else:
            vv = np.concatenate([v, [1.0]])
            ii = np.concatenate([idx, [q]])
            Hd[np.ix_(ii, ii)] += g * np.outer(vv, vv)
            Hd[q, q] += ws
            q += 1
    ne = NX * (N + 1)
    E = np.zeros((ne, n))
    E[:NX, :NX] = np.eye(NX)
    for k in range(N):
        rows = slice(NX * (k + 1), NX * (k + 2))
        E[rows, zi(k + 1)[:NX]] = np.eye(NX)
        E[rows, zi(k)[:NX]] = -A[k]
        E[rows, zi(k)[NX:NZ]] = -Bm[k]
    K = np.block([[Hd, E.T], [E, np.zeros((ne, ne))]])
    rhs = np.zeros((n + ne, NX))
    rhs[n:n + NX] = np.eye(NX)
    sol = np.linalg.solve(K, rhs)[:nzv]
    sens_x = np.stack([sol[zi(k)[:NX]] for k in range(N + 1)])
    sens_u = np.stack([sol[zi(k)[NX:NZ]] for k in range(N)])
    return sens_x, sens_u


def lqr_gain0(H, A, Bm):
    """K0 of u_0 = -K0 x_0 for the unconstrained LQ problem with stage costs 1/2 [x;u]' H_k [x;u], written as the textbook recursion
    (Q = H_xx, R = H_uu, S = H_ux; P_N = Q_N; K = (R + B'PB)^-1 (S + B'PA); P = Q + A'PA - (S + B'PA)' K)."""
    N = A.shape[0]
    P = H[N][:NX, :NX]
    K = None
    for k in range(N - 1, -1, -1):
        Q, Rr, S = H[k][:NX, :NX], H[k][NX:, NX:], H[k][NX:, :NX]
        G = S + Bm[k].T @ P @ A[k]
        K = np.linalg.solve(Rr + Bm[k].T @ P @ Bm[k], G)
        P = Q + A[k].T @ P @ A[k] - G.T @ K
        P = 0.5 * (P + P.T)
    return K


def weakly_active(qp, dz, lam, thresh=1e-4, sl=None, soft_z=None, soft_Z=None):
    """True if a present side has both its multiplier and its gap below `thresh` (the QP's solution is not differentiable there) --
    or, given the slacks and penalties, a soft side's slack bound s >= 0 has both s and its multiplier z + Z s - lam below it."""
    R, dl, du = np.asarray(qp["R"]), np.asarray(qp["dl"]), np.asarray(qp["du"])
    N = R.shape[0] - 1
    nc = R.shape[1]
    dzp = dz.copy()
    dzp[N, NX:] = 0.0
    rz = np.einsum("kcj,kj->kc", R, dzp)
    gap = np.concatenate([rz - dl, du - rz], 1)
    present = np.isfinite(gap)
    weak = bool(np.any(present & (np.abs(lam[:, :2 * nc]) < thresh) & (np.abs(np.where(present, gap, 0.0)) < thresh)))
    if sl is not None and soft_Z is not None:
        soft = present & (soft_Z >= 0.0)
        nu = soft_z + soft_Z * sl - lam[:, :2 * nc]
        weak = weak or bool(np.any(soft & (np.abs(sl) < thresh) & (np.abs(nu) < thresh)))
    return weak
