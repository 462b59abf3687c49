"""Independent numpy reference of adjoint seeds on the soft slacks ("seeds on the slacks").

A soft side i of row r_i at stage k has the slack s_i, the multiplier lam_i, the penalties z_i, Z_i, sgn_i = +1 (lower) / -1 (upper),
t_i = max(gap_i, TAU), nu_i = max(z_i + Z_i s_i - lam_i, 0), rho_i = Z_i + nu_i / max(s_i, TAU).  With the slack kept as a variable its
row of the differentiated system reads (lam_i / t_i) (s + sgn_i r_i z) + rho_i s = c_i for a seed c_i = dL/ds_i.

(a) fold: the change of the right-hand side that eliminating the slacks leaves,
        seed_z,k += - sum_{soft sides i of stage k, lam_i > 0} c_i gamma_i sgn_i r_i,    gamma_i = lam_i / (t_i rho_i + lam_i);
(b) adjoint_with_slacks: the dense KKT system in which every such slack is a variable of its own, solved for the right-hand side
    [seed_z; seed_s; 0] -- it knows nothing of the elimination.  (The slack's row is kept as the pair m + rho s = c,
    sgn r z + s - (t / lam) m = 0 with m the move of the side's multiplier: lam / t reaches 1e13 and would swallow rho on one diagonal.)
adj_ref.adjoint(seed_z + fold) must equal (b).  No code is shared with the kernel or with the other references."""
from __future__ import annotations

import numpy as np

NX, NZ = 8, 10
TAU = 1e-9          # include/ihm2mpc.h: IHM2MPC_SENS_TAU


def _soft_sides(qp, dz, lam, sl, soft_z, soft_Z, tau, with_cond=False, bound_mag=None):
    """Every soft side with a finite bound and lam > 0, in the order (stage, row, lower before upper):
    (k, column of lam / sl, sgn * r (over z_k), lam / t, rho).  with_cond: a sixth entry, the condition of gamma (see fold)."""
    R, dl, du = (np.asarray(qp[k], dtype=np.float64) for k in ("R", "dl", "du"))
    N, nc = R.shape[0] - 1, R.shape[1]
    out = []
    for k in range(N + 1):
        m = NZ if k < N else NX
        for c in range(nc):
            row = R[k, c, :m]
            move = float(row @ dz[k, :m])
            for col, bound, sgn in ((c, dl[k, c], 1.0), (nc + c, du[k, c], -1.0)):
                if not np.isfinite(bound) or not soft_Z[k, col] >= 0.0 or not lam[k, col] > 0.0:
                    continue
                s = float(sl[k, col])
                t = max(sgn * (move - bound) + s, tau)
                nu = max(soft_z[k, col] + soft_Z[k, col] * s - lam[k, col], 0.0)
                rho = soft_Z[k, col] + nu / max(s, tau)
                side = (k, col, sgn * row, float(lam[k, col]) / t, rho)
                if with_cond:
                    gamma = lam[k, col] / (t * rho + lam[k, col])
                    # the sums of the absolute terms of the two differences gamma is formed from: the gap (where it is not clipped to
                    # tau) and nu (where it is positive)
                    bm = abs(bound) if bound_mag is None else bound_mag[k, col]
                    gap_mag = float(np.abs(row * dz[k, :m]).sum() + bm + abs(s)) if t > tau else 0.0
                    nu_mag = abs(soft_z[k, col]) + abs(soft_Z[k, col] * s) + abs(lam[k, col]) if nu > 0.0 else 0.0
                    side += ((1.0 - gamma) * (gap_mag / t + nu_mag / max(s, tau) / rho if rho > 0.0 else 0.0),)
                out.append(side)
    return out


def fold(qp, dz, lam, sl, soft_z, soft_Z, seed_s, tau=TAU, with_mag=False, bound_mag=None):
    """qp, dz, lam, sl, soft_z, soft_Z as sens_ref.sensitivities takes them; seed_s (N+1, 2 nc) = dL/ds (entries of sides without a
    slack, or with lam = 0, are ignored).  Returns (N+1,10), to be added to seed_z.

    with_mag: also the magnitude that rounding errors of the fold are relative to.  A term c gamma sgn r is a product, but gamma is formed
    from two differences that cancel: the gap t (the row's move, minus the bound less the row's value, plus the slack) and
    nu = z + Z s - lam.  To first order d gamma / gamma = -(1 - gamma) (dt / t + d rho / rho) with d rho = d nu / max(s, tau), and an
    error of dt, d nu of eps times the sum of the absolute terms of the difference.  So the magnitude of a term is
    |c gamma r| (1 + (1 - gamma) (sum |terms of the gap| / t + sum |terms of nu| / max(s, tau) / rho)): |c gamma r| itself where gamma is
    0 or 1 or nothing cancels, larger where an active side's slack is about to come into use.  bound_mag (N+1, 2 nc): the sum of the
    absolute terms of (bound - the row's value at the point of linearisation) where the code under test forms that difference itself;
    None: |qp["dl"]|, |qp["du"]| as one term each."""
    N = np.asarray(qp["A"]).shape[0]
    out, mag = np.zeros((N + 1, NZ)), np.zeros((N + 1, NZ))
    for k, col, v, g, rho, *cond in _soft_sides(qp, dz, lam, sl, soft_z, soft_Z, tau, with_cond=with_mag, bound_mag=bound_mag):
        gamma = g / (g + rho)           # = lam / (t rho + lam)
        term = seed_s[k, col] * gamma * v
        out[k, :v.size] -= term
        if with_mag:
            mag[k, :v.size] += np.abs(term) * (1.0 + cond[0])
    return (out, mag) if with_mag else out


def cost_slack_seed(sl, soft_z, soft_Z):
    """dJ_slack/ds_i = z_i + Z_i s_i on the soft sides (N+1, 2 nc), zero on the hard ones."""
    soft = np.asarray(soft_Z) >= 0.0
    return np.where(soft, soft_z + np.where(soft, soft_Z, 0.0) * sl, 0.0)


def adjoint_with_slacks(qp, dz, lam, sl, soft_z, soft_Z, seed_z, seed_s, tau=TAU, solve=np.linalg.solve):
    """The dense system with the variables (z_0 .. z_{N-1}, x_N, the soft slacks and the moves of their sides' multipliers, the multipliers
    of the dynamics).  Returns zeta_z (N+1,10) (zeros on the input part of row N) and nu_0 (8) = dL/dx0.  ``solve``: a replacement of
    np.linalg.solve."""
    H, A, Bm, R, dl, du = (np.asarray(qp[k], dtype=np.float64) for k in ("H", "A", "Bm", "R", "dl", "du"))
    N, nc = A.shape[0], R.shape[1]
    nz, ne = N * NZ + NX, NX * (N + 1)
    soft = _soft_sides(qp, dz, lam, sl, soft_z, soft_Z, tau)
    taken = {(k, col) for k, col, _, _, _ in soft}
    n = nz + 2 * len(soft)
    K = np.zeros((n + ne, n + ne))
    rhs = np.zeros(n + ne)
    rhs[:nz] = np.asarray(seed_z, dtype=np.float64).reshape(-1)[:nz]
    for k in range(N + 1):
        m = NZ if k < N else NX
        o = k * NZ
        K[o:o + m, o:o + m] = H[k][:m, :m]
        move = R[k, :, :m] @ dz[k, :m]
        for c in range(nc):             # the hard sides: lam / t on the row itself
            for col, bound, sgn in ((c, dl[k, c], 1.0), (nc + c, du[k, c], -1.0)):
                if np.isfinite(bound) and lam[k, col] > 0.0 and (k, col) not in taken:
                    assert not soft_Z[k, col] >= 0.0
                    t = max(sgn * (move[c] - bound), tau)
                    K[o:o + m, o:o + m] += lam[k, col] / t * np.outer(R[k, c, :m], R[k, c, :m])
    # a soft side: its slack s and the move m = (lam / t) (s + sgn r z) of its multiplier are both variables, so that lam / t (up to 1e13 on
    # an active side) is never added to rho:   H z + sgn r m = seed_z,   m + rho s = c,   sgn r z + s - (t / lam) m = 0
    for q, (k, col, v, g, rho) in enumerate(soft):
        o, m, p, r = k * NZ, v.size, nz + 2 * q, nz + 2 * q + 1
        K[o:o + m, r] = v
        K[r, o:o + m] = v
        K[p, p] = rho
        K[p, r] = K[r, p] = 1.0
        K[r, r] = -1.0 / g
        rhs[p] = seed_s[k, col]
    E = np.zeros((ne, n))
    E[:NX, :NX] = np.eye(NX)
    for k in range(N):
        rows = slice(NX * (k + 1), NX * (k + 2))
        E[rows, (k + 1) * NZ:(k + 1) * NZ + NX] = np.eye(NX)
        E[rows, k * NZ:k * NZ + NX] = -A[k]
        E[rows, k * NZ + NX:(k + 1) * NZ] = -Bm[k]
    K[n:, :n] = E
    K[:n, n:] = E.T
    sol = solve(K, rhs)
    zeta = np.zeros((N + 1, NZ))
    zeta.reshape(-1)[:nz] = sol[:nz]
    return zeta, sol[n:n + NX]
