"""Independent numpy reference of the OCP's objective at an iterate, of its seeds dJ/dz and of its explicit partials in yref, yref_e,
W and W_e ("cost and its gradient").

    J = sum_{k<N} (c_s/2) e_k' W_k e_k + 1/2 e_N' W_e e_N + J_slack,     e_k = V z_k - yref_k,  e_N = x_N - yref_e,
    J_slack = sum over the soft sides (finite bound, Z >= 0) of z_i s_i + 1/2 Z_i s_i^2,
V = layouts.selectors().  With t_k = W_k e_k:  dJ/dz_k = c_s V' t_k,  dJ/dx_N = W_e e_N,  and at fixed z
    dJ/dyref_k = -c_s t_k,   dJ/dyref_e = -W_e e_N,   dJ/dW = (c_s/2) sum_k e_k e_k',   dJ/dW_e = 1/2 e_N e_N'.
The total derivative through the RTI QP's solution map adds adj_ref.gradients / adjw_ref.weight_gradients of adj_ref.adjoint's zeta for
the seed dJ/dz (total_gradient).  Every quantity comes with its cancellation-free magnitude, the sum of the absolute values of its terms,
which is what rounding errors are relative to.  No code is shared with the kernel."""
from __future__ import annotations

import numpy as np

import layouts as L

NC = L.NC


def finite_sides(data):
    """(N+1, 28) bool: the sides of the rows 0..13 that carry a finite bound (14 lower, then 14 upper)."""
    N = data.N
    fin = np.zeros((N + 1, 2 * NC), dtype=bool)
    fin[1:, 0:8] = np.abs(np.asarray(data.lbx)[1:]) < L.BIG
    fin[1:, NC:NC + 8] = np.abs(np.asarray(data.ubx)[1:]) < L.BIG
    fin[:N, 8:10] = np.abs(np.asarray(data.lbu)) < L.BIG
    fin[:N, NC + 8:NC + 10] = np.abs(np.asarray(data.ubu)) < L.BIG
    fin[:N, 10:12] = np.abs(np.asarray(data.lg)) < L.BIG
    fin[:N, NC + 10:NC + 12] = np.abs(np.asarray(data.ug)) < L.BIG
    if data.path_on:
        fin[1:, 12:14] = np.abs(np.asarray(data.lh)[:2]) < L.BIG
        fin[1:, NC + 12:NC + 14] = np.abs(np.asarray(data.uh)[:2]) < L.BIG
    return fin


def errors(data, x, u, yref, yref_e, W=None, W_e=None):
    """e (N,12), e_N (8), W (N,12,12), W_e (8,8) as float64; W / W_e default to the data's, a (12,12) W stands for every stage."""
    V = L.selectors()
    N = data.N
    z = np.concatenate([np.asarray(x, dtype=np.float64)[:N], np.asarray(u, dtype=np.float64)], axis=1)
    W = np.asarray(data.W if W is None else W, dtype=np.float64)
    if W.ndim == 2:
        W = np.broadcast_to(W, (N, 12, 12))
    W_e = np.asarray(data.W_e if W_e is None else W_e, dtype=np.float64)
    return z @ V.T - yref, np.asarray(x, dtype=np.float64)[N] - yref_e, W, W_e


def slack_terms(data, slk, slk_a=None):
    """(N+1,) slack cost of every stage and its magnitude: slk (N+1,28) of get_slacks, slk_a (N+1,2) of the lateral-acceleration row."""
    N = data.N
    out, mag = np.zeros(N + 1), np.zeros(N + 1)
    if data.soft_Z is not None:
        z, Z = np.asarray(data.soft_z, dtype=np.float64), np.asarray(data.soft_Z, dtype=np.float64)
        on = finite_sides(data) & (Z >= 0.0)
        s = np.where(on, slk, 0.0)
        out += (np.where(on, z, 0.0) * s + 0.5 * np.where(on, Z, 0.0) * s * s).sum(1)
        mag += (np.abs(np.where(on, z, 0.0) * s) + np.abs(0.5 * np.where(on, Z, 0.0) * s * s)).sum(1)
    if data.alat_on and data.alat_soft_Z is not None and slk_a is not None:
        az, aZ = np.asarray(data.alat_soft_z, dtype=np.float64), np.asarray(data.alat_soft_Z, dtype=np.float64)
        for m, bound in enumerate((data.alat_lb, data.alat_ub)):
            if np.isfinite(bound) and abs(bound) < L.BIG and aZ[m] >= 0.0:
                s = slk_a[1:N, m]
                out[1:N] += az[m] * s + 0.5 * aZ[m] * s * s
                mag[1:N] += np.abs(az[m] * s) + np.abs(0.5 * aZ[m] * s * s)
    return out, mag


def cost(data, x, u, yref, yref_e, W=None, W_e=None, slk=None, slk_a=None):
    """One instance.  Returns dict(cost, stage_cost (N+1), slack_cost) and, under "mag", the same keys' magnitudes."""
    e, eN, W, W_e = errors(data, x, u, yref, yref_e, W, W_e)
    cs = data.cost_scale_stage
    N = data.N
    stage, mag = np.zeros(N + 1), np.zeros(N + 1)
    stage[:N] = 0.5 * cs * np.einsum("ki,kij,kj->k", e, W, e)
    mag[:N] = 0.5 * cs * np.einsum("ki,kij,kj->k", np.abs(e), np.abs(W), np.abs(e))
    stage[N] = 0.5 * eN @ W_e @ eN
    mag[N] = 0.5 * np.abs(eN) @ np.abs(W_e) @ np.abs(eN)
    sl, slm = slack_terms(data, slk, slk_a) if slk is not None else (np.zeros(N + 1), np.zeros(N + 1))
    stage, mag = stage + sl, mag + slm
    return dict(cost=stage.sum(), stage_cost=stage, slack_cost=sl.sum(), mag=dict(cost=mag.sum(), stage_cost=mag, slack_cost=slm.sum()))


def cost_longdouble(data, x, u, yref, yref_e, W=None, W_e=None, slk=None, slk_a=None):
    """J once more, term by term in np.longdouble with plain loops (no selector matrix, no einsum): an evaluation independent of cost()."""
    ld = np.longdouble
    N, cs = data.N, ld(data.cost_scale_stage)
    W = np.asarray(data.W if W is None else W)
    W_e = np.asarray(data.W_e if W_e is None else W_e)
    J = ld(0)
    for k in range(N):
        Wk = W if W.ndim == 2 else W[k]
        y = [ld(v) for v in x[k]] + [ld(u[k][0]), ld(u[k][1]), ld(x[k][6]) - ld(u[k][0]), ld(x[k][7]) - ld(u[k][1])]
        e = [y[i] - ld(yref[k][i]) for i in range(12)]
        q = ld(0)
        for i in range(12):
            for j in range(12):
                q += e[i] * ld(Wk[i][j]) * e[j]
        J += cs * q / ld(2)
    e = [ld(x[N][i]) - ld(yref_e[i]) for i in range(8)]
    q = ld(0)
    for i in range(8):
        for j in range(8):
            q += e[i] * ld(W_e[i][j]) * e[j]
    J += q / ld(2)
    if slk is not None and data.soft_Z is not None:
        fin = finite_sides(data)
        for k in range(N + 1):
            for c in range(2 * NC):
                if fin[k, c] and data.soft_Z[k][c] >= 0.0:
                    s = ld(slk[k][c])
                    J += ld(data.soft_z[k][c]) * s + ld(data.soft_Z[k][c]) * s * s / ld(2)
    if slk_a is not None and data.alat_on and data.alat_soft_Z is not None:
        for m, bound in enumerate((data.alat_lb, data.alat_ub)):
            if np.isfinite(bound) and abs(bound) < L.BIG and data.alat_soft_Z[m] >= 0.0:
                for k in range(1, N):
                    s = ld(slk_a[k][m])
                    J += ld(data.alat_soft_z[m]) * s + ld(data.alat_soft_Z[m]) * s * s / ld(2)
    return J


def seeds(data, x, u, yref, yref_e, W=None, W_e=None):
    """The seed dJ/dz as (N+1,10) (the input part of row N is zero) and its magnitude."""
    V = L.selectors()
    e, eN, W, W_e = errors(data, x, u, yref, yref_e, W, W_e)
    cs, N = data.cost_scale_stage, data.N
    sd, mag = np.zeros((N + 1, 10)), np.zeros((N + 1, 10))
    t = np.einsum("kij,kj->ki", W, e)
    tm = np.einsum("kij,kj->ki", np.abs(W), np.abs(e))
    sd[:N] = cs * t @ V
    mag[:N] = cs * tm @ np.abs(V)
    sd[N, :8] = W_e @ eN
    mag[N, :8] = np.abs(W_e) @ np.abs(eN)
    return sd, mag


def explicit_partials(data, x, u, yref, yref_e, W=None, W_e=None):
    """dict(yref (N,12), yref_e (8), W (12,12), W_e (8,8)): the derivatives of J at fixed (x, u), and under "mag" their magnitudes."""
    e, eN, W, W_e = errors(data, x, u, yref, yref_e, W, W_e)
    cs = data.cost_scale_stage
    out = dict(yref=-cs * np.einsum("kij,kj->ki", W, e), yref_e=-(W_e @ eN),
               W=0.5 * cs * np.einsum("ki,kj->ij", e, e), W_e=0.5 * np.outer(eN, eN))
    out["mag"] = dict(yref=cs * np.einsum("kij,kj->ki", np.abs(W), np.abs(e)), yref_e=np.abs(W_e) @ np.abs(eN),
                      W=0.5 * cs * np.einsum("ki,kj->ij", np.abs(e), np.abs(e)), W_e=0.5 * np.outer(np.abs(eN), np.abs(eN)))
    return out


def total_gradient(data, qp, dz, lam, sl, soft_z, soft_Z, Gy, Gye, xplus, uplus, yref, yref_e, W=None, W_e=None, adjoint=None):
    """dict(x0, yref, yref_e, W, W_e): the total derivative of J at the returned solution (xplus, uplus) of the RTI QP `qp` (an
    assemble_qp / build_qp dict with its solution dz, lam, sl; Gy, Gye of adj_ref.gy_tables): adj_ref / adjw_ref on the seed dJ/dz plus
    the explicit partials.  ``adjoint``: a replacement of adj_ref.adjoint with its signature (a more accurate solve).  Under "adj" the
    adjoint parts alone."""
    import adj_ref as R
    import adjw_ref as RW

    N = data.N
    sd, _ = seeds(data, xplus, uplus, yref, yref_e, W, W_e)
    zeta, nu0 = (adjoint or R.adjoint)(qp, dz, lam, sl, soft_z, soft_Z, sd)
    gy, gye = R.gradients(zeta, Gy, Gye)
    zp = np.zeros((N + 1, 10)); zp[:, :8] = xplus; zp[:N, 8:] = uplus
    dw = data
    if W is not None or W_e is not None:
        import copy

        dw = copy.copy(data)        # adjw_ref reads c_s only
    gW, gWe = RW.weight_gradients(dw, zeta, zp, yref, yref_e)
    ex = explicit_partials(data, xplus, uplus, yref, yref_e, W, W_e)
    return dict(x0=nu0, yref=gy + ex["yref"], yref_e=gye + ex["yref_e"], W=gW + ex["W"], W_e=gWe + ex["W_e"],
                adj=dict(x0=nu0, yref=gy, yref_e=gye, W=gW, W_e=gWe), explicit=ex)
