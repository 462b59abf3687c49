"""NumPy restatement of the integrator IHM2MPC_INTEG_ERK_LAG (include/ihm2mpc.h) and of its sensitivities: classical RK4 on the six
vehicle states of fkin6, the two actuator lags in closed form, their stage values fitted to the first three moments of the transient.

The model and its Jacobian are the oracle's (``orc.f`` / ``orc.jac``); the stage factors are evaluated here in ``np.longdouble``,
independently of ``ihm2mpc_lag_stage_factors``.  ``pointwise=True`` gives the crude variant that samples the closed form at the stage
times (the recovery rollout's ``exact_lags``), which the fitted factors are measured against.
"""
import numpy as np

from oracle import oracle as orc

TAU = (1e-3, 0.02)          # t_T, t_delta (python/constants.py; model.hpp: k_tT, k_tdelta)
# rows of S = d x+ / d (x, u) that can be non-zero per column (model.hpp: S_COL_MASK[0])
S_COL_MASK = (0x07, 0x07, 0x07, 0x3F, 0x3F, 0x27, 0x7F, 0xBF, 0x7F, 0xBF)
_STAGE_C = (0.0, 0.5, 0.5, 1.0)
_STAGE_W = (1.0, 2.0, 2.0, 1.0)
_STAGE_S = (0, 1, 1, 2)


def structural_mask():
    """(8, 10) bool: True where the record [A | B] may be non-zero."""
    return np.array([[(S_COL_MASK[c] >> i) & 1 for c in range(10)] for i in range(8)], dtype=bool)


def stage_factors_ld(h, tau):
    """(E_0, E_1, E_2, e) in np.longdouble: Simpson's rule with these stage values integrates t^j exp(-t / tau), j = 0, 1, 2, over
    [0, h] exactly.  p1 = m1 / h^2, p2 = m2 / h^3; below r = 2 their series (the closed forms cancel like r^2 / 2 and r^3 / 6)."""
    L = np.longdouble
    h, tau = L(h), L(tau)
    r = h / tau
    e = np.exp(-r)
    if r < 2:
        p1 = L(0); p2 = L(0)
        t = L(1) / 2          # r^(k-2) / k!
        for k in range(2, 80):
            p1 += (-1) ** k * (k - 1) * t
            if k >= 3:
                p2 += (-1) ** (k + 1) * (k - 1) * (k - 2) * t / r
            t = t * r / (k + 1)
    else:
        p1 = (1 - e * (1 + r)) / (r * r)
        p2 = 2 * (1 - e * (1 + r + r * r / 2)) / (r * r * r)
    E1 = 6 * (p1 - p2)
    E2 = 12 * p2 - 6 * p1
    E0 = 6 * (-np.expm1(-r)) / r - 4 * E1 - E2
    return np.array([E0, E1, E2, e], dtype=L)


def stage_factors(h, tau, pointwise=False):
    if pointwise:
        return np.array([1.0, np.exp(-0.5 * h / tau), np.exp(-h / tau), np.exp(-h / tau)])
    return stage_factors_ld(h, tau).astype(np.float64)


def lag_step(x, u, s_ref, kappa_ref, dt, M, sens=False, pointwise=False):
    """x+ over dt by M sub-steps (and with ``sens`` the 8 x 10 derivative [A | B] of that map)."""
    x = np.array(x, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    h = dt / M
    F = np.stack([stage_factors(h, tau, pointwise) for tau in TAU])          # (2, 4)
    S = np.hstack([np.eye(8), np.zeros((8, 2))])
    for _ in range(M):
        v, a = x[:6].copy(), x[6:].copy()
        K = np.zeros(8); dK = np.zeros((8, 10))
        vacc = v.copy(); Sacc = S[:6].copy()
        for c, w, s in zip(_STAGE_C, _STAGE_W, _STAGE_S):
            E = F[:, s]
            X = np.concatenate([v + c * h * K[:6], u + (a - u) * E])
            if sens:
                K, J = orc.jac(orc.MODEL_FKIN6, X, u, s_ref, kappa_ref)
                dX = np.zeros((8, 10))
                dX[:6] = S[:6] + c * h * dK[:6]
                dX[6:] = E[:, None] * S[6:]
                dX[6, 8] += 1.0 - E[0]
                dX[7, 9] += 1.0 - E[1]
                dK = J[:, :8] @ dX
                dK[:, 8:] += J[:, 8:]
                Sacc += w * h / 6.0 * dK[:6]
            else:
                K = orc.f(orc.MODEL_FKIN6, X, u, s_ref, kappa_ref)
            vacc += w * h / 6.0 * K[:6]
        e = F[:, 3]
        x = np.concatenate([vacc, u + (a - u) * e])
        if sens:
            Sa = e[:, None] * S[6:]
            Sa[0, 8] += 1.0 - e[0]
            Sa[1, 9] += 1.0 - e[1]
            S = np.vstack([Sacc, Sa])
    return (x, S[:, :8], S[:, 8:]) if sens else x


def linearize(x, u, s_ref, kappa_ref, dt, M, track_id=None):
    """Records of a batch: x (B, N+1, 8), u (B, N, 2), tables (ntracks, nknots) or (nknots) -> A (B,N,8,8), Bm (B,N,8,2), b (B,N,8)."""
    B, N = u.shape[:2]
    s_ref = np.atleast_2d(s_ref); kappa_ref = np.atleast_2d(kappa_ref)
    tid = np.zeros(B, dtype=int) if track_id is None else np.asarray(track_id)
    A = np.zeros((B, N, 8, 8)); Bm = np.zeros((B, N, 8, 2)); b = np.zeros((B, N, 8))
    for i in range(B):
        for k in range(N):
            xn, A[i, k], Bm[i, k] = lag_step(x[i, k], u[i, k], s_ref[tid[i]], kappa_ref[tid[i]], dt, M, sens=True)
            b[i, k] = xn - x[i, k + 1]
    return A, Bm, b


def sim_step(x, u, s_ref, kappa_ref, dt, M, track_id=None):
    """Plant step of a batch: x (B, 8), u (B, 2)."""
    s_ref = np.atleast_2d(s_ref); kappa_ref = np.atleast_2d(kappa_ref)
    tid = np.zeros(len(x), dtype=int) if track_id is None else np.asarray(track_id)
    return np.stack([lag_step(x[i], u[i], s_ref[tid[i]], kappa_ref[tid[i]], dt, M) for i in range(len(x))])
