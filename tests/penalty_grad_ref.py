"""Independent numpy reference of the adjoint gradients in the slack penalties z_i, Z_i ("gradients in the soft penalties").

Notation of tests/slack_seed_ref.py.  With the slack of a soft side kept as a variable, [zeta_z; zeta_s; nu] = M^-1 [seed_z; seed_s; 0] and
a change of the penalties moves the slack's row by dz_i + s_i dZ_i, so dL/dz_i = -zeta_s,i and dL/dZ_i = -s_i zeta_s,i.

(a) zeta_s: read out of the dense system of slack_seed_ref.adjoint_with_slacks through its ``solve=`` hook -- the slack of the q-th entry
    of slack_seed_ref._soft_sides is the unknown N * 10 + 8 + 2 q.  It knows nothing of the closed form.
(b) closed_form: zeta_s,i = (c_i t_i - lam_i sgn_i r_i zeta_k) / (t_i rho_i + lam_i) from a given zeta_z (the kernel's formula, restated).
No code is shared with the kernel."""
from __future__ import annotations

import numpy as np

import slack_seed_ref as SR

NX, NZ = 8, 10


def zeta_s(qp, dz, lam, sl, z, Z, seed_z, seed_s, solve=np.linalg.solve):
    """(zeta_s (N+1, 2 nc), zeta_z (N+1,10), nu_0 (8)) of the dense system that keeps every soft slack; zeta_s is 0 on sides that carry
    no slack there (hard, no finite bound, lam = 0)."""
    kept = {}

    def hook(K, rhs):
        kept["sol"] = solve(K, rhs)
        return kept["sol"]

    zeta, nu0 = SR.adjoint_with_slacks(qp, dz, lam, sl, z, Z, seed_z, seed_s, solve=hook)
    N = np.asarray(qp["A"]).shape[0]
    nz = N * NZ + NX
    out = np.zeros_like(np.asarray(lam, dtype=np.float64))
    for q, (k, col, _, _, _) in enumerate(SR._soft_sides(qp, dz, lam, sl, z, Z, SR.TAU)):
        out[k, col] = kept["sol"][nz + 2 * q]
    return out, zeta, nu0


def closed_form(qp, dz, lam, sl, z, Z, zeta, seed_s, tau=SR.TAU):
    """(zeta_s (N+1, 2 nc), mag (N+1, 2 nc)) from zeta_z by the closed form; mag = gamma_i (|r_i zeta_k| + |c_i t_i / lam_i|) =
    (|lam_i r_i zeta_k| + |c_i t_i|) / (t_i rho_i + lam_i), the sum of the absolute terms of the quotient, which its rounding errors and
    those of zeta are relative to (both 0 on sides without a slack).  gamma_i <= 1: never larger than |r_i zeta_k| + |c_i t_i / lam_i|,
    which an inactive side (lam_i of the order of the barrier parameter) drives to 1e10 and more."""
    out = np.zeros_like(np.asarray(lam, dtype=np.float64))
    mag = np.zeros_like(out)
    for k, col, v, g, rho in SR._soft_sides(qp, dz, lam, sl, z, Z, tau):
        lm = float(lam[k, col])
        t = lm / g
        rz = float(v @ zeta[k, :v.size])            # sgn_i r_i zeta_k
        c = float(seed_s[k, col])
        out[k, col] = (c * t - lm * rz) / (t * rho + lm)
        mag[k, col] = (abs(lm * rz) + abs(c * t)) / (t * rho + lm)
    return out, mag


def gradients(zs, sl):
    """(dL/dz, dL/dZ) (N+1, 2 nc) from zeta_s and the slack values."""
    return -zs, -np.asarray(sl) * zs


def cost_partials(sl, soft_Z):
    """The explicit partials of J_slack = sum z_i s_i + Z_i s_i^2 / 2 in (z, Z) on the soft sides (N+1, 2 nc), zero on the hard ones."""
    soft = np.asarray(soft_Z) >= 0.0
    s = np.where(soft, sl, 0.0)
    return s, 0.5 * s * s


def split(a, nc):
    """((N+1,28), (N+1,2)) of the C ABI from (N+1, 2 nc); nc = 14: the second part is zeros."""
    a = np.asarray(a)
    if nc == 14:
        return a, np.zeros((a.shape[0], 2))
    return np.concatenate([a[:, :14], a[:, nc:nc + 14]], 1), np.stack([a[:, 14], a[:, nc + 14]], 1)
