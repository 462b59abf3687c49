"""The whole-solve check of the gradients in the slack penalties, shared by tests/test_oracle_penalty_grad.py (CPU: the NumPy reference
against central differences of whole oracle QP solves) and tests/test_gpu_penalty_grad.py (GPU): the cases, the seeds of the function
L = <seed, z+>, the direction in (z, Z), the step, the measure and the condition.  Nothing here reads a result.

The measure is max_m |pred_m - fd_m| / max(max_m |fd_m|, max_m free_m) over the two seeds m of an instance.  free_m = sum over the soft
sides with a finite bound of |r_i zeta_free_k| (|dz_i| + s_i |dZ_i|), with zeta_free the adjoint solution with every multiplier zero: the
unconstrained reaction to the same change of force on the row (the analogue of pred_free in tests/test_gpu_adjoint_weights.py).  The
error is not taken against |fd| alone: instances whose slacks barely matter have fd at the noise floor of the differences."""
from __future__ import annotations

import numpy as np

import adj_ref as R
import cost_cases as C

CASES = ("soft_2_per_lane", "path_soft_both_sides")     # of slack_seed_cases.CASES: B = 40, N = 40
EPS = 1e-4                                              # of the central differences
N_SEEDS = 2
SEED_SCALE = np.concatenate([C.X_SCALE, [10.0, 0.02]])
DIRECTIONS = ("z", "Z", "both")
ASSERTED = ("z", "both")            # "Z" is printed only: the reference itself has 0.75 / 0.875 on soft_2_per_lane there
KEEP_MIN = 0.75


def seeds(i, N):
    """(2, N+1, 10): the seeds dL/dz of instance i, zero on the input part of row N."""
    s = np.random.default_rng(100 + i).standard_normal((N_SEEDS, N + 1, 10)) / SEED_SCALE
    s[:, N, 8:] = 0.0
    return s


def direction(z, Z):
    """(dz, dZ) of the shape of z, Z ((N+1, 2 nc)), common to the batch: z * N(0,1), Z * N(0,1), zero on the hard sides."""
    rng = np.random.default_rng(7)
    soft = np.asarray(Z) >= 0.0
    dz = np.where(soft, z * rng.standard_normal(np.shape(z)), 0.0)
    dZ = np.where(soft, Z * rng.standard_normal(np.shape(Z)), 0.0)
    return dz, dZ


def pick(name, dz, dZ):
    return {"z": (dz, 0.0 * dZ), "Z": (0.0 * dz, dZ), "both": (dz, dZ)}[name]


def predict(grad_z, grad_Z, dz, dZ):
    """<gradient, direction> per seed: grad_* (S, N+1, C) against (N+1, C)."""
    return np.einsum("skc,kc->s", grad_z, dz) + np.einsum("skc,kc->s", grad_Z, dZ)


def free_scale(qp, step, lam, sl, z, Z, seed, dz, dZ):
    """free_m of the N_SEEDS seeds (S, N+1, 10) of one instance: step = the QP's solution dz, sl its slacks."""
    Rm, dl, du = (np.asarray(qp[k], dtype=np.float64) for k in ("R", "dl", "du"))
    nc = Rm.shape[1]
    present = np.concatenate([np.isfinite(dl), np.isfinite(du)], 1) & (np.asarray(Z) >= 0.0)
    w = np.where(present, np.abs(dz) + np.abs(sl) * np.abs(dZ), 0.0)
    out = np.zeros(len(seed))
    for m, sd in enumerate(seed):
        zeta, _ = R.adjoint(qp, step, 0.0 * lam, sl, z, Z, sd)
        zeta[-1, 8:] = 0.0
        rz = np.abs(np.einsum("kcj,kj->kc", Rm, zeta))
        out[m] = float((np.concatenate([rz, rz], 1)[:, :2 * nc] * w).sum())
    return out


def measure(pred, fd, free):
    """(B,) from (B, N_SEEDS) each."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(pred - fd).max(1) / np.maximum(np.abs(fd).max(1), free.max(1))


def verdict(tag, name, errs, zero_errs, keep, B):
    """Prints every direction's profile, asserts the condition on the asserted ones and that the zero prediction fails it there."""
    assert keep.size >= KEEP_MIN * B, (keep.size, B)
    for d in DIRECTIONS:
        (med, s5, s3), met = C.profile(errs[d][keep])
        (med0, s50, s30), met0 = C.profile(zero_errs[d][keep])
        print(f"{tag} {name} {d}: kept {keep.size} of {B}, median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max "
              f"{errs[d][keep].max():.2e}; zero prediction median {med0:.2e} share<=1e-5 {s50:.3f} share<=1e-3 {s30:.3f}")
        if d in ASSERTED:
            assert met, (d, med, s5, s3)
            assert not met0, (d, med0, s50, s30)
