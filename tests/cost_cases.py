"""The cases of the whole-solve check of the cost gradient, shared by tests/test_oracle_cost.py (CPU: the NumPy reference against central
differences of whole oracle solves) and tests/test_gpu_cost.py (GPU: the kernel's gradient against central differences of get_cost over
re-solves): the all-hard layouts, the instances (seeds of conftest.sample_x0), the start (x0, reference ramp) and the perturbation
directions of x0, yref, W and W_e with their step lengths.  Nothing here reads a result."""
from __future__ import annotations

import numpy as np

import layouts as L

# (layout, batch size, seed of the instances): the horizon 40 of the reference table at B = 67, a short horizon at B = 67
CASES = {
    "hard_n40": (L.TABLE["hard_5_per_lane"][0], 67, 1234),
    "hard_n10": (L.Layout("cost_hard_n10", N=10), 67, 4321),
}
QP_TOL = 1e-9           # of the re-solves (ocp.solver_options.qp_tol), with qp_solver_iter_max = 200
S_TARGET = 40.0
# scales of a change of the state and of the outputs y = (x, u, x[6:8] - u)
X_SCALE = np.array([1.0, 0.1, 0.05, 1.0, 0.1, 0.1, 10.0, 0.02])
Y_SCALE = np.concatenate([X_SCALE, [10.0, 0.02, 10.0, 0.02]])
# step lengths of the central differences: absolute on x0 and yref (times the scales above), relative to the weights on W, W_e.  The
# solution of the QP is rational in all of them and J is quadratic in the solution: the truncation error is of the order eps^2
EPS = {"x0": 1e-4, "yref": 1e-4, "W_diag": 1e-4, "W_off": 1e-4, "W_e_diag": 1e-4, "W_e_off": 1e-4}
DIRECTIONS = tuple(EPS)


def start(track, B, seed, N):
    """x0 (B,8), yref (B,N,12), yref_e (B,8): test_gpu_qp_layouts._start's."""
    import drive

    x0 = drive.clipped_start(track, B, seed)
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + S_TARGET * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = x0[:, 0] + S_TARGET
    return x0, yref, yref_e


def _sym_dir(rng, Wm, diagonal):
    """A symmetric direction of the size of the weights: diag(w N(0,1)), or sym(N(0,1)) sqrt(w w') with a zero diagonal."""
    w = np.abs(np.diag(Wm))
    if diagonal:
        return np.diag(w * rng.standard_normal(w.size))
    G = rng.standard_normal(Wm.shape)
    G = 0.5 * (G + G.T) * np.sqrt(np.outer(w, w))
    np.fill_diagonal(G, 0.0)
    return G


def directions(name, B, N, W0, We0):
    """dict direction -> dict(x0 (B,8), yref (B,N,12), yref_e (B,8), W (12,12), W_e (8,8)), zero where the direction does not act.  x0 and
    yref directions differ by instance; a weight direction is common to the batch (and to all stages).  The yref direction moves one
    component of one stage in each third of the horizon, and one of yref_e."""
    seed = sum(ord(c) for c in name)
    rng = np.random.default_rng(1000 + seed)
    zero = lambda: dict(x0=np.zeros((B, 8)), yref=np.zeros((B, N, 12)), yref_e=np.zeros((B, 8)), W=np.zeros((12, 12)), W_e=np.zeros((8, 8)))  # noqa: E731
    out = {d: zero() for d in DIRECTIONS}
    out["x0"]["x0"] = rng.standard_normal((B, 8)) * X_SCALE
    groups = [range(0, max(N // 3, 1)), range(N // 3, max(2 * N // 3, N // 3 + 1)), range(2 * N // 3, N)]
    for b in range(B):
        for g in groups:
            k, c = int(rng.choice(list(g))), int(rng.integers(12))
            out["yref"]["yref"][b, k, c] = rng.standard_normal() * Y_SCALE[c]
        c = int(rng.integers(8))
        out["yref"]["yref_e"][b, c] = rng.standard_normal() * X_SCALE[c]
    out["W_diag"]["W"] = _sym_dir(rng, W0, True)
    out["W_off"]["W"] = _sym_dir(rng, W0, False)
    out["W_e_diag"]["W_e"] = _sym_dir(rng, We0, True)
    out["W_e_off"]["W_e"] = _sym_dir(rng, We0, False)
    return out


def contract(grad, d):
    """<gradient, direction> per instance: grad dict(x0 (B,8), yref (B,N,12), yref_e (B,8), W (B,12,12), W_e (B,8,8))."""
    return (np.einsum("bi,bi->b", grad["x0"], d["x0"]) + np.einsum("bki,bki->b", grad["yref"], d["yref"])
            + np.einsum("bi,bi->b", grad["yref_e"], d["yref_e"]) + np.einsum("bij,ij->b", grad["W"], d["W"])
            + np.einsum("bij,ij->b", grad["W_e"], d["W_e"]))


def profile(errs):
    """The acceptance profile of tests/test_gpu_adjoint_weights.py::test_du0_dW_against_whole_solves: (median, share <= 1e-5, share <=
    1e-3) and whether it is met (median <= 1e-6, >= 75 % <= 1e-5, >= 95 % <= 1e-3)."""
    errs = np.asarray(errs)
    med, s5, s3 = float(np.median(errs)), float(np.mean(errs <= 1e-5)), float(np.mean(errs <= 1e-3))
    return (med, s5, s3), bool(med <= 1e-6 and s5 >= 0.75 and s3 >= 0.95)
