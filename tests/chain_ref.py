"""The closed loop x0 -> rti -> plant -> rti -> ... -> loss of ihm2_amd/torch_layer.py, composed by hand: what the tests of the chain
share (tests/test_gpu_torch_chain.py on the GPU, tests/test_oracle_torch_chain.py on the CPU oracle).

- backward(): the reverse sweep over the steps.  Step t's adjoint gets the loss's seeds on its outputs and, through the plant step
  behind it, S_u' g on its u[:, 0]; its x0 gets the adjoint's own x0 gradient and the plant's S_x' g -- x_{t-1} feeds the solve and the
  plant.  What a step's adjoint is comes in as a function: the library's host entries on the GPU side, the NumPy references on the
  oracle's side.
- Jitter: the reference's own rounding scale.  The layer and the composition differ by the order of sums only (torch.bmm against
  einsum over eight terms, the a_lat sum over the stages), so the composition is computed a second time with every summed
  intermediate multiplied entrywise by 1 + 8 eps r, r = +-1 at random (8: the terms of the dot product), and a gradient array may
  differ from the reference by 8 times its largest move under that, per instance (the rule of NOTES.md R26); where nothing moves the
  bits are equal (within()).
- host_forward() / host_backward(): the chain on BatchedOcpSolver's host entries (set_*, solve, sim_step_sens,
  eval_adjoint_penalty_sensitivities), one solver per step.
- OracleChain: the two-step chain on the CPU oracle (its interior point at qp_tol 1e-9, its RK4 with sensitivities), with the NumPy
  references adj_ref / penalty_grad_ref / adjw_ref as the steps' adjoints; directions(), measure(): the central-difference check.

Nothing here reads a result that it also judges."""
from __future__ import annotations

import copy

import numpy as np

import cost_cases as C
import layouts as L

EPS = float(np.finfo(np.float64).eps)
ADJ = ("x0", "yref", "yref_e", "W", "W_e")
GRADS = ADJ + ("soft_z", "soft_Z", "alat_z", "alat_Z")
INS = GRADS[1:]                 # a step's inputs beside x0, in the order of rti_solve_soft's arguments
FORWARD = ("x", "u", "s", "sa", "status")
FAIL_SHIFT = 5.0                # added to n of instance 0 at the last solver's input: far outside the hard box, an infeasible QP
KEEP_MIN = 48                   # of 64: tests/test_gpu_penalty_device.py::_central_differences' cap
DRAWS = 16                      # independent draws of Jitter's signs; an array's move is the largest over them (see within())


class Jitter:
    """a -> a (no seed) or a * (1 + 8 eps r), r = +-1 per entry."""

    def __init__(self, seed=None):
        self.rng = None if seed is None else np.random.default_rng(seed)

    def __call__(self, a):
        if self.rng is None:
            return a
        return a * (1.0 + 8.0 * EPS * self.rng.choice([-1.0, 1.0], size=np.shape(a)))


def backward(T, step_adjoint, plants, loss_seeds, jitter=None, drop_sx=False):
    """The reverse sweep.  ``step_adjoint(t, seeds) -> dict`` with at least ``x0 (B,8)``: the gradients of step t's solve for the seeds
    ``dict(x=, u=, s=, sa=)`` on its outputs (a missing key or None: no seed).  ``plants[t] = dict(Sx (B,8,8), Su (B,8,2))``: the
    Jacobians of the plant step between the steps t and t + 1.  ``loss_seeds[t]``: what the loss itself puts on step t's outputs.
    Returns the list of the steps' dicts, ``x0`` the total gradient in the step's input state and ``x0_solve`` the solve's share.
    ``drop_sx``: the composition broken on purpose (the plant's S_x' g left out), for showing that a test notices."""
    jitter = jitter or Jitter()
    out, g_next = [None] * T, None
    for t in reversed(range(T)):
        seeds = {k: v for k, v in loss_seeds.get(t, {}).items() if v is not None}
        direct = None
        if g_next is not None:
            gu = jitter(np.einsum("bij,bi->bj", plants[t]["Su"], g_next))
            direct = jitter(np.einsum("bij,bi->bj", plants[t]["Sx"], g_next))
            su = np.zeros((g_next.shape[0],) + plants[t]["u_shape"])
            if "u" in seeds:
                su += seeds["u"]
                su[:, 0] += gu
            else:
                su[:, 0] = gu
            seeds["u"] = su
        g = dict(step_adjoint(t, seeds))
        g["x0_solve"] = g["x0"]
        if direct is not None and not drop_sx:
            g["x0"] = g["x0"] + direct
        out[t], g_next = g, g["x0"]
    return out


# ---- the chain on the host entries of BatchedOcpSolver ----

def host_forward(cs, x0, ins, model, M_sim, fail_last=False):
    """cs: one handle per step with restore() and .s (tests/test_gpu_penalty_device.py::_Start); ins[t]: dict of INS.  Returns the
    list of the steps' dicts: x0 (the step's input), FORWARD and, for every step but the last, x_next, Sx, Su, model_used."""
    fw, xin = [], np.ascontiguousarray(x0)
    for t, (c, a) in enumerate(zip(cs, ins)):
        if fail_last and t == len(cs) - 1:
            xin = fail_shift(xin)
        s = c.s
        c.restore()
        s.set_instance_weights(a["W"], a["W_e"])
        s.set_instance_soft(a["soft_z"], a["soft_Z"]); s.set_instance_alat_soft(a["alat_z"], a["alat_Z"])
        s.set_x0(xin); s.set_yref(a["yref"]); s.set_yref_e(a["yref_e"])
        st = s.solve()
        rec = dict(x0=xin, x=s.get_x(), u=s.get_u(), s=s.get_slacks(), sa=s.get_alat_multipliers()[1], status=st)
        if t < len(cs) - 1:
            p = s.sim_step_sens(xin, np.ascontiguousarray(rec["u"][:, 0]), model=model, M_sim=M_sim)
            rec.update(x_next=p["x"], Sx=p["Sx"], Su=p["Su"], model_used=p["model_used"], u_shape=rec["u"].shape[1:])
            xin = p["x"]
        fw.append(rec)
    return fw


def fail_shift(x):
    """x + e, e = FAIL_SHIFT on n of instance 0 and +0.0 elsewhere: one addition per entry, as the layer's side of it does."""
    e = np.zeros_like(np.asarray(x, dtype=np.float64))
    e[0, 1] = FAIL_SHIFT
    return x + e


def host_backward(cs, fw, loss_seeds, zero_failed=False, jitter=None, drop_sx=False):
    """The gradients of every step (GRADS) from eval_adjoint_penalty_sensitivities on each step's own solver, which still holds
    that step's solve (host_forward before it, nothing in between)."""
    jitter = jitter or Jitter()

    def step_adjoint(t, seeds):
        h = cs[t].s.eval_adjoint_penalty_sensitivities(seeds.get("x"), seeds.get("u"), seeds.get("s"), seeds.get("sa"))
        g = {k: h[k] for k in ADJ + ("soft_z", "soft_Z")}
        g["alat_z"], g["alat_Z"] = h["alat_soft_z"], h["alat_soft_Z"]
        if zero_failed:
            ok = np.isin(fw[t]["status"], (0, 2))
            g = {k: np.where(ok.reshape((-1,) + (1,) * (v.ndim - 1)), v, 0.0) for k, v in g.items()}
        for k in ("alat_z", "alat_Z"):      # one pair for all stages: the sum of the per-stage rows
            g[k] = jitter(g[k]).sum(1)
        return g

    return backward(len(cs), step_adjoint, fw, loss_seeds, jitter, drop_sx)


def within(name, got, ref, moved, factor=8.0):
    """``got`` against ``ref`` per instance (first axis): the same NaN pattern, and max |got - ref| <= factor * max |moved - ref| over the
    instance's entries and over the draws ``moved`` (a list of arrays: the reference under independent draws of Jitter; one draw can
    leave an array of two entries nearly unmoved by the coincidence of its signs, DRAWS); an instance whose reference does not move
    has the reference's values exactly.  Returns the worst ratio max |got - ref| / max |moved - ref| over the instances that move (0.0
    if none does); raises AssertionError naming the array."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    moved = [np.asarray(a, dtype=np.float64) for a in (moved if isinstance(moved, (list, tuple)) else [moved])]
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN at {np.argwhere(np.isnan(got) != nan)[:6].tolist()} on one side only"
    B = ref.shape[0]
    d = np.where(nan, 0.0, np.abs(got - ref)).reshape(B, -1).max(1)
    m = np.max([np.where(nan, 0.0, np.abs(a - ref)).reshape(B, -1).max(1) for a in moved], axis=0)
    bad = np.flatnonzero(d > factor * m)
    if bad.size:
        i = int(bad[0])
        j = np.unravel_index(int(np.argmax(np.where(nan[i], 0.0, np.abs(got[i] - ref[i])))), ref[i].shape) if ref[i].ndim else ()
        raise AssertionError(f"{name}: {bad.size} of {B} instances off by more than {factor:g} times the reference's own move; instance {i}: "
                             f"|got - ref| {d[i]:.3e}, move {m[i]:.3e}, at {list(j)} got {got[i][j]!r} ref {ref[i][j]!r}")
    return float((d[m > 0.0] / m[m > 0.0]).max()) if (m > 0.0).any() else 0.0


# ---- the central-difference check of the two-step chain: what the GPU test and the oracle test share ----

FD_SEED = 900           # of tests/cost_cases.py::start
FD_VX = (2.5, 2.9)      # every car below the soft lower bound on v_x (3 m/s), spread over this range
FD_PSI = 0.06           # added to every car's heading error
FD_Z_FACTOR = 80.0      # on the quadratic penalties of the soft sides of rows 0..13


def fd_start(track, B, N):
    """x0, yref, yref_e of the central-difference check of the two-step chain: tests/cost_cases.py::start (seed FD_SEED) with every
    car below the soft lower bound on v_x, as tests/test_gpu_penalty_device.py::_Start(..., slow=True) has it, and every car's
    heading FD_PSI off the track's.

    Why not _Start's own start (seed 1234, v_x 1.6 to 2.9, the heading as it is): on the table LAY the two rate rows pin u_0 of nearly
    every instance (the QP of the short horizon is bang-bang), so step 1's penalties and weights reach x_1 through u_0 only where the
    soft lower side of the steering-rate row has its slack in use and the steering does not run into its hard box either -- a third
    of the instances; the median of |fd| over the batch, the floor of measure(), is then the noise of the differences (1e-7) and the
    NumPy reference itself misses the bars (CPU oracle, 64 of 64 kept: penalties median 6.5e-3, weights 1.0e-2).  With the heading
    off, nearly every car wants to steer back through that soft side, and with the quadratic penalties stiffened (fd_penalties) the
    slack stays small enough for the steering to stay inside its box: u_0 of step 1 then reacts to the penalties and to the weights
    on most instances.

    How these four numbers were chosen: on the CPU oracle alone (tests/test_oracle_torch_chain.py), over 126 starts -- the seeds 1234,
    900, 77, 4321, v_x ranges (1.6, 2.9), (2.2, 2.9), (2.5, 2.9), (3.5, 6.0), headings 0.03 to 0.15 off, factors 30 to 200 -- the one
    on which the NumPy reference has the most room under the bars: the largest share <= 1e-3 of its worst direction (63 of 64), then
    the largest share <= 1e-5 (57 of 64).  No result of the code under test entered the choice."""
    x0, yref, yref_e = C.start(track, B, FD_SEED, N)
    x0[:, 3] = np.linspace(FD_VX[0], FD_VX[1], B)
    x0[:, 2] += FD_PSI
    return x0, yref, yref_e


def fd_penalties(z, Z, az, aZ):
    """The per-instance penalties of tests/test_gpu_penalty_device.py::_penalties with soft_Z times FD_Z_FACTOR on the soft sides
    (fd_start)."""
    return z, np.where(Z >= 0.0, Z * FD_Z_FACTOR, Z), az, aZ


def directions(z, Z, W0, We0):
    """dict name -> (eps, dict of the moved inputs of step 1): ``x0``: X_SCALE N(0,1) per instance; ``penalties``: the direction of
    tests/test_gpu_penalty_device.py::_central_differences on (soft_z, soft_Z) (z N(0,1), Z N(0,1) on the soft sides, default_rng(77));
    ``weights``: the symmetric direction of tests/test_gpu_torch_layer.py::_central_differences on (W, W_e) (default_rng(77))."""
    import penalty_grad_cases as PC

    B = z.shape[0]
    out = {"x0": (C.EPS["x0"], dict(x0=C.X_SCALE * np.random.default_rng(78).standard_normal((B, 8))))}
    rng = np.random.default_rng(77)
    soft = Z >= 0.0
    dz = np.where(soft, z * rng.standard_normal(z.shape), 0.0)
    dZ = np.where(soft, Z * rng.standard_normal(Z.shape), 0.0)
    out["penalties"] = (PC.EPS, dict(soft_z=dz, soft_Z=dZ))
    rng = np.random.default_rng(77)

    def sym_dir(Wm):
        w = np.abs(np.diag(Wm))
        G = rng.standard_normal((B,) + Wm.shape)
        return 0.5 * (G + np.swapaxes(G, 1, 2)) * np.sqrt(np.outer(w, w))[None]

    out["weights"] = (1e-4, dict(W=sym_dir(W0), W_e=sym_dir(We0)))
    return out


def contract(grads, d):
    """<gradient, direction> per instance and seed: grads[k] (B, 2, ...) against d[k] (B, ...)."""
    B = next(iter(d.values())).shape[0]
    return sum((np.reshape(grads[k], (B, 2, -1)) * np.reshape(d[k], (B, 1, -1))).sum(-1) for k in d)


def measure(pred, fd, keep):
    """(B,): max_m |pred - fd| / max(max_m |fd|, the median of max_m |fd| over the kept instances), from (B, 2) each."""
    top = np.abs(fd).max(1)
    floor = float(np.median(top[keep])) if len(keep) else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(pred - fd).max(1) / np.maximum(top, floor)


def verdict(tag, name, pred, fd, keep, B):
    """Prints the profile of a direction, asserts the cap on the kept instances and tests/cost_cases.py::profile's bars, and that the
    zero prediction does not meet them.  Returns the printed line."""
    keep = np.asarray(keep, dtype=int)
    assert keep.size >= KEEP_MIN, (name, keep.size, B)
    errs, zero = measure(pred, fd, keep), measure(0.0 * pred, fd, keep)
    (med, s5, s3), met = C.profile(errs[keep])
    (med0, s50, s30), met0 = C.profile(zero[keep])
    line = (f"{tag} {name}: kept {keep.size} of {B}, median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {errs[keep].max():.2e}; "
            f"zero prediction median {med0:.2e} share<=1e-5 {s50:.3f} share<=1e-3 {s30:.3f}")
    print(line)
    assert met, (name, med, s5, s3, np.sort(errs[keep])[-4:])
    assert not met0, (name, med0, s50, s30)
    return line


class OracleChain:
    """x0 -> RTI QP -> plant -> RTI QP -> u_0 on the CPU oracle, instance by instance: both QPs at the start's warm start (the oracle's
    stanley_guess, the counterpart of ihm2mpc_init_guess), solved by the oracle's interior point at tests/cost_cases.py::QP_TOL; the
    plant is orc.rk4_sens (model 0, M_sim steps).  Step 1 may get its own weights (H and g rebuilt by layouts.assemble_qp)."""

    def __init__(self, track, lay, B, model=0, M_sim=25):
        from oracle import oracle as orc
        from test_oracle_slack_seeds import _problem

        self.orc, self.track, self.lay, self.B, self.N, self.model, self.M_sim = orc, track, lay, B, lay.N, model, M_sim
        self.data, self.P = _problem(lay, track)
        self.x0, self.yref, self.yref_e = fd_start(track, B, lay.N)
        self.xbar, self.ubar = orc.stanley_guess(self.P, track.s_ref, track.kappa_ref, self.x0, lay.N)
        self.lin = self.P.linearize(self.xbar, self.ubar)
        self.W0, self.We0 = np.asarray(self.data.W[0], dtype=np.float64), np.asarray(self.data.W_e, dtype=np.float64)

    def solve(self, i, x0, zw, Zw, W=None, We=None):
        """(data, qp, sol) of instance i's QP at its warm start with the input state x0 and the widened penalties (N+1, 30)."""
        import slack_seed_cases as SC

        xb, ub, yr, ye = self.xbar[i], self.ubar[i], self.yref[i], self.yref_e[i]
        A, Bm, b = (a[i] for a in self.lin)
        ref = self.P.build_qp(xb, ub, x0, yr, ye)
        d = self.data
        if W is not None:
            d = copy.copy(self.data)
            d.W, d.W_e = np.broadcast_to(W, (self.N, 12, 12)).copy(), We
        qp = L.assemble_qp(d, xb, ub, x0, yr, ye, A, Bm, b, nonlinear=ref)
        if W is not None:
            ref = dict(ref, H=qp["H"], g=qp["g"])
        return d, qp, SC.qp_solve(ref, self.data, zw, Zw, C.QP_TOL)

    def chain(self, i, x0, pen1, pen2, W=None, We=None):
        """dict: the two solves, the plant's step and Jacobians, u2_0 (2,) and whether both QPs were solved."""
        d1, qp1, s1 = self.solve(i, x0, *pen1, W=W, We=We)
        u1 = self.ubar[i, 0] + s1["dz"][0, 8:]
        x1, Sx, Su = self.orc.rk4_sens(self.model, x0, u1, self.track.s_ref, self.track.kappa_ref, float(self.P.p.dt), self.M_sim)
        d2, qp2, s2 = self.solve(i, x1, *pen2)
        return dict(d=(d1, d2), qp=(qp1, qp2), sol=(s1, s2), pen=(pen1, pen2), x1=x1, Sx=Sx, Su=Su, u2=self.ubar[i, 0] + s2["dz"][0, 8:],
                    solved=s1["status"] == 0 and s2["status"] == 0)

    def weakly_active(self, r):
        import sens_ref as S

        return any(S.weakly_active(qp, sol["dz"], sol["lam"], sl=sol["sl"], soft_z=z, soft_Z=Z) for qp, sol, (z, Z) in zip(r["qp"], r["sol"], r["pen"]))

    def reference(self, i, r, drop_sx=False):
        """The gradients of u2_0[m], m = 0, 1, in step 1's inputs from the NumPy references, composed by backward(): dict of
        x0 (2,8), soft_z, soft_Z (2,N+1,30), W (2,12,12), W_e (2,8,8)."""
        import adjw_ref as RW
        import penalty_grad_ref as PR
        from test_gpu_adjoint_weights import _solve_refined

        N = self.N
        refined = lambda M, rhs: _solve_refined(M, rhs[:, None])[:, 0]  # noqa: E731
        out = dict(x0=np.zeros((2, 8)), soft_z=np.zeros((2, N + 1, 30)), soft_Z=np.zeros((2, N + 1, 30)), W=np.zeros((2, 12, 12)), W_e=np.zeros((2, 8, 8)))
        plants = [dict(Sx=r["Sx"][None], Su=r["Su"][None], u_shape=(N, 2))]
        for m in range(2):
            def step_adjoint(t, seeds):
                qp, sol, (z, Z) = r["qp"][t], r["sol"][t], r["pen"][t]
                sd = np.zeros((N + 1, 10))
                sd[:N, 8:] = seeds["u"][0]
                zs, zeta, nu0 = PR.zeta_s(qp, sol["dz"], sol["lam"], sol["sl"], z, Z, sd, np.zeros_like(z), solve=refined)
                g = dict(x0=nu0[None])
                if t == 0:
                    g["soft_z"], g["soft_Z"] = PR.gradients(zs, sol["sl"])
                    zp = np.zeros((N + 1, 10)); zp[:, :8] = self.xbar[i]; zp[:N, 8:] = self.ubar[i]
                    zp += sol["dz"]; zp[N, 8:] = 0.0
                    g["W"], g["W_e"] = RW.weight_gradients(r["d"][0], zeta, zp, self.yref[i], self.yref_e[i])
                return g

            su = np.zeros((1, N, 2)); su[0, 0, m] = 1.0
            g = backward(2, step_adjoint, plants, {1: dict(u=su)}, drop_sx=drop_sx)[0]
            out["x0"][m] = g["x0"][0]
            for k in ("soft_z", "soft_Z", "W", "W_e"):
                out[k][m] = g[k]
        return out
