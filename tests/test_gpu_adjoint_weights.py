"""Adjoint gradients in the cost weights on the GPU (kernels_adj.hip: k_adj<true>, ihm2mpc_eval_adjoint_sensitivities_w): the epilogue
pinned to rounding through the kernel's own grad_yref, parity with the dense reference (tests/adj_ref.py + tests/adjw_ref.py) on every
layout of the QP-layout suite in both scheduler builds, central differences of whole solves in a weight direction, bit-identity of
every other output, per-instance weights, a stage-dependent shared table, the refusals and NaN rows, the persistent loop and the shim.

Magnitudes.  grad_W[i, j] is a sum over the stages of products (V zeta_k)_i (e_k)_j of both signs; an error is measured against the
cancellation-free magnitude mag_W[i, j] = c_s sum_k sym(|V zeta_k| |e_k|')[i, j] (terminal: sym(|zeta_N| |x_N - yref_e|')), which is what
the rounding errors of the sum are relative to."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import adj_ref as R
import adjw_ref as RW
import drive
import layouts as L
import sens_ref as S
from test_gpu_adjoint import _finite_where_solved, _seeds
from test_gpu_qp_layouts import TABLE, _solver, _start, _widen
from test_gpu_sensitivity import _outputs, _subset

pytestmark = pytest.mark.gpu

# The epilogue alone (test 1): grad_W from the kernel's own V zeta_k = (c_s W)^-1 grad_yref_k.  The only differences are the rounding of
# that solve, N cond(W) 2^-52 ~ 1e-11 at cond(W) = 1000, and the order of the sum: two orders of margin.  Entry by entry the rounding of
# grad_yref_k = c_s W (V zeta_k) and of the solve that undoes it is 2^-52 (|W^-1| |W| |V zeta_k|)_i: a coupling c sqrt(w_i w_j) mixes a small
# entry of V zeta_k with c times its large neighbours, and the entries of zeta differ by eight orders.  The coupling of the second case is
# therefore c = 5e-4 (COUPLING): at c = 0.05 the reconstruction itself was 4.2e-9 off on such entries (the kernel never forms W (V zeta_k)
# on this path), and that error is linear in c.
# Measured: diagonal weights 4.4e-13 at worst, coupled weights 2.1e-10 (grad_W_e, B = 96).
ROUND_TOL = 1e-9
COUPLING = 5e-4
# Against the dense solve at the GPU's own iterate (test 2): the project's ceiling for outputs derived from zeta (tests/test_gpu_adjoint.py:
# REF_TOL_Y).  grad_W is bilinear in zeta and in data that both sides share exactly (x, u, yref), so it inherits zeta's error: that error
# is one of the gains K_k on the worst-conditioned Ht, relative to the largest entry of zeta and not entry by entry (NOTES.md R5.2, R5.4);
# the error is taken relative to the largest entry of the magnitude, per instance and seed, and -- as the ceiling is stated -- entry by
# entry, relative to each entry's own magnitude; both are asserted.
# The reference has to be solved more accurately than np.linalg.solve does: M has condition numbers of 1e15 to 1e19 on these layouts, and on
# hard_narrow_rate_row and hard_10_per_lane_all_boxes the plain fp64 solve is itself 3.0e-6 / 2.4e-6 away from the solution (the kernel: 1.8e-13 /
# 1.6e-9; NOTES.md R5.5).  _solve_refined runs iterative refinement on the same matrix with the residual in extended precision and checks
# that it has converged three orders below the tolerance.
# Measured with it over every layout in both builds: 7.4e-9 of the largest entry at worst (hard_5_per_lane_stage_W), 4.7e-7 entry by entry
# (hard_9_per_lane).
REF_TOL = 1e-6

V = L.selectors()


def _sym(X):
    return 0.5 * (X + np.swapaxes(X, -1, -2))


def _zplus(x, u):
    """(.., N+1, 10) from x (.., N+1, 8), u (.., N, 2): the input part of row N is zero."""
    z = np.zeros(x.shape[:-1] + (10,))
    z[..., :8] = x
    z[..., :-1, 8:] = u
    return z


def _magnitudes(cs, a, e, zN, eN):
    """a (..,N,12) = V zeta_k, e (..,N,12) = e_k, zN, eN (..,8): the cancellation-free magnitudes of grad_W and grad_W_e."""
    mW = cs * _sym(np.einsum("...ki,...kj->...ij", np.abs(a), np.abs(e)))
    mWe = _sym(np.abs(zN)[..., :, None] * np.abs(eN)[..., None, :])
    return mW, mWe


def _coupled(W, c=COUPLING):
    """W with a small symmetric off-diagonal coupling c sqrt(w_i w_j) between neighbouring outputs (diagonally dominant: positive definite)."""
    w = np.sqrt(np.diag(W))
    n = W.shape[0]
    Wc = W.copy()
    for i in range(n - 1):
        Wc[i, i + 1] = Wc[i + 1, i] = c * w[i] * w[i + 1] * (1.0 if i % 2 == 0 else -1.0)
    return Wc


@pytest.mark.parametrize("B,coupled,per_instance", [(1, False, False), (3, True, True), (96, True, False), (96, False, True)])
def test_epilogue_pinned_to_rounding(track, B, coupled, per_instance):
    """With nonsingular weights V zeta_k = (c_s W)^-1 grad_yref_k and zeta_N = W_e^-1 grad_yref_e: grad_W and grad_W_e must be the two
    formulas evaluated in NumPy from the GPU's own grad_yref, grad_yref_e, x, u, yref, yref_e, to rounding (ROUND_TOL of the magnitude,
    entry by entry).  n_seeds 1, 3, 8 and the default seeds; shared and per-instance weights."""
    from ihm2_amd import ocp as O

    lay = TABLE["hard_5_per_lane"][0]
    s = _solver(track, lay, B, "default", "0")
    W0, We0 = O.default_weights(q_T_dot=1.0)
    if coupled:
        W0, We0 = _coupled(W0), _coupled(We0)
    fac = 1.0 + 0.25 * (np.arange(B) % 3) if per_instance else np.ones(B)
    Wb, Web = fac[:, None, None] * W0[None], (1.5 - 0.5 * fac)[:, None, None] * We0[None]
    if per_instance:
        s.set_instance_weights(Wb, Web)
    else:
        s.set_weights(W0, We0)
    x0, yref, yref_e = _start(s, track, B, 321)
    s.set_x0_sensitivities(1)
    st = s.solve()
    ok = (st == 0) | (st == 2)
    assert ok.mean() > 0.5
    N, cs = s.N, s.data.cost_scale_stage
    zp = _zplus(s.get_x(), s.get_u())
    e = zp[:, :N] @ V.T - yref                      # (B,N,12)
    eN = zp[:, N, :8] - yref_e                      # (B,8)
    seed_x, seed_u = _seeds(B, 8, N, 17)
    worst = [0.0, 0.0]
    for n in (1, 3, 8, None):
        g = s.eval_adjoint_weight_sensitivities() if n is None else s.eval_adjoint_weight_sensitivities(seed_x[:, :n], seed_u[:, :n])
        S_ = 2 if n is None else n
        assert g["W"].shape == (B, S_, 12, 12) and g["W_e"].shape == (B, S_, 8, 8)
        _finite_where_solved(g, ok)
        np.testing.assert_array_equal(g["W"], np.swapaxes(g["W"], -1, -2))
        np.testing.assert_array_equal(g["W_e"], np.swapaxes(g["W_e"], -1, -2))
        for b in np.flatnonzero(ok):
            a = np.linalg.solve(cs * Wb[b], g["yref"][b].reshape(-1, 12).T).T.reshape(S_, N, 12)       # V zeta_k
            zN = np.linalg.solve(Web[b], g["yref_e"][b].T).T                                            # (S,8)
            want_W = -cs * _sym(np.einsum("ski,kj->sij", a, e[b]))
            want_We = -_sym(zN[:, :, None] * eN[b][None, None, :])
            mW, mWe = _magnitudes(cs, a, e[b][None], zN, eN[b][None])
            for m, (got, want, mag) in enumerate(((g["W"][b], want_W, mW), (g["W_e"][b], want_We, mWe))):
                nz = mag > 0.0
                assert (got[~nz] == 0.0).all()
                worst[m] = max(worst[m], float((np.abs(got - want)[nz] / mag[nz]).max()))
    print(f"ADJW epilogue B {B} coupled {coupled} per_instance {per_instance}: worst {worst[0]:.2e} (grad_W) {worst[1]:.2e} (grad_W_e) of the magnitude")
    assert max(worst) <= ROUND_TOL, worst
    s.free()


def _solve_refined(M, rhs, steps=3):
    """M^-1 rhs by LU in fp64 and `steps` of iterative refinement with the residual in np.longdouble (80-bit on x86); the last correction
    must be below 1e-9 of the solution, i.e. the reference is then known three orders below REF_TOL."""
    import scipy.linalg as sl

    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than double here: the residual would gain nothing"
    lu = sl.lu_factor(M)
    Ml, rl = M.astype(np.longdouble), rhs.astype(np.longdouble)
    x = sl.lu_solve(lu, rhs).astype(np.longdouble)
    for _ in range(steps):
        dx = sl.lu_solve(lu, (rl - Ml @ x).astype(np.float64))
        x = x + dx
    assert np.abs(dx).max() <= 1e-9 * np.abs(x).max(), ("the refinement of the dense reference has not converged", np.abs(dx).max() / np.abs(x).max())
    return x.astype(np.float64)


def _reference_errors(s, P, data, x0, yref, yref_e, xbar, ubar, g, seed_x, seed_u, nc, z, Z, path, idx, track_id=None):
    """The kernel's grad_W / grad_W_e of the instances idx, all seeds, against adj_ref + adjw_ref at the GPU's own iterate and
    linearisation: the worst deviation relative to the largest entry of the magnitude (per instance and seed), and the worst deviation
    of an entry relative to its own magnitude.  (adjw_ref's grad_W is the sum of its per-stage terms: on the stage_W layouts this is the
    comparison with that sum.)"""
    A, Bm, b = s.get_linearization()
    o = _outputs(s, alat=nc == 15)
    lam, slk = (_widen(o["lam"], o["lam_a"]), _widen(o["slk"], o["slk_a"])) if nc == 15 else (o["lam"], o["slk"])
    N = s.N
    nz_ = N * 10 + 8
    worst = worst_entry = 0.0
    zp = _zplus(o["x"], o["u"])
    for i in idx:
        ref = P.build_qp(xbar[i], ubar[i], x0[i], yref[i], yref_e[i], track_id=0 if track_id is None else int(track_id[i])) if path else None
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref)
        dz = np.zeros((N + 1, 10)); dz[:, :8] = o["x"][i] - xbar[i]; dz[:N, 8:] = o["u"][i] - ubar[i]
        M = R.kkt_matrix(qp, dz, lam[i], slk[i], z, Z)           # adj_ref.adjoint's system, factored once for the eight seeds
        n_s = seed_x.shape[1]
        rhs = np.zeros((M.shape[0], n_s))
        for j in range(n_s):
            sd = np.zeros((N + 1, 10)); sd[:, :8] = seed_x[i, j]; sd[:N, 8:] = seed_u[i, j]
            rhs[:nz_, j] = sd.reshape(-1)[:nz_]
        sol = _solve_refined(M, rhs)
        for j in range(n_s):
            zeta = np.zeros((N + 1, 10)); zeta.reshape(-1)[:nz_] = sol[:nz_, j]
            gW, gWe = RW.weight_gradients(data, zeta, zp[i], yref[i], yref_e[i])
            _, mags = RW.stage_terms(data, zeta, zp[i], yref[i])
            mW = _sym(mags.sum(0))
            mWe = _sym(np.outer(np.abs(zeta[N, :8]), np.abs(zp[i, N, :8] - yref_e[i])))
            for got, want, mag in ((g["W"][i, j], gW, mW), (g["W_e"][i, j], gWe, mWe)):
                d = np.abs(got - want)
                worst = max(worst, float(d.max() / mag.max()))
                nz = mag > 0.0
                worst_entry = max(worst_entry, float((d[nz] / mag[nz]).max()))
    return worst, worst_entry


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("name", list(TABLE))
def test_layout_reference(track, name, build):
    """Two RTI steps per layout and build, eight random seeds, against the dense reference at the GPU's own iterate (a subset of the solved
    instances).  The layouts with stage_W hold a stage-dependent shared table: there grad_W is the sum over the stages of adjw_ref's
    per-stage terms (the derivative in a shift common to all stages)."""
    from oracle import oracle as orc

    lay, B, block = TABLE[name]
    s = _solver(track, lay, B, build, block)
    data = s.data
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    x0, yref, yref_e = _start(s, track, B, 900 + lay.seed)
    nc = 15 if lay.alat else L.NC
    z, Z = L.soft_arrays(data, nc, (data.alat_soft_z, data.alat_soft_Z) if lay.alat and data.alat_soft_Z is not None else None)
    s.set_x0_sensitivities(2)
    seed_x, seed_u = _seeds(B, 8, s.N, 40 + lay.seed)
    if lay.stage_W:
        assert not np.array_equal(data.W[0], data.W[1])
    for it in range(1 if name == "empty_table" else 2):
        xbar, ubar = s.get_x(), s.get_u()
        st = s.solve()
        ok = (st == 0) | (st == 2)
        g = s.eval_adjoint_weight_sensitivities(seed_x, seed_u)
        assert g["W"].shape == (B, 8, 12, 12) and g["W_e"].shape == (B, 8, 8, 8)
        _finite_where_solved(g, ok)
        e, e_entry = _reference_errors(s, P, data, x0, yref, yref_e, xbar, ubar, g, seed_x, seed_u, nc, z, Z, lay.path, _subset(ok))
        print(f"ADJW {name} {build} it{it}: ref {e:.2e} (entry by entry {e_entry:.2e})")
        assert e <= REF_TOL and e_entry <= REF_TOL, ("against adj_ref + adjw_ref", e, e_entry)
    s.free()


@pytest.mark.parametrize("name", ["hard_5_per_lane", "soft_4_per_lane_mixed", "path_soft_both_sides", "alat_soft"])
def test_du0_dW_against_whole_solves(track, name):
    """du0_dW() contracted with a symmetric weight direction (dW_b, dW_e,b) per instance -- sym(N(0,1)) scaled entry by entry with
    sqrt(w w'), w = |diag W| -- against central differences of whole solves under set_instance_weights(W +- eps dW), the iterate,
    multipliers and slacks restored each time (test_gpu_adjoint.py::test_du0_ds_target_against_whole_solves: its tables, its measure
    |pred - fd| / max(|fd|, |pred_free|) and its bars).  The QP's solution is rational in W: with eps = 1e-4 relative to the weights the
    truncation error of the central difference is of the order eps^2 = 1e-8 of the reaction, below the bars."""
    from ihm2_amd.solver import BatchedOcpSolver
    from oracle import oracle as orc

    lay = TABLE[name][0]
    B, s_target, eps = 64, 40.0, 1e-4
    ocp = L.make_ocp(lay)
    ocp.solver_options.qp_tol = 1e-9
    ocp.solver_options.qp_solver_iter_max = 200
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
    L.apply(s.data, lay)
    s._push_weights(); s._push_bounds()
    x0, yref, yref_e = _start(s, track, B, 1234)
    s.set_x0_sensitivities(1)
    x, u = s.get_x(), s.get_u()
    pi, lam = s.get_multipliers(); slk = s.get_slacks()
    la = s.get_alat_multipliers() if lay.alat else None
    W0, We0 = np.asarray(s.data.W[0], dtype=np.float64), np.asarray(s.data.W_e, dtype=np.float64)
    rng = np.random.default_rng(77)

    def direction(Wm):
        w = np.abs(np.diag(Wm))
        G = rng.standard_normal((B,) + Wm.shape)
        return _sym(G) * np.sqrt(np.outer(w, w))[None]

    dW, dWe = direction(W0), direction(We0)

    def solve_at(sign):
        s.set_instance_weights(W0[None] + sign * eps * dW, We0[None] + sign * eps * dWe)
        s.set_yref(yref); s.set_yref_e(yref_e)
        s.set_x(x); s.set_u(u); s.set_multipliers(pi, lam); s.set_slacks(slk)
        if la is not None:
            s.set_alat_multipliers(*la)
        return s.solve()

    st = solve_at(0.0)
    d = s.du0_dW()
    assert set(d) == {"W", "W_e"} and d["W"].shape == (B, 2, 12, 12) and d["W_e"].shape == (B, 2, 8, 8)
    pred = np.einsum("bsij,bij->bs", d["W"], dW) + np.einsum("bsij,bij->bs", d["W_e"], dWe)
    o = _outputs(s, alat=lay.alat)
    lamw, slkw = (_widen(o["lam"], o["lam_a"]), _widen(o["slk"], o["slk_a"])) if lay.alat else (o["lam"], o["slk"])
    nc = 15 if lay.alat else L.NC
    z, Z = L.soft_arrays(s.data, nc, (s.data.alat_soft_z, s.data.alat_soft_Z) if lay.alat_soft else None)
    P = orc.OracleProblem(s.data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    A, Bm, b = s.get_linearization()
    zp = _zplus(o["x"], o["u"])
    keep, free = [], np.zeros((B, 2))
    for i in np.flatnonzero(st == 0):       # the weakly active instances have no derivative: skipped, as in the forward test
        ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i]) if lay.path else None
        qp = L.assemble_qp(s.data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref)
        dz = np.zeros((s.N + 1, 10)); dz[:, :8] = o["x"][i] - x[i]; dz[:s.N, 8:] = o["u"][i] - u[i]
        if S.weakly_active(qp, dz, lamw[i], sl=slkw[i], soft_z=z, soft_Z=Z):
            continue
        keep.append(i)
        # the same prediction with all multipliers zero (dense, at the GPU's iterate): the scale of an unconstrained reaction
        for m in range(2):
            sd = np.zeros((s.N + 1, 10)); sd[0, 8 + m] = 1.0
            zeta, _ = R.adjoint(qp, dz, 0.0 * lamw[i], slkw[i], z, Z, sd)
            gW, gWe = RW.weight_gradients(s.data, zeta, zp[i], yref[i], yref_e[i])
            free[i, m] = np.sum(gW * dW[i]) + np.sum(gWe * dWe[i])
    stp = solve_at(1.0); up = s.get_u0()
    stm = solve_at(-1.0); um = s.get_u0()
    fd = (up - um) / (2 * eps)
    solved = (st == 0) & (stp == 0) & (stm == 0)
    assert solved.mean() >= 0.8, solved.mean()
    keep = [i for i in keep if solved[i]]
    assert len(keep) >= 60, len(keep)
    errs = np.array([np.abs(pred[i] - fd[i]).max() / max(np.abs(fd[i]).max(), np.abs(free[i]).max()) for i in keep])
    pinned = np.mean([np.abs(fd[i]).max() <= 1e-6 * np.abs(free[i]).max() for i in keep])
    print(f"ADJW-FD {name}: kept {len(keep)} of {B}, u_0 pinned on {pinned:.2f}, median {np.median(errs):.2e} share<=1e-5 {np.mean(errs <= 1e-5):.3f} "
          f"share<=1e-3 {np.mean(errs <= 1e-3):.3f} max {errs.max():.2e}")
    assert np.median(errs) <= 1e-6 and np.mean(errs <= 1e-5) >= 0.75 and np.mean(errs <= 1e-3) >= 0.95, \
        (np.median(errs), np.mean(errs <= 1e-5), np.sort(errs)[-4:])
    s.free()


@pytest.mark.parametrize("B", [1, 96, 4096])
def test_nothing_else_moves(track, B):
    """The new entry's grad_x0, grad_yref, grad_yref_e are the old entry's bits; the old entry's outputs, the iterate, the multipliers
    and the status are untouched by the call; two calls return the same bits; all outputs NULL is accepted; a seed gives the same bits
    alone or among eight."""
    from ihm2_amd import _lib

    lay = TABLE["path_soft_4_per_lane"][0] if B == 96 else TABLE["hard_5_per_lane"][0]
    s = _solver(track, lay, B, "default", "1")
    _start(s, track, B, 55)
    s.set_x0_sensitivities(2)
    st = s.solve()
    assert (st == 0).mean() > 0.5
    before = dict(_outputs(s), u0=s.get_u0())
    before["sens_x"], before["sens_u"] = s.get_x0_sensitivities()
    seed_x, seed_u = _seeds(B, 8, s.N, 7)
    old8, oldd = s.eval_adjoint_sensitivities(seed_x, seed_u), s.eval_adjoint_sensitivities()
    g8 = s.eval_adjoint_weight_sensitivities(seed_x, seed_u)
    again = s.eval_adjoint_weight_sensitivities(seed_x, seed_u)
    g1 = s.eval_adjoint_weight_sensitivities(seed_x[:, 0], seed_u[:, 0])
    gd = s.eval_adjoint_weight_sensitivities()
    ptr = lambda a: a.ctypes.data_as(_lib.c_double_p)       # noqa: E731
    _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w(s._h, 8, ptr(seed_x), ptr(seed_u), None, None, None, None, None))
    _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w(s._h, 2, None, None, None, None, None, None, None))
    old8_after, oldd_after = s.eval_adjoint_sensitivities(seed_x, seed_u), s.eval_adjoint_sensitivities()
    after = dict(_outputs(s), u0=s.get_u0())
    after["sens_x"], after["sens_u"] = s.get_x0_sensitivities()
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    assert set(g8) == {"x0", "yref", "yref_e", "W", "W_e"}
    for k in old8:
        np.testing.assert_array_equal(g8[k], old8[k], err_msg=k)
        np.testing.assert_array_equal(gd[k], oldd[k], err_msg=k)
        np.testing.assert_array_equal(old8_after[k], old8[k], err_msg=k)
        np.testing.assert_array_equal(oldd_after[k], oldd[k], err_msg=k)
    for k in g8:
        np.testing.assert_array_equal(again[k], g8[k], err_msg=k)
        np.testing.assert_array_equal(g1[k], g8[k][:, 0], err_msg=k)
        assert g1[k].shape == g8[k].shape[:1] + g8[k].shape[2:]
    _finite_where_solved(g8, (st == 0) | (st == 2))
    s.free()


def test_per_instance_weights(track):
    """Instance b of a batch with per-instance weights has the gradients of a handle whose shared weights are (W[b], W_e[b]), bit for bit."""
    from ihm2_amd import ocp as O

    lay = TABLE["soft_2_per_lane_split_rows"][0]
    B = 30
    assign = np.arange(B) % 3
    W0, We0 = O.default_weights()
    var = [(W0 * (1.0 + 0.5 * j), We0 * (1.0 + 0.25 * j)) for j in range(3)]
    x0 = drive.clipped_start(track, B, 4343)
    seed_x, seed_u = _seeds(B, 3, lay.N, 99)

    def run(s, rows):
        s.set_x0_sensitivities(1)
        s.set_x0(x0[rows]); s.init_guess()
        out = []
        for _ in range(2):
            s.prepare_step(40.0)
            st = s.solve()
            g, d = s.eval_adjoint_weight_sensitivities(seed_x[rows], seed_u[rows]), s.du0_dW()
            out.append((st, g["x0"], g["yref"], g["yref_e"], g["W"], g["W_e"], d["W"], d["W_e"]))
        return out

    s = _solver(track, lay, B, "default", "0")
    s.set_instance_weights(np.stack([var[a][0] for a in assign]), np.stack([var[a][1] for a in assign]))
    mixed = run(s, np.arange(B))
    s.free()
    for j in range(3):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, lay, rows.size, "default", "0")
        h.data.W = np.broadcast_to(var[j][0], h.data.W.shape).copy(); h.data.W_e = var[j][1]
        h._push_weights()
        homo = run(h, rows)
        h.free()
        for m, hh in zip(mixed, homo):
            for a, bb in zip(m, hh):
                np.testing.assert_array_equal(a[rows], bb)
    assert (mixed[-1][0] == 0).mean() > 0.5
    # the weights reach the gradient: the three tunings differ
    assert not np.array_equal(mixed[-1][4][0], mixed[-1][4][1])


def test_fdyn6u_irk(track):
    from ihm2_amd.solver import BatchedOcpSolver
    from oracle import oracle as orc

    B = 64
    ocp = make_ocp(model="fdyn6u", M=1, integrator_type="IRK")
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    x0, yref, yref_e = _start(s, track, B, 77)
    s.set_x0_sensitivities(2)
    xbar, ubar = s.get_x(), s.get_u()
    st = s.solve()
    data = s.data
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref))
    z, Z = L.soft_arrays(data)
    ok = st == 0
    assert ok.mean() > 0.5
    seed_x, seed_u = _seeds(B, 8, s.N, 5)
    g = s.eval_adjoint_weight_sensitivities(seed_x, seed_u)
    e, e_entry = _reference_errors(s, P, data, x0, yref, yref_e, xbar, ubar, g, seed_x, seed_u, L.NC, z, Z, False, _subset(ok))
    print(f"ADJW fdyn6u_irk: ref {e:.2e} (entry by entry {e_entry:.2e})")
    assert e <= REF_TOL and e_entry <= REF_TOL, (e, e_entry)
    s.free()


@pytest.mark.parametrize("plant,n_max,B,opts", [(0, 2.0, 150, {}), (0, 2.0, 150, dict(integrator_type="IRK", sim_method_num_steps=1))])
def test_after_the_persistent_loop(track, plant, n_max, B, opts, monkeypatch):
    """After run_steps_sens(n) the call differentiates the last step's solve: bit for bit what it gives after n x step()
    (test_gpu_adjoint.py::test_after_the_persistent_loop)."""
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    steps = 6
    x0 = sample_x0(track, B, seed=31)
    seed_x, seed_u = _seeds(B, 2, 40, 3)
    res = []
    for persistent in (False, True):
        s = BatchedOcpSolver(make_ocp(n_max=n_max, **opts), B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        s.set_x0_sensitivities(1)
        s.set_x0(x0); s.init_guess()
        s.step(40.0, model=plant, M_sim=30)
        if persistent:
            s.run_steps(40.0, steps, model=plant, M_sim=30, sens_u0_hist=True)
            assert s.get_launch_record()["steps"].startswith("k_steps<")
        else:
            for _ in range(steps):
                s.step(40.0, model=plant, M_sim=30)
        st = s.get_status()
        res.append((st, s.eval_adjoint_weight_sensitivities(seed_x, seed_u), s.du0_dW()))
        s.free()
    (sa, ga, da), (sb, gb, db) = res
    np.testing.assert_array_equal(sb, sa)
    for k in ga:
        np.testing.assert_array_equal(gb[k], ga[k], err_msg=k)
    for k in da:
        np.testing.assert_array_equal(db[k], da[k], err_msg=k)
    ok = np.isin(sa, (0, 2))
    assert ok.mean() > 0.7 and np.isfinite(ga["W"][ok]).all() and np.abs(ga["W"][ok]).max() > 0.0


def test_refusals_and_nan_rows(track):
    from ihm2_amd import _lib
    from ihm2_amd._lib import Ihm2mpcError
    from ihm2_amd.solver import BatchedOcpSolver

    B = 8
    sq = BatchedOcpSolver(make_ocp(nlp_solver_type="SQP", nlp_solver_max_iter=2), B, track.s_ref, track.kappa_ref)
    with pytest.raises(Ihm2mpcError, match="SQP"):
        sq.eval_adjoint_weight_sensitivities()
    sq.free()
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    with pytest.raises(Ihm2mpcError, match="off"):
        s.eval_adjoint_weight_sensitivities()
    s.set_x0_sensitivities(1)
    with pytest.raises(Ihm2mpcError, match="no solve"):
        s.du0_dW()
    x0 = sample_x0(track, B, seed=9)
    x0[0, 1] = 5.0              # far outside the hard box on n: an infeasible QP, reported by its status (test_gpu_adjoint.py's instance)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    assert st[0] not in (0, 2) and (st[1:] == 0).mean() > 0.5, st
    ok = (st == 0) | (st == 2)
    _finite_where_solved(s.eval_adjoint_weight_sensitivities(), ok)
    _finite_where_solved(s.du0_dW(), ok)
    N = s.N
    _finite_where_solved(s.eval_adjoint_weight_sensitivities(np.ones((B, 3, N + 1, 8)), None), ok)
    buf = np.zeros((B, 9, N + 1, 8))
    nul = [None] * 5
    for n in (0, 9, -1):
        with pytest.raises(Ihm2mpcError, match="1 to 8 seeds"):
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w(s._h, n, buf.ctypes.data_as(_lib.c_double_p), None, *nul))
    for n in (1, 3, 8):
        with pytest.raises(Ihm2mpcError, match="both NULL"):
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w(s._h, n, None, None, *nul))
    _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w(s._h, 2, None, None, *nul))       # every output may be NULL
    with pytest.raises(ValueError):
        s.eval_adjoint_weight_sensitivities(np.zeros((B, 2, N, 8)), None)
    s.run_steps(40.0, 2, model=0, M_sim=25)
    with pytest.raises(Ihm2mpcError, match="run_steps"):
        s.eval_adjoint_weight_sensitivities()
    s.prepare_step(40.0)
    s.solve()
    s.eval_adjoint_weight_sensitivities()          # readable again after a solve
    s.set_x0_sensitivities(0)
    with pytest.raises(Ihm2mpcError, match="off"):
        s.eval_adjoint_weight_sensitivities()
    s.free()


def test_shim(track):
    from ihm2_amd.solver import BatchedOcpSolver

    B = 16
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_x0_sensitivities(2)
    x0 = sample_x0(track, B, seed=3)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    assert st[5] == 0
    N = s.N
    seed_x, seed_u = _seeds(B, 3, N, 8)
    seed_x[:, :, [2, 4]] = 0.0            # a caller's seeds need not cover every stage
    g = s.eval_adjoint_weight_sensitivities(seed_x, seed_u)
    v = s[5]
    sx_list = [(k, seed_x[5, :, k].T) for k in range(N + 1) if k not in (2, 4)]
    su_list = [(k, seed_u[5, :, k].T) for k in range(N)]
    gW, gWe = v.eval_adjoint_weight_sensitivity(sx_list, su_list)
    assert gW.shape == (3, 12, 12) and gWe.shape == (3, 8, 8)
    np.testing.assert_array_equal(gW, g["W"][5])
    np.testing.assert_array_equal(gWe, g["W_e"][5])
    gW, gWe = v.eval_adjoint_weight_sensitivity([], [(0, np.eye(2))])
    d = s.du0_dW()
    np.testing.assert_array_equal(gW, d["W"][5])
    np.testing.assert_array_equal(gWe, d["W_e"][5])
    with pytest.raises(Exception, match="both empty"):
        v.eval_adjoint_weight_sensitivity([], None)
    with pytest.raises(Exception, match="is not supported"):
        v.eval_adjoint_solution_sensitivity(sx_list, su_list, with_respect_to="W")
    s.free()
