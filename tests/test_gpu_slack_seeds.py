"""Adjoint seeds on the soft slacks on the GPU (kernels_slackseed.hip: k_slack_fold; ihm2mpc_eval_adjoint_sensitivities_s,
ihm2mpc_eval_cost_gradient_soft): the fold alone against the host's fold fed to the _w entry, the seeds of the cost entry, the totals
against the dense system that keeps the slacks as variables, central differences of get_cost over whole re-solves on the cases
tests/test_oracle_slack_seeds.py has shown to be fair, bit-identity of everything else, refusals and NaN rows, the workspace poison.

IHM2MPC_TEST_BUILD=ilp in the environment runs the module's handles on libihm2mpc_ilp.so (the new object is built with the same flags
in both libraries; the poison child keeps the default library); test_fold_alone runs one layout in both builds in any case.

Tolerances.  FOLD_TOL: the kernel's fold and the host's differ by roundings of gamma and of a sum of at most five products, about
1e-15 of the seed, and k_adj is linear in the seed: ROUND_TOL of tests/test_gpu_adjoint_weights.py (1e-9 of the largest entry), the
composition bound of tests/test_gpu_cost.py.  VAL_TOL (1e-12 of the sum of the absolute terms) and REF_TOL (1e-6 of the largest entry,
against the dense solve) are those of tests/test_gpu_cost.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import sample_x0

import adj_ref as R
import adjw_ref as RW
import cost_cases as C
import cost_ref as CR
import layouts as L
import sens_ref as S
import slack_seed_cases as SC
import slack_seed_ref as SR
from test_gpu_adjoint import _seeds
from test_gpu_adjoint_weights import REF_TOL, ROUND_TOL, _solve_refined
from test_gpu_cost import GRADS, VAL_TOL
from test_gpu_qp_layouts import _solver as _solver_of_build
from test_gpu_qp_layouts import _start, _widen
from test_gpu_sensitivity import _outputs, _subset

pytestmark = pytest.mark.gpu

BUILD = os.environ.get("IHM2MPC_TEST_BUILD", "default")
FOLD_TOL = ROUND_TOL
LAYOUTS = {
    "cost_soft": L.Layout("cost_soft", N=10, soft=1.0, soft_rows=(1,), soft_kind="both", seed=6),
    "soft_n10_asym": SC.CASES["soft_n10_asym"][0],
    "soft_4_per_lane_mixed": L.TABLE["soft_4_per_lane_mixed"][0],
    "path_soft_both_sides": L.TABLE["path_soft_both_sides"][0],
    "alat_soft": L.TABLE["alat_soft"][0],
}


def _solver(track, lay, B, build=None):
    return _solver_of_build(track, lay, B, build or BUILD, "0")


class _Solved:
    """One solve of a layout from the start of tests/test_gpu_qp_layouts.py, and the host's view of every instance's QP at the GPU's own
    iterate: qp(i) -> (assemble_qp dict, dz, lam, sl) with the lateral-acceleration row's sides widened in where the layout has it."""

    def __init__(self, track, lay, B, seed, build=None, solves=1, tracks=None, sens_mode=1):
        """``tracks``: a case of tests/multi_track_cases.py -- the handle then holds that case's tables, per-instance track ids and
        widths (track, B and seed are the case's own), and the host's view takes every instance's own track."""
        from oracle import oracle as orc

        self.lay, self.B, self.N = lay, B, lay.N
        if tracks is None:
            self.track_id, self.widths = np.zeros(B, dtype=np.int32), (L.track_widths(lay) if lay.path else None)
            self.s = s = _solver(track, lay, B, build)
            self.P = orc.OracleProblem(s.data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
            self.x0, self.yref, self.yref_e = _start(s, track, B, seed)
        else:
            import multi_track_cases as MT

            assert (lay, B) == (tracks.lay, tracks.B)
            self.track_id, self.widths = tracks.track_id, tracks.widths
            self.s = s = MT.solver(tracks, build or BUILD)
            self.P = MT.oracle_problem(s.data, lay)
            self.x0, self.yref, self.yref_e = MT.start(s, tracks)
        self.data = s.data
        s.set_x0_sensitivities(sens_mode)
        for _ in range(solves):
            self.xbar, self.ubar = s.get_x(), s.get_u()
            self.st = s.solve()
        self.ok = (self.st == 0) | (self.st == 2)
        self.nc, self.z, self.Z = SC.soft_arrays(s.data, lay)
        self.o = o = _outputs(s, alat=True)
        self.lam, self.slk = (_widen(o["lam"], o["lam_a"]), _widen(o["slk"], o["slk_a"])) if lay.alat else (o["lam"], o["slk"])
        self.lin = s.get_linearization()

    def qp(self, i):
        N, o = self.N, self.o
        A, Bm, b = self.lin
        args = (self.xbar[i], self.ubar[i], self.x0[i], self.yref[i], self.yref_e[i])
        ref = self.P.build_qp(*args, track_id=int(self.track_id[i])) if self.lay.path else None
        qp = L.assemble_qp(self.data, *args, A[i], Bm[i], b[i], nonlinear=ref)
        dz = np.zeros((N + 1, 10)); dz[:, :8] = o["x"][i] - self.xbar[i]; dz[:N, 8:] = o["u"][i] - self.ubar[i]
        return qp, dz, self.lam[i], self.slk[i]

    def bound_mag(self, i):
        """(N+1, 2 nc): the sum of the absolute terms of (bound - the row's value at xbar) as k_slack_fold forms it from the raw bound
        and the terms of the row (the a_lat row's value counts as one term)."""
        d, N, nc, lay = self.data, self.N, self.nc, self.lay
        xb, ub = self.xbar[i], self.ubar[i]
        raw = np.zeros((N + 1, 2 * nc)); vm = np.zeros((N + 1, nc))
        raw[:, :8], raw[:, nc:nc + 8], vm[:, :8] = d.lbx, d.ubx, np.abs(xb)
        raw[:N, 8:10], raw[:N, nc + 8:nc + 10], vm[:N, 8:10] = d.lbu, d.ubu, np.abs(ub)
        raw[:N, 10:12], raw[:N, nc + 10:nc + 12] = d.lg, d.ug
        vm[:N, 10:12] = np.einsum("kij,kj->ki", np.abs(d.C), np.abs(xb[:N])) + np.einsum("kij,kj->ki", np.abs(d.D), np.abs(ub))
        if lay.path:
            raw[:, 12:14], raw[:, nc + 12:nc + 14] = np.asarray(d.lh)[:2], np.asarray(d.uh)[:2]
            common = np.abs(xb[:, 1]) + 0.5 * d.car_L * np.abs(np.sin(xb[:, 2])) + 0.5 * d.car_W * np.abs(np.cos(xb[:, 2]))
            vm[:, 12:14] = common[:, None] + self.widths[self.track_id[i]][None]
        if lay.alat:
            raw[:, 14], raw[:, nc + 14] = d.alat_lb, d.alat_ub
            du14 = self.P.build_qp(xb, ub, self.x0[i], self.yref[i], self.yref_e[i], track_id=int(self.track_id[i]))["du"][:, 14]
            vm[:, 14] = np.abs(np.where(np.isfinite(du14), d.alat_ub - du14, 0.0))
        return np.abs(raw) + np.concatenate([vm, vm], 1)

    def gy(self, i):
        t = int(self.track_id[i])
        return R.gy_tables(lambda yr, yre: self.P.build_qp(self.xbar[i], self.ubar[i], self.x0[i], yr, yre, track_id=t)["g"], self.yref[i], self.yref_e[i])


def _refined(M, rhs):
    return _solve_refined(M, rhs[:, None])[:, 0]


@pytest.mark.parametrize("name,B,build", [(n, B, None) for n in LAYOUTS for B in (3, 67)] + [("path_soft_both_sides", 67, "ilp")])
def test_fold_alone(track, name, B, build):
    """ihm2mpc_eval_adjoint_sensitivities_s with zero stage seeds and random seed_s / seed_sa, one seed (explicit zeros) and eight (NULL
    stage seeds: the entry zero-fills), against ihm2mpc_eval_adjoint_sensitivities_w fed the host's fold, to FOLD_TOL of the largest
    entry of each output, instance and seed.  The fold is not empty, and entries of sides without a slack are ignored (they are NaN)."""
    lay = LAYOUTS[name]
    c = _Solved(track, lay, B, 900 + lay.seed, build)
    s, N = c.s, c.N
    assert c.ok.mean() > 0.5, c.st
    qps = {i: c.qp(i) for i in np.flatnonzero(c.ok)}
    for n_seeds in (1, 8):
        rng = np.random.default_rng(5 + n_seeds)
        seed_s, seed_sa = rng.standard_normal((B, n_seeds, N + 1, 28)), rng.standard_normal((B, n_seeds, N + 1, 2))
        fx, fu = np.zeros((B, n_seeds, N + 1, 8)), np.zeros((B, n_seeds, N, 2))
        live = np.zeros((N + 1, 2 * c.nc), dtype=bool)
        for i, (qp, dz, lam, sl) in qps.items():
            for k, col, _, _, _ in SR._soft_sides(qp, dz, lam, sl, c.z, c.Z, SR.TAU):
                live[k, col] = True
            for q in range(n_seeds):
                sd = _widen(seed_s[i, q], seed_sa[i, q]) if lay.alat else seed_s[i, q]
                f = SR.fold(qp, dz, lam, sl, c.z, c.Z, sd)
                fx[i, q], fu[i, q] = f[:, :8], f[:N, 8:]
        assert np.abs(fx).max() > 0.0 and (not lay.alat or live[:, [14, 29]].any()), "the fold was not exercised"
        # a side that carries a slack on no instance: its seed must not be read
        dead = ~live
        d28 = np.concatenate([dead[:, :14], dead[:, c.nc:c.nc + 14]], 1)
        seed_s[:, :, d28] = np.nan
        if lay.alat:
            seed_sa[:, :, np.stack([dead[:, 14], dead[:, 29]], 1)] = np.nan
        zero = (np.zeros_like(fx), np.zeros_like(fu)) if n_seeds == 1 else (None, None)
        got = s.eval_adjoint_slack_sensitivities(*zero, seed_s, seed_sa)
        want = s.eval_adjoint_weight_sensitivities(fx, fu)
        worst = 0.0
        for k in want:
            assert got[k].shape == want[k].shape and np.isnan(got[k][~c.ok]).all() and np.isfinite(got[k][c.ok]).all(), k
            ax = tuple(range(2, want[k].ndim))
            worst = max(worst, float((np.abs(got[k][c.ok] - want[k][c.ok]).max(ax) / np.abs(want[k][c.ok]).max(ax)).max()))
        print(f"SLACK-SEED fold {name} B {B} seeds {n_seeds} {build or BUILD}: worst {worst:.2e} of the largest entry")
        assert worst <= FOLD_TOL, worst
    s.free()


@pytest.mark.parametrize("B", [3, 67])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_cost_seeds_and_totals(track, name, B):
    """ihm2mpc_eval_cost_gradient_soft after one solve.  The returned seeds against cost_ref.seeds + fold of dJ_slack/ds = z + Z s, to
    VAL_TOL of the magnitude rounding errors are relative to -- the sum of the absolute terms, a term of the fold weighted by the
    condition of its gamma (slack_seed_ref.fold; with |c gamma r| alone the worst instance of path_soft_both_sides at B = 67 stood at
    1.33 bounds: gamma is formed from two differences that cancel) -- (unsolved instances: the unfolded seeds); the cost is get_cost()'s; grad_x0 is, bit for bit,
    the _w entry's on the returned seeds; and the five totals against cost_ref.total_gradient on the dense system that keeps every slack
    as a variable (slack_seed_ref.adjoint_with_slacks, refined), at the GPU's own iterate, to REF_TOL of the largest entry of the
    magnitude (a subset of the solved instances)."""
    lay = LAYOUTS[name]
    c = _Solved(track, lay, B, 900 + lay.seed)
    s, N, o, data = c.s, c.N, c.o, c.data
    assert c.ok.mean() > 0.5, c.st
    g = s.eval_cost_gradient_soft()
    np.testing.assert_array_equal(g["cost"], s.get_cost())
    a = s.eval_adjoint_weight_sensitivities(g["seed_x"], g["seed_u"])
    np.testing.assert_array_equal(g["x0"], a["x0"])
    for k in GRADS:
        assert np.isnan(g[k][~c.ok]).all() and np.isfinite(g[k][c.ok]).all(), k
    assert np.isfinite(g["seed_x"]).all() and np.isfinite(g["seed_u"]).all()
    np.testing.assert_array_equal(g["W"], np.swapaxes(g["W"], -1, -2))
    worst_seed = folded = 0.0
    for i in range(B):
        sd, smag = CR.seeds(data, o["x"][i], o["u"][i], c.yref[i], c.yref_e[i])
        if c.ok[i]:
            qp, dz, lam, sl = c.qp(i)
            f, fmag = SR.fold(qp, dz, lam, sl, c.z, c.Z, SR.cost_slack_seed(sl, c.z, c.Z), with_mag=True, bound_mag=c.bound_mag(i))
            folded = max(folded, float(np.abs(f).max()))
            sd, smag = sd + f, smag + fmag
        got = np.concatenate([g["seed_x"][i], np.concatenate([g["seed_u"][i], np.zeros((1, 2))])], 1)
        err, bound = np.abs(got - sd), VAL_TOL * smag
        assert (smag[err > 0] > 0).all()
        worst_seed = max(worst_seed, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))))
    assert folded > 0.0, "no slack is in use: the fold was not exercised"
    worst = 0.0
    for i in _subset(c.ok)[:4]:
        qp, dz, lam, sl = c.qp(i)
        Gy, Gye = c.gy(i)
        kept = {}

        def adjoint(qp_, dz_, lam_, sl_, z_, Z_, sd, kept=kept):
            kept["zeta"], nu0 = SR.adjoint_with_slacks(qp_, dz_, lam_, sl_, z_, Z_, sd, SR.cost_slack_seed(sl_, z_, Z_), solve=_refined)
            return kept["zeta"], nu0

        t = CR.total_gradient(data, qp, dz, lam, sl, c.z, c.Z, Gy, Gye, o["x"][i], o["u"][i], c.yref[i], c.yref_e[i], adjoint=adjoint)
        zeta = kept["zeta"]
        zp = np.zeros((N + 1, 10)); zp[:, :8] = o["x"][i]; zp[:N, 8:] = o["u"][i]
        _, mags = RW.stage_terms(data, zeta, zp, c.yref[i])
        eN = np.abs(zp[N, :8] - c.yref_e[i])
        mag = dict(W=0.5 * (mags.sum(0) + mags.sum(0).T) + t["explicit"]["mag"]["W"],
                   W_e=0.5 * (np.outer(np.abs(zeta[N, :8]), eN) + np.outer(eN, np.abs(zeta[N, :8]))) + t["explicit"]["mag"]["W_e"],
                   x0=np.abs(t["x0"]), yref=np.abs(t["adj"]["yref"]) + t["explicit"]["mag"]["yref"],
                   yref_e=np.abs(t["adj"]["yref_e"]) + t["explicit"]["mag"]["yref_e"])
        for k in GRADS:
            worst = max(worst, float(np.abs(g[k][i] - t[k]).max() / mag[k].max()))
    print(f"SLACK-SEED cost {name} B {B}: seeds {worst_seed:.2e} of the bound, largest folded entry {folded:.2e}, totals against the dense "
          f"reference {worst:.2e}")
    assert worst_seed <= 1.0, worst_seed
    assert worst <= REF_TOL, worst
    s.free()


@pytest.mark.parametrize("name", list(SC.CASES))
def test_gradient_against_whole_solves(track, name):
    """<eval_cost_gradient_soft, direction> against central differences of get_cost() over re-solves from the restored start, on the
    soft layouts, instances, directions and step lengths of tests/slack_seed_cases.py / tests/cost_cases.py, with the measure and the
    acceptance profile of tests/test_oracle_slack_seeds.py (which shows the NumPy reference to meet it on these inputs, and to fail it
    without the fold)."""
    from ihm2_amd.solver import BatchedOcpSolver
    from oracle import oracle as orc
    from test_gpu_configs import _build

    lay, B, seed = SC.CASES[name]
    N = lay.N
    ocp = L.make_ocp(lay)
    ocp.solver_options.qp_tol = C.QP_TOL
    ocp.solver_options.qp_solver_iter_max = 200
    with _build(BUILD):
        s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
    L.apply(s.data, lay)
    s._push_weights(); s._push_bounds()
    data = s.data
    x0, yref, yref_e = C.start(track, B, seed, N)
    s.set_x0(x0); s.init_guess()
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
    s.set_x0_sensitivities(1)
    x, u = s.get_x(), s.get_u()
    pi, lam = s.get_multipliers(); slk = s.get_slacks()
    W0, We0 = np.asarray(data.W[0], dtype=np.float64), np.asarray(data.W_e, dtype=np.float64)
    dirs = C.directions(name, B, N, W0, We0)

    def solve_at(d, step):
        s.set_weights(W0 + step * d["W"], We0 + step * d["W_e"])
        s.set_x0(x0 + step * d["x0"]); s.set_yref(yref + step * d["yref"]); s.set_yref_e(yref_e + step * d["yref_e"])
        s.set_x(x); s.set_u(u); s.set_multipliers(pi, lam); s.set_slacks(slk)
        return s.solve()

    st = solve_at(dirs["x0"], 0.0)
    g = s.eval_cost_gradient_soft()
    slack_cost = s.get_slack_cost()
    o = _outputs(s)
    ok = st == 0
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    A, Bm, b = s.get_linearization()
    z, Z = L.soft_arrays(data)
    free = {k: np.zeros_like(g[k]) for k in GRADS}
    for i in np.flatnonzero(ok):        # the scale of an unconstrained reaction (dense, at the GPU's iterate); weakly active instances have no derivative
        ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i]) if lay.path else None
        qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref)
        dz = np.zeros((N + 1, 10)); dz[:, :8] = o["x"][i] - x[i]; dz[:N, 8:] = o["u"][i] - u[i]
        if S.weakly_active(qp, dz, o["lam"][i], sl=o["slk"][i], soft_z=z, soft_Z=Z):
            ok[i] = False
            continue
        Gy, Gye = R.gy_tables(lambda yr, yre, i=i: P.build_qp(x[i], u[i], x0[i], yr, yre)["g"], yref[i], yref_e[i])
        t = CR.total_gradient(data, qp, dz, 0.0 * o["lam"][i], o["slk"][i], z, Z, Gy, Gye, o["x"][i], o["u"][i], yref[i], yref_e[i])
        for k in GRADS:
            free[k][i] = t[k]
    errs = []
    for dname in C.DIRECTIONS:
        d, eps = dirs[dname], C.EPS[dname]
        J = []
        for sign in (1.0, -1.0):
            ok &= solve_at(d, sign * eps) == 0
            J.append(s.get_cost())
        fd = (J[0] - J[1]) / (2 * eps)
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.abs(C.contract(g, d) - fd) / np.maximum(np.abs(fd), np.abs(C.contract(free, d)))
        errs.append(e)
    keep = np.flatnonzero(ok)
    assert keep.size >= 0.75 * B, (keep.size, B)
    for dname, e in zip(C.DIRECTIONS, errs):
        (med, s5, s3), _ = C.profile(e[keep])
        print(f"SLACK-SEED-FD {name} {dname}: median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {e[keep].max():.2e}")
    allerr = np.concatenate([e[keep] for e in errs])
    (med, s5, s3), met = C.profile(allerr)
    used = float(np.mean(slack_cost[keep] > SC.SLACK_COST_MIN))
    print(f"SLACK-SEED-FD {name}: kept {keep.size} of {B}, slack cost in use {used:.2f}, median {med:.2e} share<=1e-5 {s5:.3f} "
          f"share<=1e-3 {s3:.3f} max {allerr.max():.2e}")
    assert met, (med, s5, s3)
    assert used >= 0.5, used
    s.free()


def test_same_bits_without_slacks(track):
    """On an all-hard table eval_cost_gradient_soft() is eval_cost_gradient(); on any table _s without slack seeds is _w."""
    hard = L.Layout("cost_hard", N=10)
    s = _solver(track, hard, 67)
    _start(s, track, 67, 55)
    s.set_x0_sensitivities(1)
    assert (s.solve() == 0).mean() > 0.5
    g0, g1 = s.eval_cost_gradient(), s.eval_cost_gradient_soft()
    for k in g0:
        np.testing.assert_array_equal(g1[k], g0[k], err_msg=k)
    rng = np.random.default_rng(2)          # slack seeds on a table without slacks: ignored
    w = s.eval_adjoint_weight_sensitivities(g0["seed_x"], g0["seed_u"])
    v = s.eval_adjoint_slack_sensitivities(g0["seed_x"], g0["seed_u"], rng.standard_normal((67, 11, 28)), rng.standard_normal((67, 11, 2)))
    for k in w:
        np.testing.assert_array_equal(v[k], w[k], err_msg=k)
    s.free()
    for lay in (hard, LAYOUTS["alat_soft"]):
        s = _solver(track, lay, 5)
        _start(s, track, 5, 56)
        s.set_x0_sensitivities(1)
        s.solve()
        seed_x, seed_u = _seeds(5, 3, lay.N, 7)
        for sx, su in ((seed_x, seed_u), (seed_x, None), (None, seed_u), (None, None)):
            w, v = s.eval_adjoint_weight_sensitivities(sx, su), s.eval_adjoint_slack_sensitivities(sx, su)
            for k in w:
                np.testing.assert_array_equal(v[k], w[k], err_msg=k)
        s.free()


@pytest.mark.parametrize("name,B", [("cost_soft", 3), ("alat_soft", 67)])
def test_nothing_else_moves(track, name, B):
    """With and without the two new calls between them: every getter, a following adjoint evaluation with fixed seeds and the next step
    agree bit for bit; two calls in a row return the same bits; all outputs NULL is accepted."""
    from ihm2_amd import _lib

    lay = LAYOUTS[name]
    N = lay.N
    seed_x, seed_u = _seeds(B, 3, N, 7)
    rng = np.random.default_rng(8)
    seed_s, seed_sa = rng.standard_normal((B, 3, N + 1, 28)), rng.standard_normal((B, 3, N + 1, 2))
    res = []
    for with_calls in (False, True):
        s = _solver(track, lay, B)
        _start(s, track, B, 55)
        s.set_x0_sensitivities(2)
        st = s.solve()
        assert np.isin(st, (0, 2)).mean() > 0.5
        if with_calls:
            g1, a1 = s.eval_cost_gradient_soft(), s.eval_adjoint_slack_sensitivities(seed_x, seed_u, seed_s, seed_sa)
            g2, a2 = s.eval_cost_gradient_soft(), s.eval_adjoint_slack_sensitivities(seed_x, seed_u, seed_s, seed_sa)
            for k in g1:
                np.testing.assert_array_equal(g2[k], g1[k], err_msg=k)
            for k in a1:
                np.testing.assert_array_equal(a2[k], a1[k], err_msg=k)
            _lib.check(s.lib.ihm2mpc_eval_cost_gradient_soft(s._h, *[None] * 8))
            ptr = lambda v: v.ctypes.data_as(_lib.c_double_p)  # noqa: E731
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_s(s._h, 3, None, None, ptr(seed_s), ptr(seed_sa), *[None] * 5))
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_s(s._h, 2, *[None] * 9))
        out = dict(_outputs(s, alat=True), u0=s.get_u0(), x0=s.get_x0(), cost=s.get_cost(stagewise=True))
        out["sens_x"], out["sens_u"] = s.get_x0_sensitivities()
        out.update({"adjw_" + k: v for k, v in s.eval_adjoint_weight_sensitivities(seed_x, seed_u).items()})
        out.update({"adj_" + k: v for k, v in s.eval_adjoint_sensitivities(seed_x, seed_u).items()})
        if with_calls:
            s.eval_cost_gradient_soft()
            s.eval_adjoint_slack_sensitivities(None, None, seed_s, None)
        s.step(40.0, model=0, M_sim=25)
        out.update({"next_" + k: v for k, v in _outputs(s, alat=True).items()}, next_u0=s.get_u0(), next_x0=s.get_x0())
        res.append(out)
        s.free()
    for k in res[0]:
        np.testing.assert_array_equal(res[1][k], res[0][k], err_msg=k)


def _refused(s, call, pattern):
    """call() raises, and the handle's own library (which need not be the one _lib.check reads the text from) gives the reason."""
    import re

    from ihm2_amd._lib import Ihm2mpcError

    with pytest.raises(Ihm2mpcError):
        call()
    text = s.lib.ihm2mpc_last_error().decode()
    assert re.search(pattern, text), (pattern, text)


def test_refusals_and_nan_rows(track):
    B = 8
    lay = L.Layout("slack_soft_vx", N=10, soft=1.0, soft_rows=(3,), soft_kind="both", seed=6)     # the box on n stays hard
    rng = np.random.default_rng(4)
    seed_s = rng.standard_normal((B, 11, 28))
    from ihm2_amd import _lib
    from test_gpu_cost import _solver as _solver_with_options

    sq = _solver_with_options(track, lay, B, nlp_solver_type="SQP", nlp_solver_max_iter=2)
    for call in (sq.eval_cost_gradient_soft, lambda: sq.eval_adjoint_slack_sensitivities(seed_s=seed_s)):
        _refused(sq, call, "adjoint sensitivities are implemented for SQP_RTI")
    sq.free()
    s = _solver(track, lay, B)
    calls = (s.eval_cost_gradient_soft, lambda: s.eval_adjoint_slack_sensitivities(seed_s=seed_s))
    for call in calls:
        _refused(s, call, "x0 sensitivities are off")
    s.set_x0_sensitivities(1)
    for call in calls:
        _refused(s, call, "no solve has run")
    _refused(s, lambda: _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_s(s._h, 1, *[None] * 9)), "needs n_seeds = 2")
    x0 = sample_x0(track, B, seed=9)
    x0[0, 1] = 5.0              # far outside the hard box on n: an infeasible QP, reported by its status (tests/test_gpu_adjoint.py's instance)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    assert st[0] not in (0, 2) and np.isin(st[1:], (0, 2)).mean() > 0.5, st
    ok = (st == 0) | (st == 2)
    g = s.eval_cost_gradient_soft()
    a = s.eval_adjoint_slack_sensitivities(seed_s=seed_s)
    for k in GRADS:
        assert np.isnan(g[k][~ok]).all() and np.isfinite(g[k][ok]).all(), k
        assert np.isnan(a[k][~ok]).all() and np.isfinite(a[k][ok]).all(), k
    for k in ("cost", "seed_x", "seed_u"):
        assert np.isfinite(g[k]).all(), k
    assert s.get_slack_cost()[ok].max() > 0.0
    # the batch-mates' bits do not depend on the failed instance: the same instances alone
    t = _solver(track, lay, B - 1)
    t.set_x0_sensitivities(1)
    t.set_x0(x0[1:]); t.init_guess(); t.prepare_step(40.0)
    np.testing.assert_array_equal(t.solve(), st[1:])
    gt, at = t.eval_cost_gradient_soft(), t.eval_adjoint_slack_sensitivities(seed_s=seed_s[1:])
    for k in g:
        np.testing.assert_array_equal(gt[k], g[k][1:], err_msg=k)
    for k in a:
        np.testing.assert_array_equal(at[k], a[k][1:], err_msg=k)
    t.free()
    s.run_steps(40.0, 2, model=0, M_sim=25)
    for call in calls:
        _refused(s, call, "ihm2mpc_run_steps, which computes no x0 sensitivities")
    s.prepare_step(40.0)
    s.solve()
    s.eval_cost_gradient_soft()         # readable again after a solve
    _refused(s, lambda: s.eval_cost_gradient(), "defined for all-hard constraint tables.*carry no seed")  # the old entry keeps its refusal
    s.free()


def test_instance_bounds(track):
    """Per-instance bound values on a soft table (the kernel's sl_bs): a batch of three tunings gives, bit for bit, what three batches of
    one tuning each give."""
    lay = LAYOUTS["cost_soft"]
    B, N, facs = 9, lay.N, (1.0, 0.9, 0.8)
    assign = np.arange(B) % 3
    arr = L.make_arrays(lay)
    var = [{n: np.where(np.abs(arr[n]) < L.BIG, arr[n] * f, arr[n]) for n in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")} for f in facs]
    x0 = sample_x0(track, B, seed=4343)
    rng = np.random.default_rng(3)
    seed_s = rng.standard_normal((B, 2, N + 1, 28))

    def run(s, rows):
        s.set_x0_sensitivities(1)
        s.set_x0(x0[rows]); s.init_guess(); s.prepare_step(40.0)
        st = s.solve()
        g, a = s.eval_cost_gradient_soft(), s.eval_adjoint_slack_sensitivities(seed_s=seed_s[rows])
        return [st, s.get_slack_cost()] + list(g.values()) + list(a.values())

    s = _solver(track, lay, B)
    s.set_instance_bounds(**{n: np.stack([var[a][n] for a in assign]) for n in var[0]})
    mixed = run(s, np.arange(B))
    s.free()
    assert np.isin(mixed[0], (0, 2)).mean() > 0.5 and mixed[1].max() > 0.0
    for j in range(3):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, lay, rows.size)
        for n, v in var[j].items():
            setattr(h.data, n, v)
        h._push_bounds()
        for m, hh in zip(mixed, run(h, rows)):
            np.testing.assert_array_equal(m[rows], hh)
        h.free()
    assert not np.array_equal(mixed[3][0], mixed[3][1])       # the tunings differ in dJ/dx0


def test_python_layers(track):
    lay = LAYOUTS["cost_soft"]
    B, N = 5, lay.N
    s = _solver(track, lay, B)
    _start(s, track, B, 3)
    s.set_x0_sensitivities(1)
    st = s.solve()
    assert st[2] in (0, 2)
    g = s.eval_cost_gradient_soft()
    assert {k: v.shape for k, v in g.items()} == dict(cost=(B,), x0=(B, 8), yref=(B, N, 12), yref_e=(B, 8), W=(B, 12, 12), W_e=(B, 8, 8),
                                                      seed_x=(B, N + 1, 8), seed_u=(B, N, 2))
    a = s.eval_adjoint_slack_sensitivities(seed_sa=np.zeros((B, N + 1, 2)), seed_s=np.ones((B, N + 1, 28)))
    assert {k: v.shape for k, v in a.items()} == dict(x0=(B, 8), yref=(B, N, 12), yref_e=(B, 8), W=(B, 12, 12), W_e=(B, 8, 8))
    v = s[2]
    np.testing.assert_array_equal(v.eval_and_get_optimal_value_gradient_soft(), g["x0"][2])
    with pytest.raises(Exception, match="no p_global"):
        v.eval_and_get_optimal_value_gradient_soft("p_global")
    _refused(s, v.eval_and_get_optimal_value_gradient, "defined for all-hard constraint tables")
    s.free()


def test_workspace_poison():
    """A fresh child process, started with IHM2MPC_POISON_WORKSPACE=1: both new entries give the bits of a clean twin
    (tests/slack_seed_poison_child.py; the manner of tests/test_gpu_cost.py::test_workspace_poison)."""
    env = dict(os.environ, IHM2MPC_POISON_WORKSPACE="1")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "slack_seed_poison_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "slack seed poison ok" in r.stdout, r.stdout[-2000:]
