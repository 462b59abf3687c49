"""Adjoint gradients in the slack penalties on the GPU (kernels_penaltygrad.hip: k_penalty_grad; kernels_adj.hip: k_adj<true, true>;
ihm2mpc_eval_adjoint_sensitivities_p, ihm2mpc_eval_cost_gradient_penalties): the kernels against the dense system that keeps every slack
as a variable, the closed form alone on the GPU's own zeta, bit-identity with the entries they extend, the cost's totals, central
differences over whole re-solves with the penalties moved (tests/penalty_grad_cases.py; tests/test_oracle_penalty_grad.py shows the
NumPy reference to meet the same condition), bit-identity of everything else, refusals and NaN rows, the workspace poison.

The model is tests/test_gpu_slack_seeds.py: its layouts, its _Solved (the host's view of every instance's QP at the GPU's own iterate)
and B in {3, 67}.  IHM2MPC_TEST_BUILD=ilp runs the module's handles on libihm2mpc_ilp.so; test_kernel_against_the_host runs one layout
in both builds in any case.

Tolerances.  REF_TOL (1e-6 of the largest entry, against the refined dense solve) and ROUND_TOL (1e-9, a composition of roundings) are
those of tests/test_gpu_adjoint_weights.py.  zeta_s is the quotient gamma (c t / lam - sgn r zeta_k) with gamma = lam / (t rho + lam) <= 1,
so its errors are relative to gamma (|r zeta_k| + |c t / lam|), the sum of its absolute terms (penalty_grad_ref.closed_form), and the
bound is taken of the instance's largest such sum -- not of the largest |r zeta_k| + |c t / lam| itself, which is never smaller and
which an inactive side, with lam of the order of the barrier parameter, drives to 1e10 and more: 1e-6 of that would admit anything.
dL/dZ = -s zeta_s inherits the errors times the slack, so its bound carries the instance's largest slack (capped at 1: never wider
than the bound of dL/dz)."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import sample_x0

import cost_cases as C
import cost_ref as CR
import layouts as L
import penalty_grad_cases as PC
import penalty_grad_ref as PR
import sens_ref as S
import slack_seed_cases as SC
import slack_seed_ref as SR
from test_gpu_adjoint import _seeds
from test_gpu_adjoint_weights import REF_TOL, ROUND_TOL, _solve_refined
from test_gpu_qp_layouts import _start
from test_gpu_sensitivity import _outputs, _subset
from test_gpu_slack_seeds import BUILD, LAYOUTS, _refused, _Solved, _solver

pytestmark = pytest.mark.gpu

PEN = ("soft_z", "soft_Z", "alat_soft_z", "alat_soft_Z")
ADJ = ("x0", "yref", "yref_e", "W", "W_e")
PARAMS = [(n, B, None) for n in LAYOUTS for B in (3, 67)] + [("path_soft_both_sides", 67, "ilp")]


def _refined(M, rhs):
    return _solve_refined(M, rhs[:, None])[:, 0]


def _wide(c, a28, a2):
    """(.., 2 nc) of the host's references from the C ABI's (.., 28) and (.., 2)."""
    from test_gpu_qp_layouts import _widen

    return _widen(a28, a2) if c.lay.alat else a28


_CASES = {}


def _case(track, name, B, build):
    if (name, B, build) not in _CASES:
        _CASES[name, B, build] = _solve_case(track, name, B, build)
    return _CASES[name, B, build]


def _solve_case(track, name, B, build):
    """One solve of the layout and ihm2mpc_eval_adjoint_sensitivities_p with 1 and 8 random seeds on the stages and the slacks, shared
    by the tests below (read only): the solved case, the host's QPs of the solved instances, per n_seeds (seed_z, seed_s wide, outputs).
    Seeds of sides that carry a slack on no instance are NaN: they must not be read."""
    lay = LAYOUTS[name]
    c = _Solved(track, lay, B, 900 + lay.seed, build)
    N = c.N
    assert c.ok.mean() > 0.5, c.st
    qps = {int(i): c.qp(i) for i in np.flatnonzero(c.ok)}
    live = np.zeros((B, N + 1, 2 * c.nc), dtype=bool)
    for i, (qp, dz, lam, sl) in qps.items():
        for k, col, _, _, _ in SR._soft_sides(qp, dz, lam, sl, c.z, c.Z, SR.TAU):
            live[i, k, col] = True
    runs = {}
    for n_seeds in (1, 8):
        rng = np.random.default_rng(5 + n_seeds)
        seed_x, seed_u = _seeds(B, n_seeds, N, 30 + n_seeds)
        seed_s, seed_sa = rng.standard_normal((B, n_seeds, N + 1, 28)), rng.standard_normal((B, n_seeds, N + 1, 2))
        dead = ~live.any(0)
        seed_s[:, :, np.concatenate([dead[:, :14], dead[:, c.nc:c.nc + 14]], 1)] = np.nan
        seed_sa[:, :, np.stack([dead[:, 14], dead[:, c.nc + 14]], 1) if lay.alat else np.ones((N + 1, 2), dtype=bool)] = np.nan
        got = c.s.eval_adjoint_penalty_sensitivities(seed_x, seed_u, seed_s, seed_sa)
        ref_s = c.s.eval_adjoint_slack_sensitivities(seed_x, seed_u, seed_s, seed_sa)
        seed_z = np.zeros((B, n_seeds, N + 1, 10)); seed_z[..., :8] = seed_x; seed_z[:, :, :N, 8:] = seed_u
        runs[n_seeds] = (seed_z, np.nan_to_num(_wide(c, seed_s, seed_sa)), got, ref_s)
    c.s.free()
    return c, qps, live, runs


def _got_wide(c, got, i, q):
    return _wide(c, got["soft_z"][i, q], got["alat_soft_z"][i, q]), _wide(c, got["soft_Z"][i, q], got["alat_soft_Z"][i, q])


@pytest.mark.parametrize("name,B,build", PARAMS)
def test_kernel_against_the_host(track, name, B, build):
    """The four gradients and zeta against penalty_grad_ref on the dense system (refined) at the GPU's own iterate, 1 and 8 seeds: zeta
    to REF_TOL of the instance's largest entry, the gradients to REF_TOL of the instance's largest gamma (|r zeta_k| + |c t / lam|) (a subset of
    the solved instances and, of eight seeds, the first and the last).  Something is live on every layout (alat_soft: on the a_lat
    sides); entries of sides without a slack are exactly 0; unsolved instances are NaN."""
    c, qps, live, runs = _case(track, name, B, build)
    worst_zeta = worst_g = 0.0
    for n_seeds, (seed_z, seed_s, got, _) in runs.items():
        for k in PEN + ("zeta",):
            assert np.isnan(got[k][~c.ok]).all() and np.isfinite(got[k][c.ok]).all(), k
        anything = alat_live = False
        for i in qps:
            for q in range(n_seeds):
                gz, gZ = _got_wide(c, got, i, q)
                assert not gz[~live[i]].any() and not gZ[~live[i]].any(), "a side without a slack has a gradient"
                anything |= bool(gz[live[i]].any())
                alat_live |= c.lay.alat and bool(gz[:, [14, c.nc + 14]].any())
        assert anything and (not c.lay.alat or alat_live), "no gradient is live"
        for i in _subset(c.ok)[:3]:
            qp, dz, lam, sl = qps[int(i)]
            for q in sorted({0, n_seeds - 1}):
                zs, zeta, _ = PR.zeta_s(qp, dz, lam, sl, c.z, c.Z, seed_z[i, q], seed_s[i, q], solve=_refined)
                _, mag = PR.closed_form(qp, dz, lam, sl, c.z, c.Z, zeta, seed_s[i, q])
                wz, wZ = PR.gradients(zs, sl)
                gz, gZ = _got_wide(c, got, i, q)
                worst_zeta = max(worst_zeta, float(np.abs(got["zeta"][i, q] - zeta).max() / np.abs(zeta).max()))
                scale = float(mag.max())
                worst_g = max(worst_g, float(np.abs(gz - wz).max() / scale), float(np.abs(gZ - wZ).max() / (scale * min(1.0, sl.max()))))
    print(f"PENALTY-GRAD kernel {name} B {B} {build or BUILD}: zeta {worst_zeta:.2e} of the largest entry, gradients {worst_g:.2e} of the "
          f"largest gamma (|r zeta| + |c t / lam|)")
    assert worst_zeta <= REF_TOL, worst_zeta
    assert worst_g <= REF_TOL, worst_g


@pytest.mark.parametrize("name,B,build", PARAMS)
def test_closed_form_alone(track, name, B, build):
    """The host's closed form fed the GPU's own zeta against the kernel's gradients, every solved instance and seed, to ROUND_TOL of the
    same magnitude: this separates k_penalty_grad from k_adj."""
    c, qps, live, runs = _case(track, name, B, build)
    worst = 0.0
    for n_seeds, (_, seed_s, got, _) in runs.items():
        for i, (qp, dz, lam, sl) in qps.items():
            for q in range(n_seeds):
                zs, mag = PR.closed_form(qp, dz, lam, sl, c.z, c.Z, got["zeta"][i, q], seed_s[i, q])
                wz, wZ = PR.gradients(zs, sl)
                gz, gZ = _got_wide(c, got, i, q)
                scale = float(mag.max())
                worst = max(worst, float(np.abs(gz - wz).max() / scale), float(np.abs(gZ - wZ).max() / (scale * min(1.0, sl.max()))))
    print(f"PENALTY-GRAD closed form {name} B {B} {build or BUILD}: {worst:.2e} of the largest gamma (|r zeta| + |c t / lam|)")
    assert worst <= ROUND_TOL, worst


@pytest.mark.parametrize("name,B,build", PARAMS)
def test_first_five_outputs_are_the_slack_entry_s(track, name, B, build):
    """ihm2mpc_eval_adjoint_sensitivities_p runs k_adj<true, true>, ihm2mpc_eval_adjoint_sensitivities_s k_adj<true>: the five
    gradients they share are the same bits."""
    _, _, _, runs = _case(track, name, B, build)
    for _, _, got, ref_s in runs.values():
        for k in ADJ:
            np.testing.assert_array_equal(got[k], ref_s[k], err_msg=k)


def test_same_bits_and_zeros_without_slacks(track):
    """eval_cost_gradient_penalties is eval_cost_gradient_soft on the outputs they share (a soft table, the a_lat row, an all-hard
    table); without slack seeds _p is _w; on an all-hard table the four new outputs are exact zeros."""
    hard = L.Layout("cost_hard", N=10)
    for lay, B in ((LAYOUTS["cost_soft"], 67), (LAYOUTS["alat_soft"], 5), (hard, 67)):
        s = _solver(track, lay, B)
        _start(s, track, B, 55)
        s.set_x0_sensitivities(1)
        st = s.solve()
        ok = np.isin(st, (0, 2))
        assert ok.mean() > 0.5
        g0, g1 = s.eval_cost_gradient_soft(), s.eval_cost_gradient_penalties()
        for k in g0:
            np.testing.assert_array_equal(g1[k], g0[k], err_msg=k)
        seed_x, seed_u = _seeds(B, 3, lay.N, 7)
        for sx, su in ((seed_x, seed_u), (seed_x, None), (None, seed_u), (None, None)):
            w, v = s.eval_adjoint_weight_sensitivities(sx, su), s.eval_adjoint_penalty_sensitivities(sx, su)
            for k in w:
                np.testing.assert_array_equal(v[k], w[k], err_msg=k)
            assert np.isfinite(v["zeta"][ok]).all() and np.isnan(v["zeta"][~ok]).all()
            if lay is hard:
                for k in PEN:
                    assert not v[k][ok].any() and not g1[k][ok].any() and np.isnan(v[k][~ok]).all() and np.isnan(g1[k][~ok]).all(), k
        d = s.du0_dsoft()
        v = s.eval_adjoint_penalty_sensitivities()
        for k in PEN:
            np.testing.assert_array_equal(d[k], v[k], err_msg=k)
        s.free()


@pytest.mark.parametrize("B", [3, 67])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_cost_totals(track, name, B):
    """dJ/dz = s - zeta_s, dJ/dZ = s^2 / 2 - s zeta_s of ihm2mpc_eval_cost_gradient_penalties against the dense system with the cost's
    seeds (cost_ref.seeds on the stages, z + Z s on the slacks), refined, at the GPU's own iterate, to REF_TOL of the instance's largest
    |r zeta_k| + |c t / lam| + s (a subset of the solved instances).  Sides without a slack are exactly 0, unsolved instances NaN."""
    lay = LAYOUTS[name]
    c = _Solved(track, lay, B, 900 + lay.seed)
    assert c.ok.mean() > 0.5, c.st
    g = c.s.eval_cost_gradient_penalties()
    c.s.free()
    for k in PEN:
        assert np.isnan(g[k][~c.ok]).all() and np.isfinite(g[k][c.ok]).all(), k
    gw = {k: v[:, None] for k, v in g.items() if k in PEN}
    worst, largest = 0.0, 0.0
    for i in _subset(c.ok)[:4]:
        qp, dz, lam, sl = c.qp(i)
        sd, _ = CR.seeds(c.data, c.o["x"][i], c.o["u"][i], c.yref[i], c.yref_e[i])
        cs = SR.cost_slack_seed(sl, c.z, c.Z)
        zs, zeta, _ = PR.zeta_s(qp, dz, lam, sl, c.z, c.Z, sd, cs, solve=_refined)
        _, mag = PR.closed_form(qp, dz, lam, sl, c.z, c.Z, zeta, cs)
        wz, wZ = PR.gradients(zs, sl)
        present = np.concatenate([np.isfinite(qp["dl"]), np.isfinite(qp["du"])], 1)
        ez, eZ = PR.cost_partials(np.where(present, sl, 0.0), c.Z)
        gz, gZ = _got_wide(c, gw, i, 0)
        assert not gz[~(present & (c.Z >= 0.0))].any() and not gZ[~(present & (c.Z >= 0.0))].any()
        scale = float(mag.max() + sl.max())
        worst = max(worst, float(np.abs(gz - (wz + ez)).max() / scale), float(np.abs(gZ - (wZ + eZ)).max() / (scale * min(1.0, sl.max()))))
        largest = max(largest, float(np.abs(gz).max()))
    print(f"PENALTY-GRAD cost {name} B {B}: totals against the dense reference {worst:.2e}, largest dJ/dz {largest:.2e}")
    assert largest > 0.0
    assert worst <= REF_TOL, worst


@pytest.mark.parametrize("name", PC.CASES)
def test_gradient_against_whole_solves(track, name):
    """<eval_adjoint_penalty_sensitivities, direction> for L = <seed, z+> against central differences over re-solves through
    set_soft(z +- eps dz, Z +- eps dZ) from the restored start: the cases, seeds, direction, step, measure and condition of
    tests/penalty_grad_cases.py.  The zero prediction does not meet the condition."""
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
    pi, lam0 = s.get_multipliers(); slk0 = s.get_slacks()
    z, Z = (a.copy() for a in L.soft_arrays(data))
    ddz, ddZ = PC.direction(z, Z)

    def solve_at(dz_, dZ_, step):
        s.set_soft(z + step * dz_, Z + step * dZ_)
        s.set_x(x); s.set_u(u); s.set_multipliers(pi, lam0); s.set_slacks(slk0)
        return s.solve()

    sd = np.stack([PC.seeds(i, N) for i in range(B)])
    ok = solve_at(ddz, ddZ, 0.0) == 0
    g = s.eval_adjoint_penalty_sensitivities(np.ascontiguousarray(sd[..., :8]), np.ascontiguousarray(sd[:, :, :N, 8:]))
    o = _outputs(s)
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    A, Bm, b = s.get_linearization()
    pred = {d: np.zeros((B, PC.N_SEEDS)) for d in PC.DIRECTIONS}
    free = {d: np.zeros((B, PC.N_SEEDS)) for d in PC.DIRECTIONS}
    for i in np.flatnonzero(ok):
        ref = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i]) if lay.path else None
        qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref)
        dz = np.zeros((N + 1, 10)); dz[:, :8] = o["x"][i] - x[i]; dz[:N, 8:] = o["u"][i] - u[i]
        if S.weakly_active(qp, dz, o["lam"][i], sl=o["slk"][i], soft_z=z, soft_Z=Z):
            ok[i] = False
            continue
        for d in PC.DIRECTIONS:
            dzd, dZd = PC.pick(d, ddz, ddZ)
            pred[d][i] = PC.predict(g["soft_z"][i], g["soft_Z"][i], dzd, dZd)
            free[d][i] = PC.free_scale(qp, dz, o["lam"][i], o["slk"][i], z, Z, sd[i], dzd, dZd)
    fd = {}
    for d in PC.DIRECTIONS:
        dzd, dZd = PC.pick(d, ddz, ddZ)
        Lv = []
        for sign in (1.0, -1.0):
            ok &= solve_at(dzd, dZd, sign * PC.EPS) == 0
            Lv.append(np.einsum("bski,bki->bs", sd[..., :8], s.get_x()) + np.einsum("bski,bki->bs", sd[:, :, :N, 8:], s.get_u()))
        fd[d] = (Lv[0] - Lv[1]) / (2 * PC.EPS)
    s.free()
    keep = np.flatnonzero(ok)
    errs = {d: PC.measure(pred[d], fd[d], free[d]) for d in PC.DIRECTIONS}
    zero = {d: PC.measure(0.0 * pred[d], fd[d], free[d]) for d in PC.DIRECTIONS}
    PC.verdict("PENALTY-GRAD-FD", name, errs, zero, keep, B)


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
            g1, a1 = s.eval_cost_gradient_penalties(), s.eval_adjoint_penalty_sensitivities(seed_x, seed_u, seed_s, seed_sa)
            g2, a2 = s.eval_cost_gradient_penalties(), s.eval_adjoint_penalty_sensitivities(seed_x, seed_u, seed_s, seed_sa)
            for k in g1:
                np.testing.assert_array_equal(g2[k], g1[k], err_msg=k)
            for k in a1:
                np.testing.assert_array_equal(a2[k], a1[k], err_msg=k)
            assert any(a1[k][np.isfinite(a1[k])].any() for k in PEN)
            _lib.check(s.lib.ihm2mpc_eval_cost_gradient_penalties(s._h, *[None] * 12))
            ptr = lambda v: v.ctypes.data_as(_lib.c_double_p)  # noqa: E731
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_p(s._h, 3, None, None, ptr(seed_s), ptr(seed_sa), *[None] * 10))
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_p(s._h, 2, *[None] * 14))
        out = dict(_outputs(s, alat=True), u0=s.get_u0(), x0=s.get_x0(), cost=s.get_cost(stagewise=True))
        out["sens_x"], out["sens_u"] = s.get_x0_sensitivities()
        out.update({"adjs_" + k: v for k, v in s.eval_adjoint_slack_sensitivities(seed_x, seed_u, seed_s, seed_sa).items()})
        out.update({"adj_" + k: v for k, v in s.eval_adjoint_sensitivities(seed_x, seed_u).items()})
        out.update({"cost_" + k: v for k, v in s.eval_cost_gradient_soft().items()})
        if with_calls:
            s.eval_cost_gradient_penalties()
            s.eval_adjoint_penalty_sensitivities(None, None, seed_s, None)
        s.step(40.0, model=0, M_sim=25)
        out.update({"next_" + k: v for k, v in _outputs(s, alat=True).items()}, next_u0=s.get_u0(), next_x0=s.get_x0())
        res.append(out)
        s.free()
    for k in res[0]:
        np.testing.assert_array_equal(res[1][k], res[0][k], err_msg=k)


def test_refusals_and_nan_rows(track):
    B = 8
    lay = L.Layout("slack_soft_vx", N=10, soft=1.0, soft_rows=(3,), soft_kind="both", seed=6)     # the box on n stays hard
    rng = np.random.default_rng(4)
    seed_s = rng.standard_normal((B, 11, 28))
    from ihm2_amd import _lib
    from test_gpu_cost import _solver as _solver_with_options

    sq = _solver_with_options(track, lay, B, nlp_solver_type="SQP", nlp_solver_max_iter=2)
    for call in (sq.eval_cost_gradient_penalties, lambda: sq.eval_adjoint_penalty_sensitivities(seed_s=seed_s)):
        _refused(sq, call, "adjoint sensitivities are implemented for SQP_RTI")
    sq.free()
    s = _solver(track, lay, B)
    calls = (s.eval_cost_gradient_penalties, lambda: s.eval_adjoint_penalty_sensitivities(seed_s=seed_s))
    for call in calls:
        _refused(s, call, "x0 sensitivities are off")
    s.set_x0_sensitivities(1)
    for call in calls:
        _refused(s, call, "no solve has run")
    _refused(s, lambda: _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_p(s._h, 1, *[None] * 14)), "needs n_seeds = 2")
    _refused(s, lambda: _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_p(s._h, 9, *[None] * 14)), "takes 1 to 8 seeds")
    x0 = sample_x0(track, B, seed=9)
    x0[0, 1] = 5.0              # far outside the hard box on n: an infeasible QP, reported by its status (tests/test_gpu_adjoint.py's instance)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    assert st[0] not in (0, 2) and np.isin(st[1:], (0, 2)).mean() > 0.5, st
    ok = (st == 0) | (st == 2)
    g = s.eval_cost_gradient_penalties()
    a = s.eval_adjoint_penalty_sensitivities(seed_s=seed_s)
    for k in ADJ + PEN:
        assert np.isnan(g[k][~ok]).all() and np.isfinite(g[k][ok]).all(), k
        assert np.isnan(a[k][~ok]).all() and np.isfinite(a[k][ok]).all(), k
    assert np.isnan(a["zeta"][~ok]).all() and np.isfinite(a["zeta"][ok]).all()
    assert a["soft_z"][ok].any() and g["soft_z"][ok].any()
    # the batch-mates' bits do not depend on the failed instance: the same instances alone
    t = _solver(track, lay, B - 1)
    t.set_x0_sensitivities(1)
    t.set_x0(x0[1:]); t.init_guess(); t.prepare_step(40.0)
    np.testing.assert_array_equal(t.solve(), st[1:])
    gt, at = t.eval_cost_gradient_penalties(), t.eval_adjoint_penalty_sensitivities(seed_s=seed_s[1:])
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
    s.eval_cost_gradient_penalties()         # readable again after a solve
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
        g, a = s.eval_cost_gradient_penalties(), s.eval_adjoint_penalty_sensitivities(seed_s=seed_s[rows])
        return [st] + list(g.values()) + list(a.values())

    s = _solver(track, lay, B)
    s.set_instance_bounds(**{n: np.stack([var[a][n] for a in assign]) for n in var[0]})
    mixed = run(s, np.arange(B))
    s.free()
    assert np.isin(mixed[0], (0, 2)).mean() > 0.5
    for j in range(3):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, lay, rows.size)
        for n, v in var[j].items():
            setattr(h.data, n, v)
        h._push_bounds()
        for m, hh in zip(mixed, run(h, rows)):
            np.testing.assert_array_equal(m[rows], hh)
        h.free()
    gz = mixed[7]               # the cost entry's soft_z
    assert np.nan_to_num(gz).any() and not np.array_equal(gz[0], gz[1])       # the tunings differ in dJ/dz


def test_python_layers(track):
    lay = LAYOUTS["cost_soft"]
    B, N = 5, lay.N
    s = _solver(track, lay, B)
    _start(s, track, B, 3)
    s.set_x0_sensitivities(1)
    st = s.solve()
    assert st[2] in (0, 2)
    pen = dict(soft_z=(N + 1, 28), soft_Z=(N + 1, 28), alat_soft_z=(N + 1, 2), alat_soft_Z=(N + 1, 2))
    g = s.eval_cost_gradient_penalties()
    assert {k: v.shape for k, v in g.items()} == dict(cost=(B,), x0=(B, 8), yref=(B, N, 12), yref_e=(B, 8), W=(B, 12, 12), W_e=(B, 8, 8),
                                                      seed_x=(B, N + 1, 8), seed_u=(B, N, 2), **{k: (B,) + v for k, v in pen.items()})
    adj = dict(x0=(8,), yref=(N, 12), yref_e=(8,), W=(12, 12), W_e=(8, 8), zeta=(N + 1, 10), **pen)
    a = s.eval_adjoint_penalty_sensitivities(seed_sa=np.zeros((B, N + 1, 2)), seed_s=np.ones((B, N + 1, 28)))
    assert {k: v.shape for k, v in a.items()} == {k: (B,) + v for k, v in adj.items()}
    a = s.eval_adjoint_penalty_sensitivities(seed_u=np.ones((B, 4, N, 2)))
    assert {k: v.shape for k, v in a.items()} == {k: (B, 4) + v for k, v in adj.items()}
    d = s.du0_dsoft()
    assert {k: v.shape for k, v in d.items()} == {k: (B, 2) + v for k, v in pen.items()}
    sx = [(1, np.ones((8, 3)))]
    su = [(0, np.eye(2, 3))]
    v = s[2].eval_adjoint_penalty_sensitivity(sx, su)
    assert {k: w.shape for k, w in v.items()} == {k: (3,) + w for k, w in pen.items()}
    seed_x, seed_u = np.zeros((B, 3, N + 1, 8)), np.zeros((B, 3, N, 2))
    seed_x[2, :, 1, :] = 1.0; seed_u[2, :, 0, :] = np.eye(2, 3).T
    full = s.eval_adjoint_penalty_sensitivities(seed_x, seed_u)
    for k in pen:
        np.testing.assert_array_equal(v[k], full[k][2], err_msg=k)
    s.free()


def test_workspace_poison():
    """A fresh child process, started with IHM2MPC_POISON_WORKSPACE=1: both new entries give the bits of a clean twin
    (tests/penalty_grad_poison_child.py; the manner of tests/test_gpu_slack_seeds.py::test_workspace_poison)."""
    env = dict(os.environ, IHM2MPC_POISON_WORKSPACE="1")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "penalty_grad_poison_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "penalty grad poison ok" in r.stdout, r.stdout[-2000:]
