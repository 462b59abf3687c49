"""The OCP's cost and its total gradient on the GPU (kernels_cost.hip: k_cost, k_cost_epilogue; ihm2mpc_eval_cost,
ihm2mpc_eval_cost_gradient): the values against tests/cost_ref.py on hard, soft, lateral-acceleration, per-instance and stage-dependent
weight tables, in the SQP mode and right after init_guess; the composition with the adjoint entry; central differences of get_cost over
whole re-solves on the cases tests/test_oracle_cost.py has shown to be fair; bit-identity of everything else; refusals and NaN rows; the
workspace poison; the Python layers.

Tolerances.  VAL_TOL: every compared value is a sum of products in fp64; a stage is at most 156 of them, the horizon 41 stages and a
six-step butterfly, so rounding is below about 2e-14 of the cancellation-free magnitude sum |terms| (cost_ref's "mag"); 1e-12 leaves room
for different contraction.  An explicit partial is not an output of its own: it is the total minus the adjoint entry's gradient of the
same seeds, which adds the rounding of the epilogue's addition and of that subtraction, 2^-52 (|adjoint part| + |total|) -- a bound of
the two operations, added to VAL_TOL x magnitude.  ROUND_TOL and REF_TOL are those of tests/test_gpu_adjoint_weights.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import adj_ref as R
import adjw_ref as RW
import cost_cases as C
import cost_ref as CR
import layouts as L
import sens_ref as S
from test_gpu_adjoint_weights import REF_TOL, ROUND_TOL, _solve_refined
from test_gpu_qp_layouts import TABLE, _start, _widen
from test_gpu_sensitivity import _outputs, _subset

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-12
EPS52 = 2.0 ** -52
GRADS = ("x0", "yref", "yref_e", "W", "W_e")


def _solver(track, lay, B, block="0", **opts):
    from ihm2_amd.solver import BatchedOcpSolver
    from poison_cases import environ

    with environ(IHM2MPC_BLOCK_QP=block):
        s = BatchedOcpSolver(L.make_ocp(lay, **opts), B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
    arr = L.apply(s.data, lay)
    if arr["W"] is not None:
        s._push_weights()
    s._push_bounds()
    return s


def _eval_cost(s):
    from ihm2_amd import _lib
    from ihm2_amd.solver import _ptr

    c, st, sl = np.empty(s.B), np.empty((s.B, s.N + 1)), np.empty(s.B)
    _lib.check(s.lib.ihm2mpc_eval_cost(s._h, _ptr(c), _ptr(st), _ptr(sl)))
    return dict(cost=c, stage_cost=st, slack_cost=sl)


def _offdiag_weights(B):
    """Per-instance weights with the off-diagonal tuning of tests/test_gpu_instance_tuning.py on every third instance."""
    from ihm2_amd import ocp as O

    W0, We0 = O.default_weights()
    Wo = W0.copy()
    for j in (1, 2, 3):
        Wo[0, j] = Wo[j, 0] = 0.1
    f = 1.0 + 0.25 * (np.arange(B) % 4)
    W = np.stack([(Wo if b % 3 == 2 else W0) * f[b] for b in range(B)])
    return W, np.stack([We0 * (1.5 - 0.125 * (b % 4)) for b in range(B)])


# kind -> (layout knobs, solver options, per-instance weights, solve, gradient)
KINDS = {
    "hard": (dict(), {}, False, True, True),
    "soft_state_bounds": (dict(soft=1.0, soft_rows=(1, 3), soft_kind="both", seed=6), {}, False, True, False),
    "alat_soft": (dict(path=True, alat=True, path_soft=True, alat_soft=True, alat_max=2.5, width=1.2), {}, False, True, False),
    "instance_weights": (dict(), {}, True, True, True),
    "stage_W": (dict(stage_W=True, seed=1), {}, False, True, True),
    "sqp_mode": (dict(), dict(nlp_solver_type="SQP", nlp_solver_max_iter=2), False, True, False),
    "after_init_guess": (dict(), {}, False, False, False),
}


@pytest.mark.parametrize("N", [10, 40])
@pytest.mark.parametrize("B", [3, 67])
@pytest.mark.parametrize("kind", list(KINDS))
def test_values(track, kind, B, N):
    """cost, stage_cost, slack_cost on every table; on the all-hard RTI tables also the seeds and the explicit partials."""
    knobs, opts, inst_w, solve, grad = KINDS[kind]
    lay = L.Layout("cost_" + kind, N=N, **knobs)
    s = _solver(track, lay, B, **opts)
    data = s.data
    Wb = Web = None
    if inst_w:
        Wb, Web = _offdiag_weights(B)
        s.set_instance_weights(Wb, Web)
    x0, yref, yref_e = _start(s, track, B, 50 + N)
    rti = "nlp_solver_type" not in opts
    if rti:
        s.set_x0_sensitivities(1)
    if solve:
        for _ in range(2):
            st = s.solve()
        assert np.isin(st, (0, 2)).mean() > 0.5, st
    o = _outputs(s, alat=True)
    got = _eval_cost(s)
    np.testing.assert_array_equal(s.get_cost(), got["cost"])
    np.testing.assert_array_equal(s.get_cost(stagewise=True), got["stage_cost"])
    np.testing.assert_array_equal(s.get_slack_cost(), got["slack_cost"])
    assert all(np.isfinite(v).all() for v in got.values())
    g = s.eval_cost_gradient() if grad else None
    a = s.eval_adjoint_weight_sensitivities(g["seed_x"], g["seed_u"]) if grad else None
    worst = {}

    def note(name, err, mag, extra=0.0):
        bound = VAL_TOL * mag + extra
        assert (np.asarray(mag)[np.asarray(err) > 0] > 0).all(), name
        r = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        worst[name] = max(worst.get(name, 0.0), r)

    soft_used = 0.0
    for i in range(B):
        w = dict(W=None if Wb is None else Wb[i], W_e=None if Web is None else Web[i])
        ref = CR.cost(data, o["x"][i], o["u"][i], yref[i], yref_e[i], slk=o["slk"][i], slk_a=o["slk_a"][i], **w)
        for k in ("cost", "stage_cost", "slack_cost"):
            note(k, np.abs(got[k][i] - ref[k]), ref["mag"][k])
        soft_used = max(soft_used, ref["slack_cost"])
        if grad:
            assert np.isfinite(g["cost"][i]) and g["cost"][i] == got["cost"][i]
            sd, smag = CR.seeds(data, o["x"][i], o["u"][i], yref[i], yref_e[i], **w)
            note("seed_x", np.abs(g["seed_x"][i] - sd[:, :8]), smag[:, :8])
            note("seed_u", np.abs(g["seed_u"][i] - sd[:N, 8:]), smag[:N, 8:])
            if o["status"][i] in (0, 2):
                ex = CR.explicit_partials(data, o["x"][i], o["u"][i], yref[i], yref_e[i], **w)
                for k in ("yref", "yref_e", "W", "W_e"):
                    note("explicit_" + k, np.abs((g[k][i] - a[k][i]) - ex[k]), ex["mag"][k], EPS52 * (np.abs(a[k][i]) + np.abs(g[k][i])))
    print(f"COST values {kind} B {B} N {N}: worst error / bound " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    if kind in ("soft_state_bounds", "alat_soft"):
        assert soft_used > 0.0, "no slack is in use: the soft terms were not exercised"
    if kind == "alat_soft":
        assert np.abs(o["slk_a"]).max() > 0.0 or np.abs(o["slk"]).max() > 0.0
    s.free()


def _adjoint_refined(qp, dz, lam, sl, z, Z, seed):
    """adj_ref.adjoint with the dense solve refined in extended precision (tests/test_gpu_adjoint_weights.py: _solve_refined)."""
    N = np.asarray(qp["A"]).shape[0]
    nz = N * 10 + 8
    M = R.kkt_matrix(qp, dz, lam, sl, z, Z)
    rhs = np.zeros((M.shape[0], 1))
    rhs[:nz, 0] = np.asarray(seed, dtype=np.float64).reshape(-1)[:nz]
    sol = _solve_refined(M, rhs)[:, 0]
    zeta = np.zeros((N + 1, 10))
    zeta.reshape(-1)[:nz] = sol[:nz]
    return zeta, sol[nz:nz + 8]


HARD_LAYOUTS = [n for n, (lay, _, _) in TABLE.items() if not (lay.soft or lay.path_soft or lay.alat_soft)]


@pytest.mark.parametrize("name", HARD_LAYOUTS)
def test_composition(track, name):
    """After one solve: grad_x0 is, bit for bit, that of ihm2mpc_eval_adjoint_sensitivities_w on the seeds the entry returned; the other
    four are that call's plus cost_ref's explicit partials to ROUND_TOL of |adjoint part| + |explicit part|; grad_W, grad_W_e exactly
    symmetric; and against cost_ref composed with adj_ref / adjw_ref at the GPU's own iterate (a subset of the solved instances) at
    REF_TOL, relative to the largest entry of the magnitude and, for the weights, entry by entry."""
    from oracle import oracle as orc

    lay, Bt, block = TABLE[name]
    B = min(Bt, 67)
    s = _solver(track, lay, B, block)
    data, N = s.data, s.N
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    x0, yref, yref_e = _start(s, track, B, 900 + lay.seed)
    s.set_x0_sensitivities(1)
    xbar, ubar = s.get_x(), s.get_u()
    st = s.solve()
    ok = (st == 0) | (st == 2)
    assert ok.mean() > 0.5
    g = s.eval_cost_gradient()
    a = s.eval_adjoint_weight_sensitivities(g["seed_x"], g["seed_u"])
    np.testing.assert_array_equal(g["x0"], a["x0"])
    np.testing.assert_array_equal(g["W"], np.swapaxes(g["W"], -1, -2))
    np.testing.assert_array_equal(g["W_e"], np.swapaxes(g["W_e"], -1, -2))
    for k in GRADS:
        assert np.isnan(g[k][~ok]).all() and np.isfinite(g[k][ok]).all(), k
    assert np.isfinite(g["cost"]).all() and np.isfinite(g["seed_x"]).all() and np.isfinite(g["seed_u"]).all()
    nc = 15 if lay.alat else L.NC
    o = _outputs(s, alat=lay.alat)
    lam, slk = (_widen(o["lam"], o["lam_a"]), _widen(o["slk"], o["slk_a"])) if lay.alat else (o["lam"], o["slk"])
    z, Z = L.soft_arrays(data, nc, None)
    worst_round = 0.0
    for i in np.flatnonzero(ok):
        ex = CR.explicit_partials(data, o["x"][i], o["u"][i], yref[i], yref_e[i])
        for k in ("yref", "yref_e", "W", "W_e"):
            scale = np.abs(a[k][i]) + ex["mag"][k]
            d = np.abs(g[k][i] - (a[k][i] + ex[k]))
            assert (d[scale == 0.0] == 0.0).all(), k
            worst_round = max(worst_round, float((d[scale > 0] / scale[scale > 0]).max()))
    A, Bm, b = s.get_linearization()
    worst = worst_entry = 0.0
    for i in _subset(ok)[:4]:
        ref = P.build_qp(xbar[i], ubar[i], x0[i], yref[i], yref_e[i])
        qp = L.assemble_qp(data, xbar[i], ubar[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=ref if lay.path else None)
        dz = np.zeros((N + 1, 10)); dz[:, :8] = o["x"][i] - xbar[i]; dz[:N, 8:] = o["u"][i] - ubar[i]
        Gy, Gye = R.gy_tables(lambda yr, yre, i=i: P.build_qp(xbar[i], ubar[i], x0[i], yr, yre)["g"], yref[i], yref_e[i])
        t = CR.total_gradient(data, qp, dz, lam[i], slk[i], z, Z, Gy, Gye, o["x"][i], o["u"][i], yref[i], yref_e[i], adjoint=_adjoint_refined)
        sd, _ = CR.seeds(data, o["x"][i], o["u"][i], yref[i], yref_e[i])
        zeta, _ = _adjoint_refined(qp, dz, lam[i], slk[i], z, Z, sd)
        zp = np.zeros((N + 1, 10)); zp[:, :8] = o["x"][i]; zp[:N, 8:] = o["u"][i]
        _, mags = RW.stage_terms(data, zeta, zp, yref[i])
        mag = dict(W=0.5 * (mags.sum(0) + mags.sum(0).T) + t["explicit"]["mag"]["W"],
                   W_e=0.5 * (np.outer(np.abs(zeta[N, :8]), np.abs(zp[N, :8] - yref_e[i])) + np.outer(np.abs(zp[N, :8] - yref_e[i]), np.abs(zeta[N, :8])))
                   + t["explicit"]["mag"]["W_e"],
                   x0=np.abs(t["x0"]), yref=np.abs(t["adj"]["yref"]) + t["explicit"]["mag"]["yref"],
                   yref_e=np.abs(t["adj"]["yref_e"]) + t["explicit"]["mag"]["yref_e"])
        for k in GRADS:
            d = np.abs(g[k][i] - t[k])
            worst = max(worst, float(d.max() / mag[k].max()))
            if k in ("W", "W_e"):
                nz = mag[k] > 0.0
                worst_entry = max(worst_entry, float((d[nz] / mag[k][nz]).max()))
    print(f"COST composition {name}: rounding {worst_round:.2e}, reference {worst:.2e} (weights entry by entry {worst_entry:.2e})")
    assert worst_round <= ROUND_TOL, worst_round
    assert worst <= REF_TOL and worst_entry <= REF_TOL, (worst, worst_entry)
    s.free()


@pytest.mark.parametrize("name", list(C.CASES))
def test_gradient_against_whole_solves(track, name):
    """<eval_cost_gradient, direction> against central differences of get_cost() over re-solves from the restored start, on the
    layouts, instances, directions and step lengths of tests/cost_cases.py, with the measure and the acceptance profile of
    tests/test_oracle_cost.py (which shows the NumPy reference to meet it on these inputs)."""
    from ihm2_amd.solver import BatchedOcpSolver
    from oracle import oracle as orc

    lay, B, seed = C.CASES[name]
    N = lay.N
    ocp = L.make_ocp(lay)
    ocp.solver_options.qp_tol = C.QP_TOL
    ocp.solver_options.qp_solver_iter_max = 200
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
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
    g = s.eval_cost_gradient()
    o = _outputs(s)
    ok = st == 0
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref))
    A, Bm, b = s.get_linearization()
    z, Z = L.soft_arrays(data)
    free = {k: np.zeros_like(g[k]) for k in GRADS}
    for i in np.flatnonzero(ok):        # the scale of an unconstrained reaction (dense, at the GPU's iterate); weakly active instances have no derivative
        qp = L.assemble_qp(data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i])
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
        with np.errstate(invalid="ignore"):
            e = np.abs(C.contract(g, d) - fd) / np.maximum(np.abs(fd), np.abs(C.contract(free, d)))
        errs.append(e)
    keep = np.flatnonzero(ok)
    assert keep.size >= 0.75 * B, (keep.size, B)
    for dname, e in zip(C.DIRECTIONS, errs):
        (med, s5, s3), _ = C.profile(e[keep])
        print(f"COST-FD {name} {dname}: median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {e[keep].max():.2e}")
    allerr = np.concatenate([e[keep] for e in errs])
    (med, s5, s3), met = C.profile(allerr)
    print(f"COST-FD {name}: kept {keep.size} of {B}, median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {allerr.max():.2e}")
    assert met, (med, s5, s3)
    s.free()


@pytest.mark.parametrize("B,N", [(3, 10), (67, 40)])
def test_nothing_else_moves(track, B, N):
    """With and without the two new calls between them: every getter, a following adjoint evaluation with fixed seeds and the next
    step agree bit for bit; two calls in a row return the same bits; all outputs NULL is accepted."""
    from ihm2_amd import _lib
    from test_gpu_adjoint import _seeds

    lay = L.Layout("cost_hard", N=N)
    seed_x, seed_u = _seeds(B, 3, N, 7)
    res = []
    for with_calls in (False, True):
        s = _solver(track, lay, B)
        _start(s, track, B, 55)
        s.set_x0_sensitivities(2)
        st = s.solve()
        assert (st == 0).mean() > 0.5
        if with_calls:
            c1, g1 = _eval_cost(s), s.eval_cost_gradient()
            c2, g2 = _eval_cost(s), s.eval_cost_gradient()
            for k in c1:
                np.testing.assert_array_equal(c2[k], c1[k], err_msg=k)
            for k in g1:
                np.testing.assert_array_equal(g2[k], g1[k], err_msg=k)
            _lib.check(s.lib.ihm2mpc_eval_cost(s._h, None, None, None))
            _lib.check(s.lib.ihm2mpc_eval_cost_gradient(s._h, *[None] * 8))
        out = dict(_outputs(s), u0=s.get_u0(), x0=s.get_x0())
        out["sens_x"], out["sens_u"] = s.get_x0_sensitivities()
        out.update({"adjw_" + k: v for k, v in s.eval_adjoint_weight_sensitivities(seed_x, seed_u).items()})
        out.update({"adj_" + k: v for k, v in s.eval_adjoint_sensitivities(seed_x, seed_u).items()})
        if with_calls:
            s.eval_cost_gradient()
        s.step(40.0, model=0, M_sim=25)
        out.update({"next_" + k: v for k, v in _outputs(s).items()}, next_u0=s.get_u0(), next_x0=s.get_x0())
        res.append(out)
        s.free()
    for k in res[0]:
        np.testing.assert_array_equal(res[1][k], res[0][k], err_msg=k)


def test_refusals_and_nan_rows(track):
    from ihm2_amd._lib import Ihm2mpcError
    from ihm2_amd.solver import BatchedOcpSolver

    B = 8
    sq = BatchedOcpSolver(make_ocp(nlp_solver_type="SQP", nlp_solver_max_iter=2), B, track.s_ref, track.kappa_ref)
    with pytest.raises(Ihm2mpcError, match="adjoint sensitivities are implemented for SQP_RTI"):
        sq.eval_cost_gradient()
    sq.free()
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    with pytest.raises(Ihm2mpcError, match="x0 sensitivities are off"):
        s.eval_cost_gradient()
    s.set_x0_sensitivities(1)
    with pytest.raises(Ihm2mpcError, match="no solve has run"):
        s.eval_cost_gradient()
    x0 = sample_x0(track, B, seed=9)
    x0[0, 1] = 5.0              # far outside the hard box on n: an infeasible QP, reported by its status (tests/test_gpu_adjoint.py's instance)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    assert st[0] not in (0, 2) and (st[1:] == 0).mean() > 0.5, st
    ok = (st == 0) | (st == 2)
    g = s.eval_cost_gradient()
    for k in GRADS:
        assert np.isnan(g[k][~ok]).all() and np.isfinite(g[k][ok]).all(), k
    for k in ("cost", "seed_x", "seed_u"):
        assert np.isfinite(g[k]).all(), k
    assert np.isfinite(s.get_cost(stagewise=True)).all()
    # the batch-mates' bits do not depend on the failed instance: the same instances alone
    t = BatchedOcpSolver(make_ocp(), B - 1, track.s_ref, track.kappa_ref)
    t.set_x0_sensitivities(1)
    t.set_x0(x0[1:]); t.init_guess(); t.prepare_step(40.0)
    np.testing.assert_array_equal(t.solve(), st[1:])
    gt = t.eval_cost_gradient()
    for k in g:
        np.testing.assert_array_equal(gt[k], g[k][1:], err_msg=k)
    t.free()
    s.run_steps(40.0, 2, model=0, M_sim=25)
    with pytest.raises(Ihm2mpcError, match="ihm2mpc_run_steps, which computes no x0 sensitivities"):
        s.eval_cost_gradient()
    assert np.isfinite(s.get_cost()[ok]).all()          # the cost itself is evaluated in any state
    s.prepare_step(40.0)
    s.solve()
    s.eval_cost_gradient()          # readable again after a solve
    s.free()
    for knobs in (dict(soft=1.0, soft_rows=(1,), soft_kind="both", seed=6), dict(path=True, alat=True, alat_soft=True, alat_max=2.5, width=1.2)):
        lay = L.Layout("cost_soft", N=10, **knobs)
        v = _solver(track, lay, B)
        _start(v, track, B, 3)
        v.set_x0_sensitivities(1)
        v.solve()
        with pytest.raises(Ihm2mpcError, match="defined for all-hard constraint tables.*carry no seed"):
            v.eval_cost_gradient()
        v.eval_adjoint_weight_sensitivities()       # the adjoint entries take the table
        assert np.isfinite(v.get_cost()).all()
        v.free()


def test_after_the_persistent_loop(track, monkeypatch):
    """After run_steps_sens(n) the gradient is that of n x step(), bit for bit."""
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    B, steps = 67, 4
    x0 = sample_x0(track, B, seed=31)
    res = []
    for persistent in (False, True):
        s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
        s.set_lap_wrap(True)
        s.set_x0_sensitivities(1)
        s.set_x0(x0); s.init_guess()
        s.step(40.0, model=0, M_sim=30)
        if persistent:
            s.run_steps(40.0, steps, model=0, M_sim=30, sens_u0_hist=True)
            assert s.get_launch_record()["steps"].startswith("k_steps<")
        else:
            for _ in range(steps):
                s.step(40.0, model=0, M_sim=30)
        res.append((s.get_status(), s.eval_cost_gradient(), s.get_cost(stagewise=True)))
        s.free()
    (sa, ga, ca), (sb, gb, cb) = res
    np.testing.assert_array_equal(sb, sa)
    np.testing.assert_array_equal(cb, ca)
    for k in ga:
        np.testing.assert_array_equal(gb[k], ga[k], err_msg=k)
    ok = np.isin(sa, (0, 2))
    assert ok.mean() > 0.7 and np.isfinite(ga["W"][ok]).all() and np.abs(ga["x0"][ok]).max() > 0.0


def test_workspace_poison():
    """A fresh child process, started with IHM2MPC_POISON_WORKSPACE=1: both entries give the bits of a clean twin
    (tests/cost_poison_child.py; the manner of tests/test_gpu_workspace_poison.py::test_qp_forms)."""
    env = dict(os.environ, IHM2MPC_POISON_WORKSPACE="1")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cost_poison_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cost poison ok" in r.stdout, r.stdout[-2000:]


def test_python_layers(track):
    from ihm2_amd.controller import IHM2Controller
    from ihm2_amd.solver import BatchedOcpSolver

    B = 5
    s = BatchedOcpSolver(make_ocp(N=10), B, track.s_ref, track.kappa_ref)
    s.set_x0_sensitivities(1)
    x0 = sample_x0(track, B, seed=3)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    assert st[2] == 0
    J, g = s.get_cost(), s.eval_cost_gradient()
    assert J.shape == (B,) and s.get_cost(stagewise=True).shape == (B, 11)
    assert {k: v.shape for k, v in g.items()} == dict(cost=(B,), x0=(B, 8), yref=(B, 10, 12), yref_e=(B, 8), W=(B, 12, 12), W_e=(B, 8, 8),
                                                      seed_x=(B, 11, 8), seed_u=(B, 10, 2))
    v = s[2]
    assert isinstance(v.get_cost(), float) and v.get_cost() == J[2]
    gx = v.eval_and_get_optimal_value_gradient("initial_state")
    assert gx.shape == (8,)
    np.testing.assert_array_equal(gx, g["x0"][2])
    np.testing.assert_array_equal(v.eval_and_get_optimal_value_gradient(), g["x0"][2])
    with pytest.raises(Exception, match="no p_global"):
        v.eval_and_get_optimal_value_gradient("p_global")
    s.free()
    c = IHM2Controller(track.s_ref, track.kappa_ref, batch_size=B)
    c.warm_start(x0)
    u0 = c.compute_control(x0)
    assert u0.shape == (B, 2)
    Jc = c.cost()
    assert Jc.shape == (B,)
    np.testing.assert_array_equal(Jc, c.solver.get_cost())
    assert np.isfinite(Jc).all() and (Jc > 0.0).all()
