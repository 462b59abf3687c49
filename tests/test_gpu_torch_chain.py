"""GPU: the closed loop x0 -> rti -> plant -> rti -> ... -> loss through ihm2_amd/torch_layer.py (rti_solve_soft and plant_step, one
solver per step) against the same chain composed by hand (tests/chain_ref.py): (1) bit for bit forward and to the reference's own
rounding scale backward, against the library's host entries, with a failed instance in the last step; (2) against central differences
of the whole chain through the layer, on the start and the directions that tests/test_oracle_torch_chain.py holds the NumPy reference
to on the CPU oracle.  The table is tests/test_gpu_penalty_device.py's LAY (N = 5)."""
import gc

import numpy as np
import pytest
import torch

import bitcmp
import chain_ref as CR
import layouts as L
import sens_ref as S
from test_gpu_penalty_device import LAY, N, _free, _penalties, _Start, _t
from test_gpu_qp_layouts import _widen
from test_gpu_sensitivity import _outputs

pytestmark = pytest.mark.gpu

B = 8
M_SIM = 25


def _restart(c, x0, yref=None, yref_e=None):
    """The handle of a _Start on another initial state: the initial guess from it, and the state every solve starts from kept again."""
    s = c.s
    c.x0 = np.array(x0)
    if yref is not None:
        c.yref, c.yref_e = np.array(yref), np.array(yref_e)
    s.set_x0(c.x0); s.init_guess()
    s.set_yref(c.yref); s.set_yref_e(c.yref_e); s.set_multipliers(None, None)
    c.x, c.u = s.get_x(), s.get_u()
    c.pi, c.lam = s.get_multipliers()
    c.slk = s.get_slacks()
    c.lam_a, c.slk_a = s.get_alat_multipliers()


def chain_inputs(c, T, Bn=B):
    """Per step: the handle's references, weights that differ by instance and step (symmetric), per-instance penalties of their own."""
    s = c.s
    ins = []
    for t in range(T):
        fac = (1.0 + 0.01 * np.arange(Bn) + 0.003 * t)[:, None, None]
        z, Z, az, aZ = _penalties(s, Bn, seed=5 + t)
        ins.append(dict(yref=c.yref, yref_e=c.yref_e, W=fac * np.asarray(s.data.W[0], dtype=np.float64)[None],
                        W_e=fac * np.asarray(s.data.W_e, dtype=np.float64)[None], soft_z=z, soft_Z=Z, alat_z=az, alat_Z=aZ))
    return ins


def chain_seeds(T, Bn=B, seed=11):
    """What the loss puts on the steps' outputs: random seeds on the last step's x, u, s, sa, and one on the first step's s."""
    rng = np.random.default_rng(seed)
    last = dict(x=rng.standard_normal((Bn, N + 1, 8)), u=rng.standard_normal((Bn, N, 2)), s=rng.standard_normal((Bn, N + 1, 28)),
                sa=rng.standard_normal((Bn, N + 1, 2)))
    first = dict(s=rng.standard_normal((Bn, N + 1, 28)))
    return {0: first, T - 1: last} if T > 1 else {0: last}


def layer_chain(cs, x0, ins, loss_seeds, model, zero_failed=False, fail_last=False, drop_sx=False):
    """The chain through the layer.  Returns (forward, gradients): per step a dict of numpy arrays -- CR.FORWARD and x_next,
    model_used; CR.GRADS, x0 the gradient in the state the step's solve and plant step were given.  ``drop_sx``: the plant's input state
    detached on purpose, for showing that the comparison notices (the reference keeps S_x' g)."""
    from ihm2_amd.torch_layer import plant_step, rti_solve_soft

    T = len(cs)
    xin = _t(x0, True)
    steps, loss = [], 0.0
    for t, (c, a) in enumerate(zip(cs, ins)):
        if fail_last and t == T - 1:
            e = torch.zeros_like(xin)
            e[0, 1] = CR.FAIL_SHIFT
            xin = xin + e
        ta = {k: _t(a[k], True) for k in CR.INS}
        c.restore()
        x, u, s, sa, st = rti_solve_soft(c.s, xin, *[ta[k] for k in CR.INS], zero_failed=zero_failed)
        rec = dict(xin=xin, ins=ta, x=x, u=u, s=s, sa=sa, status=st)
        for k, v in loss_seeds.get(t, {}).items():
            loss = loss + (_t(v) * rec[k]).sum()
        if t < T - 1:
            rec["x_next"], rec["model_used"] = plant_step(c.s, xin.detach() if drop_sx else xin, u[:, 0].contiguous(), model=model, M_sim=M_SIM)
            xin = rec["x_next"]
        steps.append(rec)
    wrt = [v for r in steps for v in [r["xin"]] + [r["ins"][k] for k in CR.INS]]
    g = [v.cpu().numpy() for v in torch.autograd.grad(loss, wrt)]
    n = 1 + len(CR.INS)
    grads = [dict(zip(CR.GRADS, g[n * t:n * (t + 1)])) for t in range(T)]
    fw = [{k: r[k].detach().cpu().numpy() for k in CR.FORWARD + ("x_next", "model_used") if k in r} for r in steps]
    return fw, grads


def compare_chain(cs, x0, ins, loss_seeds, model, zero_failed=False, fail_last=False, layer=None):
    """The layer's chain against the host composition on the same handles: the forward bit for bit; every gradient of every step to
    8 times the move of the reference's own array under CR.Jitter, bit for bit where nothing moves.  Returns (forward, gradients of
    the layer, the host forward, the worst ratio to the bound as (ratio, step, array))."""
    fw, grads = layer if layer is not None else layer_chain(cs, x0, ins, loss_seeds, model, zero_failed, fail_last)
    hfw = CR.host_forward(cs, x0, ins, model, M_SIM, fail_last)
    ref = CR.host_backward(cs, hfw, loss_seeds, zero_failed)
    moved = [CR.host_backward(cs, hfw, loss_seeds, zero_failed, jitter=CR.Jitter(seed=3 + j)) for j in range(CR.DRAWS)]
    for t, (a, h) in enumerate(zip(fw, hfw)):
        bitcmp.assert_all_same_bits(f"forward of step {t + 1}", a, h, keys=list(a), nan_equal=True)
    worst = (0.0, None, None)
    for t in range(len(cs)):
        for k in CR.GRADS:
            ratio = CR.within(f"step {t + 1}: gradient in {k}", grads[t][k], ref[t][k], [m[t][k] for m in moved])
            worst = max(worst, (ratio, t + 1, k))
    # where nothing is summed the bits are equal: the last step's gradients but the a_lat pair's (the sum over the stages)
    for k in CR.GRADS[:7]:
        bitcmp.assert_same_bits(f"last step: gradient in {k}", grads[-1][k], ref[-1][k], nan_equal=True)
    return fw, grads, hfw, worst


def _start_chain(track, T, model):
    cs = [_Start(track, B) for _ in range(T)]
    if model == -1:     # both branches of the switched plant (v^2 sin(beta) / l_R against 3): slow and fast cars, the wheels turned
        x0 = cs[0].x0.copy()
        x0[:, 3], x0[:, 7] = np.linspace(2.0, 12.0, B), 0.05
        for c in cs:
            _restart(c, x0)
    return cs


@pytest.mark.parametrize("case", ["solved", "failed_nan", "failed_zero"])
@pytest.mark.parametrize("model", [0, -1])
def test_chain_equals_the_host_composition(track, model, case):
    """x0 -> rti -> plant -> rti -> plant -> rti -> loss, B = 8, three solvers; the loss seeds the last step's x, u, s, sa and the
    first step's s, so x0 gets the solve's and the plant's share.  Against tests/chain_ref.py's composition of the host entries
    (set_*, solve, sim_step_sens; backward by eval_adjoint_penalty_sensitivities step by step, S_x' g and S_u' g by einsum): x, u, s,
    sa, status, x_next, model_used bit for bit; every gradient of every step (x0, yref, yref_e, W, W_e, soft_z, soft_Z, alat_z,
    alat_Z) within 8 times the largest move of the reference's own array, per instance, when every summed intermediate (S_x' g, S_u' g,
    the a_lat rows before their sum) is multiplied entrywise by 1 + 8 eps r, r = +-1 -- the two sides differ by the order of those sums
    only; the last step's gradients, where nothing is summed, bit for bit.  model -1: both branches of the switched plant occur.
    failed_*: instance 0 is pushed 5 m off the centre line at the last solver's input (an infeasible QP, asserted by its status).
    With zero_failed off its rows are NaN on both sides in every gradient that reaches back through it; with zero_failed on they are
    exact zeros in the steps whose only seed came through it.  In both, every other instance has the bits of the layer's run without
    the failure: one instance's NaN seed changes nobody else's gradient.

    The move is the largest over tests/chain_ref.py::DRAWS = 16 independent draws of the signs: with one draw the a_lat pair's array
    of two entries per instance stood still on single instances by the coincidence of its signs (moves of 0 and 1e-34 against
    differences of one ulp of the sum's terms) while every other array was within 0.31 of its one-draw move.

    Measured (MI355X), worst ratio of |layer - reference| to the move, 8 allowed: 4.0 (model -1, step 2, soft_Z); the last step's
    gradients and every forward array: the same bits."""
    T = 3
    cs = _start_chain(track, T, model)
    fail, zf = case != "solved", case == "failed_zero"

    def body():
        x0, ins, seeds = cs[0].x0, chain_inputs(cs[0], T), chain_seeds(T)
        fw, grads, hfw, worst = compare_chain(cs, x0, ins, seeds, model, zero_failed=zf, fail_last=fail)
        print(f"CHAIN-HOST model {model} {case}: worst ratio {worst[0]:.3f} of 8 (step {worst[1]}, {worst[2]}); status of the last step {fw[-1]['status']}")
        ok = np.isin(fw[-1]["status"], (0, 2))
        assert all(np.isin(f["status"], (0, 2))[1:].mean() > 0.7 for f in fw), [f["status"] for f in fw]
        if model == -1:
            assert len(set(fw[0]["model_used"].tolist())) == 2, fw[0]["model_used"]
        for t in range(T):
            assert np.abs(np.nan_to_num(grads[t]["x0"])).max() > 0.0 and np.abs(np.nan_to_num(grads[t]["soft_Z"])).max() > 0.0, t
        if not fail:
            assert ok[0]
            return
        assert not ok[0] and all(np.isin(f["status"], (0, 2))[0] for f in fw[:-1]), [f["status"] for f in fw]
        for t in range(T):
            for k in CR.ADJ:
                if zf and t >= 1:
                    assert (grads[t][k][0] == 0.0).all(), (t, k)
                elif not zf:
                    assert np.isnan(grads[t][k][0]).all(), (t, k)
            if zf and t >= 1:
                assert all((grads[t][k][0] == 0.0).all() for k in CR.GRADS), t
        # the run without the failure, through the layer: the other instances' bits
        fw0, grads0 = layer_chain(cs, x0, ins, seeds, model)
        for t in range(T):
            for k in fw0[t]:
                bitcmp.assert_same_bits(f"step {t + 1}: {k} of the instances 1.. against the run without the failure", fw[t][k][1:], fw0[t][k][1:], nan_equal=True)
            for k in CR.GRADS:
                bitcmp.assert_same_bits(f"step {t + 1}: gradient in {k} of the instances 1.. against the run without the failure",
                                        grads[t][k][1:], grads0[t][k][1:], nan_equal=True)

    try:
        body()
    finally:
        for c in cs:
            _free(c.s)


# ---- the chain against central differences of itself ----

def _kept(c, track, P, x0_in, pen, out_x, out_u, lam, slk, st):
    """The skip rule of tests/test_gpu_penalty_device.py::_central_differences on one solve: solved and not weakly active."""
    s = c.s
    z, Z, az, aZ = pen
    A, Bm, b = s.get_linearization()
    wide = lambda a28, a2: _widen(a28, np.broadcast_to(a2, (N + 1, 2)))  # noqa: E731
    keep = np.zeros(len(st), dtype=bool)
    for i in np.flatnonzero(st == 0):
        args = (c.x[i], c.u[i], x0_in[i], c.yref[i], c.yref_e[i])
        qp = L.assemble_qp(s.data, *args, A[i], Bm[i], b[i], nonlinear=P.build_qp(*args))
        step = np.zeros((N + 1, 10)); step[:, :8] = out_x[i] - c.x[i]; step[:N, 8:] = out_u[i] - c.u[i]
        keep[i] = not S.weakly_active(qp, step, lam[i], sl=slk[i], soft_z=wide(z[i], az[i]), soft_Z=wide(Z[i], aZ[i]))
    return keep


def test_chain_against_central_differences(track):
    """x0 -> rti -> plant -> rti, B = 64, two solvers at qp_tol 1e-9: the gradient of u2[:, 0, m], m = 0, 1, from autograd through both
    solves and the plant step, contracted with a direction, against central differences of the whole chain through the layer (both
    solvers restored before every evaluation), in three directions: x0 (X_SCALE N(0,1), eps 1e-4), step 1's (soft_z, soft_Z) (the
    direction and eps of the layer's penalty test) and step 1's (W, W_e) (the symmetric direction and 1e-4 of the layer's weight test).
    Skipped: an instance with a status other than 0 in one of the three evaluations of a direction, or weakly active in one of its two
    solves; at least 48 of 64 kept.  Measure: max_m |pred - fd| / max(max_m |fd|, the batch's median of max_m |fd| over the kept
    instances); bars: tests/cost_cases.py::profile (median <= 1e-6, 75 % <= 1e-5, 95 % <= 1e-3), unwidened; the zero prediction must
    miss them in each direction.  The start is tests/chain_ref.py::fd_start / fd_penalties (the instances of seed 900, v_x from 2.5 to
    2.9, the heading 0.06 rad off, the quadratic penalties times 80), chosen on the CPU oracle alone (tests/test_oracle_torch_chain.py;
    the rule of the choice is in fd_start's docstring) because on _Start's own start the rate rows pin u_0 and the NumPy reference
    itself misses the bars in the penalties and the weights.

    Measured (MI355X), 64 of 64 kept in every direction:
      x0:        median 5.0e-10, 95.3 % <= 1e-5, 100 % <= 1e-3, 1.8e-4 at worst; zero prediction median 0.98
      penalties: median 6.0e-8, 85.9 % <= 1e-5, 96.9 % <= 1e-3, 4.0e-3 at worst; zero prediction median 0.97, 30 % <= 1e-5
      weights:   median 7.3e-7, 76.6 % <= 1e-5, 95.3 % <= 1e-3, 6.2e-3 at worst; zero prediction median 0.99, 20 % <= 1e-5
    (the oracle's reference on the same start: 100 % / 100 %, 95.3 % / 100 %, 89.1 % / 98.4 %).  The weights have one instance to spare
    at each bar.  On an earlier start (seed 1234, v_x 1.6 to 2.9, 0.12 rad, times 50), where the reference had less room (81.2 % / 96.9 %
    in the weights), the layer missed the bars in two directions on instances where the reference has 1e-4 to 1e-2 too: NOTES.md R30."""
    from ihm2_amd.torch_layer import plant_step, rti_solve_soft
    from oracle import oracle as orc

    Bn = 64
    cs = [_Start(track, Bn, tight=True, slow=True) for _ in range(2)]

    def body():
        c1, c2 = cs
        x0, yref, yref_e = CR.fd_start(track, Bn, N)
        for c in cs:
            _restart(c, x0, yref, yref_e)
        pen = CR.fd_penalties(*_penalties(c1.s, Bn))
        z, Z, az, aZ = pen
        W0, We0 = np.asarray(c1.s.data.W[0], dtype=np.float64), np.asarray(c1.s.data.W_e, dtype=np.float64)
        dirs = CR.directions(z, Z, W0, We0)
        base = dict(x0=x0, soft_z=z, soft_Z=Z, W=np.broadcast_to(W0, (Bn, 12, 12)), W_e=np.broadcast_to(We0, (Bn, 8, 8)))
        tyref, tyref_e, tz, tZ, taz, taZ = (_t(a) for a in (yref, yref_e, z, Z, az, aZ))

        def chain(d=None, sign=0.0, eps=0.0, grad=False):
            a = {k: _t(v + sign * eps * d[k] if d is not None and k in d else v, grad) for k, v in base.items()}
            c1.restore(); c2.restore()
            o1 = rti_solve_soft(c1.s, a["x0"], tyref, tyref_e, a["W"], a["W_e"], a["soft_z"], a["soft_Z"], taz, taZ)
            x1, _ = plant_step(c1.s, a["x0"], o1[1][:, 0].contiguous(), model=0, M_sim=M_SIM)
            o2 = rti_solve_soft(c2.s, x1, tyref, tyref_e, None, None, tz, tZ, taz, taZ)
            return a, o1, x1, o2

        a, o1, x1, o2 = chain(grad=True)
        g = {k: np.zeros((Bn, 2) + v.shape[1:]) for k, v in base.items()}
        for m in range(2):
            gm = torch.autograd.grad(o2[1][:, 0, m].sum(), list(a.values()), retain_graph=(m == 0))
            for k, v in zip(a, gm):
                g[k][:, m] = v.cpu().numpy()
        st = [o1[4].cpu().numpy(), o2[4].cpu().numpy()]
        P = orc.OracleProblem(c1.s.data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(LAY)))
        strong = np.ones(Bn, dtype=bool)
        for c, xin, o, s_t in ((c1, x0, o1, st[0]), (c2, x1.detach().cpu().numpy(), o2, st[1])):
            q = _outputs(c.s, alat=True)
            strong &= _kept(c, track, P, xin, pen, q["x"], q["u"], _widen(q["lam"], q["lam_a"]), _widen(q["slk"], q["slk_a"]), s_t)
        lines = []
        for name, (eps, d) in dirs.items():
            pred = CR.contract(g, d)
            u, ok = [], strong.copy()
            with torch.no_grad():
                for sign in (1.0, -1.0):
                    _, p1, _, p2 = chain(d, sign, eps)
                    u.append(p2[1][:, 0].cpu().numpy())
                    ok &= (p1[4].cpu().numpy() == 0) & (p2[4].cpu().numpy() == 0)
            fd = (u[0] - u[1]) / (2 * eps)
            lines.append((name, pred, fd, np.flatnonzero(ok)))
        return lines

    try:
        lines = body()
    finally:
        for c in cs:
            _free(c.s)
    failures = []
    for name, pred, fd, keep in lines:      # every direction is printed before one is judged
        try:
            CR.verdict("CHAIN-FD", name, pred, fd, keep, Bn)
        except AssertionError as e:
            failures.append(f"{name}: {e}")
    assert not failures, "\n".join(failures)
    gc.collect()
