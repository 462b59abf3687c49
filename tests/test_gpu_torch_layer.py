"""The RTI step as a torch.autograd function (ihm2_amd/torch_layer.py: rti_solve): its gradients against the host adjoint entry bit for
bit, the gradient in the weights against central differences of whole solves through the layer itself, zero_failed, and the guards
(a setter between forward and backward, a second backward, x0 sensitivities off)."""
import gc

import numpy as np
import pytest
import torch
from conftest import make_ocp, sample_x0

import adj_ref as R
import adjw_ref as RW
import bitcmp
import layouts as L
import sens_ref as S
from test_gpu_adjoint_weights import _coupled, _sym, _zplus
from test_gpu_qp_layouts import TABLE, _start
from test_gpu_sensitivity import _outputs

pytestmark = pytest.mark.gpu


def _free(s):
    """The solver goes after every tensor that went through the layer (ihm2_amd/torch_layer.py: Lifetime): the tests run their bodies in an
    inner function, whose tensors are gone when it returns."""
    gc.collect()
    s.free()


def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0", requires_grad=grad)


class _Case:
    """test_gpu_adjoint_weights.py::test_du0_dW_against_whole_solves' handle and start on hard_5_per_lane, B = 64, with the state every
    solve starts from kept for restoring."""

    def __init__(self, track, B=64):
        from ihm2_amd.solver import BatchedOcpSolver

        self.lay = lay = TABLE["hard_5_per_lane"][0]
        ocp = L.make_ocp(lay)
        ocp.solver_options.qp_tol = 1e-9
        ocp.solver_options.qp_solver_iter_max = 200
        self.s = s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
        L.apply(s.data, lay)
        s._push_weights(); s._push_bounds()
        self.B = B
        self.x0, self.yref, self.yref_e = _start(s, track, B, 1234)
        s.set_x0_sensitivities(1)
        self.x, self.u = s.get_x(), s.get_u()
        self.pi, self.lam = s.get_multipliers()
        self.slk = s.get_slacks()
        self.W0, self.We0 = np.asarray(s.data.W[0], dtype=np.float64), np.asarray(s.data.W_e, dtype=np.float64)

    def restore(self):
        s = self.s
        s.set_x(self.x); s.set_u(self.u); s.set_multipliers(self.pi, self.lam); s.set_slacks(self.slk)


def test_gradients_equal_the_host_adjoint_entrys_bits(track):
    c = _Case(track)
    _gradients(c)
    _free(c.s)


def _gradients(c):
    from ihm2_amd.torch_layer import rti_solve

    s, B, N = c.s, c.B, c.s.N
    rng = np.random.default_rng(11)
    cx, cu = rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2))
    # weights with a coupling, not exactly symmetric as given: the layer takes them at (W + W') / 2
    fac = (1.0 + 0.01 * np.arange(B))[:, None, None]

    def scale(Wm):
        w = np.abs(np.diag(Wm))
        return np.sqrt(np.outer(w, w))[None]

    W = fac * _coupled(c.W0, 0.05)[None] + 1e-3 * scale(c.W0) * rng.standard_normal((B, 12, 12))
    We = fac * _coupled(c.We0, 0.05)[None] + 1e-3 * scale(c.We0) * rng.standard_normal((B, 8, 8))
    Ws, Wes = (W + np.swapaxes(W, 1, 2)) * 0.5, (We + np.swapaxes(We, 1, 2)) * 0.5
    assert not np.array_equal(W, Ws)
    ins = [_t(a, grad=True) for a in (c.x0, c.yref, c.yref_e, W, We)]
    c.restore()
    x, u, status = rti_solve(s, *ins)
    assert x.shape == (B, N + 1, 8) and u.shape == (B, N, 2) and status.shape == (B,) and status.dtype == torch.int32
    assert x.requires_grad and u.requires_grad and not status.requires_grad
    loss = (_t(cx) * x).sum() + (_t(cu) * u).sum()
    grads = torch.autograd.grad(loss, ins)
    torch.cuda.synchronize()
    layer = dict(zip(("x0", "yref", "yref_e", "W", "W_e"), (g.cpu().numpy() for g in grads)))
    out_layer = dict(x=x.detach().cpu().numpy(), u=u.detach().cpu().numpy(), status=status.cpu().numpy())
    # the same state through the host setters
    c.restore()
    s.set_instance_weights(Ws, Wes)
    s.set_x0(c.x0); s.set_yref(c.yref); s.set_yref_e(c.yref_e)
    st = s.solve()
    host = s.eval_adjoint_weight_sensitivities(cx, cu)
    # (tests/bitcmp.py: a failure names the array, counts the differing entries and shows the first of them with both values)
    ok = (st == 0) | (st == 2)
    bitcmp.assert_same_bits("status", out_layer["status"], st)
    bitcmp.assert_same_bits("x", out_layer["x"], s.get_x(), nan_equal=True)
    bitcmp.assert_same_bits("u", out_layer["u"], s.get_u(), nan_equal=True)
    assert ok.mean() > 0.8
    for k in host:
        bitcmp.assert_same_bits(f"gradient in {k}", layer[k], host[k], nan_equal=True)
        bitcmp.assert_same_bits(f"gradient in {k}, solved instances", layer[k], host[k], rows=ok)
        assert np.isnan(layer[k][~ok]).all() and np.isfinite(layer[k][ok]).all(), k
    np.testing.assert_array_equal(layer["W"], np.swapaxes(layer["W"], 1, 2))
    np.testing.assert_array_equal(layer["W_e"], np.swapaxes(layer["W_e"], 1, 2))
    assert np.abs(layer["W"][ok]).max() > 0.0
    # one input asks for a gradient; without weights the solver's own stay (here: the per-instance ones just set)
    c.restore()
    a = [_t(c.x0), _t(c.yref, grad=True), _t(c.yref_e)]
    x2, u2, st2 = rti_solve(s, *a)
    (g,) = torch.autograd.grad((_t(cx) * x2).sum() + (_t(cu) * u2).sum(), [a[1]])
    bitcmp.assert_same_bits("gradient in yref, asked for alone", g.cpu().numpy(), host["yref"], nan_equal=True)


def test_weight_gradient_against_central_differences_of_the_layer(track):
    """test_gpu_adjoint_weights.py::test_du0_dW_against_whole_solves through the layer: the gradient of u_0 in (W, W_e) from backward,
    contracted with a symmetric direction, against central differences of rti_solve itself at W +- 1e-4 dW; its measure
    |pred - fd| / max(|fd|, |pred_free|) and its bars.

    Measured: 63 of 64 instances kept, median 5.4e-10, every instance below 1e-5, 5.1e-6 at worst."""
    c = _Case(track)
    _central_differences(c)
    _free(c.s)


def _central_differences(c):
    from ihm2_amd.torch_layer import rti_solve

    s, B, N, lay, eps = c.s, c.B, c.s.N, c.lay, 1e-4
    x, u, x0, yref, yref_e = c.x, c.u, c.x0, c.yref, c.yref_e
    rng = np.random.default_rng(77)

    def direction(Wm):
        w = np.abs(np.diag(Wm))
        G = rng.standard_normal((B,) + Wm.shape)
        return _sym(G) * np.sqrt(np.outer(w, w))[None]

    dW, dWe = direction(c.W0), direction(c.We0)
    tx0, tyref, tyref_e = _t(x0), _t(yref), _t(yref_e)

    def solve_at(sign, grad=False):
        c.restore()
        W, We = _t(c.W0[None] + sign * eps * dW, grad), _t(c.We0[None] + sign * eps * dWe, grad)
        xs, us, st = rti_solve(s, tx0, tyref, tyref_e, W, We)
        return W, We, us, st

    W, We, us, st_t = solve_at(0.0, grad=True)
    d = dict(W=np.empty((B, 2, 12, 12)), W_e=np.empty((B, 2, 8, 8)))
    for m in range(2):
        gW, gWe = torch.autograd.grad(us[:, 0, m].sum(), (W, We), retain_graph=(m == 0))
        d["W"][:, m], d["W_e"][:, m] = gW.cpu().numpy(), gWe.cpu().numpy()
    st = st_t.cpu().numpy()
    pred = np.einsum("bsij,bij->bs", d["W"], dW) + np.einsum("bsij,bij->bs", d["W_e"], dWe)
    o = _outputs(s)
    z, Z = L.soft_arrays(s.data, L.NC, None)
    A, Bm, b = s.get_linearization()
    zp = _zplus(o["x"], o["u"])
    keep, free = [], np.zeros((B, 2))
    for i in np.flatnonzero(st == 0):       # the weakly active instances have no derivative: skipped, as in the test this one follows
        qp = L.assemble_qp(s.data, x[i], u[i], x0[i], yref[i], yref_e[i], A[i], Bm[i], b[i], nonlinear=None)
        dz = np.zeros((N + 1, 10)); dz[:, :8] = o["x"][i] - x[i]; dz[:N, 8:] = o["u"][i] - u[i]
        if S.weakly_active(qp, dz, o["lam"][i], sl=o["slk"][i], soft_z=z, soft_Z=Z):
            continue
        keep.append(i)
        for m in range(2):
            sd = np.zeros((N + 1, 10)); sd[0, 8 + m] = 1.0
            zeta, _ = R.adjoint(qp, dz, 0.0 * o["lam"][i], o["slk"][i], z, Z, sd)
            gW, gWe = RW.weight_gradients(s.data, zeta, zp[i], yref[i], yref_e[i])
            free[i, m] = np.sum(gW * dW[i]) + np.sum(gWe * dWe[i])
    with torch.no_grad():
        _, _, up, stp = solve_at(1.0)
        up, stp = up[:, 0].cpu().numpy(), stp.cpu().numpy()
        _, _, um, stm = solve_at(-1.0)
        um, stm = um[:, 0].cpu().numpy(), stm.cpu().numpy()
    fd = (up - um) / (2 * eps)
    solved = (st == 0) & (stp == 0) & (stm == 0)
    keep = [i for i in keep if solved[i]]
    errs = np.array([np.abs(pred[i] - fd[i]).max() / max(np.abs(fd[i]).max(), np.abs(free[i]).max()) for i in keep])
    print(f"LAYER-FD: kept {len(keep)} of {B}, median {np.median(errs):.2e} share<=1e-5 {np.mean(errs <= 1e-5):.3f} "
          f"share<=1e-3 {np.mean(errs <= 1e-3):.3f} max {errs.max():.2e}")
    assert len(keep) >= 60, len(keep)
    assert np.median(errs) <= 1e-6 and np.mean(errs <= 1e-5) >= 0.75 and np.mean(errs <= 1e-3) >= 0.95, \
        (np.median(errs), np.mean(errs <= 1e-5), np.sort(errs)[-4:])


def _small(track, sens=1):
    from ihm2_amd.solver import BatchedOcpSolver

    B = 8
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    if sens:
        s.set_x0_sensitivities(sens)
    x0 = sample_x0(track, B, seed=9)
    x0[0, 1] = 5.0              # far outside the hard box on n: an infeasible QP, reported by its status
    s.set_x0(x0); s.init_guess()
    N = s.N
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + 40.0 * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = x0[:, 0] + 40.0
    state = (s.get_x(), s.get_u(), s.get_multipliers(), s.get_slacks())

    def restore():
        s.set_x(state[0]); s.set_u(state[1]); s.set_multipliers(*state[2]); s.set_slacks(state[3])

    return s, restore, x0, yref, yref_e


def test_zero_failed_zeroes_the_failed_rows_and_nothing_else(track):
    from ihm2_amd.torch_layer import rti_solve

    s, restore, x0, yref, yref_e = _small(track)

    def body():
        ins = [_t(x0, True), _t(yref, True), _t(yref_e, True)]
        res = []
        for zero_failed in (False, True):
            restore()
            x, u, status = rti_solve(s, *ins, zero_failed=zero_failed)
            g = torch.autograd.grad(x.sum() + 2.0 * u.sum(), ins)
            res.append(([a.cpu().numpy() for a in g], status.cpu().numpy()))
        return res

    (nan_g, st), (zero_g, st2) = body()
    _free(s)
    np.testing.assert_array_equal(st, st2)
    bad = ~np.isin(st, (0, 2))
    assert bad[0] and 0 < bad.sum() < len(st), st
    for a, b in zip(nan_g, zero_g):
        assert np.isnan(a[bad]).all() and (b[bad] == 0.0).all() and not np.signbit(b[bad]).any()
        np.testing.assert_array_equal(a[~bad].view(np.uint64), b[~bad].view(np.uint64))
        assert np.isfinite(a[~bad]).all()


def test_guards(track):
    from ihm2_amd._lib import Ihm2mpcError
    from ihm2_amd.torch_layer import rti_solve

    s, restore, x0, yref, yref_e = _small(track)

    def body():
        ins = [_t(x0, True), _t(yref, True), _t(yref_e, True)]
        # a setter of the solver between forward and backward
        x, u, _ = rti_solve(s, *ins)
        s.set_yref(yref)
        with pytest.raises(RuntimeError, match="between this solve and its backward"):
            (x.sum() + u.sum()).backward()
        # a second backward through one graph: torch's own error
        restore()
        x, u, _ = rti_solve(s, *ins)
        loss = x.sum() + u.sum()
        loss.backward()
        assert all(t.grad is not None for t in ins)
        with pytest.raises(RuntimeError, match="second time"):
            loss.backward()
        # the layer's own argument check comes before any GPU call
        with pytest.raises(TypeError, match="yref must be float64"):
            rti_solve(s, ins[0], ins[1].detach().float(), ins[2])
        with pytest.raises(ValueError, match="x0 must be on cuda:0"):
            rti_solve(s, ins[0].detach().cpu(), ins[1], ins[2])
        # the solver outlives the tensors that went through the layer: free() refuses while the memory of one is alive -- a view counts
        torch.cuda.synchronize()
        return u.detach()[:, 0]

    u0 = body()
    gc.collect()
    with pytest.raises(RuntimeError, match="still alive"):
        s.free()
    del u0
    _free(s)
    # x0 sensitivities off: the library's refusal, as it is
    s, restore, x0, yref, yref_e = _small(track, sens=0)
    with pytest.raises(Ihm2mpcError, match="x0 sensitivities are off: ihm2mpc_set_x0_sensitivities"):
        rti_solve(s, _t(x0), _t(yref), _t(yref_e))
    _free(s)
