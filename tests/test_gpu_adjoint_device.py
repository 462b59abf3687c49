"""The adjoint entry with seeds and gradients in device memory (ihm2mpc_eval_adjoint_sensitivities_w_device) against the host entry
(ihm2mpc_eval_adjoint_sensitivities_w): the same bits in all five outputs, NULL seeds and NULL outputs, nothing else of the handle moves,
the same refusals with the same texts; and the device setters of yref / yref_e against the host setters."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

from devmem import DevMem
from test_gpu_adjoint import _finite_where_solved, _seeds
from test_gpu_qp_layouts import TABLE, _solver, _start
from test_gpu_sensitivity import _outputs

pytestmark = pytest.mark.gpu

KEYS = ("x0", "yref", "yref_e", "W", "W_e")


def _shapes(B, S, N):
    return dict(x0=(B, S, 8), yref=(B, S, N, 12), yref_e=(B, S, 8), W=(B, S, 12, 12), W_e=(B, S, 8, 8))


def _device_call(s, dm, S, seed_x, seed_u, want=KEYS):
    """The device entry on fresh output arrays filled with 0xFF bytes; returns the downloaded outputs asked for."""
    sh = _shapes(s.B, S, s.N)
    out = {k: dm.alloc(8 * int(np.prod(sh[k])), fill=0xFF) for k in want}
    s.eval_adjoint_weight_sensitivities_device(S, 0 if seed_x is None else dm.up(seed_x), 0 if seed_u is None else dm.up(seed_u),
                                               **{"grad_" + k: out.get(k, 0) for k in KEYS})
    s.synchronize()
    return {k: dm.down(out[k], sh[k]) for k in want}


@pytest.mark.parametrize("name", ["hard_5_per_lane", "path_soft_4_per_lane"])
@pytest.mark.parametrize("B", [1, 96])
def test_device_entry_gives_the_host_entrys_bits(track, B, name):
    dm = DevMem()
    s = _solver(track, TABLE[name][0], B, "default", "0")
    _start(s, track, B, 55)
    s.set_x0_sensitivities(1)
    st = s.solve()
    ok = (st == 0) | (st == 2)
    if B > 1:
        assert 0.5 < ok.mean()
    before = dict(_outputs(s), u0=s.get_u0())
    seed_x, seed_u = _seeds(B, 8, s.N, 7)
    nan_rows = 0
    for S, sx, su in ((1, seed_x[:, :1], seed_u[:, :1]), (8, seed_x, seed_u), (2, None, None), (3, seed_x[:, :3], None), (3, None, seed_u[:, :3])):
        host = s.eval_adjoint_weight_sensitivities(None if sx is None else np.ascontiguousarray(sx), None if su is None else np.ascontiguousarray(su))
        dev = _device_call(s, dm, S, sx, su)
        host_after = s.eval_adjoint_weight_sensitivities(None if sx is None else np.ascontiguousarray(sx), None if su is None else np.ascontiguousarray(su))
        for k in KEYS:
            # (assert_array_equal takes NaN at equal positions for equal: a 0xFF fill left standing is a NaN of another payload, so the
            # bits are compared where the host has numbers and the NaN rows by position)
            np.testing.assert_array_equal(dev[k], host[k], err_msg=f"S {S} {k}")
            np.testing.assert_array_equal(dev[k][ok].view(np.uint64), host[k][ok].view(np.uint64), err_msg=f"S {S} {k}")
            np.testing.assert_array_equal(host_after[k], host[k], err_msg=f"S {S} {k}: the host entry after the device call")
        _finite_where_solved(dev, ok)       # every entry written: numbers where solved, NaN rows where not
        nan_rows += int((~ok).sum())
    # a NULL output is skipped (its neighbours are the same bits); all outputs NULL is accepted
    part = _device_call(s, dm, 8, seed_x, seed_u, want=("yref", "W_e"))
    full = s.eval_adjoint_weight_sensitivities(seed_x, seed_u)
    for k in part:
        np.testing.assert_array_equal(part[k], full[k], err_msg=k)
    s.eval_adjoint_weight_sensitivities_device(8, dm.up(seed_x), dm.up(seed_u))
    s.eval_adjoint_weight_sensitivities_device(2)
    s.synchronize()
    after = dict(_outputs(s), u0=s.get_u0())
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    s.free(); dm.free()


def test_nan_rows_coincide(track):
    from ihm2_amd.solver import BatchedOcpSolver

    B = 8
    dm = DevMem()
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_x0_sensitivities(1)
    x0 = sample_x0(track, B, seed=9)
    x0[0, 1] = 5.0              # far outside the hard box on n: an infeasible QP (test_gpu_adjoint_weights.py's instance)
    s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
    st = s.solve()
    ok = (st == 0) | (st == 2)
    assert not ok[0] and ok[1:].mean() > 0.5, st
    seed_x, seed_u = _seeds(B, 2, s.N, 3)
    host = s.eval_adjoint_weight_sensitivities(seed_x, seed_u)
    dev = _device_call(s, dm, 2, seed_x, seed_u)
    _finite_where_solved(dev, ok)
    for k in KEYS:
        np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
    s.free(); dm.free()


def test_refusals_are_the_host_entrys(track):
    from ihm2_amd._lib import Ihm2mpcError
    from ihm2_amd.solver import BatchedOcpSolver

    B = 8
    dm = DevMem()
    N = 40
    seed_x, seed_u = _seeds(B, 8, N, 1)
    dsx, dsu = dm.up(np.concatenate([seed_x, seed_x[:, :1]], 1)), dm.up(seed_u)         # room for nine seeds

    def both(s, S, sx, su, dx, du, match):
        """The host entry's and the device entry's refusal of the same call: one text."""
        from ihm2_amd import _lib

        nul = [None] * 5
        ptr = lambda a: None if a is None else a.ctypes.data_as(_lib.c_double_p)        # noqa: E731
        with pytest.raises(Ihm2mpcError, match=match) as eh:
            _lib.check(s.lib.ihm2mpc_eval_adjoint_sensitivities_w(s._h, S, ptr(sx), ptr(su), *nul))
        with pytest.raises(Ihm2mpcError, match=match) as ed:
            s.eval_adjoint_weight_sensitivities_device(S, dx, du)
        assert str(ed.value) == str(eh.value)

    sq = BatchedOcpSolver(make_ocp(nlp_solver_type="SQP", nlp_solver_max_iter=2), B, track.s_ref, track.kappa_ref)
    both(sq, 2, None, None, 0, 0, "SQP")
    sq.free()
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    both(s, 2, None, None, 0, 0, "off")
    s.set_x0_sensitivities(1)
    both(s, 2, None, None, 0, 0, "no solve")
    s.set_x0(sample_x0(track, B, seed=9)); s.init_guess(); s.prepare_step(40.0)
    s.solve()
    nine = np.zeros((B, 9, N + 1, 8))
    for n in (0, 9, -1):
        both(s, n, nine, None, dsx, 0, "1 to 8 seeds")
    for n in (1, 3, 8):
        both(s, n, None, None, 0, 0, "both NULL")
    s.run_steps(40.0, 2, model=0, M_sim=25)
    both(s, 2, None, None, 0, 0, "run_steps")
    s.prepare_step(40.0)
    s.solve()
    s.eval_adjoint_weight_sensitivities_device(8, dsx, dsu)         # readable again after a solve
    s.synchronize()
    s.set_x0_sensitivities(0)
    both(s, 2, None, None, 0, 0, "off")
    s.free(); dm.free()


def test_device_setters_of_the_references_give_the_host_setters_solve(track):
    B = 96
    dm = DevMem()
    lay = TABLE["hard_5_per_lane"][0]
    res = []
    for device in (False, True):
        s = _solver(track, lay, B, "default", "0")
        x0, yref, yref_e = _start(s, track, B, 55)
        yref = yref + 0.01 * np.random.default_rng(5).standard_normal(yref.shape)
        yref_e = yref_e + 0.01 * np.random.default_rng(6).standard_normal(yref_e.shape)
        if device:
            s.set_yref_device(dm.up(yref)); s.set_yref_e_device(dm.up(yref_e))
        else:
            s.set_yref(yref); s.set_yref_e(yref_e)
        st = s.solve()
        res.append(dict(_outputs(s), status=st, qp_iter=s.get_qp_iter()))
        s.free()
    for k in res[0]:
        np.testing.assert_array_equal(res[1][k], res[0][k], err_msg=k)
    assert (res[0]["status"] == 0).mean() > 0.5
    # the perturbed references reached the solve
    s = _solver(track, lay, B, "default", "0")
    _start(s, track, B, 55)
    s.solve()
    assert not np.array_equal(s.get_u(), res[0]["u"])
    s.free(); dm.free()
