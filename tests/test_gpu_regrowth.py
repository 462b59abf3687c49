"""GPU: the handle's buffers that grow on demand -- the run histories, the IRK line search's trial-point rollouts (one per step length of its
ladder) and the per-instance slot table.  A handle that regrows one mid-run gives, bit for bit, what a twin gives that had it at full size
before the compared calls; both start those calls from the same iterate, set explicitly."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

pytestmark = pytest.mark.gpu
B, N = 64, 40


def _iterate(s):
    pi, lam = s.get_multipliers()
    return dict(x0=s.get_x0(), x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks())


def _set_iterate(s, it):
    s.set_x0(it["x0"]); s.set_x(it["x"]); s.set_u(it["u"]); s.set_multipliers(it["pi"], it["lam"]); s.set_slacks(it["slk"])


def _outputs(s):
    out = _iterate(s)
    out.update(status=s.get_status(), qp_iter=s.get_qp_iter(), res=s.get_residuals(), qp_res=s.get_qp_residuals(), u0=s.get_u0())
    return out


def _run(s, it, n_steps, **kw):
    """The compared calls: two solves, then a run_steps of n_steps; everything they leave."""
    _set_iterate(s, it)
    out = []
    for _ in range(2):
        s.prepare_step(40.0)
        s.solve()
        out.append(_outputs(s))
    hist = s.run_steps(40.0, n_steps, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True, **kw)
    out += [hist, _outputs(s)]
    return out


def _histories(track, twin):
    """A longer run_steps after a shorter one (plain, then with the x0 sensitivities' gain history); the twin reserved the longer first."""
    from ihm2_amd.solver import BatchedOcpSolver

    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_x0_sensitivities(1)
    if twin:
        s.reserve_history(12)
    s.set_x0(sample_x0(track, B, seed=91)); s.init_guess()
    it = _iterate(s)
    out = _run(s, it, 5)
    out += _run(s, it, 12, sens_u0_hist=True)
    out.append(s.get_x0_sensitivities()[1])
    s.free()
    return out


def _ladder(track, twin):
    """SQP mode, IRK integrator, merit line search: alpha_reduction 0.7 (9 trial steps) -> 0.9 (29); the twin solved with 0.9 first."""
    from ihm2_amd.solver import BatchedOcpSolver

    ocp = make_ocp(M=1, nlp_solver_type="SQP", nlp_solver_max_iter=2, globalization="MERIT_BACKTRACKING", integrator_type="IRK")
    s = BatchedOcpSolver(ocp, B, track.s_ref, track.kappa_ref)
    s.set_x0(sample_x0(track, B, seed=92)); s.init_guess()
    it = _iterate(s)
    if not twin:
        s.prepare_step(40.0); s.solve()
    s.set_sqp_options(alpha_reduction=0.9)
    if twin:
        s.prepare_step(40.0); s.solve()
    out = _run(s, it, 3)
    out.append(s.get_sqp_stats())
    s.free()
    return out


def _slot_table(track, twin):
    """Per-instance bounds, then the (soft) track rows turned on: the slot table widens under them; the twin had the rows on first."""
    from test_gpu_instance_tuning import TUNINGS, _ocp, _set_mixed, _solver, _x0

    nk = track.s_ref.shape[-1]
    ocps = [_ocp(t, "track_rows", nk) for t in TUNINGS]
    s = _solver(track, ocps[0], B, "track_rows")
    if not twin:
        s.data.path_on = 0; s._push_path()
    _set_mixed(s, ocps, np.arange(B) % len(TUNINGS))
    if not twin:
        s.data.path_on = 1; s._push_path()
    s.set_x0(_x0(track, B, seed=93)); s.init_guess()
    out = _run(s, _iterate(s), 3)
    s.free()
    return out


def _assert_equal(a, b, path="out"):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _assert_equal(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_equal(x, y, f"{path}[{i}]")
    else:
        np.testing.assert_array_equal(a, b, err_msg=path)


@pytest.mark.parametrize("case", [_histories, _ladder, _slot_table], ids=["histories", "irk_ladder", "instance_slot_table"])
def test_regrown_buffer_equals_one_at_full_size(track, case):
    grown, twin = case(track, False), case(track, True)
    _assert_equal(grown, twin)
    assert np.isin(grown[1]["status"], (0, 2)).mean() > 0.5
