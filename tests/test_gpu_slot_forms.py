"""The forms of the interior-point QP's slot phases (ihm2_amd/csrc/kernels_qp.hip: qp_wave_body, FULL): the general form, which asks every
slot in every loop whether it exists and which of its sides do, and the full form of k_qp_wave<5,0,0,1> / k_steps<5,0,0,1,0,0,0> at the
horizon 40, which asks nothing -- for the tables csrc/qp_tables.hpp: slot_table_full lets through (tests/test_slot_table_full.py walks
the predicate on the CPU).  The reference's rows are full at N = 40 only, so every case here is B = 8, N = 40: only the batch shrinks.

The oracle's tolerance (1e-9 on x and u, status and iteration counts equal) is that of tests/test_gpu_factor_sweep_forms.py; the seeds
are chosen on the CPU (tools/find_factor_sweep_seeds.py --slot-forms, from the oracle's Stanley guess; the cases here start from the
handle's init_guess and assert the same properties on what they run): 0 is the first for which the oracle alone returns status 0 on all 8 instances,
1 the next, and in both solutions rate rows and boxes are active (multipliers up to 5e4 and 8e3), so every slot's arithmetic matters.

Per-instance bounds must have the shared table's finite sides (ihm2mpc_set_instance_bounds refuses anything else), so "one instance with
an infinite side" cannot reach a handle whose shared table is full: the test checks that refusal, and runs the per-instance fallback on
a shared table that has the infinite side itself.

tests/test_gpu_factor_sweep_forms.py is unchanged: its "plain_n40" leg (environment unset) now runs the full slot form, which reports the
same qp_form.  The general-slot kernels with the horizon compiled in are compared here, IHM2MPC_QP_FORM=2 against the full form, and there
the full form against the general factor sweep."""
import numpy as np
import pytest
from conftest import make_ocp

import drive
import qp_forms as QF
from qp_forms import QP, STEPS

pytestmark = pytest.mark.gpu

B = 8
SEED_PLAIN, SEED_ACTIVE = 0, 1
# the row whose upper side the fallback cases take away: v_x of stage 17 (far from the iterate: the solution is that of the full table
# to rounding, the table is not full)
OPEN = (17, 3)


def _x0(track, seed):
    return drive.clipped_start(track, B, seed)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


def _solver(track, monkeypatch):
    from ihm2_amd.solver import BatchedOcpSolver

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_lap_wrap(True)
    return s


_ORACLE = {}


def _oracle(track, s, seed, open_side):
    """the oracle's rti_step on the handle's problem from the handle's guess, once per (seed, bounds): (out, x, u), left unchanged"""
    key = (seed, open_side)
    if key not in _ORACLE:
        from oracle import oracle as orc

        P = orc.OracleProblem(s.data.as_dict(track.s_ref, track.kappa_ref))
        x0, x, u = _x0(track, seed), s.get_x(), s.get_u()
        yref, yref_e = orc.prepare_step(s.N, x0, 40.0, x, u)
        out = P.rti_step(x, u, x0, yref, yref_e)
        assert np.all(out["status"] == 0), "the seed is chosen so that the oracle solves all instances"
        lam = out["lam"].reshape(B, s.N + 1, 2, -1)
        assert lam[..., 10:12].max() > 1e-3 and lam[..., 0:10].max() > 1e-3, "an active rate row and an active box"
        _ORACLE[key] = (out, x, u)
    return _ORACLE[key]


def _solve_against_oracle(track, s, seed, slots, open_side=False):
    """init_guess + prepare_step + solve() on the handle as it stands, against the oracle; the launch record names the slot form"""
    s.set_x0(_x0(track, seed)); s.init_guess()
    s.set_multipliers(None, None)
    out, x, u = _oracle(track, s, seed, open_side)
    s.prepare_step(40.0)
    st = s.solve()
    rec = s.get_launch_record()
    assert rec["qp"] == QP and rec["qp_form"] == "plain_n40" and rec["qp_slots"] == slots, rec
    np.testing.assert_array_equal(st, out["status"])
    np.testing.assert_array_equal(s.get_qp_iter(), out["qp_iter"])
    ex, eu = _rel(s.get_x(), x), _rel(s.get_u(), u)
    print(f"seed {seed} slots {slots}: GPU vs oracle x {ex:.2e} u {eu:.2e}, qp_iter {out['qp_iter'].tolist()}")
    assert ex < 1e-9 and eu < 1e-9


def _open_one_side(s, absent):
    s.data.ubx = np.array(s.data.ubx, dtype=np.float64)
    s.data.ubx[OPEN] = absent
    s._push_bounds()


@pytest.mark.parametrize("seed", [SEED_PLAIN, SEED_ACTIVE])
def test_full_form_against_the_oracle(track, seed, monkeypatch):
    s = _solver(track, monkeypatch)
    _solve_against_oracle(track, s, seed, "full")
    s.free()


def test_one_infinite_side_takes_the_general_form_and_the_finite_bound_brings_the_full_form_back(track, monkeypatch):
    s = _solver(track, monkeypatch)
    closed = float(np.asarray(s.data.ubx)[OPEN])
    _open_one_side(s, 1e20)
    _solve_against_oracle(track, s, SEED_PLAIN, "general", open_side=True)
    h = s.run_steps(40.0, 1, model=-1, M_sim=30, status_hist=True)
    rec = s.get_launch_record()
    assert rec["steps"] == STEPS and rec["steps_form"] == "plain_n40" and rec["steps_slots"] == "general", rec
    _open_one_side(s, closed)
    _solve_against_oracle(track, s, SEED_PLAIN, "full")
    h = s.run_steps(40.0, 1, model=-1, M_sim=30, status_hist=True)
    rec = s.get_launch_record()
    assert rec["steps"] == STEPS and rec["steps_slots"] == "full" and np.all(h["status"] == 0), rec
    s.free()


def _instance_bounds(s):
    d, N = s.data, s.N
    t = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(shape), (B,) + shape))
    return [t(d.lbx, (N + 1, 8)), t(d.ubx, (N + 1, 8)), t(d.lbu, (N, 2)), t(d.ubu, (N, 2)), t(d.lg, (N, 2)), t(d.ug, (N, 2))]


def test_per_instance_bounds(track, monkeypatch):
    """Finite per-instance bounds (the shared values, so that the shared oracle is the reference) keep the full form; an infinite side in
    one instance is refused against a full shared table and leaves the handle as it was; on a shared table with that side infinite the
    per-instance bounds run the general form; back on shared, finite bounds the full form returns."""
    from ihm2_amd._lib import Ihm2mpcError

    s = _solver(track, monkeypatch)
    arrs = _instance_bounds(s)
    s.set_instance_bounds(*arrs)
    _solve_against_oracle(track, s, SEED_PLAIN, "full")
    broken = [a.copy() for a in arrs]
    broken[1][3][OPEN] = np.inf
    with pytest.raises(Ihm2mpcError, match="finite sides"):
        s.set_instance_bounds(*broken)
    _solve_against_oracle(track, s, SEED_PLAIN, "full")
    # the shared table with the open side, then per-instance bounds in its pattern
    closed = float(np.asarray(s.data.ubx)[OPEN])
    s.set_instance_bounds()
    _open_one_side(s, 1e20)
    s.set_instance_bounds(*_instance_bounds(s))
    _solve_against_oracle(track, s, SEED_PLAIN, "general", open_side=True)
    s.set_instance_bounds()
    _open_one_side(s, closed)
    _solve_against_oracle(track, s, SEED_PLAIN, "full")
    s.free()


def test_forms_give_the_same_bits():
    """Three control steps through step() and the same three in one run_steps launch, in the full form and in the general slot form
    (IHM2MPC_QP_FORM=2: the straight-line factor sweep with the horizon compiled in, the default before the full form) -- one process
    each, the variable is read once (tests/qp_forms.py).  Between the forms everything is equal byte for byte; inside a form the two paths
    are equal too: B N = 320 is no latency batch (tests/launch_cases.py), which step() linearises and whose plant it integrates with other
    kernels than the loop (tests/test_gpu_factor_sweep_forms.py, tests/test_gpu_qp_layouts.py: KNOWN DIFFERENCE)."""
    got = {level: QF.runs(level) for level in ("2", None)}
    for level, run in got.items():
        assert run[f"b{B}_kernels"].tolist() == QF.kernels(level)
    ref = got["2"]
    keys = [f"b{B}_{p}_{k}" for p in ("step", "loop") for k in QF.PATH_KEYS]
    assert sorted(k for k in ref if k.startswith(f"b{B}_")) == sorted(keys + [f"b{B}_kernels"])
    assert (ref[f"b{B}_step_hist_status"] == 0).mean() > 0.9
    QF.compare(got[None], ref, keys, QF.same_bytes, what="full against general")
    paths = [(f"b{B}_step_{k}", f"b{B}_loop_{k}") for k in QF.PATH_KEYS if k != "res"]         # (the NLP residuals: between the forms only)
    for level, run in got.items():
        QF.compare(run, run, paths, what=f"{QF.FORMS[level][1]}: step() against run_steps")
