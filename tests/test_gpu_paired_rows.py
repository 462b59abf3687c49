"""The two layouts of the closed-loop matrices M_k in the QP's workspace (ihm2_amd/csrc/qp_mrows.hpp): the kernels with the horizon 40
compiled in -- the default (full slots) and IHM2MPC_QP_FORM=2 (general slots) -- keep them stage-pair-major and stream them back with one
16-byte load per two stages; IHM2MPC_QP_FORM=1 and =0 keep the stage-major rows and one 8-byte load per stage.  Same values, same operations
in the same order: everything a solve leaves behind is equal byte for byte between the four, after three step() calls and after one
run_steps launch of three steps.  (tests/test_qp_mrows.py walks the offsets on the CPU.)

N = 40, because the paired forms take no other horizon.  B = 3: fewer instances than a lane group, the first instance's backward prefetch
runs into the padding in front of the workspace and the last one's forward prefetch into the padding behind it; B = 67: more than one
block per compute unit's four, an odd count.  The start is the clipped one of tests/qp_forms_child.py (rate rows and boxes active, most solves
converge in 7 to 12 iterations), asserted below on what was run.

One process per form (the library reads the variable once; tests/qp_forms.py); each runs both batch sizes."""
import numpy as np
import pytest
from conftest import make_ocp

import drive
import qp_forms as QF
from qp_forms import QP, STEPS

pytestmark = pytest.mark.gpu

BATCHES = (3, 67)
PAIRED, STAGE_MAJOR = (None, "2"), ("1", "0")
KEYS = ("status", "qp_iter", "x", "u", "pi", "lam", "hist_u0", "hist_x0", "hist_status", "hist_qp_iter")
OPEN = (17, 3)      # the row of tests/test_gpu_slot_forms.py whose upper side the last case takes away


@pytest.mark.parametrize("B", BATCHES)
def test_the_forms_ran_and_the_solves_are_real(B):
    for level in QF.FORMS:
        assert QF.runs(level)[f"b{B}_kernels"].tolist() == QF.kernels(level), level
    ref = QF.runs("0")
    for path in ("step", "loop"):
        st, it = ref[f"b{B}_{path}_hist_status"], ref[f"b{B}_{path}_hist_qp_iter"]
        lam = ref[f"b{B}_{path}_lam"].reshape(B, 41, 2, -1)
        print(f"B {B} {path}: status 0 in {(st == 0).mean():.2f}, qp_iter {it.min()}..{it.max()}, lam boxes {lam[..., 0:10].max():.2e} rate rows {lam[..., 10:12].max():.2e}")
        assert (st == 0).mean() > 0.6 and it.min() >= 4, "several interior-point iterations per solve"
        assert lam[..., 0:10].max() > 1e-3 and lam[..., 10:12].max() > 1e-3, "an active box and an active rate row"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("paired", PAIRED, ids=["full_slots", "general_slots"])
@pytest.mark.parametrize("stage_major", STAGE_MAJOR, ids=["plain", "general_sweep"])
def test_paired_rows_give_the_stage_major_bits(B, paired, stage_major):
    names = [f"b{B}_{path}_{k}" for path in ("step", "loop") for k in KEYS]
    QF.compare(QF.runs(paired), QF.runs(stage_major), names, what=f"IHM2MPC_QP_FORM {paired} against {stage_major}")


def test_a_table_that_is_not_full_takes_the_paired_general_slot_kernel(track, monkeypatch):
    """One handle: the full table, then one infinite side (the general-slot kernel with the horizon compiled in: paired rows as well), then
    the finite bound again.  Every launch returns a solved batch and names its kernel; the last solve repeats the first byte for byte, so
    nothing of the rows the other kernel left in the workspace reaches a result."""
    from ihm2_amd.solver import BatchedOcpSolver

    B = 3
    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    monkeypatch.delenv("IHM2MPC_QP_FORM", raising=False)
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    s.set_lap_wrap(True)
    x0 = drive.clipped_start(track, B, 0)

    def solve(slots):
        s.set_x0(x0); s.init_guess()
        s.set_multipliers(None, None)
        s.prepare_step(40.0)
        st = s.solve()
        rec = s.get_launch_record()
        assert rec["qp"] == QP and rec["qp_form"] == "plain_n40" and rec["qp_slots"] == slots, rec
        assert np.all(st == 0) and np.all(np.isfinite(s.get_x())) and np.all(np.isfinite(s.get_u()))
        return s.get_x(), s.get_u(), s.get_qp_iter()

    def open_side(value):
        s.data.ubx = np.array(s.data.ubx, dtype=np.float64)
        s.data.ubx[OPEN] = value
        s._push_bounds()

    closed = float(np.asarray(s.data.ubx)[OPEN])
    first = solve("full")
    open_side(1e20)
    solve("general")
    h = s.run_steps(40.0, 1, model=-1, M_sim=30, status_hist=True)
    rec = s.get_launch_record()
    assert rec["steps"] == STEPS and rec["steps_form"] == "plain_n40" and rec["steps_slots"] == "general" and np.all(h["status"] == 0), rec
    open_side(closed)
    again = solve("full")
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    s.free()
