"""The followed stationarity residual of the full slot form stays in its lane's registers between two updates (ihm2_amd/csrc/kernels_qp.hip,
S:17: rg_own) instead of going through HBM.  The general slot form (IHM2MPC_QP_FORM=2: the same factor sweep, the same horizon compiled in)
keeps the residual in memory and is the reference that is not the code under test: everything a solve leaves behind is equal byte for byte
between the two.

N = 40 (the full form takes no other horizon).  B = 3: fewer instances than a compute unit's four; B = 67: more than one block, an odd count.
One process per form (tests/element_round_trips_child.py through tests/qp_forms.py), each with three step() calls and one run_steps launch of
three per batch size, at the OCP's own QP tolerance and at 1e-12.

That the comparison means something: every solve takes at least four iterations, so the residual is carried over several updates; and at
1e-12 the followed residuals pass the convergence test before the residuals formed from the data do, so that the solve goes on in exact_mode,
where the update is skipped and the residual comes from the data in every iteration -- the other path.  Whether a solve did that is not
among its outputs; the oracle restates the same rule (oracle/ihm2_oracle_qp.c) and is traced on the same inputs: an instance it saw go on in
exact_mode, solved by both forms as by the oracle.  A NaN in x0[1, 1] reaches the residual of the first iteration: codes
and bit patterns are the general form's, and the neighbours in the batch are what the clean batch gave them."""
import numpy as np
import pytest

import qp_forms as QF

pytestmark = pytest.mark.gpu

CHILD = QF.CHILD.replace("qp_forms_child.py", "element_round_trips_child.py")
BATCHES = (3, 67)
TOLS = ("d", "t")
NAN_AT = 1
FULL, GENERAL = None, "2"


def runs(level):
    return QF.runs(level, child=CHILD)


@pytest.mark.parametrize("B", BATCHES)
def test_the_forms_ran(B):
    for level in (GENERAL, FULL):
        for tol in TOLS:
            assert runs(level)[f"b{B}_{tol}_kernels"].tolist() == QF.kernels(level), (level, tol)
        for case in ("clean", "x0"):
            assert runs(level)[f"b{B}_{case}_kernels"].tolist() == list(QF.qp_record(level)), (level, case)
    assert QF.FORMS[FULL][1] == "full" and QF.FORMS[GENERAL][1] == "general"


@pytest.mark.parametrize("path", ["step", "loop"])
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("B", BATCHES)
def test_every_solve_carries_the_residual_over_several_updates(B, tol, path):
    ref = runs(GENERAL)
    it, st = ref[f"b{B}_{tol}_{path}_hist_qp_iter"], ref[f"b{B}_{tol}_{path}_hist_status"]
    print(f"B {B} tolerance {tol} {path}: qp_iter {it.min()}..{it.max()}, status 0 in {(st == 0).mean():.2f}")
    assert it.min() >= 4, "at least four iterations per solve"


@pytest.mark.parametrize("B", BATCHES)
def test_a_solve_went_on_in_exact_mode(B):
    full, gen = runs(FULL), runs(GENERAL)
    went_on = gen[f"b{B}_clean_orc_exact_went_on"]
    # (at 1e-12 of the gradient's scale the iteration counts of the GPU and of the oracle differ by one or two -- the test is decided by the
    # rounding of the factorisation, which is the mechanism itself -- so the count is printed, not compared)
    same = (gen[f"b{B}_clean_status"] == gen[f"b{B}_clean_orc_status"]) & (gen[f"b{B}_clean_status"] == 0)
    print(f"B {B}: the oracle saw {int(went_on.sum())} of {B} solves go on in exact_mode at 1e-12; {int((went_on & same).sum())} of them solved by the "
          f"general form as by the oracle (qp_iter {gen[f'b{B}_clean_qp_iter'][went_on]}, the oracle's {gen[f'b{B}_clean_orc_qp_iter'][went_on]})")
    assert (went_on & same).any(), "no solve that entered exact_mode and went on"
    QF.same_bytes(full[f"b{B}_clean_orc_exact_went_on"], went_on, "the two processes traced different oracle solves")
    QF.compare(full, gen, [f"b{B}_clean_{k}" for k in QF.SOLVE_KEYS], QF.same_bytes, what="1e-12: full against IHM2MPC_QP_FORM=2")


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("B", BATCHES)
def test_three_steps_give_the_general_forms_bits(B, tol):
    """three step() calls and one run_steps launch of three: status, qp_iter, x, u, pi, lam, the slacks, get_qp_residuals(),
    get_residuals(), u0 and the histories, byte for byte"""
    names = [f"b{B}_{tol}_{path}_{k}" for path in ("step", "loop") for k in QF.PATH_KEYS]
    QF.compare(runs(FULL), runs(GENERAL), names, QF.same_bytes, what="full against IHM2MPC_QP_FORM=2")


@pytest.mark.parametrize("B", BATCHES)
def test_a_nan_in_x0_gives_the_general_forms_codes_and_bits(B):
    full, gen = runs(FULL), runs(GENERAL)
    at = min(NAN_AT, B - 1)
    x0 = full[f"b{B}_x0_in_x0"]
    QF.same_bytes(x0, gen[f"b{B}_x0_in_x0"], "the two processes were given different x0")
    assert np.isnan(x0[at, 1]) and np.isnan(x0).sum() == 1
    st, res = gen[f"b{B}_x0_status"], gen[f"b{B}_x0_qp_res"]
    print(f"B {B}: NaN in x0[{at}, 1]: general form status {st[at]} qp_iter {gen[f'b{B}_x0_qp_iter'][at]} qp_res {res[at]}")
    assert st[at] != 0 and np.isnan(res[at]).any(), "the NaN reaches the QP's residuals"
    QF.compare(full, gen, [f"b{B}_x0_{k}" for k in QF.SOLVE_KEYS], QF.same_bytes, what="NaN in x0: full against IHM2MPC_QP_FORM=2")
    for k in QF.SOLVE_KEYS:
        QF.same_bytes(np.delete(full[f"b{B}_x0_{k}"], at, axis=0), np.delete(full[f"b{B}_clean_{k}"], at, axis=0), f"a neighbour of the NaN instance moved: {k}")
