"""The general rows of the full slot form, evaluated once per phase (ihm2_amd/csrc/kernels_qp.hip: general_rows): before each loop over
a lane's slots one pass forms [C D] v_k of all 2 N (stage, row) pairs into the transpose tile, and a general-row slot reads its word there
like a box slot reads its word of v -- the ten products of the chain the form evaluated per slot before, in their order.  The general
slot form (IHM2MPC_QP_FORM=2: the same factor sweep, the same horizon compiled in) keeps row_dot's chain per slot and is the reference
that is not the code under test: everything a solve leaves behind is equal byte for byte between the two.  (tests/test_qp_general_rows.py
walks the tile offsets and the reach statement on the CPU.)

N = 40 (the full form takes no other horizon).  B = 3: fewer instances than a compute unit's four; B = 67: more than one block, an odd
count.  One process per form (tests/qp_forms.py), each with three step() calls and one run_steps launch of three per batch size.

That the comparison means something: a rate row (rows 10, 11 of a stage) carries a multiplier above 1e-3 at stage 0 -- whose tile words
are the first two -- and at stage N - 1 -- the last two, 78 and 79, which only the lanes 14 and 15 write, as their second element; every
solve takes at least four iterations, so the tile is rewritten behind several factor sweeps, which park stores in it.  A NaN in x0[1, 1]
is z_0's lateral offset in the first iterate: it reaches C z_0, the general rows' slack residuals of stage 0, through the tile -- codes and
bit patterns are the general form's, and the neighbours in the batch are what the clean batch gave them."""
import numpy as np
import pytest

import qp_forms as QF

pytestmark = pytest.mark.gpu

BATCHES = (3, 67)
N = 40
NAN_AT = 1
FULL, GENERAL = None, "2"


def _rate_rows(lam, B):
    """the multipliers of the rate rows, (B, N + 1, side, row 10 | 11)"""
    return lam.reshape(B, N + 1, 2, -1)[..., 10:12]


@pytest.mark.parametrize("B", BATCHES)
def test_the_forms_ran(B):
    for level in (GENERAL, FULL):
        assert QF.runs(level)[f"b{B}_kernels"].tolist() == QF.kernels(level), level
        assert QF.runs(level)[f"b{B}_x0_kernels"].tolist() == list(QF.qp_record(level)), level
    assert QF.FORMS[FULL][1] == "full" and QF.FORMS[GENERAL][1] == "general"


@pytest.mark.parametrize("path", ["step", "loop"])
@pytest.mark.parametrize("B", BATCHES)
def test_the_general_rows_matter(B, path):
    ref = QF.runs(GENERAL)
    it, st = ref[f"b{B}_{path}_hist_qp_iter"], ref[f"b{B}_{path}_hist_status"]
    rate = _rate_rows(ref[f"b{B}_{path}_lam"], B)
    first, last = rate[:, 0].max(), rate[:, N - 1].max()
    print(f"B {B} {path}: qp_iter {it.min()}..{it.max()}, status 0 in {(st == 0).mean():.2f}, rate-row multipliers: stage 0 {first:.3e}, stage {N - 1} {last:.3e}")
    assert it.min() >= 4, "at least four iterations per solve"
    assert first > 1e-3, "an active rate row at stage 0"
    assert last > 1e-3, f"an active rate row at stage {N - 1}"


@pytest.mark.parametrize("B", BATCHES)
def test_three_steps_give_the_general_forms_bits(B):
    """three step() calls and one run_steps launch of three: status, qp_iter, x, u, pi, lam, the slacks, get_qp_residuals(),
    get_residuals(), u0 and the histories, byte for byte"""
    names = [f"b{B}_{path}_{k}" for path in ("step", "loop") for k in QF.PATH_KEYS]
    QF.compare(QF.runs(FULL), QF.runs(GENERAL), names, QF.same_bytes, what="full against IHM2MPC_QP_FORM=2")


@pytest.mark.parametrize("B", BATCHES)
def test_a_nan_in_x0_comes_through_the_tile_as_through_the_chain(B):
    full, gen = QF.runs(FULL), QF.runs(GENERAL)
    at = min(NAN_AT, B - 1)
    x0 = full[f"b{B}_x0_in_x0"]
    QF.same_bytes(x0, gen[f"b{B}_x0_in_x0"], "the two processes were given different x0")
    assert np.isnan(x0[at, 1]) and np.isnan(x0).sum() == 1
    st, res = gen[f"b{B}_x0_status"], gen[f"b{B}_x0_qp_res"]
    print(f"B {B}: NaN in x0[{at}, 1]: general form status {st[at]} qp_iter {gen[f'b{B}_x0_qp_iter'][at]} qp_res {res[at]}")
    # C z_0: the slack residuals of the general rows of stage 0 (res_d, the third norm) are not numbers; the instance fails
    assert st[at] != 0 and np.isnan(res[at][2]), "the NaN reaches the general rows' slack residuals"
    QF.compare(full, gen, [f"b{B}_x0_{k}" for k in QF.SOLVE_KEYS], QF.same_bytes, what="NaN in x0: full against IHM2MPC_QP_FORM=2")
    for k in QF.SOLVE_KEYS:
        QF.same_bytes(np.delete(full[f"b{B}_x0_{k}"], at, axis=0), np.delete(full[f"b{B}_clean_{k}"], at, axis=0), f"a neighbour of the NaN instance moved: {k}")
