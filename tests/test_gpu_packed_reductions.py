"""The packed reductions of the full slot form (ihm2_amd/csrc/qp_reduce.hpp): the four norms of an interior-point iteration in one
butterfly with their NaNs surfaced by a ballot, the two step bounds in one butterfly, the set-up's scales and the NLP residuals likewise.
IHM2MPC_QP_FORM=2 -- the general slot form with the same factor sweep and the same horizon compiled in -- keeps the one-value butterflies and
nanmax, and is the bit-for-bit partner: everything a solve leaves behind is equal byte for byte between the two.  (tests/test_qp_reduce.py
runs the butterfly on software lanes.)

N = 40 (the full form takes no other horizon), the reference's table.  B = 3: fewer instances than the four of a compute unit; B = 67: more
than one block, an odd count.  One process per form (the library reads the variable once; tests/qp_forms.py); each runs both batch sizes.

NaN surfacing -- instance 1 of the batch gets a NaN through a public input, and which norm it reaches:
  * yref[1, 7, 3]: the QP gradient g of stage 7, so the stationarity residual r_g of the first iterate: res_g.  Nothing else: z, the
    dynamics residual and the slots do not see yref.  The QP's data are not numbers: status 1.
  * x0[1, 1]: dx_0 = x0 - x_0 is the first iterate's z_0: the dynamics residual of stage 0 (res_b) and the general rows C z_0 + D u_0 of
    stage 0, i.e. their slack residuals (res_d).  Not res_g: dx_0 is no variable, its stationarity rows are masked, and the reference's
    Hessian couples the lateral offset with no input.  Status 1.
  * lam[1, 5, 8] through set_multipliers: the incoming multipliers enter the NLP residuals of get_residuals() alone (stationarity and
    complementarity, taken with fmax: the NaN is dropped there, in both forms and in the oracle) -- the QP starts from its own multipliers,
    so no input reaches res_m, which is formed from lam t of the iteration's own positive values.  The solve is the clean one.
The oracle (CPU) confirms the codes; between the forms status, qp_iter, the residuals' bit patterns and the neighbours are equal."""
import numpy as np
import pytest
from conftest import make_ocp

import qp_forms as QF

pytestmark = pytest.mark.gpu

BATCHES = (3, 67)
NAN_AT = 1
LEVELS = ("2", None)        # the general slot form, the bit-for-bit partner, and the full form
PATH_KEYS, SOLVE_KEYS = QF.PATH_KEYS, QF.SOLVE_KEYS         # everything the child stores
INPUTS = ("x", "u", "x0", "yref", "yref_e", "pi", "lam")


_ORACLE = {}


def _oracle(track, B, case):
    """the oracle's rti_step on the inputs the child pushed, once per (B, case), left unchanged"""
    if (B, case) not in _ORACLE:
        from oracle import oracle as orc

        P = orc.OracleProblem(make_ocp().flatten().as_dict(track.s_ref, track.kappa_ref))
        i = {k: QF.runs(None)[f"b{B}_{case}_in_{k}"].copy() for k in INPUTS}
        out = P.rti_step(i["x"], i["u"], i["x0"], i["yref"], i["yref_e"], pi=i["pi"], lam=i["lam"])
        _ORACLE[(B, case)] = (out, i["x"], i["u"])
    return _ORACLE[(B, case)]


@pytest.mark.parametrize("B", BATCHES)
def test_the_forms_ran_and_the_solves_are_real(B):
    for level in LEVELS:
        assert QF.runs(level)[f"b{B}_kernels"].tolist() == QF.kernels(level), level
        for case in ("clean", "yref", "x0", "lam"):
            assert QF.runs(level)[f"b{B}_{case}_kernels"].tolist() == list(QF.qp_record(level)), (level, case)
    ref = QF.runs("2")
    for path in ("step", "loop"):
        st, it = ref[f"b{B}_{path}_hist_status"], ref[f"b{B}_{path}_hist_qp_iter"]
        lam = ref[f"b{B}_{path}_lam"].reshape(B, 41, 2, -1)
        print(f"B {B} {path}: status 0 in {(st == 0).mean():.2f}, qp_iter {it.min()}..{it.max()}, lam boxes {lam[..., 0:10].max():.2e} rate rows {lam[..., 10:12].max():.2e}")
        assert (st == 0).mean() > 0.6 and it.min() >= 4, "several interior-point iterations per solve"
        assert lam[..., 0:10].max() > 1e-3 and lam[..., 10:12].max() > 1e-3, "an active box and an active rate row"


@pytest.mark.parametrize("B", BATCHES)
def test_clean_batch_gives_the_general_forms_bits(B):
    """three step() calls and one run_steps launch of three: everything equal byte for byte, NaN payloads of failed instances included"""
    names = [f"b{B}_{path}_{k}" for path in ("step", "loop") for k in PATH_KEYS]
    QF.compare(QF.runs(None), QF.runs("2"), names, QF.same_bytes, what="full against IHM2MPC_QP_FORM=2")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", ["yref", "x0", "lam"])
def test_a_nan_surfaces_as_before(track, B, case):
    full, gen = QF.runs(None), QF.runs("2")
    at = min(NAN_AT, B - 1)
    QF.compare(full, gen, [f"b{B}_{case}_in_{k}" for k in INPUTS], QF.same_bytes, what="the two processes were given different inputs")
    assert np.isnan(full[f"b{B}_{case}_in_{case}"][at]).sum() == 1 and np.isnan(np.delete(full[f"b{B}_{case}_in_{case}"], at, axis=0)).sum() == 0
    out, _, _ = _oracle(track, B, case)
    clean, _, _ = _oracle(track, B, "clean")
    st, res = gen[f"b{B}_{case}_status"], gen[f"b{B}_{case}_qp_res"]
    print(f"B {B} NaN in {case} of instance {at}: oracle status {out['status'][at]}, general form status {st[at]} qp_iter {gen[f'b{B}_{case}_qp_iter'][at]} qp_res {res[at]}")
    # the reference's codes: not-a-number in the QP's data is status 1, found in the first iteration; the neighbours solve as in the clean batch
    expected = clean["status"][at] if case == "lam" else 1
    assert out["status"][at] == expected, "the oracle's code"
    np.testing.assert_array_equal(np.delete(out["status"], at), np.delete(clean["status"], at))
    np.testing.assert_array_equal(st, out["status"])
    # the norm the input reaches (module docstring), in the partner form -- the full form must then show the same bits
    nan_norms = np.isnan(res[at]).tolist()
    if case == "yref":
        assert nan_norms == [True, False, False, False], res[at]
    elif case == "x0":
        assert nan_norms == [False, True, True, False], res[at]
    else:
        assert not any(nan_norms), res[at]
    QF.compare(full, gen, [f"b{B}_{case}_{k}" for k in SOLVE_KEYS], QF.same_bytes, what="full against IHM2MPC_QP_FORM=2")
    # the untouched neighbours: what the clean batch gave them, byte for byte
    for k in SOLVE_KEYS:
        QF.same_bytes(np.delete(full[f"b{B}_{case}_{k}"], at, axis=0), np.delete(full[f"b{B}_clean_{k}"], at, axis=0), f"a neighbour of the NaN instance moved: {k}")


def test_full_form_against_the_oracle(track):
    """B = 3, one solve from the oracle's own inputs: status and qp_iter equal, x and u to 1e-9 (the tolerance of tests/test_gpu_slot_forms.py),
    with an active box and an active rate row in the oracle's solution"""
    B = BATCHES[0]
    out, x, u = _oracle(track, B, "clean")
    got = QF.runs(None)
    lam = out["lam"].reshape(B, 41, 2, -1)
    assert np.any(out["status"] == 0) and lam[..., 10:12].max() > 1e-3 and lam[..., 0:10].max() > 1e-3, "a solved instance, an active rate row and an active box"
    np.testing.assert_array_equal(got[f"b{B}_clean_status"], out["status"])
    np.testing.assert_array_equal(got[f"b{B}_clean_qp_iter"], out["qp_iter"])
    ok = out["status"] == 0
    rel = lambda a, b: float(np.max(np.abs(a - b) / (1 + np.abs(b))))
    ex, eu = rel(got[f"b{B}_clean_x"][ok], x[ok]), rel(got[f"b{B}_clean_u"][ok], u[ok])
    print(f"full form against the oracle: x {ex:.2e} u {eu:.2e}, qp_iter {out['qp_iter'].tolist()}, status {out['status'].tolist()}")
    assert ex < 1e-9 and eu < 1e-9
