"""The line search of the SQP mode against the independent merit-function reference (tests/merit_ref.py), with the CPU oracle's
orc_sqp_solve as the implementation under test and no allowance for the integrator (the reference calls the oracle's own).  Proves the
reference and the conditions on every case's inputs without a GPU; tests/test_gpu_merit.py runs the same cases on the device."""
import pytest

import sqp_cases as SC


@pytest.fixture(scope="module")
def judged(track):
    cache = {}

    def get(name):
        if name not in cache:
            c = SC.make_case(track, name)
            cache[name] = SC.judge(c, SC.OracleDut(c))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(SC.CASES))
def test_oracle_line_search_lands_in_the_admissible_set_with_the_reference_merit_values(judged, name):
    fig, refs, walks = judged(name)
    assert fig["worst"] <= 1.0


@pytest.mark.parametrize("name,drop", [(n, d) for n, spec in SC.CASES.items() for d in spec.get("targets", ())])
def test_the_case_sees_the_term_it_targets(judged, name, drop):
    fig, refs, walks = judged(name)
    assert SC.mutant_is_rejected(refs, walks, drop), (name, drop)


def test_instances_that_meet_the_tolerances_are_left_alone(track):
    """Status 0, no iteration counted, step length 1, the iterate and the multipliers bit for bit, zeros in the merit read-back."""
    c = SC.make_case(track, "all_converged")
    fig, _, _ = SC.judge(c, SC.OracleDut(c), conditions=False)
    assert fig["ladder"] == 0


@pytest.mark.parametrize("keys", [("W", "W_e"), ("lbx", "ubx", "lbu", "ubu", "lg", "ug")], ids=["weights", "bounds"])
def test_instance_tuning_case_sees_whose_tables_the_merit_reads(track, monkeypatch, keys):
    """A reference that takes the neighbouring instance's weights, or its bounds, is rejected: a wrong per-instance stride cannot pass."""
    import copy

    import numpy as np

    c = SC.make_case(track, "instance_tuning")
    own = SC.merit_problem

    def neighbours(c_, b):
        c2 = copy.copy(c_)
        c2.inst = dict(c_.inst, **{k: np.roll(c_.inst[k], 1, axis=0) for k in keys})
        return own(c2, b)
    monkeypatch.setattr(SC, "merit_problem", neighbours)
    with pytest.raises(AssertionError):
        SC.judge(c, SC.OracleDut(c), verbose=False, conditions=False)
