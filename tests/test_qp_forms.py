"""tests/qp_forms.py without a GPU: the two strengths of the comparison, and the runner's memory of a child that failed."""
import numpy as np
import pytest

import qp_forms as QF


def _bits(values):
    return np.array(values, dtype=np.uint64).view(np.float64)


def test_same_bytes_sees_a_nan_payload_and_same_values_does_not():
    quiet = 0x7FF8000000000000
    a, b = _bits([0x3FF0000000000000, quiet]), _bits([0x3FF0000000000000, quiet | 1])
    assert np.isnan(a[1]) and np.isnan(b[1])
    QF.same_values(a, b)
    with pytest.raises(AssertionError):
        QF.same_bytes(a, b, "payload")
    QF.same_bytes(a, a.copy())


@pytest.mark.parametrize("same", [QF.same_values, QF.same_bytes])
def test_both_strengths_see_one_flipped_value_bit(same):
    a, b = _bits([0x3FF0000000000000, 0x4000000000000000]), _bits([0x3FF0000000000000, 0x4000000000000001])
    with pytest.raises(AssertionError):
        same(a, b, "last mantissa bit")
    with pytest.raises(AssertionError):
        QF.compare(dict(x=a), dict(x=b), ["x"], same)
    QF.compare(dict(x=a, y=b), dict(x=a, z=b), ["x", ("y", "z")], same)


def test_a_failed_child_is_not_started_again(tmp_path):
    """a stub child that notes its start and exits non-zero: the second call raises the first call's error and starts nothing"""
    log = tmp_path / "starts.txt"
    stub = tmp_path / "stub_child.py"
    stub.write_text(f"import os, sys\nopen({str(log)!r}, 'a').write(os.environ.get('IHM2MPC_QP_FORM', 'unset') + '\\n')\nsys.exit(3)\n")
    before = len(QF.STARTED)
    with pytest.raises(Exception) as first:
        QF.runs("1", child=str(stub))
    with pytest.raises(Exception) as second:
        QF.runs("1", child=str(stub))
    assert second.value is first.value and first.value.returncode == 3
    assert log.read_text() == "1\n" and QF.STARTED[before:] == [(str(stub), "1")]


def test_the_ladder_names_every_level_once():
    assert list(QF.FORMS) == list(QF.SITUATION) == list(QF.NAMES.values()) == ["0", "1", "2", None]
    assert QF.kernels(None) == [QF.QP, "plain_n40", "full", QF.STEPS, "plain_n40", "full"]
