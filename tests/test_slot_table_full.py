"""Which slot tables take the QP kernels' full slot form (csrc/qp_tables.hpp: slot_table_full, slot_bounds_full -- what api.hip evaluates
wherever it lays out or uploads a table), without a GPU: tools/probes/check_full_table.cpp, a program of its own built with the address and
undefined-behaviour sanitizers, lays the reference's rows out through the functions api.hip calls and prints the predicate per case.

The kernel asks nothing about a slot in that form, so the predicate has to: the reference's rows are full at N = 40 (8 N = 64 x 5 two-sided
rows) and at no other horizon, and one infinite side anywhere -- in the shared table or in one instance's bounds -- a soft side or a track
row takes the form away."""
import pytest

import host_probe as HP

# case -> (full, slots per lane, rows in the table)
EXPECTED = {
    "ref_N40": (1, 5, 320),
    "ref_N8": (0, 1, 64),
    "ref_N39": (0, 5, 312),
    "ref_N41": (0, 6, 328),
    "one_upper_1e20": (0, 5, 320),
    "one_upper_inf": (0, 5, 320),
    "instance_all_finite": (1, 5, 320),
    "instance_one_inf": (0, 5, 320),
    "soft": (0, None, None),
    "track_rows": (0, None, None),
    "no_table": (0, 0, 0),
}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    out = HP.run(HP.build("check_full_table", tmp_path_factory.mktemp("full_table")))
    assert HP.passed(out), HP.tail(out)
    res = {}
    for line in out.stdout.splitlines()[:-1]:
        name, full, per_lane, total = line.split()
        res[name] = (int(full), int(per_lane), int(total))
    return res


def test_every_case_is_reported(cases):
    assert list(cases) == list(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_predicate(cases, name):
    full, per_lane, total = EXPECTED[name]
    assert cases[name][0] == full
    if per_lane is not None:
        assert cases[name][1:] == (per_lane, total)
