"""The per-instance slack penalties of the host tables (csrc/qp_tables.hpp: find_penalty_mismatch, table_images, called by api.hip for
ihm2mpc_set_instance_soft / _alat_soft) without a GPU.

For every soft layout of tests/layouts.py that the issue names, and one all-hard layout, at the compiled-in horizon N = 40 and at N = 7,
the problem is written to a file as the solver pushes it and tools/probes/check_slot_penalties.cpp -- built with the address and
undefined-behaviour sanitizers -- draws penalties for B = 5 instances inside the shared pattern and checks that instance b's scattered
block is, entry for entry, the zw / Zw of lay_out_slots on rows holding b's penalties, that the (stage, side) copies are those rows'
sz / sZ, that an all-hard table is scattered onto itself, that each half of each device image sits at the offset the kernels use and
the images for B = 1 with nothing per instance are the shared tables, and that the pattern check refuses a flipped soft flag, z < 0 and a NaN with
the instance, stage and side."""
import dataclasses

import pytest

import host_probe as HP
import layouts as L
from select_probe import problem_text

SOFT = ("soft_2_per_lane", "soft_4_per_lane_mixed", "path_soft_both_sides", "soft_one_sided_rows_padding", "alat_soft")
HARD = ("hard_5_per_lane",)
LAYOUTS = {}
for _name in SOFT + HARD:
    LAYOUTS[_name] = L.TABLE[_name][0]
    LAYOUTS[_name + "_N7"] = dataclasses.replace(L.TABLE[_name][0], name=_name + "_N7", N=7)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """name -> (fit, per_lane, nsoft, soft_slots) of every layout, from one run of the probe."""
    tmp = tmp_path_factory.mktemp("slot_penalties")
    exe = HP.build("check_slot_penalties", tmp)
    files = []
    for name, lay in LAYOUTS.items():
        files.append(str(tmp / (name + ".txt")))
        with open(files[-1], "w") as f:
            f.write(problem_text(lay))
    out = HP.run(exe, *files)
    lines = [ln for ln in out.stdout.splitlines() if not ln.startswith("FAIL")]
    res = {t[0]: tuple(int(v) for v in t[1:]) for t in (ln.split() for ln in lines[:len(files)])}
    return out, res


def test_scatter_equals_layout_of_each_instances_rows_and_bad_patterns_are_refused(probe):
    out, res = probe
    assert HP.passed(out, "slot penalties: "), HP.tail(out)
    assert list(res) == list(LAYOUTS)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts_are_the_tables_they_are_meant_to_be(probe, name):
    """The soft layouts have soft slots to scatter into (at both horizons), the all-hard one has none."""
    _, res = probe
    fit, per_lane, nsoft, soft_slots = res[name]
    assert fit == 1 and per_lane >= 1
    if name.startswith(HARD):
        assert nsoft == 0 and soft_slots == 0
    else:
        assert nsoft >= 2 and soft_slots >= 2
