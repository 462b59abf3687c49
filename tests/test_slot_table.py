"""The constraint-slot tables of the QP kernels (csrc/qp_tables.hpp: lay_out_slots, called by api.hip::rebuild_slots) without a GPU.

For every layout tests/test_gpu_qp_layouts.py runs or sees refused, and the smallest shapes, the problem is written to a file as the
solver pushes it (the layout's arrays, the OCP's own track-row and a_lat settings) and tools/probes/check_slot_table.cpp -- built with
the address and undefined-behaviour sanitizers -- lays the table out through the functions api.hip calls and checks what the kernels
take from it unchecked: row coverage, one lane per split row, the leading one-sided entries with the soft ones first, padding, the
first instantiation of the catalogue that fits, the counts, the lane balance, the 256-lane table, the per-instance scatter and the
weight tables.  Here: the fit / refusal of each layout, the instantiation it is named for, and the tables themselves, entry for entry, as
digests against tests/golden/slot_tables.json -- recorded from the tables the library uploaded BEFORE the layout code moved into the
header (tests/golden/make_slot_tables.py), so they pin the entry order every bit of the QP's results depends on."""
import json
import os

import pytest

import host_probe as HP
import layouts as L
import select_probe as P
from select_probe import ROOT, problem_text

# the smallest shapes: the horizons 2 and 3 of the reference layout (fewer rows than lanes), and no row at all
SMALL = {
    "ref_N2": L.Layout("ref_N2", N=2),
    "ref_N3": L.Layout("ref_N3", N=3),
    "empty_table_N2": L.Layout("empty_table_N2", N=2, xbox="none", ubox=False, grows="none"),
}
FIT = {**{n: t[0] for n, t in L.TABLE.items()}, **SMALL}
LAYOUTS = {**FIT, **L.REFUSED}

# The per-step instantiation k_qp_wave<NSLOT, NSOFT, PATH, .> each layout is named for -- what test_gpu_qp_layouts.py's launch records
# showed for it before the layout code moved (k_qp_block<2,.,4> runs the "block_*" tables: those of <5,0,0> over 256 lanes).
NAMED_FOR = {
    "hard_5_per_lane": (5, 0, 0), "hard_5_per_lane_stage_W": (5, 0, 0), "hard_6_per_lane": (8, 0, 0), "hard_8_per_lane_stage_rows": (8, 0, 0),
    "hard_9_per_lane": (10, 0, 0), "hard_10_per_lane_all_boxes": (10, 0, 0), "hard_10_per_lane_stage_W": (10, 0, 0),
    "hard_random_one_sided": (5, 0, 0), "hard_narrow_rate_row": (5, 0, 0), "empty_table": (5, 0, 0),
    "block_hard": (5, 0, 0), "block_hard_B1": (5, 0, 0), "block_hard_stage_W": (5, 0, 0),
    "soft_2_per_lane": (8, 2, 0), "soft_2_per_lane_stage_W": (8, 2, 0), "soft_2_per_lane_split_rows": (8, 2, 0),
    "soft_3_per_lane_asym": (10, 4, 0), "soft_4_per_lane_mixed": (10, 4, 0), "soft_4_per_lane_stage_rows": (10, 4, 0),
    "soft_one_sided_rows_padding": (8, 2, 0),
    "path_hard": (8, 0, 1), "path_hard_stage_W": (8, 0, 1), "path_soft_3_per_lane": (8, 3, 1), "path_soft_3_per_lane_stage_W": (8, 3, 1),
    "path_soft_both_sides": (10, 4, 1), "path_soft_4_per_lane": (10, 4, 1), "path_soft_4_per_lane_stage_W": (10, 4, 1),
    "alat_hard": (8, 0, 2), "alat_soft": (10, 4, 2),
    "ref_N2": (5, 0, 0), "ref_N3": (5, 0, 0), "empty_table_N2": (5, 0, 0),
}


@pytest.fixture(scope="module")
def waves(tmp_path_factory):
    """(NSLOT, NSOFT, PATH) of the WAVE entries of the catalogue, in its order: from the probe's dump of csrc/qp_catalogue.hpp:
    catalogue_keys, one per entry of the lists (the set 4's entry is built twice, NF = 40 and NF = -1; the set 7 is that list once more)."""
    exe = P.build_probe(tmp_path_factory.mktemp("catalogue"))
    return [(k["nslot"], k["nsoft"], k["path"]) for k in P.catalogue(exe) if k["kind"] == P.WAVE and k["nf"] != -1 and not k["full"]]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """name -> (fit, per_lane, nsoft, total, m_act, digest) of every layout, from one run of the probe."""
    tmp = tmp_path_factory.mktemp("slot_table")
    exe = P.build_probe(tmp, "check_slot_table")
    files = []
    for name, lay in LAYOUTS.items():
        files.append(str(tmp / (name + ".txt")))
        with open(files[-1], "w") as f:
            f.write(problem_text(lay))
    out = HP.run(exe, *files)
    assert HP.passed(out, "slot tables: "), HP.tail(out)
    res = {}
    for line in out.stdout.splitlines()[:len(files)]:
        name, fit, per_lane, nsoft, total, m_act, digest = line.split()
        res[name] = (int(fit), int(per_lane), int(nsoft), int(total), int(m_act), digest)
    assert list(res) == list(LAYOUTS)
    return res


def test_catalogue_lists_are_the_ones_the_layouts_are_named_for(waves):
    assert len(waves) == 19 and set(NAMED_FOR) == set(FIT)
    assert set(NAMED_FOR.values()) == set(waves)          # every per-step instantiation has a layout


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_fits_the_instantiation_it_is_named_for(tables, waves, name):
    fit, per_lane, nsoft, _, _, _ = tables[name]
    if name in L.REFUSED:
        assert fit == 0
        return
    assert fit == 1
    lay = LAYOUTS[name]
    path = 2 if lay.alat else 1 if lay.path else 0
    first = next(w for w in waves if w[2] == path and w[1] == nsoft and w[0] >= per_lane)
    assert first == NAMED_FOR[name], (per_lane, nsoft)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_table_is_the_recorded_one_entry_for_entry(tables, name):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "slot_tables.json")))
    g = golden[name]
    assert tables[name] == (g["fit"], g["per_lane"], g["nsoft"], g["total"], g["m_act"], g["digest"])
