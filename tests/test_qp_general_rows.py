"""The general rows of the QP's full slot form, evaluated once per phase into the transpose tile (csrc/kernels_qp.hip: general_rows,
row_dot_full), without a GPU: tools/probes/check_qp_general_rows.cpp, a program of its own built with the address and undefined-behaviour
sanitizers, lays out the reference's table at N = 40 and at N = 2 through the functions api.hip calls, packs every entry with
csrc/qp_lds.hpp: qp_full_slot_pack and checks that a general-row slot's tile offset lies in [0, 16 N), is 8 (2 k + row) and its own, that box
entries are what the kernel packed before, that the reach statement holds and covers every word a slot reads, and that the pass plus the
one-word read give the bits of the ten-term chain per slot (a NaN and an infinity in the vector included)."""
import host_probe as HP


def test_general_rows_once_per_phase(tmp_path):
    out = HP.run(HP.build("check_qp_general_rows", tmp_path))
    assert HP.passed(out), HP.tail(out)
    assert "N = 40: 80 general-row slots, 240 box slots" in out.stdout, out.stdout
    assert "N = 2: 4 general-row slots" in out.stdout, out.stdout
