"""The packed wave reductions of the full slot form (csrc/qp_reduce.hpp) without a GPU: tools/probes/check_qp_reduce.cpp, a program of its own
built with the address and undefined-behaviour sanitizers, runs the header's butterfly on 64 software lanes -- the exchange steps against what
the DPP controls and the row / half swaps do, the header's ownership statements against a replay on sets, and the values against the sequential
nanmax / fmin definitions bit for bit: the unique maximum and a NaN in each of the 4 x 64 places, 10 000 random draws with inf, 0 and
denormals."""
import host_probe as HP


def test_packed_reductions_on_software_lanes(tmp_path):
    out = HP.run(HP.build("check_qp_reduce", tmp_path))
    assert HP.passed(out), HP.tail(out)
    assert "20768 value cases" in out.stdout, out.stdout       # 3 x 256 placed cases + 2 x 10 000 draws
