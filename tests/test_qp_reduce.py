"""The packed wave reductions of the full slot form (csrc/qp_reduce.hpp) without a GPU: tools/probes/check_qp_reduce.cpp, a program of its own
built with the address and undefined-behaviour sanitizers, runs the header's butterfly on 64 software lanes -- the exchange steps against what
the DPP controls and the row / half swaps do, the header's ownership statements against a replay on sets, and the values against the sequential
nanmax / fmin definitions bit for bit: the unique maximum and a NaN in each of the 4 x 64 places, 10 000 random draws with inf, 0 and
denormals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ihm2_amd", "csrc")


def test_packed_reductions_on_software_lanes(tmp_path):
    exe = str(tmp_path / "check_qp_reduce")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tools", "probes", "check_qp_reduce.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "all checks passed", out.stdout[-4000:] + out.stderr[-4000:]
    assert "20768 value cases" in out.stdout, out.stdout       # 3 x 256 placed cases + 2 x 10 000 draws
