"""div_batch<K> (ihm2_amd/csrc/qp_div.hpp) -- K fp64 quotients advanced side by side through the back end's own division sequence, written
out with the builtins -- against the compiler's `/` on the same operands, bit for bit, on the GPU: tools/probes/div_proto.hip, a program of
its own (`check`), one wave per launch, the reference quotients from a kernel of their own.  Widths 1, 2, 3, 5 and 10.  Operands: 10^6
random sign / exponent / mantissa pairs over the whole range (denormals included); 1.0 / x at every exponent; every pair of a table of
special values -- +-0, +-inf, quiet and signalling NaNs with payloads, denormals, the ends of the normal range, neighbours of 1 --;
140 000 pairs whose quotient is denormal, rounds to zero or overflows.  The operand order of the two v_div_scale and of v_div_fixup is what
this decides: a swapped pair shows at once in the scaled ranges and in the NaN payloads."""
import os
import subprocess

import pytest

import host_probe as HP

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 10)
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("div_proto")), "div_proto")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-I", HP.CSRC,
                           os.path.join(HP.ROOT, "tools", "probes", "div_proto.hip"), "-o", exe])
    out = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    return out


def test_every_width_ran_on_all_operands(report):
    lines = report.stdout.splitlines()
    assert [ln.split(":")[0] for ln in lines[:len(WIDTHS)]] == [f"width {w}" for w in WIDTHS], HP.tail(report)
    for ln in lines[:len(WIDTHS)]:
        assert int(ln.split()[2]) >= 1_150_000, ln


@pytest.mark.parametrize("width", WIDTHS)
def test_quotients_are_those_of_the_division(report, width):
    line = next(ln for ln in report.stdout.splitlines() if ln.startswith(f"width {width}:"))
    assert line.endswith(" 0 differ from /"), line


def test_probe_passed(report):
    assert HP.passed(report), HP.tail(report)
