"""The stage-pair-major layout of M_k (csrc/qp_mrows.hpp) without a GPU: tools/probes/check_qp_mrows.cpp, a program of its own built with the
address and undefined-behaviour sanitizers, walks the writer's and the readers' byte offsets and the reach of the sweeps' unclamped prefetch for
every even horizon in 2..64, and checks that the offset functions refuse the odd ones.  Built with the ring depth and the padding the kernels
are built with, read from their sources."""
import os
import re

import host_probe as HP


def test_paired_rows_layout(tmp_path):
    ring = re.search(r"#define SWEEP_RING (\d+)", open(os.path.join(HP.CSRC, "kernels_qp.hip")).read()).group(1)
    pad = re.search(r"#define QM_PAD (\d+)", open(os.path.join(HP.CSRC, "ihm2mpc_internal.h")).read()).group(1)
    out = HP.run(HP.build("check_qp_mrows", tmp_path, defines=("SWEEP_RING=" + ring, "QM_PAD=" + pad)))
    assert HP.passed(out), HP.tail(out)
    # the shipped case: N = 40 fetches 4 pair rows (8 stage rows) past either end of the block, inside the padding
    m = re.search(r"N 40 ring %s: fetches \[(-?\d+), (\d+)\) of a block of 20480 bytes, padding (\d+)" % ring, out.stdout)
    assert m and -int(m.group(3)) <= int(m.group(1)) < 0 and 20480 < int(m.group(2)) <= 20480 + int(m.group(3)), out.stdout
