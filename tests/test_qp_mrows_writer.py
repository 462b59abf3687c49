"""The factor sweep's store schedule of the stage-pair-major M_k (csrc/qp_mrows.hpp: qm_pair_half_holder) without a GPU:
tools/probes/check_qp_mrows.cpp, a program of its own built with the address and undefined-behaviour sanitizers, replays the two 8-byte
stores of every lane and stage for every even horizon in 2..64: every byte of an instance's block is written exactly once by the end of the
sweep, no store leaves the block, and each half of a 16-byte slot is stored by the lane the header names.  Only the eight diagonal slots have
both halves in one lane: a 16-byte store per slot needs a transpose across lanes, not one more stage of holding two values."""
import os
import re

import host_probe as HP


def test_store_schedule_of_the_paired_rows(tmp_path):
    ring = re.search(r"#define SWEEP_RING (\d+)", open(os.path.join(HP.CSRC, "kernels_qp.hip")).read()).group(1)
    pad = re.search(r"#define QM_PAD (\d+)", open(os.path.join(HP.CSRC, "ihm2mpc_internal.h")).read()).group(1)
    out = HP.run(HP.build("check_qp_mrows", tmp_path, defines=("SWEEP_RING=" + ring, "QM_PAD=" + pad)))
    assert HP.passed(out), HP.tail(out)
    m = re.search(r"N 40 writer: (\d+) bytes written once, (\d+) of 64 slots have both halves in one lane", out.stdout)
    assert m and int(m.group(1)) == 40 * 512 and int(m.group(2)) == 8, out.stdout
