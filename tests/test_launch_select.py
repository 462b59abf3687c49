"""The launch decisions beside the choice of instantiations (csrc/qp_select.hpp: select_linearize, select_sim, select_run, ladder_length,
ladder_first) without a GPU, through the sanitizer-built tools/probes/check_qp_select.cpp:

* every row of tests/launch_cases.py -- the kernels the GPU tests read from the launch record -- and the 128-interval switch at its boundary;
* the plants without a kernel; how ihm2mpc_run_steps proceeds around 4 x n_cu instances, under IHM2MPC_PERSISTENT_ROUNDS and freeze;
* the backtracking ladder's length and the rule for its first launch.
(The instantiations: tests/test_qp_select.py, tests/test_steps_catalogue.py.)"""
import dataclasses
import itertools

import pytest

import launch_cases as LC
import poison_cases as PC
import select_probe as P
import steps_cases as S
from ihm2_amd.solver import decode_launch_record
from test_steps_catalogue import case_facts


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("launch_select")
    return P.build_probe(tmp), tmp


def _lay(N):
    """The reference's rows at the horizon N."""
    return dataclasses.replace(PC.MISC_LAYOUT, name=f"launch_ref_N{N}", N=N)


def _facts(model=LC.FKIN6, integ=LC.ERK, sim_integ=LC.ERK, B=5, plant=0, cols=False, **more):
    return P.Facts(model=model, integrator=integ, sim_integrator=sim_integ, B=B, plant=plant, linearize_cols=cols, **more)


def _enum(prefix, name):
    """The enumerator named for a kernel of the launch record: LIN_K_LINEARIZE_COLS, SIM_K_SIM_STEP_KIN_LAG, SIM_KERNEL_NONE."""
    return prefix + ("KERNEL_NONE" if name is None else name.upper())


def test_every_row_of_the_table(probe):
    """The two names as BatchedOcpSolver decodes them from the record the selectors leave, and the enumerators behind them."""
    rows = LC.ROWS
    res = P.select(*probe, [(_lay(r.N), _facts(r.model, r.integ, r.sim_integ, r.B, r.plant, r.cols)) for r in rows])
    for r, out in zip(rows, res):
        d = decode_launch_record(out["rec"])
        assert (d["linearize"], d["sim"]) == (r.lin, r.sim), (r, d)
        assert (out["lin"], out["sim"]) == (_enum("LIN_", r.lin), _enum("SIM_", r.sim)), (r, out)
    print(f"{len(rows)} rows")


def test_a_job_without_the_launch_items_keeps_its_line(probe):
    """The four launch items of a job may be left out together: the line is then the twelve-integer one, and the choices of the QP and the
    loop in it are those of the job with the defaults written out."""
    exe, tmp = probe
    lay, facts = PC.MISC_LAYOUT, P.Facts(B=PC.MISC_B)
    full = P.select(exe, tmp, [(lay, facts)])[0]
    job = " ".join([str(tmp / (lay.name + ".txt"))] + [str(v) for v in facts.tokens()[:12]])
    t = P._lines(exe, job)[0].split()
    assert t[:2] + t[4:5] + t[7:8] == [lay.name, "qp", "steps", "rec"] and len(t) == 24
    assert (int(t[2]), int(t[3]), int(t[5]), int(t[6])) == (full["qp"], full["qp_lds"], full["steps"], full["steps_lds"])
    rec = [int(v) for v in t[8:]]
    assert rec[:15] == full["rec"][:15] and rec[15] == full["rec"][15] & ~0xFF and full["rec"][15] & 0xFF


def test_the_switch_flips_both_choices_together(probe):
    """The batches that take the column kernel are the ones whose kinematic plant is the state-only rollout: one predicate."""
    pairs = LC.BOUNDARY_PAIRS + [((8, N), (B, N)) for N, B in LC.PAST_THE_SWITCH.items()]
    shapes = [s for p in pairs for s in p]
    res = P.select(*probe, [(_lay(N), _facts(B=B)) for B, N in shapes])
    got = {s: (decode_launch_record(r["rec"])["linearize"], decode_launch_record(r["rec"])["sim"]) for s, r in zip(shapes, res)}
    for below, above in pairs:
        assert LC.latency_batch(*below) and not LC.latency_batch(*above)
        assert got[below] == ("k_linearize_cols", "k_sim_step"), (below, got[below])
        assert got[above] == ("k_linearize", "k_sim_step_kin"), (above, got[above])
    assert (2 * 64, 3 * 43) == (128, 129)


def test_no_plant_kernel_exactly_for_the_lag_integrator_with_another_plant(probe):
    """ihm2mpc_sim_step, _step and _run_steps refuse what select_sim has no kernel for: ERK_LAG integrates the plain kinematic plant only."""
    combos = list(itertools.product((LC.ERK, LC.IRK_GL, LC.ERK_LAG), (LC.ERK, LC.IRK_GL, LC.IRK_RADAU, LC.ERK_LAG), (3, 5), LC.PLANTS))
    res = P.select(*probe, [(_lay(40), _facts(integ=i, sim_integ=si, B=B, plant=p)) for i, si, B, p in combos])
    none = {(i, si, B, p) for (i, si, B, p), r in zip(combos, res) if r["sim"] == "SIM_KERNEL_NONE"}
    assert none == {c for c in combos if c[1] == LC.ERK_LAG and c[3] in (-2, -1, 1, 2)}
    for c, r in zip(combos, res):
        assert (decode_launch_record(r["rec"])["sim"] is None) == (c in none)


RESIDENCY = [  # (B, IHM2MPC_PERSISTENT_ROUNDS, freeze) -> select_run's outcome, on 256 compute units
    ((1024, False, False), "persistent"), ((1025, False, False), "not_resident"),
    ((1025, True, False), "persistent"), ((1025, True, True), "refused"),
    ((1024, False, True), "persistent"), ((1025, False, True), "refused"),
]


def test_residency(probe):
    c = S.BY_NAME["k_steps<5,0,0,1,0,0,0>"]
    jobs = [case_facts(c, B=B, n_cu=256, persistent_rounds=rounds, freeze=freeze) for (B, rounds, freeze), _ in RESIDENCY]
    for ((B, rounds, freeze), want), r in zip(RESIDENCY, P.select(*probe, jobs)):
        d = decode_launch_record(r["rec"])
        assert r["run"] == want, (B, rounds, freeze, r)
        assert r["steps"] is not None          # the loop exists: the batch decides
        if want == "persistent":
            assert d["steps"] == c.name and d["steps_fallback"] is None
        elif want == "refused":                 # the call fails: no record of a loop or of launches per step
            assert d["steps"] is None and r["rec"][5:15] == [0] * 10
        else:
            assert (d["steps"], d["steps_fallback"]) == ("per_step", want)


@pytest.mark.parametrize("name", list(S.FALLBACK))
def test_fallbacks_have_no_instantiation_and_no_freeze(probe, name):
    """The fallbacks of tests/steps_cases.py: launches per step for the reason they list, whatever the switch says; refused with freeze."""
    c = S.FALLBACK[name]
    jobs = [case_facts(c, persistent_rounds=rounds, freeze=freeze) for rounds in (False, True) for freeze in (False, True)]
    runs = [r["run"] for r in P.select(*probe, jobs)]
    assert c.reason == "no_instantiation" and runs == [c.reason, "refused"] * 2, runs


def test_ladder(probe):
    exe = probe[0]
    assert P.ladder(exe, 0.05, 0.7, 1, 40) == (9, 9)                    # the reference's options: 0.7^8 = 0.0576 >= 0.05 > 0.7^9
    assert P.ladder(exe, 0.05, 0.99, 1, 40) == (None, None)             # 299 trial steps: more than IHM2MPC_LS_MAX_TRIALS = 64
    assert P.ladder(exe, 0.05, 0.9, 16, 40)[0] == 29                    # tests/test_gpu_workspace_poison.py's two-launch ladder
    # one launch while the whole ladder is at most 16384 rollouts, else the first three step lengths for everybody
    assert 9 * 45 * 40 == 16200 and 9 * 46 * 40 == 16560
    assert P.ladder(exe, 0.05, 0.7, 45, 40) == (9, 9)
    assert P.ladder(exe, 0.05, 0.7, 46, 40) == (9, 3)
    # a ladder of two has no second launch at any batch
    for B in (1, 46, 4096, 1 << 20):
        assert P.ladder(exe, 0.5, 0.7, B, 40) == (2, 2)
