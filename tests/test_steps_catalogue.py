"""The case table of the persistent loop (tests/steps_cases.py) against the catalogue (csrc/qp_catalogue.hpp) and the selection
(csrc/qp_select.hpp), without a GPU, through the sanitizer-built tools/probes/check_qp_select.cpp (run as a stand-alone program):

* the names of the catalogue's k_steps keys are exactly CASES + UNREACHED, so that an entry added without a case fails here;
* for every case, select_steps on the case's layout and options chooses the instantiation the case is named for, in the form the case
  lists -- the choice itself runs here, not a restatement of it -- and for every fallback it chooses none, with the fallback's reason;
* from every case's start the oracle solves at least 60 % of the instances in its first step, so that the comparison of
  tests/test_gpu_steps_catalogue.py is one of solved problems."""
import re

import numpy as np
import pytest

import launch_cases as LC
import layouts as L
import rollout_ref as R
import select_probe as P
import steps_cases as S
from ihm2_amd.solver import decode_launch_record

N_NAMES = 87            # 16 + 20 + 28 + 18 + 5


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("steps_catalogue")
    return P.build_probe(tmp), tmp


def steps_names(exe):
    """The k_steps names of the catalogue, name -> the sets that hold it (the record's name does not carry the form of the factor sweep
    and the slot phases: the keys of the sets 4, 6 and 7 repeat names)."""
    names = {}
    for k in P.catalogue(exe):
        if k["kind"] == P.STEPS:
            names.setdefault(P.key_name(k), []).append(k["set"])
    return names


def parse_name(name):
    f = [int(v) for v in re.fullmatch(r"k_steps<([\d,]+)>", name).group(1).split(",")]
    return dict(nslot=f[0], nsoft=f[1], path=f[2], uni=f[3], sqp=f[4], irk=f[5], dyn=f[6], sens=f[7] if len(f) == 8 else 0)


def test_case_table_is_the_catalogue(probe):
    names = steps_names(probe[0])
    other_forms = {k for k, v in names.items() if set(v) <= {4, 6, 7}}
    assert not other_forms, other_forms                   # the sets 4, 6 and 7 repeat names of the sets 0 and 5
    cases, unreached = set(S.BY_NAME), set(S.UNREACHED)
    print(f"{len(names)} k_steps names: {len(cases)} cases, {len(unreached)} unreached {sorted(unreached)}")
    assert len(names) == N_NAMES
    assert not (cases & unreached)
    assert cases | unreached == set(names), (sorted(set(names) - cases - unreached), sorted((cases | unreached) - set(names)))
    for c in S.CASES:       # the set a case is filed under (it decides whether the ILP build is run) holds its name
        assert c.qp_set in names[c.name], c
    assert all(c.name == "per_step" and c.reason in ("no_instantiation", "not_resident") for c in S.FALLBACK.values())


def test_case_fields_say_what_the_name_says():
    for c in S.CASES:
        k = parse_name(c.name)
        lay = S.LAYOUTS[c.layout]
        assert (k["sqp"], k["irk"], k["dyn"], k["sens"] != 0) == (int(c.sqp), c.irk, int(c.model != "fkin6"), c.sens != 0), c
        assert k["uni"] == (0 if lay.stage_W or lay.grows == "stagevary" else 1), c
        assert k["path"] == (2 if lay.alat else 1 if lay.path else 0), c
        assert not LC.latency_batch(c.B, lay.N) and (c.B * lay.N) % 64 != 0          # k_linearize_cols / the state-only plant are not run; a ragged last wave
    # the plants rotate within every (IRK, DYN) class: the kinematic plant on lane N and a called dynamic plant both occur
    for cls in {(c.irk, c.model) for c in S.CASES}:
        plants = {c.plant for c in S.CASES if (c.irk, c.model) == cls}
        assert 0 in plants and plants - {0}, (cls, plants)


def _case(name):
    return S.FALLBACK[name[9:]] if name.startswith("fallback:") else S.ILP_CASES[name[4:]] if name.startswith("ilp:") else S.BY_NAME[name]


CASE_IDS = list(S.BY_NAME) + ["ilp:" + k for k in S.ILP_CASES]
FALLBACK_IDS = ["fallback:" + k for k in S.FALLBACK]


def case_facts(case, **more):
    """What the handle of a case is configured with (tests/test_gpu_steps_catalogue.py builds it from the same options)."""
    lay = S.LAYOUTS[case.layout]
    return lay, P.facts_of_data(L.make_ocp(lay, **case.ocp_opts()).flatten(), **{"B": case.B, "sens": case.sens, **more})


@pytest.fixture(scope="module")
def selected(probe):
    """id -> the launch record ihm2mpc_run_steps leaves for the case, decoded: one run of the probe over all cases and fallbacks."""
    ids = CASE_IDS + FALLBACK_IDS
    res = P.select(*probe, [case_facts(_case(i)) for i in ids])
    return {i: decode_launch_record(r["rec"]) for i, r in zip(ids, res)}


@pytest.mark.parametrize("name", CASE_IDS)
def test_layout_gives_the_table_of_the_name(selected, name):
    """select_steps (csrc/qp_select.hpp) on the case's layout and options: the loop the case is named for, in the form it lists."""
    c = _case(name)
    rec = selected[name]
    assert rec["steps"] == c.name, rec
    assert (rec["steps_form"], rec["steps_slots"]) == c.form, rec


@pytest.mark.parametrize("name", FALLBACK_IDS)
def test_fallback_selects_no_loop(selected, name):
    c = _case(name)
    rec = selected[name]
    assert rec["steps"] == "per_step" == c.name and rec["steps_fallback"] == c.reason, rec
    assert rec["steps_form"] is None and rec["steps_slots"] is None


def test_batch_above_four_per_cu_is_not_resident(probe):
    """B = 1100 on 256 compute units (tests/test_gpu_closed_loop.py and tests/test_gpu_sens_steps.py assert it on hardware)."""
    c = S.BY_NAME["k_steps<5,0,0,1,0,0,0>"]
    for sens in (0, 1):
        rec = decode_launch_record(P.select(*probe, [case_facts(c, B=1100, n_cu=256, sens=sens)])[0]["rec"])
        assert (rec["steps"], rec["steps_fallback"]) == ("per_step", "not_resident"), rec
        assert rec["qp"] == "k_qp_wave<5,0,0,1>"


def problem(track, case):
    """(data, OracleProblem) of a case: the layout's arrays on the OCP with the case's model, integrator and solver options."""
    lay = S.LAYOUTS[case.layout]
    data = L.make_ocp(lay, **case.ocp_opts()).flatten()
    L.apply(data, lay)
    return data, S.oracle_problem(track, data, lay)


def oracle_first_step(track, case):
    """The statuses of the oracle's first step from the case's start (the warm start restated by tests/rollout_ref.py)."""
    data, P = problem(track, case)
    x0, yref, yref_e = S.start(track, case)
    RP = R.RolloutProblem.from_data(data, track.s_ref, track.kappa_ref, np.zeros(case.B, dtype=np.int32))
    x, u = R.rollout(RP, x0, oracle=P)
    x, u = np.ascontiguousarray(x), np.ascontiguousarray(u)
    if case.sqp:
        return P.sqp_solve(x, u, x0, yref, yref_e, **{**S.sqp_kwargs(data), "max_iter": 1})["status"]
    return S.oracle_rti_step(P, data, track, x, u, x0, yref, yref_e)["status"]


@pytest.mark.parametrize("name", CASE_IDS + FALLBACK_IDS)
def test_oracle_solves_the_first_step_of_the_case(track, name):
    """At least 60 % of the instances end the first step accepted (0; in the SQP mode 0 or 2)."""
    case = _case(name)
    st = oracle_first_step(track, case)
    ok = np.isin(st, case.accepted)
    print(f"{name}: seed {case.seed} status {st.tolist()}")
    assert ok.mean() >= 0.6, (name, st.tolist())
