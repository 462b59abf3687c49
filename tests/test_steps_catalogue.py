"""The case table of the persistent loop (tests/steps_cases.py) against the catalogue (csrc/qp_catalogue.hpp), without a GPU:

* the names the STEPS entries expand to are exactly CASES + UNREACHED, so that an entry added without a case fails here;
* every case's layout gives the slot table (slots per lane -> NSLOT, NSOFT, PATH) its name says, through the sanitizer-built
  tools/probes/check_slot_table.cpp (run as a stand-alone program, as tests/test_slot_table.py does);
* from every case's start the oracle solves at least 60 % of the instances in its first step, so that the comparison of
  tests/test_gpu_steps_catalogue.py is one of solved problems."""
import os
import re
import subprocess

import numpy as np
import pytest

import layouts as L
import rollout_ref as R
import steps_cases as S
from test_slot_table import CSRC, ROOT, problem_text

N_NAMES = 87            # 16 + 20 + 28 + 18 + 5


def steps_entries():
    """set -> [(NSLOT, NSOFT, PATH, UNI, IRK, DYN)] of the STEPS entries of the catalogue, in its order."""
    text = open(os.path.join(CSRC, "qp_catalogue.hpp")).read()
    lists = re.findall(r"#define QP_INSTANCES_(\d)\(WAVE, BLOCK, STEPS\)((?:.*\\\n)*.*)\n", text)
    assert [n for n, _ in lists] == list("0123456")
    sets = {int(n): [tuple(int(v) for v in m) for m in re.findall(r"\bSTEPS\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", body)] for n, body in lists}
    assert re.search(r"#define QP_INSTANCES_7 QP_INSTANCES_4\n", text)
    sets[7] = sets[4]
    return sets


def expand(sets):
    """The k_steps names of the catalogue, name -> the sets that hold it.  THE EXPANSION RULE (kernels_qp.hip: the STEPS macro per QP_SET):

    sets 0, 1, 2   every entry in both SQP modes, SENS = 0
    set 3          RTI only, SENS = 1 (the eighth field of the name)
    set 5          RTI only, SENS = 0
    sets 4, 6, 7   RTI only, SENS = 0, other forms of the factor sweep / the slot phases: the launch record's name does not carry the
                   form, so these add no name -- each must already be one of the sets 0 and 5"""
    names = {}
    for n, entries in sets.items():
        for (ns, no, pt, un, irk, dyn) in entries:
            for sqp in ((0, 1) if n in (0, 1, 2) else (0,)):
                names.setdefault(S.steps_name((ns, no, pt, un), sqp, irk, dyn, sens=1 if n == 3 else 0), []).append(n)
    return names


def parse_name(name):
    f = [int(v) for v in re.fullmatch(r"k_steps<([\d,]+)>", name).group(1).split(",")]
    return dict(nslot=f[0], nsoft=f[1], path=f[2], uni=f[3], sqp=f[4], irk=f[5], dyn=f[6], sens=f[7] if len(f) == 8 else 0)


def test_case_table_is_the_catalogue():
    names = expand(steps_entries())
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
        assert c.B * lay.N > 128 and (c.B * lay.N) % 64 != 0          # past the switch to k_linearize_cols / the state-only plant; a ragged last wave
    # the plants rotate within every (IRK, DYN) class: the kinematic plant on lane N and a called dynamic plant both occur
    for cls in {(c.irk, c.model) for c in S.CASES}:
        plants = {c.plant for c in S.CASES if (c.irk, c.model) == cls}
        assert 0 in plants and plants - {0}, (cls, plants)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """layout -> (fit, per_lane, nsoft) of every layout of the cases and fallbacks, from one run of the probe."""
    tmp = tmp_path_factory.mktemp("steps_catalogue")
    exe = str(tmp / "check_slot_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tools", "probes", "check_slot_table.cpp")])
    used = sorted({c.layout for c in list(S.CASES) + list(S.FALLBACK.values()) + list(S.ILP_CASES.values())})
    files = []
    for name in used:
        files.append(str(tmp / (name + ".txt")))
        with open(files[-1], "w") as f:
            f.write(problem_text(S.LAYOUTS[name]))
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    res = {}
    for line in out.stdout.splitlines()[:len(files)]:
        name, fit, per_lane, nsoft = line.split()[:4]
        res[name] = (int(fit), int(per_lane), int(nsoft))
    assert list(res) == used
    return res


def _case(name):
    return S.FALLBACK[name[9:]] if name.startswith("fallback:") else S.ILP_CASES[name[4:]] if name.startswith("ilp:") else S.BY_NAME[name]


@pytest.mark.parametrize("name", list(S.BY_NAME) + ["ilp:" + k for k in S.ILP_CASES])
def test_layout_gives_the_table_of_the_name(tables, name):
    """find_inst: the first STEPS entry, in catalogue order over the sets, whose other fields are the key's and whose NSLOT holds the
    table's slots per lane."""
    c = _case(name)
    name = c.name
    k = parse_name(name)
    fit, per_lane, nsoft = tables[c.layout]
    assert fit == 1
    sets = steps_entries()
    first = next(e for n in sorted(sets) if (n == 3) == (k["sens"] != 0) and (k["sqp"] == 0 or n in (0, 1, 2)) for e in sets[n]
                 if e[1:] == (nsoft, k["path"], k["uni"], k["irk"], k["dyn"]) and e[0] >= per_lane)
    assert first[0] == k["nslot"] and nsoft == k["nsoft"], (per_lane, nsoft, first)


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


@pytest.mark.parametrize("name", list(S.BY_NAME) + ["ilp:" + k for k in S.ILP_CASES] + ["fallback:" + k for k in S.FALLBACK])
def test_oracle_solves_the_first_step_of_the_case(track, name):
    """At least 60 % of the instances end the first step accepted (0; in the SQP mode 0 or 2)."""
    case = _case(name)
    st = oracle_first_step(track, case)
    ok = np.isin(st, case.accepted)
    print(f"{name}: seed {case.seed} status {st.tolist()}")
    assert ok.mean() >= 0.6, (name, st.tolist())
