"""The choice of the QP instantiations and the launch record (csrc/qp_select.hpp) without a GPU, through the sanitizer-built
tools/probes/check_qp_select.cpp.  The expectations are the tables the GPU tests assert on hardware -- a wrong choice gives the same
results there, only slower, so the choice is tested here as well:

* the forms of the factor sweep and the slot phases under IHM2MPC_QP_FORM, as tests/qp_forms.py lists them for both records;
* the per-step QP of every layout of tests/layouts.py (tests/test_slot_table.py: NAMED_FOR), and the four-wave kernel's conditions as
  tests/test_gpu_closed_loop.py and tests/test_gpu_qp_layouts.py see them;
* the record of every key of the catalogue, and of every linearisation and plant kernel, through BatchedOcpSolver's decoder.
(The step loops: tests/test_steps_catalogue.py.)"""
import dataclasses
import os
import re

import pytest

import layouts as L
import poison_cases as PC
import qp_forms as QF
import select_probe as P
import steps_cases as S
from ihm2_amd.solver import decode_launch_record
from test_slot_table import FIT, NAMED_FOR

FORM_OF_NF = {0: "general", -1: "plain", 40: "plain_n40"}
SLOTS_OF_FULL = ("general", "full")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("qp_select")
    return P.build_probe(tmp), tmp


def _records(probe, jobs):
    return [decode_launch_record(r["rec"]) for r in P.select(*probe, jobs)]


# ---- forms under the switch ----

QP_FORMS = QF.SITUATION          # the switch's level -> QpSituation.qp_form


def _both(rec):
    return (rec["qp"], rec["qp_form"], rec["qp_slots"]), (rec["steps"], rec["steps_form"], rec["steps_slots"])


def test_forms_of_the_reference_layout_under_the_switch(probe):
    """The handle of tests/poison_child.py: the reference layout at N = 40, B = 5, IHM2MPC_BLOCK_QP = 0."""
    lay = PC.MISC_LAYOUT
    assert lay.N == 40
    recs = _records(probe, [(lay, P.Facts(B=PC.MISC_B, block_qp=False, qp_form=f)) for f in QP_FORMS.values()])
    for form, rec in zip(QP_FORMS, recs):
        assert _both(rec) == (QF.qp_record(form), QF.steps_record(form)), (form, rec)


def test_fdyn6_stays_on_the_general_form(probe):
    """The dynamic model as written needs the symmetrising tile, which the straight-line stage does not keep."""
    recs = _records(probe, [(PC.MISC_LAYOUT, P.Facts(model=1, B=PC.MISC_B, block_qp=False, qp_form=f)) for f in QP_FORMS.values()])
    for rec in recs:
        assert _both(rec) == ((QF.QP, "general", "general"), ("k_steps<5,0,0,1,0,0,1>", "general", "general")), rec


def test_other_horizons_take_the_run_time_form(probe):
    """N != 40 with the reference's rows in 5 slots per lane: "plain" unless the switch keeps every launch on the general form."""
    lay = dataclasses.replace(PC.MISC_LAYOUT, name="misc_ref_N39", N=39)
    recs = _records(probe, [(lay, P.Facts(B=PC.MISC_B, block_qp=False, qp_form=f)) for f in QP_FORMS.values()])
    for form, rec in zip(QP_FORMS, recs):
        want = ("general", "general") if form == "0" else ("plain", "general")
        assert _both(rec) == ((QF.QP,) + want, (QF.STEPS,) + want), (form, rec)


# ---- the per-step QP ----

def _uni(lay):
    return 0 if lay.stage_W or lay.grows == "stagevary" else 1


def test_every_layout_selects_the_wave_kernel_it_is_named_for(probe):
    """A batch above the CU count: k_qp_wave<NSLOT, NSOFT, PATH, UNI> of NAMED_FOR, whatever IHM2MPC_BLOCK_QP says."""
    names = list(FIT)
    for block_qp in (True, False):
        recs = _records(probe, [(FIT[n], P.Facts(B=P.N_CU + 44, block_qp=block_qp)) for n in names])
        for n, rec in zip(names, recs):
            assert rec["qp"] == "k_qp_wave<%d,%d,%d,%d>" % (NAMED_FOR[n] + (_uni(FIT[n]),)), (n, rec)


def test_four_wave_kernel_for_at_most_one_instance_per_cu(probe):
    """tests/test_gpu_closed_loop.py (B = 1) and tests/test_gpu_qp_layouts.py (block_*): the reference layout on k_qp_block<2,1,4>; with
    per-instance bounds or IHM2MPC_BLOCK_QP = 0 on k_qp_wave<5,0,0,1>; one instance more than CUs on k_qp_wave as well."""
    lay = L.TABLE["block_hard"][0]
    jobs = [P.Facts(B=1), P.Facts(B=64), P.Facts(B=P.N_CU), P.Facts(B=1, inst_b=True), P.Facts(B=1, block_qp=False), P.Facts(B=P.N_CU + 1)]
    recs = _records(probe, [(lay, f) for f in jobs])
    assert [r["qp"] for r in recs] == ["k_qp_block<2,1,4>"] * 3 + ["k_qp_wave<5,0,0,1>"] * 3, recs
    assert all(r["qp_form"] == "general" and r["qp_slots"] == "general" for r in recs[:3])
    rec = _records(probe, [(L.TABLE["block_hard_stage_W"][0], P.Facts(B=33))])[0]
    assert rec["qp"] == "k_qp_block<2,0,4>", rec


def test_launch_uses_the_lds_of_the_choice(probe):
    """The LDS bytes the launch asks for come with the choice: the QP's own for the per-step kernel, and for the loop the larger of the
    QP's and the sensitivity body's (csrc/qp_lds.hpp: StepsLds) -- at N = 40 the QP's either way."""
    r0, r1 = P.select(*probe, [(PC.MISC_LAYOUT, P.Facts(B=5, sens=s)) for s in (0, 1)])
    assert r0["qp_lds"] == r0["steps_lds"] == r1["steps_lds"] and r0["qp_lds"] % 8 == 0 and 0 < r0["qp_lds"] <= 160 * 1024


# ---- the record ----

def test_record_of_every_key_decodes_to_its_name_and_forms(probe):
    keys = P.catalogue(probe[0])
    recs, _ = P.records(probe[0])
    assert len(keys) == len(recs)
    for k, rec in zip(keys, recs):
        d = decode_launch_record(rec)
        which = "steps" if k["kind"] == P.STEPS else "qp"
        name = P.key_name(k)
        if k["kind"] == P.STEPS:
            assert name == S.steps_name((k["nslot"], k["nsoft"], k["path"], k["uni"]), k["sqp"], k["irk"], k["dyn"], k["sens"])
        else:
            assert name.startswith("k_qp_wave<" if k["kind"] == P.WAVE else "k_qp_block<")
        assert (d[which], d[which + "_form"], d[which + "_slots"]) == (name, FORM_OF_NF[k["nf"]], SLOTS_OF_FULL[k["full"]]), (k, d)
        other = "qp" if which == "steps" else "steps"
        assert d[other] is None and d[other + "_form"] is None and d[other + "_slots"] is None and d["linearize"] is None and d["sim"] is None


def _documented_codes(text, after, before):
    """code -> kernel name from the comment of ihm2mpc_get_launch_record: the list "0 none yet, 1 k_..., 2 k_..." between two phrases."""
    part = text[text.index(after):text.index(before)]
    return {int(c): n for c, n in re.findall(r"\b([1-5]) (k_\w+|a plant step with sensitivities)", part[part.index("0 none yet"):])}


def test_linearisation_and_plant_codes_decode_to_the_documented_names(probe):
    hdr = open(os.path.join(P.ROOT, "include", "ihm2mpc.h")).read()
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ihm2mpc_get_launch_record\(", hdr, flags=re.S).group(1)
    doc = " ".join(doc.replace("*", " ").split())
    lin = _documented_codes(doc, "the last linearisation launch", "the last plant launch")
    sim = _documented_codes(doc, "the last plant launch", "Launches inside k_steps")
    # the header names the ERK_LAG kernels by their plain names "with the closed-form lags", and the sensitivity step by its entry point
    assert lin == {1: "k_linearize", 2: "k_linearize_dyn", 3: "k_linearize_cols", 4: "k_linearize_irk", 5: "k_linearize"}
    assert sim == {1: "k_sim_step_kin", 2: "k_sim_step", 3: "k_sim_irk", 4: "k_sim_step_kin", 5: "a plant step with sensitivities"}
    lin[5] += "_lag"; sim[4] += "_lag"; sim[5] = "k_sim_sens"
    _, kernels = P.records(probe[0])
    assert len(kernels) == 12
    for enum, rec in kernels.items():
        d = decode_launch_record(rec)
        field, table = ("linearize", lin) if enum.startswith("LIN_") else ("sim", sim)
        code = (rec[15] & 15) if field == "linearize" else (rec[15] >> 4) & 15
        assert rec[:15] == [0] * 15 and rec[15] == (code if field == "linearize" else code << 4)
        if enum.endswith("_NONE"):
            assert code == 0 and d[field] is None
        else:           # the enumerator is named for the kernel: LIN_K_LINEARIZE_COLS, SIM_K_SIM_STEP_KIN_LAG
            assert d[field] == table[code] == enum[4:].lower(), (enum, d)
    assert sorted((r[15] & 15) for e, r in kernels.items() if e.startswith("LIN_")) == list(range(6))
    assert sorted((r[15] >> 4) for e, r in kernels.items() if e.startswith("SIM_")) == list(range(6))
