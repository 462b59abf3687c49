"""Every device buffer of the solver handle belongs to one of two classes, stated where it is declared (csrc/ihm2mpc_internal.h):
StateBuf -- contents that carry meaning from call to call, or whose documented default is zero -- and WorkBuf -- workspace and outputs, which
a call must write before it, or a getter after it, reads.  IHM2MPC_POISON_WORKSPACE fills the WorkBufs of doubles with NaN
(tests/test_gpu_workspace_poison.py runs everything on such a handle).  Parsed here, without a GPU: a buffer added later cannot escape the
instrument by being declared as a bare DevBuf, or as a workspace of doubles the switch does not know by name."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ihm2_amd", "csrc")

# workspace that is never poisoned, with the reason written next to its declaration: the argument blocks hold pointers and counts
ZERO_FILLED = {"ls_args", "step_args", "sens_args"}

WORKSPACE = set("""lin q_g q_rg q_P q_M scratch res qp_res dyn10 ls_phi ls_x ls_u ls_pi ls_lam ls_slk ls_wpi ls_wlam ls_alpha ls_merit
                   hist_u0 hist_x0 hist_k sens_xbar sens_ubar sens_u0 sens_x sens_u adj_sx adj_su adj_gx0 adj_gy adj_gye adj_gW adj_gWe
                   step_args ls_args sens_args ls_done ls_status ls_iter ls_qp_acc ls_pending hist_st hist_it""".split())
# (u0 is state: the plant of the next step reads the last solve's control, 0 before the first solve)
STATE = set("""x u x0 yref yref_e pi lam slk lam_a slk_a xc s_guess status qp_iter active track_id u0
               s_ref kappa_ref Hs Gy lbx ubx lbu ubu CD lg ug widths X_ref Y_ref phi_ref Wd st_lb st_ub irk_tab sim_irk_tab
               iHs iGy iWd i_slot_lb i_slot_ub i_st_lb i_st_ub i_lbu i_ubu i_lg i_ug
               slot_kc slot_lb slot_ub slot_kc_blk slot_lb_blk slot_ub_blk""".split())


def handle_body(text):
    m = re.search(r"^struct ihm2mpc_handle \{\n(.*?)^\};", text, re.S | re.M)
    assert m, "struct ihm2mpc_handle not found"
    return m.group(1)


def classify(body):
    """({member: (class, element type)}, [lines that declare a buffer without a class])"""
    code = re.sub(r"//[^\n]*", "", body)
    members, bare = {}, []
    for stmt in code.split(";"):
        stmt = " ".join(stmt.split())
        m = re.match(r"^(DevBuf|StateBuf|WorkBuf)<([\w:]+)> ([\w, ]+)$", stmt)
        if m is None:
            if re.search(r"\b(DevBuf|StateBuf|WorkBuf)\b", stmt):
                bare.append(stmt)       # a declaration this parser does not read is a finding as well
            continue
        for name in m.group(3).split(","):
            if m.group(1) == "DevBuf":
                bare.append(stmt)
            members[name.strip()] = (m.group(1), m.group(2))
    return members, bare


def test_every_buffer_of_the_handle_carries_a_class():
    members, bare = classify(handle_body(open(os.path.join(CSRC, "ihm2mpc_internal.h")).read()))
    assert not bare, bare
    assert len(members) > 90
    work = {n for n, (c, _) in members.items() if c == "WorkBuf"}
    state = {n for n, (c, _) in members.items() if c == "StateBuf"}
    assert work == WORKSPACE, (sorted(work - WORKSPACE), sorted(WORKSPACE - work))
    assert state == STATE, (sorted(state - STATE), sorted(STATE - state))


def test_the_parser_sees_an_unclassified_buffer():
    body = "    StateBuf<double> x;   // (B,NS,8)\n    DevBuf<double> fresh, other;\n    WorkBuf<int32_t> n;\n    std::vector<DevBuf<double>> pool;\n"
    members, bare = classify(body)
    assert members["x"] == ("StateBuf", "double") and members["n"] == ("WorkBuf", "int32_t")
    assert len(bare) == 3 and "fresh" in bare[0] and "pool" in bare[2]


def test_the_switch_knows_every_workspace_of_doubles_by_name():
    members, _ = classify(handle_body(open(os.path.join(CSRC, "ihm2mpc_internal.h")).read()))
    doubles = {n for n, (c, t) in members.items() if c == "WorkBuf" and t == "double"}
    api = open(os.path.join(CSRC, "api.hip")).read()
    m = re.search(r"const Poisonable POISONABLE\[\] = \{(.*?)\};", api, re.S)
    assert m
    named = set(re.findall(r"PB\((\w+)\)", m.group(1)))
    assert named == doubles - ZERO_FILLED, (sorted(named ^ (doubles - ZERO_FILLED)))
    # the local buffers of api.hip are classified as well: DevBuf appears only as the parameter type of alloc_all
    uses = [ln.strip() for ln in api.splitlines() if re.search(r"\bDevBuf<", ln)]
    assert uses == ["int alloc_all(DevBuf<T> &b, size_t n, Rest &&...rest)"], uses
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")) and f != "api.hip":
            assert not re.search(r"\b(DevBuf|StateBuf|WorkBuf)<", open(os.path.join(CSRC, f)).read()), f
