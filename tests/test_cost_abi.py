"""The boundary of the cost and its gradient (no GPU): ihm2mpc_eval_cost and ihm2mpc_eval_cost_gradient are declared behind their comments,
which state the formulae and the soft-side refusal, bound in _lib.SYMBOLS with the header's signatures and exported; the Python entry
points exist in the agreed shapes; the acados-shaped method refuses what it does not differentiate in."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()


def _doc(hdr, pattern, what):
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*" + pattern, hdr, flags=re.S)
    assert m, f"{what} is not declared behind its comment with the agreed signature"
    return " ".join(re.sub(r"\n \*", "\n", m.group(1)).split())      # without the comment's leading asterisks


def test_eval_cost_is_declared_with_its_contract():
    hdr = _header()
    doc = _doc(hdr, r"int ihm2mpc_eval_cost\(ihm2mpc_handle \*h, double \*cost, double \*stage_cost, double \*slack_cost\);", "ihm2mpc_eval_cost")
    for words in ("J = sum_{k<N} (c_s/2) e_k' W_k e_k + 1/2 e_N' W_e e_N + J_slack", "z_i s_i + 1/2 Z_i s_i^2", "e_k = V z_k - yref_k",
                  "e_N = x_N - yref_e", "y = (x, u, x[6:8] - u)", "cost_scale_stage", "as acados documents get_cost", "any may be NULL",
                  "cost (B)", "stage_cost (B,N+1)", "slack_cost (B)", "both solver modes", "ihm2mpc_init_guess", "ihm2mpc_run_steps",
                  "changes no output", "lateral-acceleration row", "Blocking"):
        assert words in doc, f"the comment of ihm2mpc_eval_cost does not mention {words!r}"
    assert "equal to acados" not in hdr
    table = hdr.split("#ifndef IHM2MPC_H")[0]
    assert "ihm2mpc_eval_cost " in table and "ihm2mpc_eval_cost_gradient <-" in table, "missing from the table of replaced acados calls"


def test_eval_cost_gradient_is_declared_with_its_contract():
    hdr = _header()
    doc = _doc(hdr, r"int ihm2mpc_eval_cost_gradient\(ihm2mpc_handle \*h, double \*cost, double \*grad_x0, double \*grad_yref, double \*grad_yref_e,\s*"
                    r"double \*grad_W, double \*grad_W_e, double \*seed_x, double \*seed_u\);", "ihm2mpc_eval_cost_gradient")
    for words in ("t_k = W_k e_k", "seed_z,k = c_s V' t_k", "seed_x,k = c_s (t[0:8] + (0,..,0, t[10], t[11]))", "seed_u,k = c_s (t[8:10] - t[10:12])",
                  "seed_x,N = W_e e_N", "dJ/dx0 = grad_x0", "dJ/dyref_k = grad_yref_k - c_s t_k", "dJ/dyref_e = grad_yref_e - W_e e_N",
                  "dJ/dW = grad_W + (c_s/2) sum_{k<N} e_k e_k'", "dJ/dW_e = grad_W_e + 1/2 e_N e_N'", "common to all stages", "exactly symmetric",
                  "RTI step's solution", "eval_and_get_optimal_value_gradient", "n_seeds = 1", "any may be NULL", "grad_W (B,12,12)",
                  "seed_x (B,N+1,8)", "seed_u (B,N,2)", "NaN", "stay finite", "mode 1 or 2", "ihm2mpc_run_steps_sens", "SQP mode",
                  "must follow the solve directly", "soft side", "all-hard tables only", "carry no seed", "no host round trip", "Blocking"):
        assert words in doc, f"the comment of ihm2mpc_eval_cost_gradient does not mention {words!r}"


def test_binding_and_export():
    from ihm2_amd import _lib

    assert _lib.SYMBOLS["ihm2mpc_eval_cost"] == (ctypes.c_int, [ctypes.c_void_p] + [_lib.c_double_p] * 3)
    assert _lib.SYMBOLS["ihm2mpc_eval_cost_gradient"] == (ctypes.c_int, [ctypes.c_void_p] + [_lib.c_double_p] * 8)
    lib = _lib.load()
    assert hasattr(lib, "ihm2mpc_eval_cost") and hasattr(lib, "ihm2mpc_eval_cost_gradient")


def test_python_entry_points():
    from ihm2_amd.controller import IHM2Controller
    from ihm2_amd.solver import AcadosOcpSolver, BatchedOcpSolver

    p = inspect.signature(BatchedOcpSolver.get_cost).parameters
    assert list(p) == ["self", "stagewise"] and p["stagewise"].default is False
    assert list(inspect.signature(BatchedOcpSolver.eval_cost_gradient).parameters) == ["self"]
    assert list(inspect.signature(AcadosOcpSolver.get_cost).parameters) == ["self"]
    p = inspect.signature(AcadosOcpSolver.eval_and_get_optimal_value_gradient).parameters
    assert list(p) == ["self", "with_respect_to"] and p["with_respect_to"].default == "initial_state"
    assert list(inspect.signature(IHM2Controller.cost).parameters) == ["self"]


def test_shim_refuses_what_it_does_not_differentiate_in():
    from ihm2_amd.solver import AcadosOcpSolver

    view = AcadosOcpSolver.__new__(AcadosOcpSolver)       # no batch behind it: the refusals come first
    with pytest.raises(Exception, match="no p_global"):
        view.eval_and_get_optimal_value_gradient("p_global")
    with pytest.raises(Exception, match="is not supported"):
        view.eval_and_get_optimal_value_gradient("params_global")
