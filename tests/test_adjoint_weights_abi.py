"""The boundary of the adjoint gradients in the cost weights (no GPU): ihm2mpc_eval_adjoint_sensitivities_w is declared right after
ihm2mpc_eval_adjoint_sensitivities with its contract, bound with the header's signature and exported; the Python entry points exist in
the agreed call shapes; the acados-shaped method still refuses "W"."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()


def test_entry_point_is_declared_with_its_contract():
    hdr = _header()
    m = re.search(r"double \*grad_x0, double \*grad_yref, double \*grad_yref_e\);\s*/\*((?:(?!\*/).)*)\*/\s*"
                  r"int ihm2mpc_eval_adjoint_sensitivities_w\(ihm2mpc_handle \*h, int32_t n_seeds, const double \*seed_x, const double \*seed_u,\s*"
                  r"double \*grad_x0, double \*grad_yref, double \*grad_yref_e,\s*double \*grad_W, double \*grad_W_e\);", hdr, flags=re.S)
    assert m, "ihm2mpc_eval_adjoint_sensitivities_w is not declared right after ihm2mpc_eval_adjoint_sensitivities, behind its comment"
    doc = " ".join(m.group(1).split())
    for words in ("grad_W = -c_s sum_{k<N} sym((V zeta_k) e_k')", "grad_W_e = -sym(zeta_N[0:8] (x+_N - yref_e)')", "cost_scale_stage",
                  "e_k = V z+_k - yref_k", "sym(X) = (X + X') / 2", "symmetric", "stage-dependent shared table", "common shift",
                  "Bounds are not differentiated", "grad_W (B,n_seeds,12,12)", "grad_W_e (B,n_seeds,8,8)", "NaN", "any may be NULL",
                  "unit seeds on u_0", "mode 1 or 2", "ihm2mpc_run_steps_sens", "SQP mode", "1..8", "must follow the solve directly",
                  "first use"):
        assert words in doc, f"the comment of ihm2mpc_eval_adjoint_sensitivities_w does not mention {words!r}"
    assert "ihm2mpc_eval_adjoint_sensitivities_w <-" in hdr.split("#ifndef IHM2MPC_H")[0], "missing from the table of replaced acados calls"


def test_binding_and_export():
    from ihm2_amd import _lib

    assert _lib.SYMBOLS["ihm2mpc_eval_adjoint_sensitivities_w"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [_lib.c_double_p] * 7)
    assert hasattr(_lib.load(), "ihm2mpc_eval_adjoint_sensitivities_w")
    ilp = os.path.join(ROOT, "ihm2_amd", "libihm2mpc_ilp.so")
    if os.path.exists(ilp):        # the other scheduler's build holds the kernel too
        assert hasattr(ctypes.CDLL(ilp), "ihm2mpc_eval_adjoint_sensitivities_w")


def test_python_entry_points():
    from ihm2_amd.solver import AcadosOcpSolver, BatchedOcpSolver

    p = inspect.signature(BatchedOcpSolver.eval_adjoint_weight_sensitivities).parameters
    assert list(p) == ["self", "seed_x", "seed_u"] and p["seed_x"].default is None and p["seed_u"].default is None
    assert list(inspect.signature(BatchedOcpSolver.du0_dW).parameters) == ["self"]
    assert list(inspect.signature(AcadosOcpSolver.eval_adjoint_weight_sensitivity).parameters) == ["self", "seed_x", "seed_u"]
    # the existing entry keeps its shape
    assert list(inspect.signature(BatchedOcpSolver.eval_adjoint_sensitivities).parameters) == ["self", "seed_x", "seed_u"]


def test_old_shim_method_still_refuses_the_weights():
    from ihm2_amd.solver import AcadosOcpSolver

    view = AcadosOcpSolver.__new__(AcadosOcpSolver)       # no batch behind it: the refusal comes first
    with pytest.raises(Exception, match="is not supported"):
        view.eval_adjoint_solution_sensitivity([], [], with_respect_to="W")
    with pytest.raises(Exception, match="both empty"):
        view.eval_adjoint_weight_sensitivity([], None)
