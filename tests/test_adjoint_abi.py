"""The boundary of the adjoint sensitivities (no GPU): ihm2mpc_eval_adjoint_sensitivities is declared with its contract, bound with the
header's signature and exported; the Python entry points exist in the agreed call shapes."""
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
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ihm2mpc_eval_adjoint_sensitivities\(ihm2mpc_handle \*h, int32_t n_seeds, const double \*seed_x, "
                  r"const double \*seed_u,\s*double \*grad_x0, double \*grad_yref, double \*grad_yref_e\);", hdr, flags=re.S)
    assert m, "ihm2mpc_eval_adjoint_sensitivities is not declared right after its comment with the agreed signature"
    doc = " ".join(m.group(1).split())
    for words in ("eval_adjoint_solution_sensitivity", "dL/dx0 = nu_0", "dL/dyref_k = Gy_k' zeta_k", "seed_x (B,n_seeds,N+1,8)",
                  "seed_u (B,n_seeds,N,2)", "grad_x0 (B,n_seeds,8)", "grad_yref (B,n_seeds,N,12)", "grad_yref_e (B,n_seeds,8)", "NaN",
                  "unit seeds on u_0", "mode 1 or 2", "ihm2mpc_run_steps", "SQP mode", "1..8", "must follow the solve directly"):
        assert words in doc, f"the comment of ihm2mpc_eval_adjoint_sensitivities does not mention {words!r}"
    assert "ihm2mpc_eval_adjoint_sensitivities <-" in hdr.split("#ifndef IHM2MPC_H")[0], "missing from the table of replaced acados calls"


def test_binding_and_export():
    from ihm2_amd import _lib

    assert _lib.SYMBOLS["ihm2mpc_eval_adjoint_sensitivities"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [_lib.c_double_p] * 5)
    assert hasattr(_lib.load(), "ihm2mpc_eval_adjoint_sensitivities")
    ilp = os.path.join(ROOT, "ihm2_amd", "libihm2mpc_ilp.so")
    if os.path.exists(ilp):        # the other scheduler's build holds the kernel too
        assert hasattr(ctypes.CDLL(ilp), "ihm2mpc_eval_adjoint_sensitivities")


def test_python_entry_points():
    from ihm2_amd.solver import AcadosOcpSolver, BatchedOcpSolver

    p = inspect.signature(BatchedOcpSolver.eval_adjoint_sensitivities).parameters
    assert list(p) == ["self", "seed_x", "seed_u"] and p["seed_x"].default is None and p["seed_u"].default is None
    assert list(inspect.signature(BatchedOcpSolver.du0_ds_target).parameters) == ["self"]
    p = inspect.signature(AcadosOcpSolver.eval_adjoint_solution_sensitivity).parameters
    assert list(p)[:4] == ["self", "seed_x", "seed_u", "with_respect_to"] and p["with_respect_to"].default == "x0"


def test_shim_refuses_p_global_before_touching_the_batch():
    from ihm2_amd.solver import AcadosOcpSolver

    view = AcadosOcpSolver.__new__(AcadosOcpSolver)       # no batch behind it: the refusal comes first
    with pytest.raises(Exception, match="no p_global"):
        view.eval_adjoint_solution_sensitivity([], [], with_respect_to="p_global")
    with pytest.raises(Exception, match="is not supported"):
        view.eval_adjoint_solution_sensitivity([], [], with_respect_to="W")
