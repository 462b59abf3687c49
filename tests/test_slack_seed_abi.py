"""The boundary of the adjoint seeds on the soft slacks (no GPU): ihm2mpc_eval_adjoint_sensitivities_s and
ihm2mpc_eval_cost_gradient_soft are declared behind comments that state the fold and what is ignored, bound in _lib.SYMBOLS with the
header's signatures and exported by both builds; the Python entry points exist in the agreed shapes and the old ones keep theirs."""
import ctypes
import inspect
import os

from test_cost_abi import _doc, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_with_their_contracts():
    hdr = _header()
    doc = _doc(hdr, r"int ihm2mpc_eval_adjoint_sensitivities_s\(ihm2mpc_handle \*h, int32_t n_seeds, const double \*seed_x, const double \*seed_u,\s*"
                    r"const double \*seed_s, const double \*seed_sa,\s*"
                    r"double \*grad_x0, double \*grad_yref, double \*grad_yref_e, double \*grad_W, double \*grad_W_e\);",
               "ihm2mpc_eval_adjoint_sensitivities_s")
    for words in ("seed_s (B,n_seeds,N+1,28)", "seed_sa (B,n_seeds,N+1,2)", "gamma_i = lam_i / (t_i rho_i + lam_i)", "sgn_i = +1 on a lower side",
                  "c_i gamma_i sgn_i r_i", "without a slack", "is ignored", "all four NULL with n_seeds == 2", "no fold runs",
                  "bits of ihm2mpc_eval_adjoint_sensitivities_w", "neither 0 nor 2", "Blocking"):
        assert words in doc, f"the comment of ihm2mpc_eval_adjoint_sensitivities_s does not mention {words!r}"
    doc = _doc(hdr, r"int ihm2mpc_eval_cost_gradient_soft\(ihm2mpc_handle \*h, double \*cost, double \*grad_x0, double \*grad_yref, double \*grad_yref_e,\s*"
                    r"double \*grad_W, double \*grad_W_e, double \*seed_x, double \*seed_u\);", "ihm2mpc_eval_cost_gradient_soft")
    for words in ("every constraint table", "c_i = dJ_slack/ds_i = z_i + Z_i s_i", "the seeds the adjoint saw, after the fold", "no fold runs",
                  "bits of ihm2mpc_eval_cost_gradient", "Blocking"):
        assert words in doc, f"the comment of ihm2mpc_eval_cost_gradient_soft does not mention {words!r}"
    table = hdr.split("#ifndef IHM2MPC_H")[0]
    assert "ihm2mpc_eval_adjoint_sensitivities_s, ihm2mpc_eval_cost_gradient_soft <-" in table, "missing from the table of replaced acados calls"


def test_binding_and_export():
    from ihm2_amd import _lib

    assert _lib.SYMBOLS["ihm2mpc_eval_adjoint_sensitivities_s"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [_lib.c_double_p] * 9)
    assert _lib.SYMBOLS["ihm2mpc_eval_cost_gradient_soft"] == (ctypes.c_int, [ctypes.c_void_p] + [_lib.c_double_p] * 8)
    lib = _lib.load()
    assert hasattr(lib, "ihm2mpc_eval_adjoint_sensitivities_s") and hasattr(lib, "ihm2mpc_eval_cost_gradient_soft")
    ilp = os.path.join(ROOT, "ihm2_amd", "libihm2mpc_ilp.so")
    if os.path.exists(ilp):
        other = ctypes.CDLL(ilp)
        assert hasattr(other, "ihm2mpc_eval_adjoint_sensitivities_s") and hasattr(other, "ihm2mpc_eval_cost_gradient_soft")


def test_python_entry_points():
    from ihm2_amd.solver import AcadosOcpSolver, BatchedOcpSolver

    p = inspect.signature(BatchedOcpSolver.eval_adjoint_slack_sensitivities).parameters
    assert list(p) == ["self", "seed_x", "seed_u", "seed_s", "seed_sa"] and all(p[k].default is None for k in list(p)[1:])
    assert list(inspect.signature(BatchedOcpSolver.eval_cost_gradient_soft).parameters) == ["self"]
    p = inspect.signature(AcadosOcpSolver.eval_and_get_optimal_value_gradient_soft).parameters
    assert list(p) == ["self", "with_respect_to"] and p["with_respect_to"].default == "initial_state"
    view = AcadosOcpSolver.__new__(AcadosOcpSolver)       # no batch behind it: the refusals come first
    for what, text in (("p_global", "no p_global"), ("params_global", "is not supported")):
        try:
            view.eval_and_get_optimal_value_gradient_soft(what)
        except Exception as e:
            assert text in str(e)
        else:
            raise AssertionError(f"with_respect_to = {what!r} was accepted")
