"""The boundary of the gradients in the slack penalties (no GPU): ihm2mpc_eval_adjoint_sensitivities_p and
ihm2mpc_eval_cost_gradient_penalties are declared behind comments that state the formula, the sign, the lam_i = 0 rule and that bounds
stay undifferentiated, bound in _lib.SYMBOLS with the header's signatures and exported by both builds; the Python entry points exist in
the agreed shapes; the new kernel's object is in both libraries' build."""
import ctypes
import inspect
import os
import re

from test_cost_abi import _doc, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ihm2mpc_eval_adjoint_sensitivities_p", "ihm2mpc_eval_cost_gradient_penalties")


def test_entries_are_declared_with_their_contracts():
    hdr = _header()
    doc = _doc(hdr, r"int ihm2mpc_eval_adjoint_sensitivities_p\(ihm2mpc_handle \*h, int32_t n_seeds, const double \*seed_x, const double \*seed_u,\s*"
                    r"const double \*seed_s, const double \*seed_sa,\s*"
                    r"double \*grad_x0, double \*grad_yref, double \*grad_yref_e, double \*grad_W, double \*grad_W_e,\s*"
                    r"double \*grad_z, double \*grad_Z,[^\n]*\n\s*double \*grad_za, double \*grad_Za,[^\n]*\n\s*double \*zeta\);", NEW[0])
    for words in ("zeta_s,i = (c_i t_i - lam_i sgn_i r_i zeta_k) / (t_i rho_i + lam_i)", "dL/dz_i = -zeta_s,i", "dL/dZ_i = -s_i zeta_s,i",
                  "sgn_i = +1 on a lower and -1 on an", "(lam_i = 0) is dropped", "|c_i| tau / z_i", "both gradients 0, not NaN",
                  "bits of ihm2mpc_eval_adjoint_sensitivities_s", "neither 0 nor 2", "Bounds stay undifferentiated", "Blocking"):
        assert words in doc, f"the comment of {NEW[0]} does not mention {words!r}"
    doc = _doc(hdr, r"int ihm2mpc_eval_cost_gradient_penalties\(ihm2mpc_handle \*h, double \*cost, double \*grad_x0, double \*grad_yref, double \*grad_yref_e,\s*"
                    r"double \*grad_W, double \*grad_W_e, double \*grad_z, double \*grad_Z, double \*grad_za,\s*"
                    r"double \*grad_Za, double \*seed_x, double \*seed_u\);", NEW[1])
    for words in ("dJ/dz_i = s_i - zeta_s,i", "dJ/dZ_i = s_i^2 / 2 - s_i zeta_s,i", "bits of ihm2mpc_eval_cost_gradient_soft",
                  "Bounds stay undifferentiated", "Blocking"):
        assert words in doc, f"the comment of {NEW[1]} does not mention {words!r}"
    table = hdr.split("#ifndef IHM2MPC_H")[0]
    assert ", ".join(NEW) + " <-" in table, "missing from the table of replaced acados calls"


def test_binding_and_export():
    from ihm2_amd import _lib

    assert _lib.SYMBOLS[NEW[0]] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [_lib.c_double_p] * 14)
    assert _lib.SYMBOLS[NEW[1]] == (ctypes.c_int, [ctypes.c_void_p] + [_lib.c_double_p] * 12)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    ilp = os.path.join(ROOT, "ihm2_amd", "libihm2mpc_ilp.so")
    if os.path.exists(ilp):
        other = ctypes.CDLL(ilp)
        assert all(hasattr(other, n) for n in NEW)
    mk = open(os.path.join(ROOT, "ihm2_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bkernels_penaltygrad\.hip\b", mk, flags=re.M), "the new object is not among the sources both libraries link"


def test_python_entry_points():
    from ihm2_amd.solver import AcadosOcpSolver, BatchedOcpSolver

    p = inspect.signature(BatchedOcpSolver.eval_adjoint_penalty_sensitivities).parameters
    assert list(p) == ["self", "seed_x", "seed_u", "seed_s", "seed_sa"] and all(p[k].default is None for k in list(p)[1:])
    assert list(inspect.signature(BatchedOcpSolver.eval_cost_gradient_penalties).parameters) == ["self"]
    assert list(inspect.signature(BatchedOcpSolver.du0_dsoft).parameters) == ["self"]
    assert list(inspect.signature(AcadosOcpSolver.eval_adjoint_penalty_sensitivity).parameters) == ["self", "seed_x", "seed_u"]
    view = AcadosOcpSolver.__new__(AcadosOcpSolver)       # no batch behind it: the refusal of empty seeds comes first
    try:
        view.eval_adjoint_penalty_sensitivity([], [])
    except Exception as e:
        assert "seed_x and seed_u are both empty" in str(e)
    else:
        raise AssertionError("empty seeds were accepted")
