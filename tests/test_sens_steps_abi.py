"""The boundary of the persistent loop with x0 sensitivities (no GPU): ihm2mpc_run_steps_sens is declared with its contract, bound with
the header's signature and exported; the launch record documents its SENS slot; the Python entry points take the gain history."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()


def test_entry_point_is_declared_with_its_contract():
    hdr = _header()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ihm2mpc_run_steps_sens\(ihm2mpc_handle \*h, int32_t model, int32_t M_sim, double s_target, "
                  r"int32_t n_steps, int32_t freeze,\s*double lap_stop, double \*u0_hist, double \*x0_hist, int32_t \*status_hist, "
                  r"int32_t \*qp_iter_hist,\s*double \*sens_u0_hist\);", hdr, flags=re.S)
    assert m, "ihm2mpc_run_steps_sens is not declared right after its comment with the agreed signature"
    doc = " ".join(m.group(1).split())
    for words in ("eval_param_sens", "sens_u0_hist (n_steps,B,2,8)", "bit for bit", "NaN", "freeze", "ihm2mpc_get_x0_sensitivities",
                  "ihm2mpc_get_sens_u0_device", "mode 1 or 2"):
        assert words in doc, f"the comment of ihm2mpc_run_steps_sens does not mention {words!r}"
    # the plain loop keeps its signature
    assert re.search(r"int ihm2mpc_run_steps\(ihm2mpc_handle \*h, int32_t model, int32_t M_sim, double s_target, int32_t n_steps, int32_t freeze,\s*"
                     r"double lap_stop, double \*u0_hist, double \*x0_hist, int32_t \*status_hist, int32_t \*qp_iter_hist\);", hdr)


def test_launch_record_documents_the_sens_slot():
    hdr = _header()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ihm2mpc_get_launch_record\(", hdr, flags=re.S)
    assert m and "[14] SENS" in m.group(1)


def test_binding_and_export():
    from ihm2_amd import _lib

    sig = _lib.SYMBOLS["ihm2mpc_run_steps_sens"]
    plain = _lib.SYMBOLS["ihm2mpc_run_steps"]
    assert sig == (ctypes.c_int, plain[1] + [_lib.c_double_p])
    assert hasattr(_lib.load(), "ihm2mpc_run_steps_sens")


def test_python_entry_points():
    from ihm2_amd.closed_loop_sim import ClosedLoopResult
    from ihm2_amd.solver import BatchedOcpSolver

    p = inspect.signature(BatchedOcpSolver.run_steps).parameters
    assert "sens_u0_hist" in p and p["sens_u0_hist"].default is None
    names = list(ClosedLoopResult.__dataclass_fields__)
    assert names[-1] == "feedback_gain" and ClosedLoopResult.__dataclass_fields__["feedback_gain"].default is None
