"""The boundary of the plant step with forward sensitivities (no GPU): ihm2mpc_sim_step_sens and its device variant are declared behind
their contract, bound with the header's signature and exported by both builds of the library; the Python entry points exist and the
acados shim names ``sens_forw`` where the sensitivities were not asked for."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int ihm2mpc_sim_step_sens\(ihm2mpc_handle \*h, int32_t model, int32_t M_sim, const double \*x, const double \*u,\s*"
        r"double \*x_next, double \*S_x, double \*S_u, int32_t \*model_used\);\s*"
        r"int ihm2mpc_sim_step_sens_device\(ihm2mpc_handle \*h, int32_t model, int32_t M_sim, const void \*x, const void \*u,\s*"
        r"void \*x_next, void \*S_x, void \*S_u, void \*model_used\);")
TABLE_LINE = 'ihm2mpc_sim_step_sens <- AcadosSimSolver.solve() with sens_forw; get("Sx" | "Su" | "S_forw")'


def _header():
    return open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()


def test_entries_are_declared_behind_their_contract():
    hdr = _header()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*" + DECL, hdr, flags=re.S)
    assert m, "the two entries are not declared right after their comment with the agreed signatures"
    doc = " ".join(line.strip().lstrip("*").strip() for line in m.group(1).splitlines())
    doc = " ".join(doc.split())
    for words in ("x (B,8)", "u (B,2)", "x_next (B,8)", "S_x (B,8,8)", "S_u (B,8,2)", "d x_next,i / d x_j", "model_used (B)", "branch",
                  "PIECEWISE", "IHM2MPC_INTEG_ERK ", "IHM2MPC_INTEG_ERK_LAG", "IHM2MPC_INTEG_IRK_GL4", "Any output may be NULL",
                  "IHM2MPC_PLANT_", "fdyn10", "stream-ordered", TABLE_LINE):
        assert words in doc, f"the comment of ihm2mpc_sim_step_sens does not mention {words!r}"
    # in the plant section, behind the plant's other entries
    assert hdr.index("int ihm2mpc_sim_advance(") < hdr.index("int ihm2mpc_get_x0(") < m.start() < hdr.index("int ihm2mpc_step(")
    # the table of replaced acados calls at the top of the header
    assert hdr.count(TABLE_LINE) == 2 and hdr.index(TABLE_LINE) < hdr.index("ihm2mpc_compute_control   <-")


def test_launch_record_documents_the_plant_code():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ihm2mpc_get_launch_record\(", _header(), flags=re.S)
    assert m and re.search(r"5 a plant step with sensitivities \(ihm2mpc_sim_step_sens", " ".join(m.group(1).split()))


def test_binding_and_export():
    from ihm2_amd import _lib

    H, dp, ip, vp = ctypes.c_void_p, _lib.c_double_p, _lib.c_int32_p, ctypes.c_void_p
    assert _lib.SYMBOLS["ihm2mpc_sim_step_sens"] == (ctypes.c_int, [H, ctypes.c_int32, ctypes.c_int32, dp, dp, dp, dp, dp, ip])
    assert _lib.SYMBOLS["ihm2mpc_sim_step_sens_device"] == (ctypes.c_int, [H, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, vp, vp])
    lib = _lib.load()
    ilp = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libihm2mpc_ilp.so"))
    for name in ("ihm2mpc_sim_step_sens", "ihm2mpc_sim_step_sens_device"):
        assert hasattr(lib, name) and hasattr(ilp, name), name


def test_python_entry_points():
    from ihm2_amd.closed_loop_sim import Simulator
    from ihm2_amd.sim import AcadosSimOpts
    from ihm2_amd.solver import BatchedOcpSolver

    p = inspect.signature(BatchedOcpSolver.sim_step_sens).parameters
    assert list(p) == ["self", "x", "u", "model", "M_sim"] and p["model"].default == 0 and p["M_sim"].default == 100
    p = inspect.signature(BatchedOcpSolver.closed_loop_matrix).parameters
    assert list(p) == ["self", "model", "M_sim"] and p["model"].default == 0 and p["M_sim"].default == 100
    assert "piecewise" in BatchedOcpSolver.sim_step_sens.__doc__ and "model_used" in BatchedOcpSolver.sim_step_sens.__doc__
    assert AcadosSimOpts().sens_forw is False            # the named deviation from acados: solve() stays on the kernel it ran
    assert callable(Simulator.simulate_sens) and callable(Simulator.closed_loop_matrix)


def _sim(kind="fkin6", **opts):
    from ihm2_amd import ocp as O
    from ihm2_amd.sim import AcadosSim, AcadosSimOpts

    sim = AcadosSim()
    sim.model = O.get_acados_model_from_explicit_dynamics("ihm2_" + kind, getattr(O, kind + "_model"), 8, 2, 3000)
    sim.solver_options = AcadosSimOpts(T=0.05, num_steps=4, integrator_type="IRK", collocation_type="GAUSS_RADAU_IIA", **opts)
    return sim


def test_shim_names_sens_forw_where_it_is_off():
    from ihm2_amd.sim import AcadosSimSolver

    s = AcadosSimSolver(_sim())
    for f in ("Sx", "Su", "S_forw"):
        with pytest.raises(ValueError, match="sens_forw"):
            s.get(f)
    with pytest.raises(ValueError, match="unknown field 'Sxx': x, CPUtime"):          # the others keep their message
        s.get("Sxx")
    assert np.array_equal(s.get("x"), np.zeros(8))
    on = AcadosSimSolver(_sim(sens_forw=True))
    assert on.sens_forw
    with pytest.raises(ValueError, match="solve"):
        on.get("S_forw")


def test_fdyn10_refuses_sens_forw():
    from ihm2_amd import ocp as O
    from ihm2_amd.sim import AcadosSimSolver

    sim = _sim()
    sim.model = O.get_acados_model_from_explicit_dynamics("ihm2_fdyn10", O.fdyn10_model, 15, 5, 3000)
    assert sim.model.kind == "fdyn10"
    AcadosSimSolver(sim)                                   # accepted without sensitivities
    sim.solver_options.sens_forw = True
    with pytest.raises(ValueError, match="sens_forw.*fdyn10"):
        AcadosSimSolver(sim)
