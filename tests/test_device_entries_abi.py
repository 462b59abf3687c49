"""The device-pointer entries for parameters in and gradients out (ihm2mpc_set_yref_device, _set_yref_e_device,
_set_instance_weights_device, _get_instance_weight_tables, _eval_adjoint_sensitivities_w_device) and the torch layer on top of them, as
far as no GPU is needed: declared, bound with the header's argument counts, exported, wrapped; the package imports no torch; the layer's
argument check names the argument it refuses."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("ihm2mpc_set_yref_device", "ihm2mpc_set_yref_e_device", "ihm2mpc_set_instance_weights_device",
           "ihm2mpc_get_instance_weight_tables", "ihm2mpc_eval_adjoint_sensitivities_w_device")


def _declarations():
    text = open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ihm2mpc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_the_five_entries():
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, f"{name} is not declared in include/ihm2mpc.h"
    hdr = open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()
    # what the header owes the caller: what each entry mirrors, who vouches without the check, how long the seeds live, what is left out
    for word in ("ihm2mpc_set_yref_device / _set_yref_e_device <- ihm2mpc_set_yref", "ihm2mpc_set_instance_weights_device <- ihm2mpc_set_instance_weights",
                 "ihm2mpc_eval_adjoint_sensitivities_w_device <- ihm2mpc_eval_adjoint_sensitivities_w", "THE CALLER VOUCHES", "THE CALLER KEEPS",
                 "Not offered with device pointers"):
        assert word in hdr, word


def test_ctypes_table_has_the_headers_argument_counts():
    from ihm2_amd import _lib

    decl = _declarations()
    for name in ENTRIES:
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is ctypes.c_int
        assert len(argtypes) == len(decl[name].split(",")), name
    assert _lib.SYMBOLS["ihm2mpc_set_instance_weights_device"][1][-1] is ctypes.c_int32
    assert _lib.SYMBOLS["ihm2mpc_eval_adjoint_sensitivities_w_device"][1][1] is ctypes.c_int32


def test_library_exports_them_and_the_solver_wraps_them():
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
    for method in ("set_yref_device", "set_yref_e_device", "set_instance_weights_device", "get_instance_weight_tables",
                   "eval_adjoint_weight_sensitivities_device"):
        assert callable(getattr(BatchedOcpSolver, method, None)), method


def test_importing_the_package_pulls_in_no_torch():
    code = "import sys; import ihm2_amd, ihm2_amd.solver; assert 'torch' not in sys.modules, 'torch was imported'; print('ok')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    # the solver module, which the layer builds on, has no torch in it at all
    assert not re.search(r"\btorch\b", open(os.path.join(ROOT, "ihm2_amd", "solver.py")).read().replace("torch_layer", ""))


def test_serial_number_moves_with_setters_and_solves_only():
    """The wrappers are in place (no handle needed): the setters and the solving calls advance the serial, getters and eval_* do not."""
    from ihm2_amd.solver import BatchedOcpSolver

    moving = ("set_x0", "set_yref", "set_yref_e", "set_x0_device", "set_yref_device", "set_instance_weights", "set_instance_weights_device",
              "set_weights", "set_multipliers", "init_guess", "prepare_step", "solve_async", "compute_control", "run_steps", "step", "sim_advance")
    still = ("get_x", "get_u", "get_status", "get_x_device", "eval_adjoint_weight_sensitivities", "eval_adjoint_weight_sensitivities_device",
             "get_instance_weight_tables", "du0_dW", "synchronize")

    class Probe:
        _serial = 0

    for name in moving:
        p = Probe()
        with pytest.raises(Exception):      # the body fails on the probe (no handle) -- after the serial has moved
            getattr(BatchedOcpSolver, name)(p)
        assert p._serial == 1, name
    for name in still:
        p = Probe()
        with pytest.raises(Exception):
            getattr(BatchedOcpSolver, name)(p)
        assert p._serial == 0, name


def test_argument_check_of_the_layer_names_the_argument():
    import torch
    from ihm2_amd.torch_layer import check_rti_inputs

    B, N = 3, 5
    cpu = torch.device("cpu")

    def good():
        return dict(x0=torch.zeros(B, 8, dtype=torch.float64), yref=torch.zeros(B, N, 12, dtype=torch.float64),
                    yref_e=torch.zeros(B, 8, dtype=torch.float64), W=torch.zeros(B, 12, 12, dtype=torch.float64),
                    W_e=torch.zeros(B, 8, 8, dtype=torch.float64))

    check_rti_inputs(B, N, cpu, **good())
    g = good(); g.pop("W"); g.pop("W_e")
    check_rti_inputs(B, N, cpu, **g)
    for name in good():
        a = good(); a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match=rf"\b{name} must be float64"):
            check_rti_inputs(B, N, cpu, **a)
        a = good(); a[name] = a[name].numpy()
        with pytest.raises(TypeError, match=rf"\b{name} must be a torch.Tensor"):
            check_rti_inputs(B, N, cpu, **a)
        # a CPU tensor where the solver's device is another one (the meta device stands for it: this test runs without a GPU)
        a = {k: (v if k == name else v.to("meta")) for k, v in good().items()}
        with pytest.raises(ValueError, match=rf"\b{name} must be on meta \(the solver's device\), it is on cpu"):
            check_rti_inputs(B, N, torch.device("meta"), **a)
        a = good(); a[name] = torch.zeros((B + 1,) + tuple(a[name].shape[1:]), dtype=torch.float64)
        with pytest.raises(ValueError, match=rf"\b{name} must have shape"):
            check_rti_inputs(B, N, cpu, **a)
        a = good(); a[name] = a[name].transpose(0, 1).contiguous().transpose(0, 1)
        assert not a[name].is_contiguous() and a[name].shape == good()[name].shape
        with pytest.raises(ValueError, match=rf"\b{name} must be contiguous"):
            check_rti_inputs(B, N, cpu, **a)
    a = good(); a["W_e"] = None
    with pytest.raises(ValueError, match=r"\bW_e is missing"):
        check_rti_inputs(B, N, cpu, **a)
    a = good(); a["W"] = None
    with pytest.raises(ValueError, match=r"\bW is missing"):
        check_rti_inputs(B, N, cpu, **a)
    with pytest.raises(ValueError, match=r"\bx0 must be on cuda:0"):
        check_rti_inputs(B, N, torch.device("cuda", 0), **good())
