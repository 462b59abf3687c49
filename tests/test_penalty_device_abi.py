"""The penalty side of the device-pointer entries (ihm2mpc_set_instance_soft_device, _set_instance_alat_soft_device,
_get_instance_penalty_tables, _get_slacks_device, _eval_adjoint_sensitivities_p_device) and the layer on top of them
(ihm2_amd/torch_layer.py: rti_solve_soft, plant_step), as far as no GPU is needed: declared, bound with the header's argument counts,
exported by both builds, wrapped with the serial rule; the package imports no torch; the layer's argument check names the argument it
refuses."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("ihm2mpc_set_instance_soft_device", "ihm2mpc_set_instance_alat_soft_device", "ihm2mpc_get_instance_penalty_tables",
           "ihm2mpc_get_slacks_device", "ihm2mpc_eval_adjoint_sensitivities_p_device")
WRAPPERS = ("set_instance_soft_device", "set_instance_alat_soft_device", "get_instance_penalty_tables", "get_slacks_device",
            "eval_adjoint_penalty_sensitivities_device")


def _header():
    return open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ihm2mpc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_the_five_entries():
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, f"{name} is not declared in include/ihm2mpc.h"
    hdr = _header()
    # what each entry mirrors, who vouches without the check, how long the caller's memory lives, what a pattern change does
    for word in ("ihm2mpc_set_instance_soft_device / _set_instance_alat_soft_device <- ihm2mpc_set_instance_soft",
                 "ihm2mpc_get_slacks_device <- ihm2mpc_get_slacks", "ihm2mpc_eval_adjoint_sensitivities_p_device <- ihm2mpc_eval_adjoint_sensitivities_p",
                 "NO HOST COPY", "marks them as no longer fitting"):
        assert word in hdr, word
    block = hdr[hdr.index("the penalty side of the same loop"):]
    assert block.count("THE CALLER VOUCHES") == 1 and block.count("THE CALLER KEEPS") == 3
    # the list of what is not offered has shrunk to what remains
    m = re.search(r"Not offered with device pointers:(.*?)\*/", hdr, re.S)
    left = " ".join(m.group(1).replace("*", " ").split())
    assert left == "the cost-gradient entries (ihm2mpc_eval_cost_gradient ), the persistent loop (ihm2mpc_run_steps ) and the SQP mode.", left


def test_ctypes_table_has_the_headers_argument_counts():
    from ihm2_amd import _lib

    decl = _declarations()
    for name in ENTRIES:
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is ctypes.c_int
        assert len(argtypes) == len(decl[name].split(",")), name
    for name in ENTRIES[:2]:
        assert _lib.SYMBOLS[name][1][1:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    assert len(_lib.SYMBOLS["ihm2mpc_eval_adjoint_sensitivities_p_device"][1]) == 16      # the host entry's, with void pointers
    assert len(_lib.SYMBOLS["ihm2mpc_eval_adjoint_sensitivities_p"][1]) == 16
    assert _lib.SYMBOLS["ihm2mpc_eval_adjoint_sensitivities_p_device"][1][1] is ctypes.c_int32


def test_both_builds_export_them_and_the_solver_wraps_them():
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    ilp = os.path.join(os.path.dirname(_lib.LIB_PATH), "libihm2mpc_ilp.so")
    for path in (_lib.LIB_PATH, ilp):
        lib = ctypes.CDLL(path)
        for name in ENTRIES:
            assert hasattr(lib, name), f"{name} is not exported by {os.path.basename(path)}"
    for method in WRAPPERS:
        assert callable(getattr(BatchedOcpSolver, method, None)), method
    # the new kernels live in a file of their own beside kernels_weights.hip, which the Makefile builds into both libraries
    mk = open(os.path.join(ROOT, "ihm2_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bkernels_penalties\.hip\b", mk, re.M)
    src = open(os.path.join(ROOT, "ihm2_amd", "csrc", "kernels_penalties.hip")).read()
    assert "k_penalty_tables" in src and "__global__" in src


def test_importing_the_package_pulls_in_no_torch():
    code = "import sys; import ihm2_amd, ihm2_amd.solver; assert 'torch' not in sys.modules, 'torch was imported'; print('ok')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    assert not re.search(r"\btorch\b", open(os.path.join(ROOT, "ihm2_amd", "solver.py")).read().replace("torch_layer", ""))


def test_serial_number_moves_with_the_two_setters_only():
    """On a probe without a handle, as tests/test_device_entries_abi.py: the two setters advance the serial, the getters, the eval_*
    call and the plant step with sensitivities (what plant_step calls between a solve and its backward) do not."""
    from ihm2_amd.solver import BatchedOcpSolver

    class Probe:
        _serial = 0

    # each wrapper with arguments of its own signature, so that its body runs and fails on the probe's missing handle
    for name, args, moves in (("set_instance_soft_device", (0, 0), 1), ("set_instance_alat_soft_device", (0, 0), 1),
                              ("get_instance_penalty_tables", (), 0), ("get_slacks_device", (0, 0), 0),
                              ("eval_adjoint_penalty_sensitivities_device", (2,), 0), ("sim_step_sens_device", (0, 0), 0)):
        p = Probe()
        with pytest.raises(AttributeError, match="B|lib|_h"):      # the body ran: it missed the probe's handle -- after the serial has moved
            getattr(BatchedOcpSolver, name)(p, *args)
        assert p._serial == moves, name


def test_layer_signatures():
    from ihm2_amd import torch_layer as T

    assert list(inspect.signature(T.rti_solve).parameters) == ["solver", "x0", "yref", "yref_e", "W", "W_e", "zero_failed"]
    assert list(inspect.signature(T.rti_solve_soft).parameters) == ["solver", "x0", "yref", "yref_e", "W", "W_e", "soft_z", "soft_Z", "alat_z",
                                                                    "alat_Z", "zero_failed"]
    assert list(inspect.signature(T.plant_step).parameters) == ["solver", "x", "u", "model", "M_sim"]
    par = inspect.signature(T.check_rti_inputs).parameters
    assert list(par)[:8] == ["B", "N", "device", "x0", "yref", "yref_e", "W", "W_e"]
    for name in ("soft_z", "soft_Z", "alat_z", "alat_Z"):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default is None
    assert "piecewise" in T.plant_step.__doc__


def test_argument_check_names_the_penalty_it_refuses():
    import torch
    from ihm2_amd.torch_layer import check_rti_inputs

    B, N = 3, 5
    cpu = torch.device("cpu")
    f64 = dict(dtype=torch.float64)

    def base():
        return [torch.zeros(B, 8, **f64), torch.zeros(B, N, 12, **f64), torch.zeros(B, 8, **f64)]

    def good():
        return dict(soft_z=torch.zeros(B, N + 1, 28, **f64), soft_Z=torch.zeros(B, N + 1, 28, **f64), alat_z=torch.zeros(B, 2, **f64),
                    alat_Z=torch.zeros(B, 2, **f64))

    check_rti_inputs(B, N, cpu, *base(), **good())
    check_rti_inputs(B, N, cpu, *base(), **{k: v for k, v in good().items() if k.startswith("alat")})
    check_rti_inputs(B, N, cpu, *base(), **{k: v for k, v in good().items() if k.startswith("soft")})
    for name in good():
        a = good(); a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match=rf"\b{name} must be float64"):
            check_rti_inputs(B, N, cpu, *base(), **a)
        a = good(); a[name] = a[name].numpy()
        with pytest.raises(TypeError, match=rf"\b{name} must be a torch.Tensor"):
            check_rti_inputs(B, N, cpu, *base(), **a)
        # a CPU tensor where the solver's device is another one (the meta device stands for it: this test runs without a GPU)
        a = {k: (v if k == name else v.to("meta")) for k, v in good().items()}
        with pytest.raises(ValueError, match=rf"\b{name} must be on meta \(the solver's device\), it is on cpu"):
            check_rti_inputs(B, N, torch.device("meta"), *[t.to("meta") for t in base()], **a)
        a = good(); a[name] = torch.zeros((B + 1,) + tuple(a[name].shape[1:]), **f64)
        with pytest.raises(ValueError, match=rf"\b{name} must have shape"):
            check_rti_inputs(B, N, cpu, *base(), **a)
        a = good(); a[name] = a[name].transpose(0, 1).contiguous().transpose(0, 1)
        assert not a[name].is_contiguous() and a[name].shape == good()[name].shape
        with pytest.raises(ValueError, match=rf"\b{name} must be contiguous"):
            check_rti_inputs(B, N, cpu, *base(), **a)
        # a pair given by halves: the missing half is named
        other = {"soft_z": "soft_Z", "soft_Z": "soft_z", "alat_z": "alat_Z", "alat_Z": "alat_z"}[name]
        a = good(); a[other] = None
        with pytest.raises(ValueError, match=rf"\b{other} is missing: .* \({name} was given\)"):
            check_rti_inputs(B, N, cpu, *base(), **a)
    # the old check is what it was
    with pytest.raises(ValueError, match=r"\bW_e is missing: W and W_e are given together or not at all \(W was given\)"):
        check_rti_inputs(B, N, cpu, *base(), torch.zeros(B, 12, 12, **f64), None)
