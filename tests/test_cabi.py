"""The C-ABI shared library loads and exports every symbol include/ihm2mpc.h declares (no compute:
runs without a GPU), and the product never routes through the oracle."""
import ctypes
import os
import re

import pytest

import host_probe as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ihm2mpc_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_boundary():
    syms = _declared_symbols()
    for must in ("ihm2mpc_create", "ihm2mpc_free", "ihm2mpc_solve", "ihm2mpc_set_x0", "ihm2mpc_get_u0",
                 "ihm2mpc_get_status", "ihm2mpc_set_tracks", "ihm2mpc_set_weights", "ihm2mpc_prepare_step", "ihm2mpc_get_sqp_merit"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    from ihm2_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared_symbols():
        assert hasattr(lib, name), f"{name} declared in include/ihm2mpc.h but not exported"
    assert set(_lib.SYMBOLS) == set(_declared_symbols())      # the ctypes table covers the header, no extras


def test_no_gpu_means_loud_failure_not_fallback():
    import shutil

    from ihm2_amd import _lib

    lib = _lib.load()
    if shutil.which("rocminfo") and os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    cfg = _lib.Config(batch=1, N=10, M=25, model=0, ntracks=1, nknots=10, device=0, nlp_solver_type=0,
                      nlp_solver_max_iter=1, ipm_iter_max=10, dt=0.05, cost_scale_stage=0.05, ipm_tol=1e-6,
                      ipm_mu0=0.03, ipm_tau0=0.1, nlp_tol=1e-6)
    h = ctypes.c_void_p()
    assert lib.ihm2mpc_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b"hip" in lib.ihm2mpc_last_error().lower()


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "ihm2_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in text.lower().replace("no cpu fallback", ""), f"{f} mentions the oracle"


def test_sensitivity_factorisation_is_written_once():
    """k_sens and k_adj differentiate one linear system: the row weights (the calls of side_sigma) and the entries of Ht (htilde) are
    written in one file of csrc, which both kernels include -- not in a copy per kernel."""
    csrc = os.path.join(ROOT, "ihm2_amd", "csrc")
    calls, defs = [], []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp", ".h", ".cpp")):
            continue
        code = re.sub(r"//.*", "", open(os.path.join(csrc, f), errors="ignore").read())
        if re.search(r"(?<!double )\bside_sigma\(", code):       # a call, not the definition `double side_sigma(`
            calls.append(f)
        if "auto htilde = " in code:
            defs.append(f)
    assert len(calls) == 1, f"side_sigma( is called in {calls}"
    assert len(defs) == 1, f"htilde is defined in {defs}"
    assert calls == defs


def test_constraint_rows_at_xbar_are_written_once():
    """k_sens, k_adj, k_slack_fold and k_penalty_grad differentiate the same constraint rows: rcoef is defined in one file of csrc, the
    fragment all four include; the row evaluation (the track rows' `dfoot`) stands there and in kernels_qp.hip, which forms the QP's own
    rows, and nowhere else; side_slack_share is defined in one file."""
    csrc = os.path.join(ROOT, "ihm2_amd", "csrc")
    rcoef, rows, share = [], [], []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp", ".h", ".cpp")):
            continue
        code = re.sub(r"//.*", "", open(os.path.join(csrc, f), errors="ignore").read())
        if "auto rcoef = " in code:
            rcoef.append(f)
        if re.search(r"\bdfoot\b", code):
            rows.append(f)
        if re.search(r"\bdouble side_slack_share\(", code):
            share.append(f)
    assert len(rcoef) == 1, f"rcoef is defined in {rcoef}"
    assert rows == sorted(["kernels_qp.hip"] + rcoef), f"the row evaluation is written in {rows}"
    assert len(share) == 1, f"side_slack_share is defined in {share}"
    for f in ("sens_factor_body.hpp", "kernels_slackseed.hip", "kernels_penaltygrad.hip"):      # ... and every user includes that file
        assert f'#include "{rcoef[0]}"' in open(os.path.join(csrc, f)).read(), f


def test_lean_trig_functions_of_the_models_match_libm(tmp_path):
    """The models' sincos / tanh (csrc/model.hpp: fast_sincos, tanh_e) restated in C with the same constants and operation order:
    within 2.5e-16 absolute of libm over +-64 rad / +-200 (tools/probes/check_fast_trig.c)."""
    src = os.path.join(ROOT, "tools", "probes", "check_fast_trig.c")
    out = HP.run(HP.build("check_fast_trig", tmp_path, extra=("-O2", "-ffp-contract=off", "-lm"), lang="c"))
    assert out.returncode == 0, out.stdout
    # the constants in the header are the ones the C check uses
    hdr = open(os.path.join(ROOT, "ihm2_amd", "csrc", "model.hpp")).read()
    for c in ("6.36619772367581382433e-01", "1.57079632679489655800e+00", "6.12323399573676603587e-17", "-1.49738490485916983693e-33",
              "1.58969099521155010221e-10", "-1.13596475577881948265e-11"):
        assert c in hdr and c in open(src).read()


def test_qp_lds_layout_holds_its_arrays_and_its_neighbour_assumptions(tmp_path):
    """The LDS layout of the interior-point QP (csrc/qp_lds.hpp) as host C++ (tools/probes/check_qp_lds.cpp, N = 2..64, every class of the
    catalogue): arrays disjoint and in order, total and factor-sweep offsets equal to the closed forms held before, every consumer's
    reach inside the block -- except the sweeps' earlier form at N = 2, 3, which starts 60 / 24 words in front of it."""
    ring = re.search(r"#define SWEEP_RING (\d+)", open(os.path.join(HP.CSRC, "kernels_qp.hip")).read()).group(1)
    out = HP.run(HP.build("check_qp_lds", tmp_path, defines=("SWEEP_RING=" + ring,)))
    assert HP.passed(out, "qp_lds: "), HP.tail(out)
    for path, uni in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 1)):
        assert f"path {path} uni {uni} N 2: the earlier form's vector sweep reaches word -60" in out.stdout
        assert f"path {path} uni {uni} N 3: the earlier form's vector sweep reaches word -24" in out.stdout
    assert out.stdout.count("reaches word") == 10


def test_oracle_and_library_share_the_interior_point_constants():
    """The checker and the product define the algorithm's constants independently (the product never includes anything under oracle/): same values."""
    import re

    def define(path, name):
        m = re.search(r"#define\s+%s\s+([0-9.eE+-]+)" % name, open(os.path.join(ROOT, path)).read())
        assert m, (path, name)
        return float(m.group(1))

    assert define("include/ihm2mpc.h", "IHM2MPC_IPM_STEP_FRACTION") == define("oracle/ihm2_oracle.h", "ORC_IPM_STEP_FRACTION")
    assert define("include/ihm2mpc.h", "IHM2MPC_IRK_NEWTON_ITER") == define("oracle/ihm2_oracle.h", "ORC_IRK_NEWTON_ITER")


def test_launch_record_getter_is_declared_documented_and_bound():
    """ihm2mpc_get_launch_record (which instantiation the launchers last launched): declared with a comment that names the fields the
    tests read, in the ctypes table with the header's signature, and wrapped by BatchedOcpSolver.get_launch_record."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import BatchedOcpSolver

    hdr = open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ihm2mpc_get_launch_record\(ihm2mpc_handle \*h, int32_t \*rec\);", hdr, flags=re.S)
    assert m, "ihm2mpc_get_launch_record is not declared right after its comment"
    doc = m.group(1)
    for word in ("k_qp_wave", "k_qp_block", "k_steps", "NSLOT", "NSOFT", "PATH", "UNI", "SQP", "IRK", "DYN", "rec (16 int32)"):
        assert word in doc, f"the comment of ihm2mpc_get_launch_record does not mention {word}"
    assert "ihm2mpc_get_launch_record" in _declared_symbols()
    assert _lib.SYMBOLS["ihm2mpc_get_launch_record"] == (ctypes.c_int, [ctypes.c_void_p, _lib.c_int32_p])
    assert callable(getattr(BatchedOcpSolver, "get_launch_record", None))
