"""The forms of the interior-point QP at N = 40 under IHM2MPC_QP_FORM, once: the ladder of levels, the runner of tests/qp_forms_child.py (one
fresh process per level -- the library reads the variable once per process -- and per pytest process, its output kept for every module that
asks) and the comparison of what the levels leave behind.  Imports nothing that opens the GPU or loads the library: tests/test_qp_select.py
reads the ladder on the CPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np

QP, STEPS = "k_qp_wave<5,0,0,1>", "k_steps<5,0,0,1,0,0,0>"
# level (the value of IHM2MPC_QP_FORM, None: unset) -> (form of the factor sweep, form of the slot phases) both launch records report
# (csrc/qp_select.hpp: factor_form, slot_form)
FORMS = {"0": ("general", "general"), "1": ("plain", "general"), "2": ("plain_n40", "general"), None: ("plain_n40", "full")}
SITUATION = {"0": 0, "1": 1, "2": 2, None: 3}         # level -> QpSituation.qp_form (tests/select_probe.py: Facts.qp_form)
NAMES = {"0": "0", "1": "1", "2": "2", "unset": None}   # a level as test ids and command lines spell it
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "qp_forms_child.py")
TIMEOUT = 300

# what the child stores per path ("b<B>_<step|loop>_<key>") and per single solve ("b<B>_<case>_<key>")
SOLVE_KEYS = ("status", "qp_iter", "x", "u", "pi", "lam", "slk", "qp_res", "res", "u0")
PATH_KEYS = SOLVE_KEYS + ("hist_u0", "hist_x0", "hist_status", "hist_qp_iter")


def qp_record(level):
    return (QP,) + FORMS[level]


def steps_record(level):
    return (STEPS,) + FORMS[level]


def kernels(level):
    """the six-entry record the child stores per batch size: step()'s QP and the loop, with their forms"""
    return list(qp_record(level) + steps_record(level))


def environ(level):
    """the parent's environment with IHM2MPC_QP_FORM removed or set"""
    env = dict(os.environ)
    env.pop("IHM2MPC_QP_FORM", None)
    if level is not None:
        env["IHM2MPC_QP_FORM"] = level
    return env


STARTED = []        # (child, level) of every process runs() started, in order
_RUNS = {}          # (child, level) -> the child's arrays, or the exception its run ended with


def runs(level, child=CHILD):
    """What the child left behind at the level: started once, one child after the other.  A child that failed is not started again: every
    later caller gets the first caller's exception."""
    key = (child, level)
    if key not in _RUNS:
        STARTED.append(key)
        try:
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "out.npz")
                subprocess.run([sys.executable, child, out], env=environ(level), check=True, timeout=TIMEOUT)
                _RUNS[key] = dict(np.load(out))
        except Exception as e:      # noqa: BLE001  (an abort, a time limit, an unreadable file: all remembered)
            _RUNS[key] = e
    if isinstance(_RUNS[key], Exception):
        raise _RUNS[key]
    return _RUNS[key]


def same_values(a, b, msg=""):
    np.testing.assert_array_equal(a, b, err_msg=msg)


def same_bytes(a, b, msg=""):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), msg


def compare(got, want, names, same=same_values, what=""):
    """got[name] against want[name] for every name (or pair of names: got's, want's)"""
    for n in names:
        g, w = (n, n) if isinstance(n, str) else n
        same(got[g], want[w], f"{what}: {g}" + ("" if g == w else f" against {w}"))
