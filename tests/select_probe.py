"""tools/probes/check_qp_select.cpp from Python: the stand-alone program that runs csrc/qp_select.hpp (the choice of the QP and step-loop
instantiations and of the linearisation and plant kernels, how run_steps proceeds, the line search's ladder, and the launch record) on the
CPU.  A helper of tests/test_qp_select.py, tests/test_steps_catalogue.py, tests/test_launch_select.py and tests/test_slot_table.py: each builds the probe once, with the address and undefined-behaviour sanitizers, and reads its lines."""
import dataclasses

import numpy as np

import host_probe as HP
import layouts as L
from host_probe import ROOT  # noqa: F401  (tests/test_slot_table.py and tests/test_qp_select.py take it from here)

KEY_FIELDS = ("set", "kind", "nslot", "nsoft", "path", "uni", "sqp", "irk", "dyn", "sens", "nf", "full")
WAVE, BLOCK, STEPS = 1, 2, 3            # QpKey.kind (csrc/qp_catalogue.hpp)
N_CU = 256                              # compute units of the MI355X


def build_probe(tmp, name="check_qp_select"):
    """The sanitizer build of tools/probes/<name>.cpp in the directory tmp; returns the program's path."""
    return HP.build(name, tmp)


def _lines(exe, *args):
    out = HP.run(exe, *args)
    assert out.returncode == 0, HP.tail(out)
    return out.stdout.splitlines()


def catalogue(exe):
    """Every key of the catalogue in selection order, as dicts of KEY_FIELDS (`--catalogue`)."""
    return [dict(zip(KEY_FIELDS, (int(v) for v in line.split()))) for line in _lines(exe, "--catalogue")]


def key_name(k):
    """The name the launch record gives a key's kernel (BatchedOcpSolver.get_launch_record)."""
    if k["kind"] == WAVE:
        return "k_qp_wave<%d,%d,%d,%d>" % (k["nslot"], k["nsoft"], k["path"], k["uni"])
    if k["kind"] == BLOCK:
        return "k_qp_block<%d,%d,4>" % (k["nslot"], k["uni"])
    return "k_steps<%d,%d,%d,%d,%d,%d,%d%s>" % (k["nslot"], k["nsoft"], k["path"], k["uni"], k["sqp"], k["irk"], k["dyn"], ",1" if k["sens"] else "")


def records(exe):
    """(`--records`) the record encode_launch writes for every key alone, in catalogue order, and enumerator name -> the record note_lin /
    note_sim writes for it."""
    keys, kernels = [], {}
    for line in _lines(exe, "--records"):
        head, _, rec = line.partition("rec")
        rec = [int(v) for v in rec.split()]
        assert len(rec) == 16
        if head.strip():
            kernels[head.strip()] = rec
        else:
            keys.append(rec)
    return keys, kernels


@dataclasses.dataclass(frozen=True)
class Facts:
    """The configuration a handle is in, beside its problem: what api.hip: ihm2_situation reads, and the arguments of the call.  The defaults: the reference's OCP, one
    controller's worth of buffers, an MI355X."""
    model: int = 0                  # IHM2MPC_MODEL_*
    integrator: int = 0             # IHM2MPC_INTEG_* of the shooting intervals
    sim_integrator: int = 0         # ... of the plant
    sqp: bool = False
    globalization: int = 0          # 1: MERIT_BACKTRACKING
    B: int = 5
    n_cu: int = N_CU
    sens: int = 0
    inst_b: bool = False
    block_qp: bool = True
    qp_form: int = 3                # IHM2MPC_QP_FORM; 3: unset
    buffers: int = None             # None: what ihm2mpc_create and ihm2mpc_run_steps allocate for this configuration
    plant: int = 0                  # the plant model of ihm2mpc_step / ihm2mpc_run_steps / ihm2mpc_sim_step: -2 .. 2
    freeze: bool = False            # ihm2mpc_run_steps' freeze
    linearize_cols: bool = False    # IHM2MPC_LINEARIZE_COLS=1
    persistent_rounds: bool = False  # IHM2MPC_PERSISTENT_ROUNDS=1

    def tokens(self):
        irk = self.integrator in (1, 2)
        buffers = self.buffers
        if buffers is None:     # the tableau with a collocation integrator; the line search's buffers in the SQP mode, its rollouts with collocation
            buffers = (1 if irk else 0) | (2 if self.sqp else 0) | (4 if self.sqp and self.integrator != 0 and self.globalization else 0)
        return [self.model, self.integrator, self.sim_integrator, int(self.sqp), self.globalization, self.B, self.n_cu, int(self.sens != 0),
                int(self.inst_b), int(self.block_qp), self.qp_form, buffers, self.plant, int(self.freeze), int(self.linearize_cols),
                int(self.persistent_rounds)]


def facts_of_data(data, **more):
    """The Facts of an OcpData (BatchedOcpSolver.__init__ passes the same fields to ihm2mpc_create and ihm2mpc_set_sqp_options)."""
    from ihm2_amd.solver import _GLOBALIZATION

    sqp = data.nlp_solver_type == "SQP"
    return Facts(model=data.model, integrator=data.integrator, sim_integrator=data.sim_integrator, sqp=sqp,
                 globalization=_GLOBALIZATION[data.globalization] if sqp else 0, **more)


def problem_text(lay, data=None) -> str:
    """The problem of a layout as tools/probes/problem_file.hpp reads it: what test_gpu_qp_layouts.py::_solver leaves in the handle."""
    data = L.make_ocp(lay).flatten() if data is None else data
    arr = L.apply(data, lay)

    def nums(a):
        return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())

    out = [lay.name, str(lay.N)] + [nums(arr[n]) for n in ("lbx", "ubx", "lbu", "ubu", "C", "D", "lg", "ug")]
    soft = data.soft_Z is not None and bool(np.any(np.asarray(data.soft_Z) >= 0.0))         # BatchedOcpSolver._push_soft
    out.append("1 " + nums(data.soft_z) + " " + nums(data.soft_Z) if soft else "0")
    out.append("1 " + nums(data.lh) + " " + nums(data.uh) if data.path_on else "0")
    if data.path_on and data.alat_on:
        out.append("1 " + nums([data.alat_lb, data.alat_ub]))
        out.append("0" if data.alat_soft_Z is None else "1 " + nums(np.zeros(2) if data.alat_soft_z is None else data.alat_soft_z) + " " + nums(data.alat_soft_Z))
    else:
        out.append("0")
    W = np.asarray(data.W)          # ihm2mpc_set_weights: the stages' weights are one matrix
    out.append("1" if W.ndim == 2 or bool(np.all(W == W[0])) else "0")
    return "\n".join(out) + "\n"


def select(exe, tmp, jobs):
    """Runs the probe on jobs = [(layout, Facts)], one argument each.  Returns per job a dict: `qp` / `steps` the position of the chosen key
    in catalogue() or None, `qp_lds` / `steps_lds` the LDS bytes of the launch, `lin` / `sim` the enumerators of select_linearize / select_sim,
    `run` select_run's outcome (persistent, no_instantiation, not_resident, refused), `rec` the sixteen integers of the launch record."""
    files, args = {}, []
    for lay, facts in jobs:
        if lay.name not in files:
            files[lay.name] = str(tmp / (lay.name + ".txt"))
            with open(files[lay.name], "w") as f:
                f.write(problem_text(lay))
        args.append(" ".join([files[lay.name]] + [str(v) for v in facts.tokens()]))
    lines = _lines(exe, *args)
    assert lines[-1] == "qp selection: all checks passed" and len(lines) == len(jobs) + 1, lines[-5:]
    out = []
    for (lay, _), line in zip(jobs, lines):
        t = line.split()
        assert t[0] == lay.name and (t[1], t[4], t[7], t[9], t[11], t[13]) == ("qp", "steps", "lin", "sim", "run", "rec") and len(t) == 30, line
        pos = lambda v: None if v == "none" else int(v)       # noqa: E731
        out.append(dict(qp=pos(t[2]), qp_lds=int(t[3]), steps=pos(t[5]), steps_lds=int(t[6]), lin=t[8], sim=t[10], run=t[12],
                        rec=[int(v) for v in t[14:]]))
    return out


def ladder(exe, alpha_min, alpha_red, B, N):
    """(`--ladder`) (ladder_length, ladder_first) of the SQP options on a collocation handle of B instances and the horizon N; the length
    is None where it exceeds IHM2MPC_LS_MAX_TRIALS (ihm2mpc_set_sqp_options refuses the pair)."""
    (line,) = _lines(exe, "--ladder", repr(float(alpha_min)), repr(float(alpha_red)), str(B), str(N))
    t = line.split()
    assert t[0] == "ladder"
    return (None, None) if t[1:] == ["too_long"] else (int(t[1]), int(t[2]))
