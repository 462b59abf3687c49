"""One configuration per instantiation of the persistent control-step loop k_steps<NSLOT, NSOFT, PATH, UNI, SQP, IRK, DYN[, SENS]>
(csrc/qp_catalogue.hpp: the STEPS entries; kernels_qp.hip expands them), the configurations that must go per step, and the entries
no configuration reaches.  A helper: tests/test_steps_catalogue.py checks the table against the catalogue without a GPU,
tests/test_gpu_steps_catalogue.py launches every entry.

Each case is derived by reading csrc/qp_select.hpp: select_steps -- and tests/test_steps_catalogue.py runs that function on every
case, without a GPU (tools/probes/check_qp_select.cpp).  It asks find_form for the key

    {QP_STEPS, slots.per_lane, slots.nsoft, path_class, uniform_H && uniform_CD, sqp, irk, dyn, sens}

and takes the first catalogue entry with these fields and at least this NSLOT:

    NSLOT, NSOFT   the slot table rebuild_slots lays out from the rows (qp_tables.hpp: lay_out_slots): slots per lane of 64, and the
                   leading one-sided entries per lane it was laid out for -> the layout (tests/layouts.py)
    PATH           path_class: 0 none, 1 the track rows, 2 with the lateral-acceleration row (no k_steps has it) -> the layout
    UNI            batch-shared, stage-independent weights and general rows; 0 with Layout.stage_W -> the layout
    SQP            cfg.nlp_solver_type == SQP -> the live options (python/main.py:230-237: SQP, 2 iterations, MERIT_BACKTRACKING)
    IRK            0 RK4, 1 collocation (one Gauss-Legendre step per interval), 2 RK4 with the closed-form actuator lags (ERK_LAG)
    DYN            cfg.model != fkin6 -> fdyn6u (fdyn6 as written is not used: most of its QPs are infeasible)
    SENS           ihm2mpc_run_steps_sens (set_x0_sensitivities(1 or 2) + run_steps(sens_u0_hist=...))

Several catalogue sets hold one name in more than one form of the factor sweep and the slot phases (sets 4, 6, 7: find_form prefers
them where the handle may take them).  The launch record's name does not tell the forms apart, its steps_form / steps_slots fields do:
FORMS below says which object the cases of those names run, and the GPU test asserts it (tests/test_gpu_factor_sweep_forms.py and
tests/test_gpu_slot_forms.py compare the forms with one another)."""
from __future__ import annotations

import dataclasses

import layouts as L

Lay = L.Layout

# Layouts needed only here (not in L.TABLE, which feeds the recorded digests of tests/test_slot_table.py): the all-hard tables of 8
# and 10 slots per lane at short horizons (L.TABLE has them at N = 64 and N = 53) -- every state boxed gives 12 rows per stage,
# 480 slots at N = 40 (7.5 per lane -> 8) and 516 at N = 43 (8.06 per lane -> 9, the NSLOT = 10 instantiations) -- and the reference
# layout at N = 3, where the SQP loops' sweeps would start in front of the block's LDS (select_steps: qp_sweeps_inside).
EXTRA = {
    "hard_8_per_lane_N40": Lay("hard_8_per_lane_N40", N=40, xbox="all"),
    "hard_8_per_lane_N40_stage_W": Lay("hard_8_per_lane_N40_stage_W", N=40, xbox="all", stage_W=True, seed=31),
    "hard_10_per_lane_N43": Lay("hard_10_per_lane_N43", N=43, xbox="all"),
    "hard_10_per_lane_N43_stage_W": Lay("hard_10_per_lane_N43_stage_W", N=43, xbox="all", stage_W=True, seed=32),
    "ref_N3": Lay("ref_N3", N=3),
}
LAYOUTS = {**{n: t[0] for n, t in L.TABLE.items()}, **EXTRA}

# (NSLOT, NSOFT, PATH, UNI) of the k_steps instantiations -> the layout that gives the table
TABLES = {
    (5, 0, 0, 1): "hard_5_per_lane", (5, 0, 0, 0): "hard_5_per_lane_stage_W",
    (8, 0, 0, 1): "hard_8_per_lane_N40", (8, 0, 0, 0): "hard_8_per_lane_N40_stage_W",
    (10, 0, 0, 1): "hard_10_per_lane_N43",
    (8, 2, 0, 1): "soft_2_per_lane", (10, 4, 0, 1): "soft_3_per_lane_asym",
    (8, 0, 1, 1): "path_hard", (8, 3, 1, 1): "path_soft_3_per_lane", (10, 4, 1, 1): "path_soft_both_sides",
}
HARD = [(5, 0, 0, 0), (5, 0, 0, 1), (8, 0, 0, 0), (8, 0, 0, 1), (10, 0, 0, 1)]
SOFT = [(8, 2, 0, 1), (10, 4, 0, 1), (8, 0, 1, 1), (8, 3, 1, 1), (10, 4, 1, 1)]

LIVE = dict(nlp_solver_type="SQP", nlp_solver_max_iter=2, globalization="MERIT_BACKTRACKING")       # python/main.py:230-237
INTEG = {0: ("ERK", dict(integrator_type="ERK")), 1: ("IRK", dict(integrator_type="IRK", sim_method_num_steps=1)),       # python/main.py:234-236
         2: ("ERK_LAG", dict(integrator_type="ERK_LAG", sim_method_num_steps=4))}
MODEL_CODE = {"fkin6": 0, "fdyn6u": 2}          # include/ihm2mpc.h: IHM2MPC_MODEL_*, also the plant argument of step / run_steps
B = 5           # x N = 40: 200 intervals, no latency batch (launch_cases.latency_batch: k_linearize_cols and the state-only plant); a ragged last wave


@dataclasses.dataclass(frozen=True)
class Case:
    name: str               # the launch record run_steps must leave: "k_steps<...>", or "per_step" for a FALLBACK entry
    layout: str             # key of LAYOUTS
    model: str = "fkin6"    # the OCP's model
    irk: int = 0            # key of INTEG
    sqp: bool = False       # the live SQP options, else RTI
    sens: int = 0           # 0: run_steps; 1, 2: run_steps_sens with this x0 sensitivity mode
    plant: int = 0          # the plant argument: 0 kinematic (on lane N of the loop), 2 fdyn6u, -1 / -2 the speed-switched plants
    M_sim: int = 30
    seed: int = 0           # of conftest.sample_x0
    qp_set: int = 0         # the catalogue set that holds the name (the ILP library has objects of its own for the sets 0, 1 and 3)
    opts: tuple = ()        # further solver options, as (name, value) pairs
    reason: str = ""        # FALLBACK entries: the steps_fallback the launch record must report
    form: tuple = ("general", "general")        # the launch record's (steps_form, steps_slots): which object of the name find_form takes
    B: int = B
    tracks: int = 1         # 2: the handle holds the two tables of tests/multi_track_cases.py, instance b on track b mod 2 (TWO_TRACK)

    def ocp_opts(self) -> dict:
        o = dict(model=self.model, **INTEG[self.irk][1])
        if self.sqp:
            o.update(LIVE)
        o.update(dict(self.opts))
        return o

    @property
    def accepted(self):
        return (0, 2) if self.sqp else (0,)          # 2: the SQP mode's iteration limit (python/main.py:326 keeps the iterate)


def s_target(lay) -> float:
    """The reference point's lead on the car: 40 m at the horizon 40 (python/main.py:303-322), a metre per stage at the others."""
    return float(lay.N)


def start(track, case):
    """(x0, yref, yref_e) of a case: the start of tests/test_gpu_qp_layouts.py::_start, with the lead of s_target."""
    import numpy as np

    import drive

    N = LAYOUTS[case.layout].N
    lead = s_target(LAYOUTS[case.layout])
    if case.tracks > 1:         # per track from that track's own table (``track`` is not used)
        import multi_track_cases as MT

        return MT.start_arrays(LAYOUTS[case.layout], case.B, case.seed, lead)
    x0 = drive.clipped_start(track, case.B, case.seed)
    yref = np.zeros((case.B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + lead * np.arange(N)[None] / N
    yref_e = np.zeros((case.B, 8)); yref_e[:, 0] = x0[:, 0] + lead
    return x0, yref, yref_e


def sqp_kwargs(data) -> dict:
    """The arguments of OracleProblem.sqp_solve that restate the handle's SQP options (BatchedOcpSolver.__init__ -> set_sqp_options)."""
    return dict(globalization=data.globalization, tol=data.sqp_tol, alpha_min=data.alpha_min, alpha_reduction=data.alpha_reduction,
                eps_sufficient_descent=data.eps_sufficient_descent, use_sufficient_descent=bool(data.use_sufficient_descent),
                full_step_dual=bool(data.full_step_dual))


def track_ids(case):
    """The per-instance track ids of a case, None on one track."""
    import multi_track_cases as MT

    return MT.track_ids(case.B) if case.tracks > 1 else None


def oracle_problem(track, data, lay, tables=None, widths=None):
    """The OracleProblem of a handle's data.  The C oracle has no ERK_LAG integrator: for such a handle it is used for everything but the
    dynamics (its own records are replaced, see oracle_rti_step), as tests/test_gpu_lag_integrator.py does.  ``tables`` = (s_ref,
    kappa_ref) of several tracks and ``widths`` (ntracks, 2) replace the track's table and the layout's widths."""
    from oracle import oracle as orc

    s_ref, kappa_ref = (track.s_ref, track.kappa_ref) if tables is None else tables
    desc = dict(data.as_dict(s_ref, kappa_ref, track_widths=L.track_widths(lay) if widths is None else widths))
    if data.integrator == 3:        # ocp.INTEG_ERK_LAG
        desc["integrator"], desc["M"] = orc.INTEG_RK4, 25
    return orc.OracleProblem(desc)


def rti_status_of_qp(r) -> int:
    """orc_rti_step's rule: the RTI status of an orc.qp_solve result (1 not finite / failed, 4 infeasible or iteration limit unconverged, else 0)."""
    import numpy as np

    return 1 if r["status"] == 3 or not np.all(np.isfinite(r["dz"])) else 4 if r["status"] in (2, 4) else 0


def oracle_rti_step(P, data, track, x, u, x0, yref, yref_e, track_id=None):
    """OracleProblem.rti_step (x, u updated in place; status, qp_iter, pi, lam).  ERK_LAG: OracleProblem.build_qp at the iterate with
    A, B, b replaced by those of tests/lag_ref.py, orc.qp_solve, the step applied by orc_rti_step's rule
    (tests/test_gpu_lag_integrator.py::test_rti_step_matches_the_oracle_qp_on_lag_ref_records).  ``track_id``: per-instance track ids
    of a problem with several tables (not with ERK_LAG: lag_ref takes one table)."""
    import numpy as np

    if data.integrator != 3:
        return P.rti_step(x, u, x0, yref, yref_e, track_id=track_id)
    assert track_id is None
    import lag_ref
    from oracle import oracle as orc

    B, N = x.shape[0], data.N
    A, Bm, b = lag_ref.linearize(x, u, track.s_ref, track.kappa_ref, data.dt, data.M)
    status = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
    pi = np.zeros((B, N + 1, 8)); lam = np.zeros((B, N + 1, 2 * L.NC))
    soft = {} if data.soft_Z is None else dict(zip(("soft_z", "soft_Z"), L.soft_arrays(data)))
    for i in range(B):
        qp = P.build_qp(x[i], u[i], x0[i], yref[i], yref_e[i])
        r = orc.qp_solve(qp["H"], qp["g"], A[i], Bm[i], b[i], qp["dx0"], qp["R"], qp["dl"], qp["du"], iter_max=P.p.ipm_iter_max, tol=P.p.ipm_tol,
                         mu0=P.p.ipm_mu0, tau0=P.p.ipm_tau0, **soft)
        iters[i] = r["iters"]
        status[i] = rti_status_of_qp(r)
        if status[i] == 0:
            x[i] += r["dz"][:, :8]; u[i] += r["dz"][:N, 8:]
            pi[i], lam[i] = r["pi"], r["lam"]
    return dict(status=status, qp_iter=iters, pi=pi, lam=lam)


def steps_name(table, sqp, irk, dyn, sens=0):
    return "k_steps<%d,%d,%d,%d,%d,%d,%d%s>" % (*table, int(sqp), irk, int(dyn), ",1" if sens else "")


# The sample_x0 seed of a case is 700 + the layout's own seed, as tests/test_gpu_qp_layouts.py starts its loops.  From these starts the oracle
# solves every instance's first step (tests/test_steps_catalogue.py asserts 60 %), so no case needed another seed.

# Two names exist in further forms (qp_select.hpp: find_form; the launch record tells them apart in steps_form / steps_slots), and the cases
# assert the one they run:
#   k_steps<5,0,0,1,0,0,0>  on the reference layout at N = 40 the table is full (qp_tables.hpp: slot_table_full): the set-7 object, horizon
#                           40 compiled in and straight-line slot phases.  The ILP library links that object from the default build, so
#                           the "ilp" run of this name takes a 5-slot table that is not full (ILP_CASES): the set-4 object, of which the
#                           ILP library has a build of its own.  The general form of set 0 runs only for a table without active rows
#                           (tests/test_gpu_qp_layouts.py: empty_table, in both builds) or under IHM2MPC_QP_FORM=0.
#   k_steps<5,0,0,1,0,2,0>  the set-6 object with the horizon 40 compiled in (set 5's general form: under IHM2MPC_QP_FORM=0 only)
FORMS = {"k_steps<5,0,0,1,0,0,0>": ("plain_n40", "full"), "k_steps<5,0,0,1,0,2,0>": ("plain_n40", "general")}


def _cases():
    out = []
    count = {}

    def add(table, sqp, irk, dyn, sens, qp_set):
        # the plant argument rotates within each (IRK, DYN) class over 0, the OCP's own model (for fkin6: the other speed-switched
        # plant) and a speed-switched plant, so that both the kinematic plant on lane N and a called dynamic plant occur in every class
        i = count[(irk, dyn)] = count.get((irk, dyn), -1) + 1
        plant = ((0, 2, -2) if dyn else (0, -1, -2))[i % 3]
        opts, M_sim = (), 30
        if irk == 2 and i % 2 == 0:       # the closed-form lags in the plant as well: lane N of the loop, the kinematic plant only
            opts, plant, M_sim = (("sim_integrator_type", "ERK_LAG"),), 0, 4
        name = steps_name(table, sqp, irk, dyn, sens)
        lay = LAYOUTS[TABLES[table]]
        out.append(Case(name, TABLES[table], "fdyn6u" if dyn else "fkin6", irk, bool(sqp), (1 + i % 2) if sens else 0, plant, M_sim,
                        700 + lay.seed, qp_set, opts, form=FORMS.get(name, ("general", "general"))))

    for sqp in (0, 1):          # the sets 0, 1 and 2 are built in both SQP modes
        for t in HARD:          # set 0: RK4 on every all-hard table, collocation on the batch-shared ones
            add(t, sqp, 0, 0, 0, 0)
            if t[3] == 1:
                add(t, sqp, 1, 0, 0, 0)
        for t in SOFT:          # set 1
            for irk in (0, 1):
                add(t, sqp, irk, 0, 0, 1)
        for t in [(5, 0, 0, 1), (8, 0, 0, 1)] + SOFT:       # set 2: the dynamic OCP model (no <10,0,0>, no UNI = 0)
            for irk in (0, 1):
                add(t, sqp, irk, 1, 0, 2)
    for t in HARD:              # set 3: the RTI loops of the sets 0 and 1 with SENS = 1
        add(t, 0, 0, 0, 1, 3)
        if t[3] == 1:
            add(t, 0, 1, 0, 1, 3)
    for t in SOFT:
        for irk in (0, 1):
            add(t, 0, irk, 0, 1, 3)
    for t in HARD:              # set 5: the closed-form lags, RTI, all-hard, without sensitivities
        add(t, 0, 2, 0, 0, 5)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the cases that run on another layout in the ILP build (see FORMS): 5 slots per lane, a random subset of the state boxes, one-sided rows
ILP_CASES = {"k_steps<5,0,0,1,0,0,0>": dataclasses.replace(BY_NAME["k_steps<5,0,0,1,0,0,0>"], layout="hard_random_one_sided", seed=703,
                                                           form=("plain_n40", "general"))}

# Configurations ihm2mpc_run_steps must launch per step, with the steps_fallback of the launch record (qp_select.hpp: select_steps chooses
# none: "no_instantiation"; the other reason, "not_resident", needs more than 4 x 256 instances and is asserted in
# tests/test_gpu_closed_loop.py and tests/test_gpu_sens_steps.py at B = 1100).  id -> case
_NO = "no_instantiation"
FALLBACK = {
    # find_form finds no entry: UNI = 0 exists for <5,0,0> and <8,0,0> with RK4 and the kinematic model only
    "stage_W_soft": Case("per_step", "soft_2_per_lane_stage_W", seed=707, reason=_NO),
    "stage_W_10_slots": Case("per_step", "hard_10_per_lane_N43_stage_W", seed=732, reason=_NO),
    "stage_W_irk": Case("per_step", "hard_5_per_lane_stage_W", irk=1, seed=701, reason=_NO),
    "stage_W_dyn": Case("per_step", "hard_5_per_lane_stage_W", model="fdyn6u", plant=2, seed=701, reason=_NO),
    # path_class 2: no k_steps has the lateral-acceleration row
    "alat_row": Case("per_step", "alat_hard", seed=700, reason=_NO),
    # set 5 is all-hard, and is not in set 3: ihm2mpc_run_steps_sens on an ERK_LAG handle
    "lag_soft": Case("per_step", "soft_2_per_lane", irk=2, seed=706, reason=_NO),
    "lag_sens": Case("per_step", "hard_5_per_lane", irk=2, sens=1, seed=700, reason=_NO),
    # set 3 has the kinematic model only
    "dyn_sens": Case("per_step", "hard_5_per_lane", model="fdyn6u", sens=2, plant=2, seed=700, reason=_NO),
    # select_steps: a plant with the closed-form lags rides on lane N of the loop that linearises with them, irk != 2 has none
    "lag_plant_rk4_ocp": Case("per_step", "hard_5_per_lane", M_sim=4, seed=700, opts=(("sim_integrator_type", "ERK_LAG"),), reason=_NO),
    # select_steps: qp_sweeps_inside -- the SQP loops keep the sweeps' earlier form, whose prefetch starts in front of the LDS at N = 2, 3
    # (B = 50: 150 intervals -- at 128 and fewer the per-step plant is the state-only rollout, which rounds differently from the loop's)
    "sqp_N3": Case("per_step", "ref_N3", sqp=True, seed=701, reason=_NO, B=50),
}

# Two-track variants of the cases with track rows (PATH = 1: hard, soft, one with the SENS guest, one with collocation, whose
# linearisation and plant take the track id by other ways; PATH = 2 has no k_steps and goes per step): the handle holds the two tables of
# tests/multi_track_cases.py with that module's widths, instance b on track b mod 2, B = 8 (320 intervals: no latency batch).  A sibling
# table -- CASES, FALLBACK, expected_records() and the record bookkeeping of tests/test_gpu_steps_catalogue.py do not see it;
# tests/test_gpu_multi_track.py runs it and tests/test_oracle_multi_track.py checks the oracle's first step on both tracks.
# id -> (case, the launch record run_steps must leave)
_TWO = dict(tracks=2, B=8)
TWO_TRACK = {
    "hard": (dataclasses.replace(BY_NAME["k_steps<8,0,1,1,0,0,0>"], **_TWO), "k_steps<8,0,1,1,0,0,0>"),
    "soft": (dataclasses.replace(BY_NAME["k_steps<10,4,1,1,0,0,0>"], **_TWO), "k_steps<10,4,1,1,0,0,0>"),
    "soft_sens": (dataclasses.replace(BY_NAME["k_steps<8,3,1,1,0,0,0,1>"], **_TWO), "k_steps<8,3,1,1,0,0,0,1>"),
    "soft_irk": (dataclasses.replace(BY_NAME["k_steps<10,4,1,1,0,1,0>"], **_TWO), "k_steps<10,4,1,1,0,1,0>"),
    "alat_row": (dataclasses.replace(FALLBACK["alat_row"], **_TWO), "per_step:" + _NO),
}

# Catalogue entries no handle configuration can select: name -> the line of select_steps / find_form / rebuild_slots that rules it out
UNREACHED: dict = {}

# (build, record) pairs tests/test_gpu_steps_catalogue.py must have collected: every case in the default build, the names of the sets
# 0, 1 and 3 in the ILP build (that library links the default objects of the other sets), the fallbacks with their reason
ILP_SETS = (0, 1, 3)


def expected_records():
    exp = {("default", c.name) for c in CASES} | {("ilp", c.name) for c in CASES if c.qp_set in ILP_SETS}
    return exp | {("default", "per_step:" + c.reason) for c in FALLBACK.values()}
