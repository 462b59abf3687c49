"""GPU: no result depends on device memory nobody wrote.

DevBuf::alloc zero-fills every buffer of a handle and almost every test creates a fresh handle, so a kernel that reads a workspace word
before anything wrote it sees 0.0 everywhere in the suite -- and the leftovers of the previous solve or of a neighbouring instance in a
long-lived handle.  Here every case runs on two handles of one configuration, one of them created with IHM2MPC_POISON_WORKSPACE=1 (all
workspace of doubles is NaN instead of zero, at allocation and regrowth; csrc/ihm2mpc_internal.h: WorkBuf), and then again on each handle
from the same, explicitly restored starting state (the workspace then holds the first pass's leftovers).  Everything a getter returns is
compared for equality of bits: poisoned against clean, replay against first pass.  tests/poison_cases.py has the runner and the cases;
tests/test_poison_starts.py asserts on the CPU that the oracle solves the starts used here.

Covered: every per-step QP instantiation (tests/layouts.py::TABLE at B = 5, the four-wave kernel's layouts at B = 1 and 3 as well, both
scheduler builds; the LDS classes at N = 2 and 4 and the horizons around the sweeps' ring depth), every instantiation of the persistent
loop and its fallbacks (tests/steps_cases.py), the forms of the factor sweep and the slot phases (IHM2MPC_QP_FORM, one process each), and
whatever else owns workspace: the plants with their three integrators, the Cartesian side, the track kernels, the latency linearisation
of one instance, the SQP mode's line search with the two-launch ladder, x0 sensitivities and adjoints, the warm start and the recovery of
failed instances, per-instance tuning."""
import os
import subprocess
import sys

import numpy as np
import pytest

import launch_cases as LC
import layouts as L
import poison_cases as PC
import qp_forms as QF
import steps_cases as S
from test_gpu_configs import _build
from test_gpu_qp_layouts import EXPECTED_QP

pytestmark = pytest.mark.gpu

# (build, name) of what ran on a poisoned handle: the per-step QP kernels and the persistent loops (or their fallback's reason)
QP_RECORDS = set()
STEPS_RECORDS = set()


def _solver(track, lay, B, build="default", block="0", **opts):
    """tests/test_gpu_qp_layouts.py::_solver, with solver options (tests/test_gpu_steps_catalogue.py::_solver)."""
    from ihm2_amd.solver import BatchedOcpSolver

    with _build(build), PC.environ(IHM2MPC_BLOCK_QP=block):
        s = BatchedOcpSolver(L.make_ocp(lay, **opts), B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
    arr = L.apply(s.data, lay)
    if arr["W"] is not None:
        s._push_weights()
    s._push_bounds()
    return s


def _put(s, x0, yref, yref_e):
    s.set_x0(x0); s.init_guess()
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
    return yref, yref_e


# ---- every per-step QP instantiation ----

QP_RUNS = [(cid, b) for cid in PC.QP_CASES for b in (("default", "ilp") if cid.split("-")[0] in L.TABLE else ("default",))]


@pytest.mark.parametrize("cid,build", QP_RUNS)
def test_qp_instantiation(track, cid, build):
    """Three solve() calls, each with the x0 sensitivities (mode 1 at B = 3, else 2) and the adjoint gradients behind it."""
    _, lay, B, block, seed, kernel = PC.QP_CASES[cid]
    x0, yref, yref_e = PC.qp_start(track, lay, B, seed)
    mode = 1 if B == 3 else 2

    def make():
        s = _solver(track, lay, B, build, block)
        s.set_x0_sensitivities(mode)
        return s

    def calls(s, tag):
        out = []
        for _ in range(PC.QP_SOLVES):
            s.solve_async()
            rec = s.get_launch_record()
            assert rec["qp"] == kernel, (rec["qp"], kernel)
            if tag == "poisoned":
                QP_RECORDS.add((build, rec["qp"]))
            out.append(PC.outputs(s, sens=True, adjoint=True))
        return out

    PC.run_twin(make, lambda s: _put(s, x0, yref, yref_e), calls)


# ---- every persistent loop ----

def _steps_case(name, build):
    if name.startswith("fallback:"):
        return S.FALLBACK[name[9:]]
    return S.ILP_CASES.get(name, S.BY_NAME[name]) if build == "ilp" else S.BY_NAME[name]


LOOPS = ([(c.name, "default") for c in S.CASES] + [(c.name, "ilp") for c in S.CASES if c.qp_set in S.ILP_SETS] +
         [("fallback:" + k, "default") for k in S.FALLBACK])


@pytest.mark.parametrize("name,build", LOOPS)
def test_persistent_loop(track, name, build):
    """One solve() -- it forms u0, which the plant of the next step reads: the pass then starts from nothing but the state set
    explicitly --, one step(), then run_steps of 3 steps with all histories (run_steps_sens where the case has sensitivities)."""
    case = _steps_case(name, build)
    lay = S.LAYOUTS[case.layout]
    x0, yref, yref_e = S.start(track, case)
    tgt = S.s_target(lay)
    expect = case.name if case.name != "per_step" else "per_step:" + case.reason
    rti = not case.sqp

    def make():
        s = _solver(track, lay, case.B, build, "0", **case.ocp_opts())
        s.set_lap_wrap(True)
        if case.sens:
            s.set_x0_sensitivities(case.sens)
        return s

    def calls(s, tag):
        sens = bool(case.sens)
        out = []
        s.solve_async()
        out.append(PC.outputs(s, sqp=case.sqp, sens=sens, adjoint=sens and rti and case.model == "fkin6" and case.irk != 2))
        s.step(tgt, model=case.plant, M_sim=case.M_sim)
        out.append(PC.outputs(s, sqp=case.sqp, sens=sens))
        h = s.run_steps(tgt, 3, model=case.plant, M_sim=case.M_sim, freeze=False, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True,
                        sens_u0_hist=True if sens else None)
        rec = s.get_launch_record()
        got = rec["steps"] if rec["steps"] != "per_step" else "per_step:" + str(rec["steps_fallback"])
        assert got == expect, (got, expect)
        if rec["steps"] != "per_step":
            assert (rec["steps_form"], rec["steps_slots"]) == case.form, rec
        if tag == "poisoned":
            STEPS_RECORDS.add((build, got))
        out.append({"hist_" + k: v for k, v in h.items()})
        out.append(PC.outputs(s, sqp=case.sqp, sens=sens))
        return out

    PC.run_twin(make, lambda s: _put(s, x0, yref, yref_e), calls, accepted=case.accepted)


# ---- the forms of the factor sweep and the slot phases: IHM2MPC_QP_FORM is read once per process ----

@pytest.mark.parametrize("form", list(QF.NAMES))
def test_qp_forms(form):
    """The reference layout at N = 40 (poison_child.py: three solves, a step and a persistent run on a poisoned and a clean handle)."""
    env = QF.environ(QF.NAMES[form])           # (IHM2MPC_POISON_WORKSPACE, if the caller narrows it to a list of buffers, goes through)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "poison_child.py")
    r = subprocess.run([sys.executable, child, form], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "forms ok" in r.stdout, r.stdout[-2000:]


# ---- everything else that owns workspace ----

MISC = PC.MISC_LAYOUT
RADAU = dict(sim_integrator_type="IRK", sim_collocation_type="GAUSS_RADAU_IIA")
PLANT_INTEG = {"RK4": {}, "RADAU": RADAU, "ERK_LAG": dict(sim_integrator_type="ERK_LAG")}


def _misc_start(track, B=PC.MISC_B):
    return PC.qp_start(track, MISC, B, PC.MISC_SEED)


@pytest.mark.parametrize("integ", list(PLANT_INTEG))
def test_plants_and_integrators(track, integ):
    """sim_step and sim_advance of every plant (0, 1, 2, the speed switches -1, -2; the closed-form lags exist for the kinematic plant
    only), after one solve that forms the control."""
    B = PC.MISC_B
    x0, yref, yref_e = _misc_start(track)
    plants = (0,) if integ == "ERK_LAG" else (0, 1, 2, -1, -2)
    M_sim = {"RK4": 20, "RADAU": 10, "ERK_LAG": 4}[integ]         # (RK4 is stable on the actuator lags from 18 sub-steps)
    rng = np.random.default_rng(5)
    u = np.stack([rng.uniform(-300, 300, B), rng.uniform(-0.3, 0.3, B)], 1)

    def calls(s, tag):
        s.solve_async()
        out = [PC.outputs(s)]
        for model in plants:
            out.append(dict(model=np.int64(model), sim_step=s.sim_step(x0, u, model=model, M_sim=M_sim)))
            s.sim_advance(model=model, M_sim=M_sim)
            out.append(dict(x0_advanced=s.get_x0()))
        return out

    PC.run_twin(lambda: _solver(track, MISC, B, **PLANT_INTEG[integ]), lambda s: _put(s, x0, yref, yref_e), calls)


@pytest.mark.parametrize("integ", ["RK4", "RADAU"])
def test_fdyn10_plant(track, integ):
    B = PC.MISC_B
    from test_oracle_dyn10 import _states

    x, u = _states(track, B, seed=4)
    Ms = (100, 60) if integ == "RK4" else (20, 10)

    def calls(s, tag):
        return [dict(xn=s.sim_step_dyn10(x, u, M_sim=M)) for M in Ms]

    PC.run_twin(lambda: _solver(track, MISC, B, **PLANT_INTEG[integ]), lambda s: None, calls, share=None)


def _fit_tracks_padded(s, center_lines):
    """ihm2mpc_fit_tracks as the C ABI returns it: (ntracks, max_pts, 4) twice, the host arrays filled with a sentinel first."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import _ptr

    npts = np.array([len(c) for c in center_lines], dtype=np.int32)
    mx = int(npts.max())
    xy = np.zeros((len(center_lines), mx, 2))
    for t, c in enumerate(center_lines):
        xy[t, :npts[t]] = np.asarray(c, dtype=np.float64)
    cX = np.full((len(center_lines), mx, 4), 7.0); cY = np.full((len(center_lines), mx, 4), 7.0)
    _lib.check(s.lib.ihm2mpc_fit_tracks(s._h, mx, npts.ctypes.data_as(_lib.c_int32_p), _ptr(xy), 2.0, _ptr(cX), _ptr(cY)))
    return npts, cX, cY


def test_cartesian_side_and_tracks(track):
    """sim_step_cart, project, sim_advance_cart on two tracks; build_tracks and fit_tracks on two tracks of different lengths.  The
    coefficients fit_tracks returns past a shorter track's points are 0 (include/ihm2mpc.h), on both handles."""
    from ihm2_amd import track as T
    from ihm2_amd.closed_loop_sim import frenet_to_cartesian
    from ihm2_amd.solver import BatchedOcpSolver

    B = PC.MISC_B
    plans = [T.track_table(n) for n in PC.TWO_TRACKS]
    geos = [T.load_track_geometry_data(n) for n in PC.TWO_TRACKS]
    assert len(geos[0].center_line) != len(geos[1].center_line)
    tid, xf, yref, yref_e = PC.two_track_start(plans)
    xc = np.zeros((B, 8))
    for t, p in enumerate(plans):
        xc[tid == t] = frenet_to_cartesian(p, xf[tid == t])
    rng = np.random.default_rng(6)
    u = np.stack([rng.uniform(-300, 300, B), rng.uniform(-0.3, 0.3, B)], 1)

    def make():
        s = BatchedOcpSolver(L.make_ocp(MISC), B, np.stack([p.s_ref for p in plans]), np.stack([p.kappa_ref for p in plans]), track_id=tid)
        L.apply(s.data, MISC); s._push_bounds()
        return s

    def tables(s):          # state the calls overwrite (build_tracks, sim_advance_cart): set again before the replay
        s.set_tracks(np.stack([p.s_ref for p in plans]), np.stack([p.kappa_ref for p in plans]))
        s.set_track_geometry(np.stack([p.X_ref for p in plans]), np.stack([p.Y_ref for p in plans]), np.stack([p.phi_ref for p in plans]))
        s.set_cart_state(xc, xf[:, 0].copy())

    def start(s):
        tables(s)
        return _put(s, xf, yref, yref_e)

    def calls(s, tag):
        out = []
        for model in (3, 4, -3):
            out.append(dict(cart=s.sim_step_cart(xc, u, model=model, n_steps=2)))
        got, sg = s.project(xc, xf[:, 0] + 0.3)
        out.append(dict(frenet=got, s_guess=sg))
        s.solve_async()
        out.append(PC.outputs(s))
        s.sim_advance_cart()
        xcn, sgn = s.get_cart_state()
        out.append(dict(x_cart=xcn, s_guess=sgn, x0=s.get_x0()))
        npts, cX, cY = _fit_tracks_padded(s, [g.center_line for g in geos])
        for t in range(2):      # the defined value of the rows no track point stands behind
            assert npts[t] == npts.max() or ((cX[t, npts[t]:] == 0.0).all() and (cY[t, npts[t]:] == 0.0).all()), (tag, t)
        assert npts.min() < npts.max() and np.isfinite(cX).all() and np.isfinite(cY).all()
        out.append(dict(cX=cX, cY=cY))
        s.build_tracks([cX[t, :npts[t]] for t in range(2)], [cY[t, :npts[t]] for t in range(2)])
        out.append(dict(zip(("s_ref", "kappa_ref", "X_ref", "Y_ref", "phi_ref"), s.get_tracks())))
        return out

    PC.run_twin(make, start, calls, restore=tables)


def test_single_instance_control(track):
    """compute_control at B = 1: the latency linearisation, one sensitivity column per wavefront (k_linearize_cols)."""
    x0, yref, yref_e = _misc_start(track, 1)

    def calls(s, tag):
        out = []
        xc = x0.copy()
        for _ in range(3):
            u0, st = s.compute_control(xc, 40.0)
            assert s.get_launch_record()["linearize"] == LC.names(s)[0] == "k_linearize_cols"
            out.append(dict(PC.outputs(s), u0_returned=u0, status_returned=st))
            xc = s.sim_step(xc, u0, model=0, M_sim=20)
        return out

    PC.run_twin(lambda: _solver(track, MISC, 1, block="1"), lambda s: _put(s, x0, yref, yref_e), calls)


def test_sqp_line_search_with_the_two_launch_ladder(track):
    """The per-step SQP solve with the collocation integrator and alpha_reduction = 0.9: 29 trial step lengths.  At B = 16 (29 x 16 x 40 >
    16384 trial intervals) api.hip::sqp_iterations rolls out the first three for everybody, and the rest only for the instances the first
    line-search launch leaves pending -- the rows of ls_phi of the others stay unwritten past the third length."""
    B = PC.SQP_B
    x0, yref, yref_e = PC.qp_start(track, MISC, B, PC.SQP_SEED)
    opts = dict(integrator_type="IRK", sim_method_num_steps=1, **S.LIVE)
    assert 29 * B * MISC.N > 16384

    def make():
        s = _solver(track, MISC, B, **opts)
        s.set_sqp_options(alpha_reduction=PC.SQP_ALPHA_RED)
        return s

    def start(s):
        _put(s, x0, yref, yref_e)
        s.set_u(PC.perturb_steering(s.get_u()))
        return yref, yref_e

    def calls(s, tag):
        out = []
        for _ in range(2):
            s.solve_async()
            out.append(PC.outputs(s, sqp=True))
        return out

    first = PC.run_twin(make, start, calls, accepted=(0, 2))
    ok = [np.isin(o["status"], (0, 2)) for o in first]
    deep = sum(int((o["alpha"][m] < PC.SQP_DEEP).sum()) for o, m in zip(first, ok))
    early = sum(int((o["alpha"][m] >= PC.SQP_DEEP).sum()) for o, m in zip(first, ok))
    print(f"step lengths past the third rung: {deep}, within it: {early}")
    assert deep >= 1, "no step length past the third rung: the second pair of launches settled nothing"
    assert early >= 1, "every instance went past the third rung: no row of ls_phi stayed unwritten beside the masked rollout"


@pytest.mark.parametrize("mode", [1, 2])
def test_sensitivities_and_adjoints_after_a_solve(track, mode):
    """set_x0_sensitivities(1 | 2) AFTER a first solve (the buffers are allocated between two solves), then the adjoint calls with given
    seeds, with a NULL seed and with the unit seeds on u_0."""
    B = PC.MISC_B
    x0, yref, yref_e = _misc_start(track)

    def calls(s, tag):
        s.set_x0_sensitivities(0)
        s.solve_async()
        out = [PC.outputs(s)]
        s.set_x0_sensitivities(mode)
        s.solve_async()
        out.append(PC.outputs(s, sens=True, adjoint=True))
        sx, su = PC.adjoint_seeds(B, s.N, S=5)          # more seeds than before: the adjoint buffers regrow
        out.append(s.eval_adjoint_weight_sensitivities(sx, su))
        out.append(s.eval_adjoint_sensitivities(None, su))
        return out

    PC.run_twin(lambda: _solver(track, MISC, B), lambda s: _put(s, x0, yref, yref_e), calls)


def test_guess_and_recovery(track):
    """init_guess; reinit_failed after one instance was failed by a NaN in its yref (status 1, no fault), then a solve of all."""
    B = PC.MISC_B
    x0, yref, yref_e = _misc_start(track)
    bad = yref.copy(); bad[3, 5, 1] = np.nan

    def calls(s, tag):
        out = []
        s.init_guess()
        out.append(PC.iterate(s))
        s.solve_async()
        out.append(PC.outputs(s))
        s.set_yref(bad)
        st = s.solve()
        assert st[3] == 1 and (np.delete(st, 3) == 0).all(), st
        out.append(PC.outputs(s))
        s.reinit_failed()
        out.append(PC.iterate(s))
        s.set_yref(yref)
        s.solve_async()
        out.append(PC.outputs(s))
        return out

    PC.run_twin(lambda: _solver(track, MISC, B), lambda s: _put(s, x0, yref, yref_e), calls)


def test_instance_tuning(track):
    """Per-instance weights and bounds on soft_one_sided_rows_padding (split soft rows, one-sided entries, padding)."""
    from ihm2_amd import ocp as O

    lay, B = L.TABLE[PC.TUNING_LAYOUT][0], PC.MISC_B
    x0, yref, yref_e = PC.qp_start(track, lay, B, 900 + lay.seed)
    var = [PC.tuning_bounds(lay, b) for b in range(B)]
    per = {n: np.stack([v[n] for v in var]) for n in var[0]}
    W0, We0 = O.default_weights()
    f = np.array([PC.tuning_weight_factor(b) for b in range(B)])
    W, We = f[:, None, None] * W0[None], f[:, None, None] * We0[None]

    def make():
        s = _solver(track, lay, B)
        s.set_instance_weights(W, We)
        s.set_instance_bounds(**per)
        return s

    def calls(s, tag):
        out = []
        for _ in range(2):
            s.solve_async()
            assert s.get_launch_record()["qp"].startswith("k_qp_wave<8,2,0,")
            out.append(PC.outputs(s))
        return out

    PC.run_twin(make, lambda s: _put(s, x0, yref, yref_e), calls)


def test_every_instantiation_ran_on_a_poisoned_handle():
    """The module's launch records against the catalogues' lists: every per-step QP kernel of tests/test_gpu_qp_layouts.py::EXPECTED_QP in
    both builds, every name of tests/steps_cases.py::expected_records()."""
    from test_gpu_configs import ILP_LIB

    builds = ("default", "ilp") if os.path.exists(ILP_LIB) else ("default",)
    expected_qp = {(b, k) for b in builds for k in EXPECTED_QP}
    assert QP_RECORDS == expected_qp, (sorted(expected_qp - QP_RECORDS), sorted(QP_RECORDS - expected_qp))
    expected_steps = {r for r in S.expected_records() if r[0] in builds}
    assert STEPS_RECORDS == expected_steps, (sorted(expected_steps - STEPS_RECORDS), sorted(STEPS_RECORDS - expected_steps))
