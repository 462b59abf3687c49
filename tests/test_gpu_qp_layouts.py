"""Every instantiation of the QP kernels on constraint layouts built for them (tests/layouts.py), in both scheduler builds.

Which instantiation runs is decided by the slot table api.hip::rebuild_slots lays out from the rows (csrc/qp_tables.hpp: lay_out_slots --
slots per lane, leading one-sided entries per lane; tests/test_slot_table.py checks the tables themselves without a GPU) and by the
catalogue of instantiations it is selected from (csrc/qp_catalogue.hpp: the lists of the sets 0 .. 6).  Each layout below is
named for the table it is meant to give; the launch record (BatchedOcpSolver.get_launch_record) says what actually ran, and the last test checks
that the module as a whole launched exactly the list of instantiations written there.

Per solvable layout, over 3 RTI iterations from sample_x0:
* GPU against the oracle: statuses, iteration counts, x / u, pi / lam and the soft slacks;
* the GPU's own step (x - x_lin, u - u_lin, pi, lam, slacks) against an independent KKT check of the numpy-assembled QP
  (layouts.assemble_qp; the two track rows and the a_lat row are nonlinear and taken from OracleProblem.build_qp), with the
  multipliers of absent sides exactly 0;
* the persistent loop (run_steps) against launches per step (step()), bit for bit, where it has a k_steps instantiation and where it
  falls back.
Plus per-instance bounds on unusual packings and the refusals of tables past a limit."""
import contextlib
import os

import numpy as np
import pytest
from conftest import sample_x0

import drive
import launch_cases as LC
import layouts as L

pytestmark = pytest.mark.gpu

# (build, instantiation) of everything the module launched
RECORDS = set()

Lay = L.Layout
TABLE, REFUSED = L.TABLE, L.REFUSED       # the layouts and the tables they are named for: tests/layouts.py

EXPECTED_QP = {
    "k_qp_wave<5,0,0,0>", "k_qp_wave<5,0,0,1>", "k_qp_wave<8,0,0,0>", "k_qp_wave<8,0,0,1>", "k_qp_wave<10,0,0,0>", "k_qp_wave<10,0,0,1>",
    "k_qp_wave<8,2,0,0>", "k_qp_wave<8,2,0,1>", "k_qp_wave<10,4,0,0>", "k_qp_wave<10,4,0,1>",
    "k_qp_wave<8,0,1,0>", "k_qp_wave<8,0,1,1>", "k_qp_wave<8,3,1,0>", "k_qp_wave<8,3,1,1>", "k_qp_wave<10,4,1,0>", "k_qp_wave<10,4,1,1>",
    "k_qp_wave<8,0,2,1>", "k_qp_wave<10,4,2,1>",
    "k_qp_block<2,0,4>", "k_qp_block<2,1,4>",
}
# the persistent loop of the kinematic RTI / ERK configuration (NSLOT, NSOFT, PATH, UNI, SQP = IRK = DYN = 0), and its fallback
EXPECTED_STEPS = {
    "k_steps<5,0,0,0,0,0,0>", "k_steps<5,0,0,1,0,0,0>", "k_steps<8,0,0,0,0,0,0>", "k_steps<8,0,0,1,0,0,0>", "k_steps<10,0,0,1,0,0,0>",
    "k_steps<8,2,0,1,0,0,0>", "k_steps<10,4,0,1,0,0,0>", "k_steps<8,0,1,1,0,0,0>", "k_steps<8,3,1,1,0,0,0>", "k_steps<10,4,1,1,0,0,0>",
    "per_step:no_instantiation",
}


def _build(which):
    from test_gpu_configs import _build as b

    return b(which)


@contextlib.contextmanager
def _block_qp(mode):
    saved = os.environ.get("IHM2MPC_BLOCK_QP")
    os.environ["IHM2MPC_BLOCK_QP"] = mode           # read when a handle is created
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("IHM2MPC_BLOCK_QP", None)
        else:
            os.environ["IHM2MPC_BLOCK_QP"] = saved


def _solver(track, lay, B, build, block="1"):
    from ihm2_amd.solver import BatchedOcpSolver

    with _build(build), _block_qp(block):
        s = BatchedOcpSolver(L.make_ocp(lay), B, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
    arr = L.apply(s.data, lay)
    if arr["W"] is not None:
        s._push_weights()
    s._push_bounds()
    return s


def _start(s, track, B, seed):
    x0 = drive.clipped_start(track, B, seed)
    s.set_x0(x0); s.init_guess()
    N = s.N
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + 40.0 * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = x0[:, 0] + 40.0
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
    return x0, yref, yref_e


def _note(build, rec):
    if rec["qp"] is not None:
        RECORDS.add((build, rec["qp"]))


def _widen(a28, a2):
    return np.concatenate([a28[..., :L.NC], a2[..., :1], a28[..., L.NC:], a2[..., 1:]], -1)


def _kkt_subset(ok, B):
    idx = np.flatnonzero(ok)
    return np.unique(np.concatenate([idx[:12], idx[-4:]])) if idx.size else idx       # the first instances and the ragged last wave's


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("name", list(TABLE))
def test_layout_matches_oracle_and_kkt(track, name, build):
    from oracle import oracle as orc

    lay, B, block = TABLE[name]
    s = _solver(track, lay, B, build, block)
    data = s.data
    P = orc.OracleProblem(data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    x0, yref, yref_e = _start(s, track, B, 900 + lay.seed)
    nc = 15 if lay.alat else L.NC
    z, Z = L.soft_arrays(data, nc, (data.alat_soft_z, data.alat_soft_Z) if lay.alat and data.alat_soft_Z is not None else None)
    tol = data.ipm_tol
    x, u = s.get_x(), s.get_u()            # the oracle's iterate
    pi = lam = None
    solved = 0
    # (the empty table: one Newton step from the guess -- nothing bounds the iterates of an unconstrained OCP after it)
    for it in range(1 if name == "empty_table" else 3):
        xg_lin, ug_lin = s.get_x(), s.get_u()
        st = s.solve()
        rec = s.get_launch_record()
        _note(build, rec)
        out = P.rti_step(x, u, x0, yref, yref_e, pi=pi, lam=lam)
        pi, lam = out["pi"], out["lam"]
        np.testing.assert_array_equal(st, out["status"])
        ok = st == 0
        solved = max(solved, int(ok.sum()))
        itg = s.get_qp_iter()
        if ok.any():
            same = itg[ok] == out["qp_iter"][ok]
            assert same.mean() >= 0.999 and np.abs(itg[ok] - out["qp_iter"][ok]).max() <= 1       # (one marginal test may tip, as in test_both_builds_agree_on_4096_instances)
        eq = ok & (itg == out["qp_iter"])
        xg, ug = s.get_x(), s.get_u()
        pig, lamg = s.get_multipliers()
        slg = s.get_slacks()
        if lay.alat:
            lam_a, slk_a = s.get_alat_multipliers()
            lamg, slg = _widen(lamg, lam_a), _widen(slg, slk_a)
        if eq.any():
            assert np.max(np.abs(xg[eq] - x[eq]) / (1 + np.abs(x[eq]))) < 1e-7
            assert np.max(np.abs(ug[eq] - u[eq]) / (1 + np.abs(u[eq]))) < 1e-7
            sp = max(1.0, float(np.abs(pi[eq][:, 1:]).max())); sl_ = max(1.0, float(np.abs(lam[eq]).max()))
            assert np.abs(pig[eq][:, 1:] - pi[eq][:, 1:]).max() <= 1e-6 * sp          # (pi_0 is not defined: x_0 is eliminated)
            assert np.abs(lamg[eq] - lam[eq]).max() <= 1e-6 * sl_
        # independent KKT of the GPU's own step, and its slacks against the oracle QP's, where the QP reports convergence (status 0 also
        # takes a QP stopped loosely converged at its iteration limit, as acados' RTI does)
        conv = ok & np.all(s.get_qp_residuals() <= tol, axis=1)
        assert conv.sum() >= 0.5 * ok.sum()
        sub = _kkt_subset(conv, B)
        if sub.size:
            A, Bm, b = P.linearize(np.ascontiguousarray(xg_lin[sub]), np.ascontiguousarray(ug_lin[sub]))
        for j, i in enumerate(sub):
            ref = P.build_qp(xg_lin[i], ug_lin[i], x0[i], yref[i], yref_e[i])
            qp = L.assemble_qp(data, xg_lin[i], ug_lin[i], x0[i], yref[i], yref_e[i], A[j], Bm[j], b[j], nonlinear=ref if lay.path else None)
            dz = np.zeros((s.N + 1, L.NZ)); dz[:, :8] = xg[i] - xg_lin[i]; dz[:s.N, 8:] = ug[i] - ug_lin[i]
            r = L.kkt_report(qp, dz, pig[i], lamg[i], slg[i], z, Z)
            sg, sb = L.scales(qp)
            assert r["absent"] == 0.0, (i, r)
            # (complementarity against R z - dl itself: the interior point's own slack t meets R z - dl - t to tol * sb, which a multiplier
            # lam carries into lam (R z - dl) as lam * tol * sb;
            # and the slack's stationarity z + Z s - lam - lam_s = rs, |rs| <= tol * sg, into (z + Z s - lam) s as s * tol * sg)
            comp_tol = 1.01 * tol * (sg + float(np.abs(lamg[i]).max()) * sb + float(np.abs(slg[i]).max()) * sg)
            assert r["stat"] <= 1.01 * tol * sg and r["comp"] <= comp_tol and r["dual"] <= 1.01 * tol * sg, (i, r, sg, comp_tol)
            assert r["eq"] <= 1.01 * tol * sb and r["ineq"] <= 1.01 * tol * sb and r["lam_min"] >= 0.0, (i, r, sb)
            if data.soft_Z is not None or lay.alat_soft:
                sol = orc.qp_solve(**ref, iter_max=data.ipm_iter_max, tol=tol, mu0=data.ipm_mu0, tau0=data.ipm_tau0, soft_z=z, soft_Z=Z) \
                    if not lay.alat else None
                if sol is not None and sol["iters"] == itg[i]:
                    assert np.max(np.abs(slg[i] - sol["sl"]) / (1 + np.abs(sol["sl"]))) < 1e-7
            if lay.name == "empty_table":
                assert itg[i] == 1 and r["stat"] < 1e-10
    assert solved >= 0.6 * B, (name, solved)
    s.free()


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("name", list(TABLE))
def test_persistent_loop_equals_step_by_step_on_layout(track, name, build):
    lay, B, _ = TABLE[name]
    steps = 3
    res = []
    for persistent in (False, True):
        s = _solver(track, lay, B, build, "0")
        s.set_lap_wrap(True)
        _start(s, track, B, 700 + lay.seed)
        s.step(40.0, model=0, M_sim=25)
        _note(build, s.get_launch_record())
        if persistent:
            h = s.run_steps(40.0, steps, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
            rec = s.get_launch_record()
            RECORDS.add((build, rec["steps"] if rec["steps"] != "per_step" else "per_step:" + rec["steps_fallback"]))
            assert rec["steps"] is not None
        else:
            h = drive.per_step(s, 40.0, steps, model=0, M_sim=25)
        res.append((h, s.get_x(), s.get_u(), s.get_multipliers(), s.get_slacks()))
        s.free()
    (ha, xa, ua, ma, sa), (hb, xb, ub, mb, sb) = res
    np.testing.assert_array_equal(ha["status"], hb["status"]); np.testing.assert_array_equal(ha["qp_iter"], hb["qp_iter"])
    if LC.latency_batch(B, lay.N):
        # KNOWN DIFFERENCE: on a latency batch ihm2mpc_step's kinematic plant is the state-only rollout (kernels_linearize.hip::ihm2_launch_sim,
        # k_sim_step), whose RK4 rounds differently from the persistent loop's plant (the shooting intervals' integrator): x0 differs in
        # the last bit (seen: 6 of 24 entries, 5.6e-17), the interior point carries that into lam at 2e-11 relative
        for a, b, k in [(ha["x0"], hb["x0"], "x0"), (ha["u0"], hb["u0"], "u0"), (xa, xb, "x"), (ua, ub, "u"), (ma[1], mb[1], "lam"), (sa, sb, "slk")]:
            assert np.max(np.abs(a - b) / (1 + np.abs(b))) < 1e-9, k
        return
    for k in ("x0", "u0"):
        np.testing.assert_array_equal(ha[k], hb[k], err_msg=k)
    np.testing.assert_array_equal(xa, xb); np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(ma[0], mb[0]); np.testing.assert_array_equal(ma[1], mb[1]); np.testing.assert_array_equal(sa, sb)
    if name != "empty_table":           # (nothing bounds an unconstrained closed loop: only the equality is asked of it)
        assert (ha["status"][-1] == 0).mean() > 0.5


def _variant(arr, f):
    """The layout's bounds with every finite value scaled by f (the pattern of finite sides stays)."""
    out = {}
    for n in ("lbx", "ubx", "lbu", "ubu", "lg", "ug"):
        a = arr[n].copy()
        fin = np.abs(a) < L.BIG
        a[fin] *= f
        out[n] = a
    return out


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("name", ["soft_2_per_lane_split_rows", "soft_one_sided_rows_padding", "path_soft_4_per_lane", "hard_random_one_sided"])
def test_instance_bounds_on_layout_equal_homogeneous_handles(track, name, build):
    """Per-instance bounds scattered into the packed pattern (split soft rows, leading one-sided entries, padding): instance b of a mixed
    batch gives what a handle whose shared bounds are b's gives, bit for bit."""
    lay, B, _ = TABLE[name]
    B = 40
    facs = (1.0, 0.9, 0.8)
    assign = np.arange(B) % len(facs)
    arr = L.make_arrays(lay)
    var = [_variant(arr, f) for f in facs]

    def run(s, x0):
        s.set_x0(x0); s.init_guess()
        out = []
        for _ in range(3):
            s.prepare_step(40.0)
            st = s.solve()
            _note(build, s.get_launch_record())
            pi, lam = s.get_multipliers()
            out.append(dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), status=st, qp_iter=s.get_qp_iter()))
        return out

    x0 = drive.clipped_start(track, B, 4242)
    s = _solver(track, lay, B, build, "0")
    per = {n: np.stack([var[assign[b]][n] for b in range(B)]) for n in var[0]}
    s.set_instance_bounds(**per)
    mixed = run(s, x0)
    s.free()
    for j in range(len(facs)):
        rows = np.flatnonzero(assign == j)
        h = _solver(track, lay, rows.size, build, "0")
        for n, a in var[j].items():
            setattr(h.data, n, a)
        h._push_bounds()
        homo = run(h, x0[rows])
        h.free()
        for m, hh in zip(mixed, homo):
            for k in m:
                np.testing.assert_array_equal(m[k][rows], hh[k], err_msg=k)
    assert (mixed[-1]["status"] == 0).mean() > 0.5


@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("name", list(REFUSED))
def test_layout_past_a_limit_is_refused_and_the_handle_recovers(track, name, build):
    from ihm2_amd._lib import Ihm2mpcError

    lay = REFUSED[name]
    B = 70
    s = _solver(track, lay, B, build, "0")
    before = s.get_launch_record()
    x0 = sample_x0(track, B, seed=55)
    s.set_x0(x0)
    with pytest.raises(Ihm2mpcError, match="the constraint rows fit no QP kernel"):
        s.init_guess()
    with pytest.raises(Ihm2mpcError, match="the constraint rows fit no QP kernel"):
        s.solve()
    assert s.get_launch_record() == before            # nothing was launched
    assert np.all(np.isfinite(s.get_x())) and np.all(np.isfinite(s.get_u()))
    # a fitting layout on the same handle: solves, and gives what a fresh handle gives
    fit = L.Layout("fit", N=lay.N, seed=lay.seed, path=lay.path, alat=lay.alat, alat_max=lay.alat_max)       # the handle keeps its track rows
    L.apply(s.data, fit)
    s._push_bounds()
    fresh = _solver(track, fit, B, build, "0")
    out = []
    for h in (s, fresh):
        _start(h, track, B, 56)
        st = h.solve()
        _note(build, h.get_launch_record())
        out.append((st, h.get_x(), h.get_u(), h.get_multipliers()[1]))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)
    assert (out[0][0] == 0).mean() > 0.8
    s.free(); fresh.free()


# The LDS classes of the QP (csrc/qp_lds.hpp: rows per stage, track-row slopes, a_lat row, batch-shared H / [C D] kept in LDS) at the two shortest
# horizons the sweeps treat differently: N = 2 is under every ring depth, N = 4 the first the sweeps' earlier form stays inside the block with.
# The fourth class, all sides hard with batch-shared weights, is test_gpu_factor_sweep_forms.py::test_horizons_around_the_ring_depth[2] and [4].
# class -> (layout, kernel, sample_x0 seed per horizon: those of tools/find_factor_sweep_seeds.py, 4 for N = 2 and 1 for N = 4; with the a_lat row the
# seed 1 leaves two of the eight QPs at N = 4 infeasible in the oracle as well, the seed 4 none)
SHORT = {
    "hard_stage_W": (dict(stage_W=True, seed=21), "k_qp_wave<5,0,0,0>", {2: 4, 4: 1}),
    "path_hard": (dict(path=True), "k_qp_wave<8,0,1,1>", {2: 4, 4: 1}),
    "alat_hard": (dict(path=True, alat=True, alat_max=4.5), "k_qp_wave<8,0,2,1>", {2: 4, 4: 4}),
}


@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("cls", list(SHORT))
def test_lds_class_at_the_shortest_horizons(track, cls, N):
    """One RTI step of 8 instances against the oracle, to the tolerances of test_layout_matches_oracle_and_kkt."""
    from oracle import oracle as orc

    kw, kernel, seeds = SHORT[cls]
    lay, B = Lay(f"short_{cls}", N=N, **kw), 8
    s = _solver(track, lay, B, "default", "0")
    P = orc.OracleProblem(s.data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay)))
    x0, yref, yref_e = _start(s, track, B, seeds[N])
    x, u = s.get_x(), s.get_u()
    st = s.solve()
    assert s.get_launch_record()["qp"] == kernel
    out = P.rti_step(x, u, x0, yref, yref_e)
    np.testing.assert_array_equal(st, out["status"])
    np.testing.assert_array_equal(s.get_qp_iter(), out["qp_iter"])
    ok = st == 0
    assert ok.sum() >= 0.6 * B, st
    xg, ug = s.get_x(), s.get_u()
    pig, lamg = s.get_multipliers()
    if lay.alat:
        lamg = _widen(lamg, s.get_alat_multipliers()[0])
    pi, lam = out["pi"], out["lam"]
    ex = np.max(np.abs(xg[ok] - x[ok]) / (1 + np.abs(x[ok]))); eu = np.max(np.abs(ug[ok] - u[ok]) / (1 + np.abs(u[ok])))
    sp = max(1.0, float(np.abs(pi[ok][:, 1:]).max())); sl_ = max(1.0, float(np.abs(lam[ok]).max()))
    epi = np.abs(pig[ok][:, 1:] - pi[ok][:, 1:]).max() / sp; elam = np.abs(lamg[ok] - lam[ok]).max() / sl_
    print(f"{cls} N={N}: x {ex:.2e} u {eu:.2e} pi {epi:.2e} lam {elam:.2e}, status {st.tolist()}, qp_iter {out['qp_iter'].tolist()}")
    assert ex < 1e-7 and eu < 1e-7 and epi <= 1e-6 and elam <= 1e-6
    s.free()


def test_every_instantiation_was_launched_in_both_builds():
    """The records of this module against the explicit list: adding or removing an instantiation (or moving a layout to another one)
    must touch this list."""
    expected = {(b, k) for b in ("default", "ilp") for k in EXPECTED_QP | EXPECTED_STEPS}
    assert RECORDS == expected, (sorted(expected - RECORDS), sorted(RECORDS - expected))
