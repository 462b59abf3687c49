"""csrc/kernels_cart.hip against the oracle at the edge states of tests/cart_edge_states.py: the Cartesian plants (k_sim_cart: kin6,
dyn6, the speed switch and the "no reversing" clamp, one and five plant steps, two switch speeds), the projection (k_project: window
clamps at both table ends, the wrap inside the window, one-knot and whole-table windows, the lap seams, headings across +-pi, two
different tracks in one batch), the device-resident ROS step (set_cart_state / sim_advance_cart / get_cart_state, in place, against the
host path bit for bit), the 15-state plant (k_sim_dyn10 and the Radau IIA plant) and the isolation of non-finite instances.
tests/test_oracle_cart_edge_states.py certifies the oracle at these inputs on the CPU; the tolerances are the project's own, stored
with each entry, and every entry of every table is compared."""
import ctypes

import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import cart_edge_states as CE
import edge_states as E
from test_oracle_cart_edge_states import MARGIN, PLANTS, TRACKS, _plant_steps, dyn10_step, plant_decisions

pytestmark = pytest.mark.gpu

PLANT_CASES = [(p, c) for p in PLANTS for c in CE.PLANT_CONFIGS if c != "VDYN_5" or p == "ros"]


def _solver(B, tracks, track_id=None, geometry=True, **opts):
    from ihm2_amd.solver import BatchedOcpSolver

    tabs = [np.stack([getattr(t, a) for t in tracks]) for a in ("s_ref", "kappa_ref", "X_ref", "Y_ref", "phi_ref")]
    s = BatchedOcpSolver(make_ocp(**opts), B, tabs[0], tabs[1], track_id=track_id)
    if geometry:
        s.set_track_geometry(*tabs[2:])
    return s


@pytest.fixture(scope="module")
def tracks():
    from ihm2_amd.track import track_table

    return [track_table(t) for t in TRACKS]


@pytest.fixture(scope="module")
def plant_entries():
    return CE.plant_table()


@pytest.fixture(scope="module")
def proj_entries(tracks):
    return [CE.projection_table(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref) for t in tracks]


@pytest.fixture(scope="module")
def dyn10_entries(track):
    return CE.dyn10_table(E.table(track.s_ref, track.kappa_ref))


@pytest.fixture(scope="module")
def plant_solver(tracks, plant_entries):
    s = _solver(len(plant_entries), tracks[:1])
    yield s
    s.free()


@pytest.fixture(scope="module")
def one_solver(tracks):
    s = _solver(1, tracks[:1])
    yield s
    s.free()


def _sim_cart(s, x, u, plant, config, n_steps=None):
    M, dt, n, v_dyn = CE.PLANT_CONFIGS[config]
    return s.sim_step_cart(x, u, model=PLANTS[plant], M_sim=M, dt_sim=dt, n_steps=n if n_steps is None else n_steps, v_dyn=v_dyn)


# ---- 1. k_sim_cart ----
@pytest.mark.parametrize("plant,config", PLANT_CASES)
def test_cartesian_plant_matches_oracle_at_edge_states(plant_solver, plant_entries, plant, config):
    """The table itself as the batch (B = 85: a ragged second wave).  Under the switch (-3) the reference's decisions are asserted per
    entry on the GPU's own numbers: the result is, bit for bit, the forced plant of the model the reference chose with the clamp the
    reference applied -- exact zeros --, and five steps in one call are five calls of one step."""
    s = plant_solver
    x, u = CE.plant_arrays(plant_entries)
    names = np.array([e.name for e in plant_entries])
    got = _sim_cart(s, x, u, plant, config)
    want = _plant_steps(x, u, plant, config)[-1]
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    err = (np.abs(got - want) / (1.0 + np.abs(want))).max(axis=1)
    tol = np.array([e.tolerance(plant, config) for e in plant_entries])
    w = int(np.argmax(err / tol))
    print(f"plant {plant} {config}: worst {err[w]:.2e} of {tol[w]:.1e} at {names[w]}; largest error {err.max():.2e} at {names[int(np.argmax(err))]}")
    assert np.all(err < tol), [(names[i], float(f"{err[i]:.3g}"), tol[i]) for i in np.flatnonzero(err >= tol)]
    if plant != "ros":
        return
    steps = plant_decisions(x, u, config)
    xk = x
    for k, st in enumerate(steps):
        forced = np.where(st["kin"][:, None], _sim_cart(s, xk, u, "kin6", config, n_steps=1), _sim_cart(s, xk, u, "dyn6", config, n_steps=1))
        xk = _sim_cart(s, xk, u, "ros", config, n_steps=1)
        # the clamp the reference applied, on the GPU's pre-clamp state: the same decision (the margins are certified on the CPU)
        a, b, c = forced[:, 3] < 0.0, forced[:, 3] < 0.01, forced[:, 6] <= 0.1
        np.testing.assert_array_equal(a | (b & c), st["clamped"], err_msg=f"step {k}")
        np.testing.assert_array_equal(np.stack([a, b, c], 1), st["conds"], err_msg=f"step {k}")
        forced[st["clamped"], 3:6] = 0.0
        np.testing.assert_array_equal(xk, forced, err_msg=f"step {k}: the model the reference chose, the clamp it applied")
        assert np.all(xk[st["clamped"], 3:6] == 0.0) and not np.any(np.signbit(xk[st["clamped"], 3:6]))
        assert np.all(np.any(xk[~st["clamped"], 3:6] != 0.0, axis=1))
    np.testing.assert_array_equal(xk, got, err_msg="n_steps in one call against single steps")
    first = steps[0]
    assert first["kin"].any() and (~first["kin"]).any() and first["clamped"].any() and (~first["clamped"]).any()


def test_cartesian_plant_on_a_batch_of_one(one_solver, plant_solver, plant_entries):
    """B = 1: lane 0 of a wave that is otherwise masked off returns what the entry's lane of the full batch returned."""
    x, u = CE.plant_arrays(plant_entries)
    for plant, config in (("ros", "STEPS_5"), ("dyn6", "RK4_1")):
        full = _sim_cart(plant_solver, x, u, plant, config)
        for i in range(len(plant_entries)):
            np.testing.assert_array_equal(_sim_cart(one_solver, x[i:i + 1], u[i:i + 1], plant, config)[0], full[i], err_msg=plant_entries[i].name)


# ---- 2. k_project ----
def _assert_projection(got, nxt, want, wnxt, xc, names, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)          # NaN where the reference is NaN
    np.testing.assert_array_equal(np.isnan(nxt), np.isnan(wnxt), err_msg=what)
    np.testing.assert_array_equal(got[:, 3:], xc[:, 3:], err_msg=what)                   # components 3..7 bit-equal, NaN rows included
    with np.errstate(invalid="ignore"):          # (NaN against NaN is agreement: the patterns are equal)
        err = np.maximum(np.nan_to_num(np.abs(got[:, :3] - want[:, :3])).max(axis=1), np.nan_to_num(np.abs(nxt - wnxt)))
    w = int(np.argmax(err))
    print(f"{what}: worst {err[w]:.2e} of {CE.PROJ_TOL:.1e} at {names[w]}; NaN rows {int(np.isnan(got).any(axis=1).sum())}")
    assert np.all(err < CE.PROJ_TOL), [(names[i], float(f"{err[i]:.3g}")) for i in np.flatnonzero(err >= CE.PROJ_TOL)]


@pytest.mark.parametrize("s_tol", CE.S_TOLS)
def test_projection_matches_oracle_at_edge_states(tracks, proj_entries, one_solver, s_tol):
    from oracle import oracle as orc

    t, entries = tracks[0], proj_entries[0]
    B = len(entries)
    names = [e.name for e in entries]
    xc, sg = CE.projection_arrays(entries)
    s = _solver(B, tracks[:1])
    got, nxt = s.project(xc, sg, s_tol=s_tol)
    s.free()
    want, wnxt = orc.cart_to_frenet(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, xc, sg, s_tol=s_tol)
    assert np.isnan(want).any() and np.isfinite(want).all(axis=1).sum() >= B - 6
    _assert_projection(got, nxt, want, wnxt, xc, names, f"projection s_tol {s_tol}")
    for i in range(B):          # and on a batch of one
        g1, n1 = one_solver.project(xc[i:i + 1], sg[i:i + 1], s_tol=s_tol)
        np.testing.assert_array_equal(g1[0], got[i], err_msg=names[i]); np.testing.assert_array_equal(n1[0], nxt[i], err_msg=names[i])


@pytest.mark.parametrize("flip", [0, 1])
def test_projection_on_two_different_tracks(tracks, proj_entries, flip):
    """fsds_competition_1 and _2 in one handle, the entries of each built on its own knots and interleaved by track_id: every entry
    reads the t * nknots base of every table, and the last knot of the last table (the ``last_knot`` and ``guess_above`` entries)."""
    from oracle import oracle as orc

    B = len(proj_entries[0])
    tid = ((np.arange(B) + flip) % 2).astype(np.int32)
    arrs = [CE.projection_arrays(en) for en in proj_entries]
    xc = np.stack([arrs[t][0][b] for b, t in enumerate(tid)]); sg = np.array([arrs[t][1][b] for b, t in enumerate(tid)])
    names = [f"{e.name}@{t}" for e, t in zip(proj_entries[0], tid)]
    tabs = [np.stack([getattr(t, a) for t in tracks]) for a in ("s_ref", "X_ref", "Y_ref", "phi_ref")]
    assert not np.array_equal(tabs[1][0], tabs[1][1])
    s = _solver(B, tracks, track_id=tid)
    for s_tol in CE.S_TOLS:
        got, nxt = s.project(xc, sg, s_tol=s_tol)
        want, wnxt = orc.cart_to_frenet(*tabs, xc, sg, s_tol=s_tol, track_id=tid)
        _assert_projection(got, nxt, want, wnxt, xc, names, f"two tracks, flip {flip}, s_tol {s_tol}")
    s.free()


# ---- 3. the device-resident ROS step ----
def _solved_pair(B, tracks, tid, seed):
    """Two handles with the same iterate and u0: one RTI solve from the same warm start."""
    out = []
    x0 = np.stack([sample_x0(tracks[t], B, seed=seed)[b] for b, t in enumerate(tid)])
    for _ in range(2):
        s = _solver(B, tracks, track_id=tid)
        s.set_x0(x0); s.init_guess(); s.prepare_step(40.0)
        st = s.solve()
        assert (st == 0).mean() > 0.9
        out.append(s)
    np.testing.assert_array_equal(out[0].get_u0(), out[1].get_u0())
    return out, x0


def _ros_steps(dev, host, tracks, tid, xc, sg, names, tol_plant, check_margins):
    """Three consecutive ROS steps: the device-resident path on ``dev`` against the host path on ``host`` bit for bit, and against the
    oracle restarted from the GPU's state of the step before."""
    from oracle import oracle as orc

    tabs = [np.stack([getattr(t, a) for t in tracks]) for a in ("s_ref", "X_ref", "Y_ref", "phi_ref")]
    u0 = host.get_u0()
    dev.set_cart_state(xc, sg)
    g_xc, g_sg = dev.get_cart_state()
    np.testing.assert_array_equal(g_xc, xc); np.testing.assert_array_equal(g_sg, sg)          # set -> get, bit for bit
    for k in range(3):
        dev.sim_advance_cart(model=-3, M_sim=10, dt_sim=0.01, n_steps=5, v_dyn=3.0, s_tol=2.0)
        d_xc, d_sg = dev.get_cart_state(); d_x0 = dev.get_x0()
        h_xc = host.sim_step_cart(xc, u0, model=-3, M_sim=10, dt_sim=0.01, n_steps=5, v_dyn=3.0)
        h_x0, h_sg = host.project(h_xc, sg, s_tol=2.0)
        np.testing.assert_array_equal(d_xc, h_xc, err_msg=f"step {k}: Cartesian state"); np.testing.assert_array_equal(d_sg, h_sg, err_msg=f"step {k}: guess")
        np.testing.assert_array_equal(d_x0, h_x0, err_msg=f"step {k}: x0")
        if check_margins:
            for st in plant_decisions(xc, u0, "STEPS_5"):
                exact = (st["hypot"] == 3.0) & (k == 0)
                assert np.all((st["m_switch"] >= MARGIN) | exact) and np.all(st["m_clamp"] >= MARGIN), f"step {k}: an undecided reference"
        o_xc = _plant_steps(xc, u0, "ros", "STEPS_5")[-1]
        e1 = (np.abs(d_xc - o_xc) / (1.0 + np.abs(o_xc))).max(axis=1)
        o_x0, o_sg = orc.cart_to_frenet(*tabs, d_xc, sg, s_tol=2.0, track_id=tid)
        assert np.all(np.isfinite(o_x0)) and np.all(np.isfinite(d_x0))
        e2 = np.maximum(np.abs(d_x0 - o_x0).max(axis=1), np.abs(d_sg - o_sg))
        w1, w2 = int(np.argmax(e1 / tol_plant)), int(np.argmax(e2))
        print(f"ROS step {k}: plant worst {e1[w1]:.2e} of {tol_plant[w1]:.1e} at {names[w1]}; projection worst {e2[w2]:.2e} of {CE.PROJ_TOL:.1e} at {names[w2]}")
        assert np.all(e1 < tol_plant), [(names[i], e1[i]) for i in np.flatnonzero(e1 >= tol_plant)]
        assert np.all(e2 < CE.PROJ_TOL), [(names[i], e2[i]) for i in np.flatnonzero(e2 >= CE.PROJ_TOL)]
        xc, sg = d_xc, d_sg


def test_device_resident_ros_step_on_the_cartesian_table(tracks, plant_entries):
    """``ihm2mpc_sim_advance_cart`` launches k_sim_cart IN PLACE on the handle's Cartesian state with the handle's u0 and projects into
    x0.  The table's velocities, headings and actuator states, each car placed 0.3 m beside a knot of its own."""
    t = tracks[0]
    B = len(plant_entries)
    tid = np.zeros(B, dtype=np.int32)
    (dev, host), _ = _solved_pair(B, tracks[:1], tid, seed=11)
    xc, _ = CE.plant_arrays(plant_entries)
    k = t.s_ref.size // 3 + 5 * np.arange(B) + 3
    tx, ty = t.X_ref[k + 1] - t.X_ref[k], t.Y_ref[k + 1] - t.Y_ref[k]
    xc[:, 0], xc[:, 1] = t.X_ref[k] - 0.3 * ty / np.hypot(tx, ty), t.Y_ref[k] + 0.3 * tx / np.hypot(tx, ty)
    tol = np.array([e.tolerance("ros", "STEPS_5") for e in plant_entries])
    _ros_steps(dev, host, tracks[:1], tid, xc, t.s_ref[k].copy(), [e.name for e in plant_entries], tol, check_margins=True)
    dev.free(); host.free()


def test_device_resident_ros_step_on_a_ragged_batch_over_two_tracks(tracks):
    from ihm2_amd.closed_loop_sim import frenet_to_cartesian

    B = 70
    tid = (np.arange(B) % 2).astype(np.int32)
    (dev, host), x0 = _solved_pair(B, tracks, tid, seed=12)
    x0[:, 4] = 0.05 * x0[:, 3] * np.sign(x0[:, 5])
    x0[:6, 3] = np.linspace(0.02, 2.9, 6); x0[:6, 4] = 0.0          # slow cars: the kinematic side of the switch
    xc = np.stack([frenet_to_cartesian(tracks[t], x0[b:b + 1])[0] for b, t in enumerate(tid)])
    _ros_steps(dev, host, tracks, tid, xc, x0[:, 0] + 0.5, [f"car {b}" for b in range(B)], np.full(B, CE.PLANT_TOL["STEPS_5"]), check_margins=True)
    dev.free(); host.free()


def test_cart_state_entry_points_refuse_and_stay_usable(tracks, plant_entries):
    t = tracks[0]
    B = 70
    tid = np.zeros(B, dtype=np.int32)
    s = _solver(B, tracks[:1], geometry=False)
    s.set_x0(sample_x0(t, B, seed=13)); s.init_guess(); s.prepare_step(40.0); s.solve()
    xc, _ = CE.plant_arrays(plant_entries)
    xc = xc[:B].copy()
    k = t.s_ref.size // 3 + 7 * np.arange(B)
    xc[:, 0], xc[:, 1] = t.X_ref[k] + 0.1, t.Y_ref[k] - 0.1
    sg = t.s_ref[k].copy()
    s.set_cart_state(xc, sg)
    with pytest.raises(Exception, match="geometry"):
        s.sim_advance_cart()
    with pytest.raises(Exception, match="geometry"):
        s.project(xc, sg)
    s.set_track_geometry(t.X_ref, t.Y_ref, t.phi_ref)
    for kw, msg in ((dict(model=7), "plant"), (dict(model=0), "plant"), (dict(M_sim=0), "M_sim"), (dict(n_steps=0), "n_steps"), (dict(dt_sim=0.0), "dt_sim"),
                    (dict(dt_sim=-0.01), "dt_sim"), (dict(dt_sim=np.nan), "dt_sim"), (dict(s_tol=0.0), "s_tol"), (dict(s_tol=-2.0), "s_tol"), (dict(s_tol=np.nan), "s_tol")):
        with pytest.raises(Exception, match=msg):
            s.sim_advance_cart(**kw)
    u = np.zeros((B, 2))
    for kw in (dict(model=7), dict(M_sim=0), dict(n_steps=0), dict(dt_sim=0.0)):
        with pytest.raises(Exception):
            s.sim_step_cart(xc, u, **kw)
    with pytest.raises(Exception, match="s_tol"):
        s.project(xc, sg, s_tol=0.0)
    dp = ctypes.POINTER(ctypes.c_double)
    null = ctypes.cast(None, dp)
    assert s.lib.ihm2mpc_set_cart_state(s._h, null, sg.ctypes.data_as(dp)) != 0 and s.lib.ihm2mpc_set_cart_state(s._h, xc.ctypes.data_as(dp), null) != 0
    assert b"null" in s.lib.ihm2mpc_last_error()
    # none of the refusals touched the state; NULL for either output of the getter is accepted
    g_xc, g_sg = np.empty((B, 8)), np.empty(B)
    assert s.lib.ihm2mpc_get_cart_state(s._h, g_xc.ctypes.data_as(dp), null) == 0 and s.lib.ihm2mpc_get_cart_state(s._h, null, g_sg.ctypes.data_as(dp)) == 0
    assert s.lib.ihm2mpc_get_cart_state(s._h, null, null) == 0
    np.testing.assert_array_equal(g_xc, xc); np.testing.assert_array_equal(g_sg, sg)
    # and the handle works: the step it then takes is the host path's
    u0 = s.get_u0()
    s.sim_advance_cart()
    h_xc = s.sim_step_cart(xc, u0)
    h_x0, h_sg = s.project(h_xc, sg)
    d_xc, d_sg = s.get_cart_state()
    np.testing.assert_array_equal(d_xc, h_xc); np.testing.assert_array_equal(d_sg, h_sg); np.testing.assert_array_equal(s.get_x0(), h_x0)
    s.free()


# ---- 4. k_sim_dyn10 ----
@pytest.mark.parametrize("two_tracks", [False, True])
@pytest.mark.parametrize("config", list(CE.DYN10_CONFIGS))
def test_dyn10_plant_matches_oracle_at_edge_states(track, dyn10_entries, config, two_tracks):
    """RK4_1: ONE RK4 step over 0.002 s on every entry (a handle with tf = 40 x 0.002); RK4_100: a whole plant step on every entry but
    the named "single-step only" ones (they run, as neighbours); RADAU_100: the reference's plant integrator, every entry.  two_tracks:
    the same table twice with every instance but the first on the second one (the tid * nknots base, the last knot of the last table)."""
    from ihm2_amd.solver import BatchedOcpSolver

    B = len(dyn10_entries)
    M, dt = CE.DYN10_CONFIGS[config]
    opts = dict(tf=40 * dt)
    if config.startswith("RADAU"):
        opts.update(sim_integrator_type="IRK", sim_collocation_type="GAUSS_RADAU_IIA")
    if two_tracks:
        s_ref, k_ref = np.stack([track.s_ref, track.s_ref]), np.stack([track.kappa_ref, track.kappa_ref])
        tid = np.ones(B, dtype=np.int32); tid[0] = 0
    else:
        s_ref, k_ref, tid = track.s_ref, track.kappa_ref, None
    s = BatchedOcpSolver(make_ocp(**opts), B, s_ref, k_ref, track_id=tid)
    x, u = CE.dyn10_arrays(dyn10_entries)
    got = s.sim_step_dyn10(x, u, M_sim=M)
    s.free()
    want = dyn10_step(config, x, u, track.s_ref, track.kappa_ref)
    compared = np.array([not (e.single_step_only and config == "RK4_100") for e in dyn10_entries])
    assert compared.all() or (config == "RK4_100" and (~compared).sum() == len(CE.SINGLE_STEP_ONLY))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    names = np.array([e.name for e in dyn10_entries])[compared]
    err = (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max(axis=1)[compared]
    tol = np.array([e.tolerance(config) for e, c in zip(dyn10_entries, compared) if c])
    w = int(np.argmax(err / tol))
    print(f"fdyn10 {config}{' two tracks' if two_tracks else ''}: worst {err[w]:.2e} of {tol[w]:.1e} at {names[w]} ({compared.sum()} of {B} entries)")
    assert np.all(err < tol), [(names[i], float(f"{err[i]:.3g}")) for i in np.flatnonzero(err >= tol)]


# ---- 5. isolation ----
BAD = CE.non_finite_cart_states()
SLOTS = {"nan_in_X": 5, "nan_in_phi": 41, "nan_guess": 63, "inf_in_vx": 64}          # inside, and on either side of, the wave boundary


def _with_bad_slots(xc, sg):
    xm, gm = xc.copy(), sg.copy()
    for name, i in SLOTS.items():
        xb, g = BAD[name]
        if name == "nan_guess":
            gm[i] = np.nan
        else:
            comp = int(np.flatnonzero(~np.isfinite(xb))[0])
            xm[i, comp] = xb[comp]
    return xm, gm


def test_non_finite_instances_stay_alone_in_the_cartesian_kernels(tracks, plant_entries):
    """NaN in X, NaN in phi, a NaN guess and inf in v_x among benign neighbours: k_sim_cart, k_project and the in-place
    ``sim_advance_cart`` return, and every other instance's numbers are bit-identical to the batch with benign values in those slots.
    Arithmetic on NaN and a bounded scan: nothing here faults."""
    t = tracks[0]
    B = len(plant_entries)
    tid = np.zeros(B, dtype=np.int32)
    (dev, host), _ = _solved_pair(B, tracks[:1], tid, seed=14)
    xc, u = CE.plant_arrays(plant_entries)
    k = t.s_ref.size // 3 + 5 * np.arange(B) + 3
    xc[:, 0], xc[:, 1] = t.X_ref[k] + 0.2, t.Y_ref[k] + 0.1
    sg = t.s_ref[k].copy()
    xm, gm = _with_bad_slots(xc, sg)
    keep = np.ones(B, dtype=bool); keep[list(SLOTS.values())] = False
    for plant in ("ros", "dyn6", "kin6"):
        clean, bad = _sim_cart(host, xc, u, plant, "STEPS_5"), _sim_cart(host, xm, u, plant, "STEPS_5")
        np.testing.assert_array_equal(bad[keep], clean[keep], err_msg=plant)
        for name in ("nan_in_X", "nan_in_phi", "inf_in_vx"):
            assert not np.all(np.isfinite(bad[SLOTS[name]])), (plant, name)
    (cf, cg), (bf, bg) = host.project(xc, sg), host.project(xm, gm)
    np.testing.assert_array_equal(bf[keep], cf[keep]); np.testing.assert_array_equal(bg[keep], cg[keep])
    assert np.all(np.isnan(bf[SLOTS["nan_in_X"], :2])) and np.isnan(bf[SLOTS["nan_in_phi"], 2]) and np.isnan(bg[SLOTS["inf_in_vx"]])
    assert np.all(np.isfinite(bf[SLOTS["nan_guess"]])) and np.isfinite(bg[SLOTS["nan_guess"]])          # the whole table as its window
    res = []
    for x_, g_ in ((xc, sg), (xm, gm)):
        dev.set_cart_state(x_, g_)
        dev.sim_advance_cart()
        res.append((*dev.get_cart_state(), dev.get_x0()))
    for a, b in zip(*res):
        np.testing.assert_array_equal(b[keep], a[keep])
    assert not np.all(np.isfinite(res[1][0][~keep])) and np.all(np.isfinite(res[0][2]))
    dev.free(); host.free()


def test_non_finite_instances_stay_alone_in_the_dyn10_plant(track, dyn10_entries):
    from ihm2_amd.solver import BatchedOcpSolver

    B = len(dyn10_entries)
    s = BatchedOcpSolver(make_ocp(), B, track.s_ref, track.kappa_ref)
    x, u = CE.dyn10_arrays(dyn10_entries)
    clean = s.sim_step_dyn10(x, u, M_sim=100)
    xm = x.copy()
    slots = {5: (0, np.nan), 41: (2, np.nan), 63: (3, np.inf), 64: (6, np.nan)}          # NaN in s, NaN in psi, inf in v_x, NaN in a wheel speed
    for i, (comp, v) in slots.items():
        xm[i, comp] = v
    bad = s.sim_step_dyn10(xm, u, M_sim=100)
    s.free()
    keep = np.ones(B, dtype=bool); keep[list(slots)] = False
    np.testing.assert_array_equal(bad[keep], clean[keep])
    for i in slots:
        assert not np.all(np.isfinite(bad[i])), i
