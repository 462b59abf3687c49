"""Certifies the inputs of tests/test_gpu_cart_edge_states.py before a kernel sees them.  At every entry of tests/cart_edge_states.py
the C oracle agrees with an independent mirror (kin6 with NumPy, dyn6 and fdyn10 solve the reference's implicit residuals, the
projection with a NumPy restatement and with closed-form geometry), every plant output is finite -- the car at rest included --, every
decision (speed switch, clamp, nearest knot, segment choice, wraps, fmod) has a margin of 1e-6 or an exact input, and the oracle is so
well conditioned that a disagreement beyond an entry's tolerance is the kernel's.  ``pytest -s -k docstring`` prints the fresh tables."""
import re

import numpy as np
import pytest

import cart_edge_states as CE
import edge_states as E
from oracle import models_np as mnp
from oracle import oracle as orc
from project_np import cart_to_frenet_np

Z2 = np.zeros(2)
PLANTS = {"kin6": orc.MODEL_KIN6, "dyn6": orc.MODEL_DYN6, "ros": -3}
TRACKS = ("fsds_competition_1", "fsds_competition_2")
MARGIN = 1e-6


@pytest.fixture(scope="module")
def plant_entries():
    return CE.plant_table()


@pytest.fixture(scope="module")
def tracks():
    from ihm2_amd.track import track_table

    return [track_table(t) for t in TRACKS]


@pytest.fixture(scope="module")
def proj_entries(tracks):
    return [CE.projection_table(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref) for t in tracks]


@pytest.fixture(scope="module")
def dyn10_entries(track):
    return CE.dyn10_table(E.table(track.s_ref, track.kappa_ref))


# ---- the tables ----
def test_tables_cover_the_families(plant_entries, proj_entries, dyn10_entries, tracks):
    assert {e.family for e in plant_entries} == {"base", "heading", "steering", "speed", "standstill", "wheels", "sideways", "switch", "clamp", "crossing", "combo"}
    x, u = CE.plant_arrays(plant_entries)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.abs(x[:, 7]) < np.pi / 2)
    assert (np.abs(x[:, 2]) > 1e5).sum() >= 2 and (x[:, 3] == 0).any() and (x[:, 3] < 0).any()
    rest = np.all(x[:, 3:6] == 0, axis=1)
    assert rest.sum() >= 2 and (u[rest, 0] > 0).any() and (u[rest, 0] == 0).any()
    left, right = x[:, 3] - CE.HALF_TRACK * x[:, 5], x[:, 3] + CE.HALF_TRACK * x[:, 5]
    assert ((left < 0) & (x[:, 3] > 0)).any() and ((right < 0) & (x[:, 3] > 0)).any()
    assert ((np.abs(x[:, 4]) > 10 * np.abs(x[:, 3])) & (x[:, 3] > 0)).any() and ((np.abs(x[:, 4]) > 10 * np.abs(x[:, 3])) & (x[:, 3] < 0)).any()
    # every table has a ragged last wave, and a B = 1 handle is another case
    for n in (len(plant_entries), len(proj_entries[0]), len(dyn10_entries)):
        assert n % 64 != 0 and n > 64
    assert len(proj_entries[0]) == len(proj_entries[1]) and tracks[0].s_ref.size == tracks[1].s_ref.size
    assert [e.name for e in proj_entries[0]] == [e.name for e in proj_entries[1]]
    # the "single-step only" list is a condition: names of the table, at most 15 % of it
    names = {e.name for e in dyn10_entries}
    assert set(CE.SINGLE_STEP_ONLY) <= names and len(CE.SINGLE_STEP_ONLY) <= 0.15 * len(dyn10_entries)
    assert set(CE.RAISED) <= {e.name for e in plant_entries} and set(CE.RAISED_DYN10) <= names
    assert not set(CE.RAISED_DYN10) & set(CE.SINGLE_STEP_ONLY) or all("RK4_100" not in CE.RAISED_DYN10[n] for n in CE.SINGLE_STEP_ONLY if n in CE.RAISED_DYN10)
    for e in plant_entries:
        for (m, cfg), tol in e.raised.items():
            assert m in PLANTS and tol >= CE.PLANT_TOL[cfg]
    # the table is data and imports nothing of the project: its copies of the constants are the project's
    from ihm2_amd import constants as c

    assert CE.HALF_TRACK == 0.5 * c.axle_track and CE.R_W == mnp.R_w and c.axle_track == mnp.axle_track


# ---- independent mirrors ----
def test_kin6_matches_numpy_mirror_at_edge_states(plant_entries):
    for e in plant_entries:
        f = orc.f(orc.MODEL_KIN6, e.x, e.u, Z2, Z2)
        assert np.all(np.isfinite(f)), e.name
        np.testing.assert_allclose(f, mnp.kin6(e.x, e.u), rtol=1e-13, atol=1e-12, err_msg=e.name)          # tolerance of test_oracle_cart.py


def test_dyn6_solves_the_implicit_residual_at_edge_states(plant_entries):
    scale = np.array([1, 1, 1, mnp.m * 10, mnp.m * 10, mnp.I_z * 10, 1e3, 1e2])
    for e in plant_entries:
        xdot = orc.f(orc.MODEL_DYN6, e.x, e.u, Z2, Z2)
        assert np.all(np.isfinite(xdot)), e.name
        assert np.max(np.abs(mnp.dyn6_residual(xdot, e.x, e.u)) / scale) < 1e-11, e.name                    # tolerance of test_oracle_cart.py


def test_fdyn10_solves_the_implicit_residual_at_edge_states(track, dyn10_entries):
    x, u = CE.dyn10_arrays(dyn10_entries)
    xd = orc.f_dyn10(x, u, track.s_ref, track.kappa_ref)
    for b, e in enumerate(dyn10_entries):
        assert np.all(np.isfinite(xd[b])), e.name
        res = mnp.fdyn10_residual(xd[b], x[b], u[b], track.s_ref, track.kappa_ref)
        scale = np.maximum(1.0, np.abs(np.array([1, 1, 1, mnp.m * xd[b, 3], mnp.m * xd[b, 4], mnp.I_z * xd[b, 5]] + [mnp.I_w * v for v in xd[b, 6:10]] + [1] * 5)))
        assert np.max(np.abs(res) / scale) < 1e-11, (e.name, res)                                           # tolerance of test_oracle_dyn10.py


def _plant_steps(x, u, plant, config):
    """The oracle's states after each plant step of a configuration: (n_steps, B, 8)."""
    M, dt, n_steps, v_dyn = CE.PLANT_CONFIGS[config]
    out = []
    for _ in range(n_steps):
        x = orc.sim_step_cart(x, u, PLANTS[plant], M, dt=dt, v_dyn=v_dyn)
        out.append(x)
    return np.stack(out)


@pytest.mark.parametrize("config", list(CE.PLANT_CONFIGS))
@pytest.mark.parametrize("plant", list(PLANTS))
def test_every_plant_output_is_finite(plant_entries, plant, config):
    """The car at rest included: atan2(0, 0) = 0 and a zero derivative part in the oracle's complex-step arithmetic."""
    x, u = CE.plant_arrays(plant_entries)
    xs = _plant_steps(x, u, plant, config)
    bad = ~np.all(np.isfinite(xs), axis=(0, 2))
    assert not bad.any(), [plant_entries[i].name for i in np.flatnonzero(bad)]


def test_standstill_under_the_dynamic_model(plant_entries):
    """f = 0 but for the actuators where no force acts; with throttle the car accelerates straight ahead."""
    e = {p.name: p for p in plant_entries}
    f0 = orc.f(orc.MODEL_DYN6, e["standstill_straight_wheels"].x, e["standstill_straight_wheels"].u, Z2, Z2)
    assert np.all(f0 == 0.0)
    f1 = orc.f(orc.MODEL_DYN6, e["standstill_throttle"].x, e["standstill_throttle"].u, Z2, Z2)
    assert np.all(np.isfinite(f1)) and f1[3] > 1.0 and np.all(f1[:3] == 0.0)
    _, J = orc.jac(orc.MODEL_DYN6, e["standstill_throttle"].x, e["standstill_throttle"].u, Z2, Z2, complex_step=True)
    assert np.all(np.isfinite(J))


def test_projection_matches_numpy_restatement_at_edge_states(tracks, proj_entries):
    for t, entries in zip(tracks, proj_entries):
        xc, sg = CE.projection_arrays(entries)
        for s_tol in CE.S_TOLS:
            got, nxt = orc.cart_to_frenet(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, xc, sg, s_tol=s_tol)
            for b, e in enumerate(entries):
                want, wnxt = cart_to_frenet_np(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, xc[b], sg[b], s_tol)
                np.testing.assert_array_equal(np.isnan(got[b]), np.isnan(want), err_msg=e.name)               # NaN for NaN
                np.testing.assert_allclose(got[b], want, rtol=0, atol=1e-10, err_msg=f"{e.name} s_tol {s_tol}")
                np.testing.assert_allclose(nxt[b], wnxt, rtol=0, atol=1e-10, err_msg=f"{e.name} s_tol {s_tol}")
                s1 = orc.project(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, xc[b, 0], xc[b, 1], sg[b], s_tol)[0]
                assert s1 == got[b, 0] or (np.isnan(s1) and np.isnan(got[b, 0])), e.name
                np.testing.assert_array_equal(got[b, 3:], xc[b, 3:])
    # the two behaviours of the reference as written: one knot -> 0 / 0, a NaN guess -> the whole table
    t, entries = tracks[0], proj_entries[0]
    names = [e.name for e in entries]
    xc, sg = CE.projection_arrays(entries)
    for s_tol in CE.S_TOLS:
        got, nxt = orc.cart_to_frenet(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, xc, sg, s_tol=s_tol)
        b = names.index("guess_below_table_by_60")
        assert np.all(np.isnan(got[b, :3])) and np.isnan(nxt[b])
        nan_rows = np.isnan(got).any(axis=1)
        np.testing.assert_array_equal(nan_rows, sg + s_tol < t.s_ref[0])          # exactly the windows of one knot
        assert nan_rows.sum() >= (1 if s_tol > 3.0 else 2 if s_tol > 1.0 else 3), (s_tol, np.array(names)[nan_rows])
        b = names.index("guess_nan")
        lap = t.s_ref.size // 3
        assert np.isfinite(got[b]).all() and t.s_ref[0] <= got[b, 0] < t.s_ref[lap]          # the first of the three equal knots wins


def test_projection_on_a_straight_and_on_a_circle_taken_to_their_ends():
    # straight track along -x (heading pi): s = -X, n = -Y
    s_ref = np.linspace(-50, 100, 301); X_ref = -s_ref; Y_ref = np.zeros_like(s_ref); phi_ref = np.full_like(s_ref, np.pi)
    xc = np.array([[50.0 - 0.1, 0.7, np.pi - 0.2, 5.0, 0.1, 0.0, 10.0, 0.01],            # at the first knot
                   [-100.0 + 0.1, -1.1, -np.pi + 0.3, 8.0, 0, 0, 0, 0],                   # at the last knot, heading across -pi
                   [-100.0 + 0.1, -1.1, 0.3 + 3 * np.pi, 8.0, 0, 0, 0, 0],
                   [-100.0 + 0.2, 0.4, 3.1415, 2.0, 0, 0, 0, 0],                          # guess beyond the table
                   [50.0 - 0.2, 0.4, -3.1415, 2.0, 0, 0, 0, 0]])                          # guess before the table, inside the window
    xf, sg = orc.cart_to_frenet(s_ref, X_ref, Y_ref, phi_ref, xc, np.array([-50.0, 100.0, 99.0, 130.0, -51.5]))
    np.testing.assert_allclose(xf[:, 0], [-49.9, 99.9, 99.9, 99.8, -49.8], atol=1e-12)
    np.testing.assert_allclose(xf[:, 1], [-0.7, 1.1, 1.1, -0.4, -0.4], atol=1e-12)
    np.testing.assert_allclose(xf[:, 2], [-0.2, 0.3, 0.3, 3.1415 - np.pi, np.pi - 3.1415], atol=1e-12)
    np.testing.assert_array_equal(xf[:, 3:], xc[:, 3:])
    np.testing.assert_allclose(sg, np.fmod(xf[:, 0] + 0.05 * xc[:, 3], 50.0), atol=1e-12)
    # a guess before the table by more than the window: one knot, NaN
    xf, sg = orc.cart_to_frenet(s_ref, X_ref, Y_ref, phi_ref, xc[:1], np.array([-53.0]))
    assert np.all(np.isnan(xf[0, :3])) and np.isnan(sg[0]) and np.array_equal(xf[0, 3:], xc[0, 3:])
    # circle of radius R, counter-clockwise, closed: first knot = last knot in space, headings from pi / 2 to 5 pi / 2
    R, nk = 30.0, 2001
    s_ref = np.linspace(0, 2 * np.pi * R, nk); th = s_ref / R
    X_ref, Y_ref, phi_ref = R * np.cos(th), R * np.sin(th), th + np.pi / 2
    # (on a CURVE the nearest knot as the first or last of its window takes the knot at the window's other end for its neighbour, as
    # written -- at a table end no guess avoids that, the restatement test pins it; a guess beyond the end leaves two knots, prev = next)
    for th0, n, guess in ((2 * np.pi - 1e-3, -1.2, 2 * np.pi * R + 30.0), (2 * np.pi - 1e-3, 0.8, 2 * np.pi * R + 2.5),
                          (np.pi / 2 + 1e-3, 0.3, R * np.pi / 2), (3 * np.pi / 2 - 1e-3, 0.3, R * 3 * np.pi / 2)):          # track heading across +-pi
        X, Y = (R - n) * np.cos(th0), (R - n) * np.sin(th0)
        xf, _ = orc.cart_to_frenet(s_ref, X_ref, Y_ref, phi_ref, np.array([[X, Y, th0 + np.pi / 2 + 0.1, 5, 0, 0, 0, 0.0]]), np.array([guess]))
        assert abs(xf[0, 0] - R * th0) < 2e-3 and abs(xf[0, 1] - n) < 2e-3 and abs(xf[0, 2] - 0.1) < 2e-3, (th0, xf[0, :3])      # chord vs arc


# ---- decision margins ----
def plant_decisions(x, u, config):
    """What the reference decides at every step of the switched plant under a configuration: per step (kin (B), clamped (B), the three
    clamp conditions (B, 3)) and the margins of all of them, (n_steps, B): np.inf where a decision cannot change the result, 0 where it
    sits on its threshold."""
    M, dt, n_steps, v_dyn = CE.PLANT_CONFIGS[config]
    steps = []
    for _ in range(n_steps):
        v = np.hypot(x[:, 3], x[:, 4])
        kin = v < v_dyn
        m_switch = np.abs(v / v_dyn - 1.0)
        pre = np.where(kin[:, None], orc.sim_step_cart(x, u, orc.MODEL_KIN6, M, dt=dt), orc.sim_step_cart(x, u, orc.MODEL_DYN6, M, dt=dt))
        a, b, c = pre[:, 3] < 0.0, pre[:, 3] < 0.01, pre[:, 6] <= 0.1
        ma, mb, mc = np.abs(pre[:, 3]) / 0.01, np.abs(pre[:, 3] / 0.01 - 1.0), np.abs(pre[:, 6] / 0.1 - 1.0)
        mc = np.where((pre[:, 6] == 0.1) & (x[:, 6] == 0.1) & (u[:, 0] == 0.1), np.inf, mc)          # T_dot = 0 exactly: an exact input
        # clamped = a or (b and c): the margin of the outcome
        m_bc = np.where(b & c, np.minimum(mb, mc), np.maximum(np.where(b, 0.0, mb), np.where(c, 0.0, mc)))
        m_clamp = np.where(b & c, np.maximum(m_bc, np.where(a, ma, 0.0)), np.where(a, ma, np.minimum(ma, m_bc)))
        clamped = a | (b & c)
        x = orc.sim_step_cart(x, u, -3, M, dt=dt, v_dyn=v_dyn)
        want = pre.copy()
        want[clamped, 3:6] = 0.0
        np.testing.assert_array_equal(x, want)
        steps.append(dict(kin=kin, clamped=clamped, conds=np.stack([a, b, c], 1), m_switch=m_switch, m_clamp=m_clamp, hypot=v))
    return steps


@pytest.mark.parametrize("config", list(CE.PLANT_CONFIGS))
def test_plant_decisions_have_a_margin_or_an_exact_input(plant_entries, config):
    x, u = CE.plant_arrays(plant_entries)
    v_dyn = CE.PLANT_CONFIGS[config][3]
    steps = plant_decisions(x, u, config)
    for k, st in enumerate(steps):
        for i, e in enumerate(plant_entries):
            if k == 0 and v_dyn in e.exact_switch:
                assert st["hypot"][i] == v_dyn and not st["kin"][i], e.name          # hypot(3, 0) == 3.0: not below, the dynamic model
            else:
                assert st["m_switch"][i] >= MARGIN, (e.name, k, st["hypot"][i])
            assert st["m_clamp"][i] >= MARGIN, (e.name, k, st["m_clamp"][i])
    # both sides of every threshold occur
    first = steps[0]
    assert first["kin"].any() and (~first["kin"]).any() and first["clamped"].any() and (~first["clamped"]).any()
    if config != "RK4_1":
        for j in range(3):
            assert first["conds"][:, j].any() and (~first["conds"][:, j]).any()
        names = [e.name for e in plant_entries]
        c = dict(zip(names, first["clamped"]))
        assert c["clamp_braking_crawl"] and c["clamp_coast_below_T_low"] and c["clamp_T_exactly_0p1"] and c["clamp_reverse_by_steering"] and c["clamp_T_falls_below"]
        assert not (c["clamp_coast_below_T_high"] or c["clamp_coast_above_T_low"] or c["clamp_coast_above_T_high"])
        i = names.index("clamp_reverse_by_steering")
        assert list(first["conds"][i]) == [True, True, False]                    # by v_x+ < 0 alone
        sw = {n: k for n, k in zip(names, first["kin"]) if n.startswith("switch_")}
        vd = _num(v_dyn)
        assert sw[f"switch_{vd}_kin"] and not sw[f"switch_{vd}_dyn"] and not sw[f"switch_{vd}_exact"]
    if config == "STEPS_5":
        kin = np.stack([st["kin"] for st in steps]); cl = np.stack([st["clamped"] for st in steps])
        names = [e.name for e in plant_entries]
        i = names.index("crossing_accelerates_through_3"); assert kin[0, i] and not kin[-1, i] and 1 <= np.argmin(kin[:, i]) <= 3
        i = names.index("crossing_brakes_through_3"); assert not kin[0, i] and kin[-1, i] and 1 <= np.argmax(kin[:, i]) <= 3
        i = names.index("crossing_brakes_to_the_clamp"); assert not cl[0, i] and cl[-1, i] and 1 <= np.argmax(cl[:, i]) <= 3


def _num(v):
    return f"{v:g}"


@pytest.mark.parametrize("s_tol", CE.S_TOLS)
def test_projection_decisions_have_a_margin_or_an_exact_input(tracks, proj_entries, s_tol):
    for t, entries in zip(tracks, proj_entries):
        for e in entries:
            m = {}
            cart_to_frenet_np(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, e.x, e.s_guess, s_tol, m)
            for k in ("nearest", "angle", "wrap", "fmod"):
                assert m[k] >= MARGIN, (e.name, s_tol, k, m[k])
            if e.on_knot >= 0:          # on the threshold on purpose: bit-equal to the knot, squared distance exactly 0
                assert e.x[0] == t.X_ref[e.on_knot] and e.x[1] == t.Y_ref[e.on_knot]


def test_projection_entries_reach_the_window_edges(tracks, proj_entries):
    """With s_tol = 2: the nearest knot is the first and the last of its window (the wrap of id_prev / id_next) for the entries named so,
    and windows at both table ends, of one knot and of the whole table occur."""
    t, entries = tracks[0], proj_entries[0]
    n = t.s_ref.size

    def window(e, s_tol):
        lo = max(np.searchsorted(t.s_ref, np.fmax(e.s_guess - s_tol, t.s_ref[0]), side="right") - 1, 0)
        up = np.searchsorted(t.s_ref, np.fmin(e.s_guess + s_tol, t.s_ref[-1]), side="right") - 1
        lo, up = (lo - 1 if lo > 0 else lo), (up + 1 if up < n - 1 else up)
        d2 = (t.X_ref[lo:up + 1] - e.x[0]) ** 2 + (t.Y_ref[lo:up + 1] - e.x[1]) ** 2
        return lo, up, int(np.argmin(d2))

    by = {e.name: e for e in entries}
    lo, up, i = window(by["nearest_is_first_of_window"], 2.0); assert i == 0 and up - lo >= 3
    lo, up, i = window(by["nearest_is_last_of_window"], 2.0); assert i == up - lo and up - lo >= 3
    lo, up, i = window(by["nearest_is_first_of_narrow_window"], 1e-3); assert i == 0 and up - lo >= 2
    lo, up, i = window(by["nearest_is_last_of_narrow_window"], 1e-3); assert i == up - lo and up - lo >= 2
    lo, up, i = window(by["guess_below_table_by_60"], 50.0); assert lo == up == 0
    lo, up, i = window(by["guess_above_table_by_60"], 50.0); assert (lo, up) == (n - 2, n - 1)
    lo, up, i = window(by["guess_nan"], 2.0); assert (lo, up) == (0, n - 1)
    lo, up, i = window(by["first_knot_left"], 2.0); assert lo == 0 and i == 0
    lo, up, i = window(by["last_knot_left"], 2.0); assert up == n - 1 and i == up - lo


# ---- conditioning, measured on the oracle only ----
def _spread(xq, xp, xn, x, scale):
    """The move of the increment under a perturbation of the input, less the rounding grid of the result, relative to ``scale``."""
    with np.errstate(invalid="ignore"):
        d = np.maximum(np.abs((xq - xp) - (xn - x)) - np.spacing(np.abs(xn)), 0.0)
    return np.max(d / scale)


def plant_sensitivity(e, plant, config):
    """One-ulp sensitivity of a Cartesian plant configuration at one entry, relative to 1 + |x+|.  Under the switch an entry that sits on
    it exactly is a decision on an exact input: v_x and v_y are not perturbed there; nor is T where T+ = 0.1 bit for bit decides the
    clamp, nor the velocities of the car at rest (atan2(0, 0) = 0 while atan2(5e-324, 0) = pi / 2: ``e.exact``) -- those are perturbed after the first RK4 sub-step instead, see below."""
    x, u = e.x[None], e.u[None]
    xn = _plant_steps(x, u, plant, config)[-1]
    s = 0.0
    for i in range(8):
        if (plant == "ros" and i in (3, 4) and CE.PLANT_CONFIGS[config][3] in e.exact_switch) or ("*", i) in e.exact or (plant, i) in e.exact:
            continue
        for up in (np.inf, -np.inf):
            xp = x.copy()
            xp[0, i] = np.nextafter(x[0, i], up)
            s = max(s, _spread(_plant_steps(xp, u, plant, config)[-1], xp, xn, x, 1.0 + np.abs(xn)))
    # The velocities of the car at rest, left out above, are ordinary numbers after the first RK4 sub-step, and from there on every
    # evaluation rounds them: they are perturbed THERE (forced models only: the split of the first plant step into 1 + (M - 1) sub-steps
    # takes no decision again), each unless it still sits on its input bit for bit.  Without this the modes that the crawling car
    # amplifies most are never excited, and two builds of the oracle itself (with and without fused multiply-add) differ by more than
    # 16 x the figure: 1.9e-7 against 1.0e-8 at standstill_no_throttle under dyn6, five steps.
    M, dt, n_steps, _ = CE.PLANT_CONFIGS[config]
    held = [i for i in range(8) if ("*", i) in e.exact]
    if plant != "ros" and held and M > 1:
        def tail(x1):
            x1 = orc.sim_step_cart(x1, u, PLANTS[plant], M - 1, dt=dt * (M - 1) / M)
            for _ in range(n_steps - 1):
                x1 = orc.sim_step_cart(x1, u, PLANTS[plant], M, dt=dt)
            return x1
        x1 = orc.sim_step_cart(x, u, PLANTS[plant], 1, dt=dt / M)
        xn1 = tail(x1)
        for i in held:
            if x1[0, i] == x[0, i]:
                continue
            for up in (np.inf, -np.inf):
                xp = x1.copy()
                xp[0, i] = np.nextafter(x1[0, i], up)
                s = max(s, _spread(tail(xp), xp, xn1, x1, 1.0 + np.abs(xn1)))
    return s


def dyn10_step(config, x, u, s_ref, kappa_ref):
    M, dt = CE.DYN10_CONFIGS[config]
    if config.startswith("RADAU"):
        return orc.sim_step_dyn10_irk(x, u, s_ref, kappa_ref, M=M, dt=dt)
    return orc.sim_step_dyn10(x, u, s_ref, kappa_ref, M, dt=dt)


def dyn10_sensitivities(entries, config, s_ref, kappa_ref):
    """The same for fdyn10, relative to max(1, |x+|): name -> sensitivity, every perturbed state of every entry in ONE batched call.  An
    ulp of s that takes the start into another segment of the curvature table is not applied (test_oracle_edge_states.py says why)."""
    x, u = CE.dyn10_arrays(entries)
    xs, us, owner = [x], [u], [np.arange(len(entries))]
    for i in range(15):
        for up in (np.inf, -np.inf):
            xp = x.copy()
            xp[:, i] = np.nextafter(x[:, i], up)
            keep = np.ones(len(entries), dtype=bool)
            if i == 0:
                keep = np.searchsorted(s_ref, xp[:, 0], side="right") == np.searchsorted(s_ref, x[:, 0], side="right")
            xs.append(xp[keep]); us.append(u[keep]); owner.append(np.flatnonzero(keep))
    xs, us, owner = np.concatenate(xs), np.concatenate(us), np.concatenate(owner)
    out = dyn10_step(config, xs, us, s_ref, kappa_ref)
    xn = out[:len(entries)]
    assert np.all(np.isfinite(xn)), [entries[i].name for i in np.flatnonzero(~np.isfinite(xn).all(axis=1))]
    with np.errstate(invalid="ignore"):
        d = np.maximum(np.abs((out - xs) - (xn - x)[owner]) - np.spacing(np.abs(xn))[owner], 0.0) / np.maximum(1.0, np.abs(xn))[owner]
    d = np.where(np.isnan(d), np.inf, d).max(axis=1)
    sens = np.zeros(len(entries))
    np.maximum.at(sens, owner, d)
    return {e.name: float(v) for e, v in zip(entries, sens)}


def projection_sensitivity(t, e, s_tol):
    """Absolute move of (s, n, psi, next guess) under one ulp of X, Y, phi or the guess (psi less the move of phi itself)."""
    ref = np.concatenate([a.ravel() for a in orc.cart_to_frenet(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, e.x[None], [e.s_guess], s_tol=s_tol)])
    s = 0.0
    for i in range(4):
        for up in (np.inf, -np.inf):
            x, g = e.x.copy(), e.s_guess
            if i < 3:
                x[i] = np.nextafter(x[i], up)
            else:
                g = np.nextafter(g, up)
            if e.on_knot >= 0 and i < 2:
                continue                        # bit-equal to the knot on purpose: an exact input
            got = np.concatenate([a.ravel() for a in orc.cart_to_frenet(t.s_ref, t.X_ref, t.Y_ref, t.phi_ref, x[None], [g], s_tol=s_tol)])
            with np.errstate(invalid="ignore"):
                d = np.abs(got - ref)[[0, 1, 2, 8]]
                if i == 2:          # psi moves with phi one to one, on the rounding grid of phi + pi (wrap_to_pi as written): the format's
                    d[2] = max(abs(abs(got[2] - ref[2]) - abs(x[2] - e.x[2])) - np.spacing(abs(e.x[2]) + np.pi), 0.0)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), e.name
            s = max(s, np.nanmax(np.append(d, 0.0)))
    return s


SENS_CONFIGS = [(p, c) for p in PLANTS for c in CE.PLANT_CONFIGS if c != "VDYN_5" or p == "ros"]


@pytest.fixture(scope="module")
def plant_sens(plant_entries):
    return {e.name: {(p, c): plant_sensitivity(e, p, c) for p, c in SENS_CONFIGS} for e in plant_entries}


@pytest.fixture(scope="module")
def dyn10_sens(track, dyn10_entries):
    per = {c: dyn10_sensitivities(dyn10_entries, c, track.s_ref, track.kappa_ref) for c in CE.DYN10_CONFIGS}
    return {e.name: {c: per[c][e.name] for c in CE.DYN10_CONFIGS} for e in dyn10_entries}


def test_cartesian_plants_are_well_conditioned(plant_entries, plant_sens):
    """The conditioning cap: the oracle's one-ulp sensitivity stays below a tenth of the tolerance the entry carries for that plant and
    configuration; a raised tolerance lies within [16, 18] x the measured sensitivity and is raised for cause."""
    bad = []
    for e in plant_entries:
        for (p, c), s in plant_sens[e.name].items():
            if not s < 0.1 * e.tolerance(p, c):
                bad.append((e.name, p, c, float(f"{s:.2g}"), e.tolerance(p, c)))
            if (p, c) in e.raised:
                assert s >= 0.1 * CE.PLANT_TOL[c] and 16.0 * s <= e.raised[(p, c)] <= 18.0 * s, (e.name, p, c, s, e.raised[(p, c)])
    assert not bad, bad


def test_fdyn10_is_well_conditioned_or_single_step_only(dyn10_entries, dyn10_sens):
    """Over a whole plant step (RK4 x 100 over 0.05 s) the entries that one ulp moves by more than 1e-6 are not raised: they are the
    named "single-step only" list, compared over one RK4 step of 0.002 s, where every entry is well conditioned.  The Radau IIA plant
    (the reference's own integrator, python/main.py:395-400) is stable where RK4 x 100 is not: every entry is compared under it, and this
    test keeps it so (the GPU test has it on the condition that at least 85 % of the table is comparable)."""
    bad = []
    for e in dyn10_entries:
        s1, s100, sr = (dyn10_sens[e.name][c] for c in ("RK4_1", "RK4_100", "RADAU_100"))
        if not s1 < 0.1 * e.tolerance("RK4_1"):
            bad.append((e.name, "RK4_1", s1))
        if not sr < 0.1 * e.tolerance("RADAU_100"):
            bad.append((e.name, "RADAU_100", sr))
        if e.single_step_only:
            assert s100 > 1e-6, (e.name, s100)          # on the list for cause
        elif not s100 < 0.1 * e.tolerance("RK4_100"):
            bad.append((e.name, "RK4_100", float(f"{s100:.2g}")))
        for c, tol in e.raised.items():
            s = dyn10_sens[e.name][c]
            assert s >= 0.1 * CE.DYN10_TOL and 16.0 * s <= tol <= 18.0 * s and tol <= 16e-6, (e.name, c, s, tol)
    assert not bad, bad


@pytest.mark.parametrize("s_tol", CE.S_TOLS)
def test_projection_is_well_conditioned(tracks, proj_entries, s_tol):
    worst = max((projection_sensitivity(t, e, s_tol), e.name) for t, entries in zip(tracks, proj_entries) for e in entries)
    print(f"projection s_tol {s_tol}: worst one-ulp sensitivity {worst[0]:.1e} at {worst[1]}")
    assert worst[0] < 0.1 * CE.PROJ_TOL, worst


def _family_rows(entries, sens, keys):
    fams = list(dict.fromkeys(e.family for e in entries))
    return {f: [max(sens[e.name][k] for e in entries if e.family == f) for k in keys] for f in fams}


def _check_rows(rows, header):
    doc = CE.__doc__[CE.__doc__.index(header):]
    for fam, vals in rows.items():
        m = re.search(r"^%s +(.*)$" % fam, doc, flags=re.M)
        assert m, f"no row for family {fam} in the docstring of cart_edge_states.py"
        old = [float(v) for v in re.findall(r"[0-9.]+e[-+][0-9]+", m.group(1))]
        assert len(old) == len(vals), fam
        for d, f in zip(old, vals):
            assert d / 4.0 <= max(f, 1e-17) <= 4.0 * d, (fam, old, vals)


def test_sensitivity_tables_of_the_docstring_are_current(plant_entries, plant_sens, dyn10_entries, dyn10_sens):
    """The tables at the top of tests/cart_edge_states.py are what this module measures (to a factor of 4: the smallest figures are a few
    roundings and move with the last bit of libm)."""
    keys = [(p, c) for p in ("kin6", "dyn6") for c in ("RK4_10", "RK4_1", "STEPS_5")]
    rows = _family_rows(plant_entries, plant_sens, keys)
    for fam, vals in rows.items():
        print(f"{fam:<12s}" + "".join(f"{max(v, 1e-17):>12.1e}" for v in vals))
    rows10 = _family_rows(dyn10_entries, dyn10_sens, list(CE.DYN10_CONFIGS))
    for fam, vals in rows10.items():
        print(f"{fam:<12s}" + "".join(f"{max(v, 1e-17):>11.1e}" for v in vals))
    _check_rows(rows, "family          kin6 RK4_10")
    _check_rows(rows10, "family           RK4_1")
