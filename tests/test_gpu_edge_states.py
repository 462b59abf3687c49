"""Every model-evaluating kernel against the oracle at the edge states of tests/edge_states.py: headings in every quadrant of the
sine / cosine reduction and beyond its range, steering angles up to 1.5, speeds at and around zero and negative, arc lengths on knots,
outside the curvature table and crossing several knots per interval in both directions, 1 + kappa n = 0.5, both sides of the
kinematic / dynamic plant switch, and combinations.  tests/test_oracle_edge_states.py certifies the oracle at these inputs on the CPU;
the tolerances are the project's own, stored with each entry, and each test reads from the launch record which kernel it ran."""
import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import edge_states as E
import launch_cases as LC

pytestmark = pytest.mark.gpu

MODELS = ["fkin6", "fdyn6", "fdyn6u"]
INTEG = {"ERK": dict(M=25), "IRK_GL": dict(M=1, integrator_type="IRK", collocation_type="GAUSS_LEGENDRE"),
         "IRK_RADAU": dict(M=1, integrator_type="IRK", collocation_type="GAUSS_RADAU_IIA")}
# (B, N, two tracks): no latency batch (launch_cases.latency_batch), with a ragged last wave (k_linearize / k_linearize_dyn /
# k_linearize_irk); a latency batch (k_linearize_cols for fkin6 with ERK); N + 1 no multiple of 4 (a ragged tail in the three-pass tiling of the collocation quads);
# the same track tabulated twice with every instance but the first on the second table, so that every entry reads the tid * nknots base
# and the last knot of the last table
SHAPES = {"batch": (5, 40, False), "columns": (3, 40, False), "odd_horizon": (27, 5, False), "two_tracks": (5, 40, True)}


@pytest.fixture(scope="module")
def entries(track):
    return E.table(track.s_ref, track.kappa_ref)


def _iterate(entries, B, N, first=0):
    """Node (b, k) of the batch holds entry idx[b, k], interval (b, k) its input: x (B, N+1, 8), u (B, N, 2)."""
    idx = E.grid(entries, B, N, first)
    X, U = E.arrays(entries)
    return idx, np.ascontiguousarray(X[idx]), np.ascontiguousarray(U[idx[:, :N]])


def _handles(track, model, integ, B, N, two_tracks=False, **opts):
    from ihm2_amd.solver import BatchedOcpSolver
    from oracle import oracle as orc

    ocp = make_ocp(N=N, model=model, **{**INTEG[integ], **opts})
    if two_tracks:
        s_ref, k_ref = np.stack([track.s_ref, track.s_ref]), np.stack([track.kappa_ref, track.kappa_ref])
        tid = np.ones(B, dtype=np.int32)
        tid[0] = 0
    else:
        s_ref, k_ref, tid = track.s_ref, track.kappa_ref, None
    s = BatchedOcpSolver(ocp, B, s_ref, k_ref, track_id=tid)
    P = orc.OracleProblem(ocp.flatten().as_dict(s_ref, k_ref))
    return s, P, tid


MODEL_CODE = {"fkin6": 0, "fdyn6": 1, "fdyn6u": 2}
# what the oracle's successor state is moved by before it becomes node k + 1: b_k is then of this size and its subtraction exact
OFFSET = 1e-3 * np.array([1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0])


def _assert_linearization(got, ref, ks, idx, entries, model, integ, what):
    """On the intervals k in ks, which start from table entries: A, B relative to the column scale, b absolute, at the tolerance the
    entry carries for this model and integrator, with nothing taken off.  On every interval: finite, structural zeros exact."""
    (A, Bm, b), (Ao, Bo, bo) = got, ref
    names = np.array([e.name for e in entries])[idx[:, ks]]
    tol_ab = E.tolerances(entries, "AB", model, integ)[idx[:, ks]]
    tol_b = E.tolerances(entries, "b", model, integ)[idx[:, ks]]
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(Bm)) and np.all(np.isfinite(b))
    err_a = (np.abs(A - Ao) / np.maximum(np.abs(Ao).max(axis=2, keepdims=True), 1e-30)).max(axis=(2, 3))[:, ks]
    err_b = (np.abs(Bm - Bo) / np.maximum(np.abs(Bo).max(axis=2, keepdims=True), 1e-30)).max(axis=(2, 3))[:, ks]
    err_c = np.abs(b - bo).max(axis=2)[:, ks]
    assert np.abs(bo[:, ks]).max() < 0.01          # the defects are the offset: no rounding at the size of an unrelated neighbour
    for err, tol, q in ((err_a, tol_ab, "A"), (err_b, tol_ab, "B"), (err_c, tol_b, "b")):
        w = np.unravel_index(np.argmax(err / tol), err.shape)
        print(f"{what} {q}: worst {err[w]:.2e} of {tol[w]:.1e} at {names[w]}; largest error {err.max():.2e}")
        bad = err >= tol
        assert not bad.any(), (what, q, sorted({(n, float(f"{e:.3g}")) for n, e in zip(names[bad], err[bad])})[:12])
    assert np.all(A[:, :, 3:, :3] == 0) and np.all(A[:, :, 6:, :6] == 0), what          # structural zeros are exact
    if model == "fkin6":
        assert np.all(A[:, :, 3:5, 5] == 0), what                                          # r enters psi_dot only


# ---- a. the linearisation kernels ----
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("integ", list(INTEG))
@pytest.mark.parametrize("model", MODELS)
def test_linearisation_matches_oracle_at_edge_states(track, entries, model, integ, shape):
    """Interval (b, k) of the grid starts from entry idx[b, k] and is compared once, in the launch of its parity: there node k + 1 is
    the oracle's successor state of node k plus OFFSET, so that the defect b_k = Phi(x_k, u_k) - x_{k+1} is small and its absolute bound
    holds as it stands.  (The intervals of the other parity then start from those successor states: they are not entries, and only
    finiteness and the structural zeros are asked of them.)  Over the two launches every entry has been compared on every interval the
    grid gives it, on its own lane."""
    B, N, two = SHAPES[shape]
    s, P, tid = _handles(track, model, integ, B, N, two)
    idx = E.grid(entries, B, N, first=7 * list(SHAPES).index(shape))
    on_last_table = slice(None) if tid is None else tid == tid.max()
    assert np.unique(idx[on_last_table][:, :N]).size == len(entries)          # every entry is linearised (two tracks: on the second table)
    kernel = LC.names(s)[0]
    assert LC.latency_batch(B, N) == (shape == "columns")
    X, U = E.arrays(entries)
    for parity in (0, 1):
        x, u = np.ascontiguousarray(X[idx]), np.ascontiguousarray(U[idx[:, :N]])
        ks = np.arange(parity, N, 2)
        succ = P.sim_step(x[:, ks].reshape(-1, 8), u[:, ks].reshape(-1, 2), MODEL_CODE[model], P.M, integrator=P.p.integrator,
                          track_id=None if tid is None else np.repeat(tid, ks.size))
        x[:, ks + 1] = succ.reshape(B, ks.size, 8) + OFFSET
        s.set_x0(x[:, 0]); s.set_x(x); s.set_u(u)
        s.linearize()
        assert s.get_launch_record()["linearize"] == kernel
        _assert_linearization(s.get_linearization(), P.linearize(x, u, track_id=tid), ks, idx, entries, model, integ,
                              f"{model} {integ} {shape} parity {parity}")
    s.free()


# ---- b. the plants ----
def _plant_reference(P, x, u, plant, M_sim, integrator):
    if plant >= 0:
        return P.sim_step(x, u, plant, M_sim, integrator=integrator), None
    kin = E.switch_value(x) <= 3.0                    # python/main.py:482-489, chosen per instance
    dyn = 2 if plant == -2 else 1
    return np.where(kin[:, None], P.sim_step(x, u, 0, M_sim, integrator=integrator), P.sim_step(x, u, dyn, M_sim, integrator=integrator)), kin


@pytest.mark.parametrize("plant", [0, 1, 2, -1, -2])
@pytest.mark.parametrize("config", ["ERK_25", "ERK_1", "ERK_25_rollout", "RADAU_4"])
def test_plant_step_matches_oracle_at_edge_states(track, entries, plant, config):
    """``sim_step`` on the table itself (B = 87, no multiple of 64).  ERK_25: k_sim_step_kin for the kinematic plant (the shooting
    intervals' integrator), k_sim_step for the others; ERK_25_rollout: the state-only rollout for the kinematic plant as well (the handle
    of a collocation OCP); ERK_1: ONE RK4 step, i.e. four model evaluations almost bare -- over dt = 0.002, the API refuses a single step
    over 0.05 as unstable on the actuator lags; RADAU_4: the collocation plants, four steps."""
    from oracle import oracle as orc

    B = len(entries)
    x, u = E.arrays(entries)
    M_sim = {"ERK_25": 25, "ERK_1": 1, "ERK_25_rollout": 25, "RADAU_4": 4}[config]
    opts = {"ERK_25": {}, "ERK_1": dict(tf=40 * 0.002), "ERK_25_rollout": dict(integrator_type="IRK", sim_method_num_steps=1),
            "RADAU_4": dict(sim_integrator_type="IRK", sim_collocation_type="GAUSS_RADAU_IIA")}[config]
    s, P, _ = _handles(track, "fkin6", "ERK", B, 40, **opts)
    xn = s.sim_step(x, u, model=plant, M_sim=M_sim)
    assert s.get_launch_record()["sim"] == LC.names(s, plant)[1]
    s.free()
    xo, kin = _plant_reference(P, x, u, plant, M_sim, orc.INTEG_IRK_RADAU4 if config == "RADAU_4" else orc.INTEG_RK4)
    if kin is not None:
        sw = np.array([e.family == "switch" for e in entries])
        assert kin[sw].sum() == (~kin[sw]).sum() == sw.sum() // 2          # both sides of the switch occur, 1e-6 apart
    assert np.all(np.isfinite(xn))
    err = (np.abs(xn - xo) / (1.0 + np.abs(xo))).max(axis=1)
    # the tolerance of the model that integrates the instance: the switched plants take the kinematic one below the threshold
    cfg = "ERK_25" if config == "ERK_25_rollout" else config
    dyn = {0: "fkin6", 1: "fdyn6", 2: "fdyn6u", -1: "fdyn6", -2: "fdyn6u"}[plant]
    tol = E.tolerances(entries, "plant", dyn, cfg)
    if kin is not None:
        tol = np.where(kin, E.tolerances(entries, "plant", "fkin6", cfg), tol)
    w = int(np.argmax(err / tol))
    print(f"plant {plant} {config}: worst {err[w]:.2e} of {tol[w]:.1e} at {entries[w].name}")
    assert np.all(err < tol), [(entries[i].name, float(f"{err[i]:.3g}")) for i in np.flatnonzero(err >= tol)]


# ---- c. the persistent loop's own copy of the integrator ----
@pytest.mark.parametrize("build", ["default", "ilp"])
@pytest.mark.parametrize("integ", ["ERK", "IRK_GL"])
@pytest.mark.parametrize("model", ["fkin6", "fdyn6u"])
def test_persistent_loop_equals_one_step_at_edge_states(track, entries, model, integ, build, monkeypatch):
    """One control step from an edge-state iterate: ``run_steps(n_steps=1)`` (k_steps: device_steps.hpp / irk_body.hpp inlined into
    the loop) leaves the linearisation records, statuses, iterates, multipliers and x0 of one ``step()`` from the same start, bit for
    bit.  QPs may fail at such iterates: then on both sides, and the failed instances keep their iterate.  The plant state (lane N of the
    loop) is the oracle's ``sim_step``.  Single-wave QP kernel on both sides, as in test_persistent_loop_equals_step_by_step."""
    from test_gpu_configs import _build

    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")
    B, N = 5, 40
    idx, x, u = _iterate(entries, B, N, first=3)
    res = []
    for persistent in (False, True):
        with _build(build):
            s, P, _ = _handles(track, model, integ, B, N)
        s.set_x0(sample_x0(track, B, seed=5)); s.init_guess()
        s.step(40.0, model=0, M_sim=25)                     # a first solve at a warm start: u0 and statuses exist
        u0 = s.get_u0()
        s.set_x(x); s.set_u(u); s.set_x0(x[:, 0]); s.set_multipliers(None, None)
        if persistent:
            h = s.run_steps(40.0, 1, model=0, M_sim=25, u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True)
            rec = s.get_launch_record()["steps"]
            assert rec is not None and rec.startswith("k_steps<"), rec          # the loop itself, not launches per step
            assert rec.split(",")[5:7] == ["1" if integ != "ERK" else "0", "1>" if model != "fkin6" else "0>"], rec
            np.testing.assert_array_equal(h["status"][0], s.get_status()); np.testing.assert_array_equal(h["x0"][0], s.get_x0())
        else:
            s.step(40.0, model=0, M_sim=25)
        res.append((s.get_linearization(), s.get_status(), s.get_qp_iter(), s.get_x(), s.get_u(), s.get_x0(), s.get_u0(), s.get_multipliers(), u0))
        s.free()
    (la, sta, ita, xa, ua, x0a, u0a, ma, u0s), (lb, stb, itb, xb, ub, x0b, u0b, mb, u0p) = res
    np.testing.assert_array_equal(u0s, u0p)
    for a, b, k in zip(la, lb, "ABb"):
        np.testing.assert_array_equal(a, b, err_msg="linearisation record " + k)
    np.testing.assert_array_equal(sta, stb); np.testing.assert_array_equal(ita, itb)
    np.testing.assert_array_equal(xa, xb); np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(x0a, x0b); np.testing.assert_array_equal(u0a, u0b)
    np.testing.assert_array_equal(ma[0], mb[0]); np.testing.assert_array_equal(ma[1], mb[1])
    # the records are those of the shifted iterate: interval k starts from the entry of node k + 1
    assert np.all(np.isfinite(la[0])) and np.all(np.isfinite(la[2]))
    failed = stb != 0
    print(f"{model} {integ} {build}: statuses {np.bincount(stb)}")
    if failed.any():                                        # failed instances keep their (shifted) iterate
        np.testing.assert_array_equal(xb[failed][:, :N - 1], x[failed][:, 1:N]); np.testing.assert_array_equal(ub[failed][:, :N - 1], u[failed][:, 1:])
    xo = P.sim_step(x[:, 0], u0s, 0, 25)
    err = (np.abs(x0b - xo) / (1.0 + np.abs(xo))).max(axis=1)
    tol = E.tolerances(entries, "plant", "fkin6", "ERK_25")[idx[:, 0]]
    assert np.all(err < tol), (err, tol)


# ---- d. isolation: a non-finite state stays in its own interval ----
BAD = E.non_finite_states()


@pytest.mark.parametrize("integ", list(INTEG))
@pytest.mark.parametrize("model", MODELS)
def test_non_finite_state_stays_in_its_interval(track, entries, model, integ):
    """NaN in s, NaN in psi, s = +inf at one node (b, k) of the batch of (a): the call returns (``seek`` is a bounded walk), interval
    (b, k) has non-finite records, the defect b of interval (b, k - 1) -- which subtracts that node -- is non-finite in that component
    alone, and every other number of the batch is bit-identical to the batch without the replacement.  (b, k) = (1, 15) is interval 55:
    lane 55 of the first wave, and with collocation the quad in the middle of the fourth wave."""
    B, N, _ = SHAPES["batch"]
    s, P, _ = _handles(track, model, integ, B, N)
    idx, x, u = _iterate(entries, B, N)
    s.set_x0(x[:, 0]); s.set_x(x); s.set_u(u); s.linearize()
    clean = s.get_linearization()
    bi, ki = 1, 15
    for name, (xbad, _) in BAD.items():
        xm = x.copy()
        comp = int(np.flatnonzero(~np.isfinite(xbad))[0])
        xm[bi, ki, comp] = xbad[comp]
        s.set_x(xm); s.linearize()
        A, Bm, b = s.get_linearization()
        assert not np.all(np.isfinite(A[bi, ki])) and not np.all(np.isfinite(b[bi, ki])), name
        assert np.all(A[bi, ki, 3:, :3] == 0) and np.all(A[bi, ki, 6:, :6] == 0), name
        assert not np.isfinite(b[bi, ki - 1, comp]), name
        keep = np.ones((B, N), dtype=bool); keep[bi, ki] = False
        for got, ref, q in zip((A, Bm, b), clean, "ABb"):
            if q == "b":
                got, ref = got.copy(), ref.copy()
                got[bi, ki - 1, comp] = ref[bi, ki - 1, comp] = 0.0
            np.testing.assert_array_equal(got[keep], ref[keep], err_msg=f"{name} {q}")
    s.free()


@pytest.mark.parametrize("plant", [0, 2, -2])
@pytest.mark.parametrize("config", ["ERK_25", "RADAU_4"])
def test_non_finite_state_stays_in_its_plant_instance(track, entries, plant, config):
    B = len(entries)
    x, u = E.arrays(entries)
    opts = {} if config == "ERK_25" else dict(sim_integrator_type="IRK", sim_collocation_type="GAUSS_RADAU_IIA")
    M_sim = 25 if config == "ERK_25" else 4
    s, _, _ = _handles(track, "fkin6", "ERK", B, 40, **opts)
    clean = s.sim_step(x, u, model=plant, M_sim=M_sim)
    i = 41                              # the middle of the first wave of the one-lane plants, the middle of a wave of quads
    for name, (xbad, _) in BAD.items():
        xm = x.copy()
        xm[i] = xbad
        xn = s.sim_step(xm, u, model=plant, M_sim=M_sim)
        assert not np.all(np.isfinite(xn[i])), name
        keep = np.arange(B) != i
        np.testing.assert_array_equal(xn[keep], clean[keep], err_msg=name)
    s.free()
