"""Plant steps with forward sensitivities on the GPU (kernels_simsens.hip, ihm2mpc_sim_step_sens): S_x, S_u and x_next against the
oracle's ``rk4_sens`` (ERK_LAG: tests/lag_ref.py) on warm-start states and on the edge states of tests/edge_states.py, the switched
plants against calls with the model fixed, consistency with the linearisation records and with ``sim_step``, central differences of
``ihm2mpc_sim_step`` itself, and that the call moves nothing else of the handle.

Shapes: B = 1 (a lone lane / quad), 3 (a ragged quad), 65 (two waves, the second ragged) on handles with N = 2 (latency batches, where
``sim_step`` takes the state-only rollout), and B = 5 at N = 40.  M_sim = 25 and 30 for RK4, 1 and 4 for ERK_LAG and collocation.

Every test prints the figures it asserts; NOTES.md (R13) has them as measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest
from conftest import make_ocp, sample_x0

import edge_states as E
import lag_ref
import launch_cases as LC
import sim_sens_cases as SC

pytestmark = pytest.mark.gpu

NAME = {0: "fkin6", 1: "fdyn6", 2: "fdyn6u"}
INTEG = {"ERK": (0, {}, (25, 30)),
         "IRK_GL4": (1, dict(sim_integrator_type="IRK", sim_collocation_type="GAUSS_LEGENDRE"), (1, 4)),
         "IRK_RADAU4": (2, dict(sim_integrator_type="IRK", sim_collocation_type="GAUSS_RADAU_IIA"), (1, 4))}
LAG = dict(integrator_type="ERK_LAG", sim_integrator_type="ERK_LAG")
SHAPES = {"B1": (1, 2), "B3": (3, 2), "B65": (65, 2), "B5_N40": (5, 40)}
DT = 0.05


def _solver(track, B, N=2, model="fkin6", M=25, **opts):
    from ihm2_amd.solver import BatchedOcpSolver

    return BatchedOcpSolver(make_ocp(N=N, M=M, model=model, **opts), B, track.s_ref, track.kappa_ref)


def _pairs(track, B, seed=3):
    """Warm-start states of sample_x0 with some lateral velocity, controls near the actuator states."""
    x = sample_x0(track, B, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    x[:, 4] = rng.uniform(-0.3, 0.3, B)
    u = np.stack([x[:, 6] + rng.uniform(-100, 100, B), x[:, 7] + rng.uniform(-0.05, 0.05, B)], 1)
    return x, u


_CACHE = {}


def _reference(track, model, code, M, B, seed=3):
    """(x_next, S_x, S_u) of orc.rk4_sens per instance: computed once per case, shared, never written to."""
    from oracle import oracle as orc

    key = ("pairs", model, code, M, B, seed)
    if key not in _CACHE:
        x, u = _pairs(track, B, seed)
        out = [orc.rk4_sens(model, x[i], u[i], track.s_ref, track.kappa_ref, DT, M, integrator=code) for i in range(B)]
        _CACHE[key] = tuple(np.stack([o[j] for o in out]) for j in range(3))
        for a in _CACHE[key]:
            a.setflags(write=False)
    return _CACHE[key]


def _col_err(S, ref):
    return np.abs(S - ref) / np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-30)


def _assert_zeros(Sx, what=""):
    assert np.all(Sx[:, 3:, :3] == 0) and np.all(Sx[:, 6:, :6] == 0), what          # structural zeros are exact


# ---- a. parity with the reference ----
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("integ", list(INTEG))
def test_matches_reference(track, integ, shape):
    """Models 0, 1, 2 at both sub-step counts on one handle.  A, B relative to the column scale < 1e-10 (fkin6 with RK4) / 1e-9 (the
    dynamic models, collocation), x_next relative to 1 + |x| < 1e-10: the project's tolerances of the linearisation and the plants."""
    code, opts, Ms = INTEG[integ]
    B, N = SHAPES[shape]
    s = _solver(track, B, N, **opts)
    x, u = _pairs(track, B)
    for model in (0, 1, 2):
        for M in Ms:
            out = s.sim_step_sens(x, u, model=model, M_sim=M)
            assert s.get_launch_record()["sim"] == "k_sim_sens"
            xo, Ao, Bo = _reference(track, model, code, M, B)
            tol = 1e-10 if (model == 0 and integ == "ERK") else 1e-9
            eA, eB = _col_err(out["Sx"], Ao).max(), _col_err(out["Su"], Bo).max()
            ex = (np.abs(out["x"] - xo) / (1.0 + np.abs(xo))).max()
            print(f"{integ} x {M} {NAME[model]} {shape}: S_x {eA:.2e} S_u {eB:.2e} of {tol:.0e}, x_next {ex:.2e} of 1e-10")
            assert eA < tol and eB < tol and ex < 1e-10
            _assert_zeros(out["Sx"], (integ, model, M))
            np.testing.assert_array_equal(out["model_used"], np.full(B, model, dtype=np.int32))
    s.free()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_erk_lag_matches_lag_ref(track, shape):
    B, N = SHAPES[shape]
    s = _solver(track, B, N, M=4, **LAG)
    x, u = _pairs(track, B)
    mask = lag_ref.structural_mask()
    for M in (1, 4):
        out = s.sim_step_sens(x, u, model=0, M_sim=M)
        ref = [lag_ref.lag_step(x[i], u[i], track.s_ref, track.kappa_ref, DT, M, sens=True) for i in range(B)]
        xo, Ao, Bo = (np.stack([r[j] for r in ref]) for j in range(3))
        eA, eB = _col_err(out["Sx"], Ao).max(), _col_err(out["Su"], Bo).max()
        ex = (np.abs(out["x"] - xo) / (1.0 + np.abs(xo))).max()
        print(f"ERK_LAG x {M} {shape}: S_x {eA:.2e} S_u {eB:.2e} x_next {ex:.2e}")
        assert eA < 1e-10 and eB < 1e-10 and ex < 1e-10
        S = np.concatenate([out["Sx"], out["Su"]], axis=2)
        assert np.all(S[:, ~mask] == 0) and np.all(np.isfinite(S))
        # bit for bit the plant the handle already has (plant code 4: k_sim_step_kin with the closed-form lags)
        xn = s.sim_step(x, u, model=0, M_sim=M)
        assert (s.get_launch_record()["sim"]) == "k_sim_step_kin_lag"
        np.testing.assert_array_equal(out["x"], xn)
    s.free()


# ---- b. edge states ----
EDGE = {"ERK": ("ERK", 25), "IRK_GL": ("IRK_GL4", 1), "IRK_RADAU": ("IRK_RADAU4", 1)}


@pytest.fixture(scope="module")
def entries(track):
    return E.table(track.s_ref, track.kappa_ref)


def _edge_reference(track, entries, model, code, M):
    from oracle import oracle as orc

    X, U = E.arrays(entries)
    out = [orc.rk4_sens(model, X[i], U[i], track.s_ref, track.kappa_ref, DT, M, integrator=code) for i in range(len(X))]
    return tuple(np.stack([o[j] for o in out]) for j in range(3))


@pytest.mark.parametrize("config", list(EDGE))
@pytest.mark.parametrize("model", [0, 1, 2])
def test_edge_states(track, entries, model, config):
    """Every entry of the table, laid out with its grid on B = 87 instances (entry (first + b STRIDE) mod len: each once, on a lane of
    its own), at the entry's own tolerances: "AB" for S relative to the column scale, "b" absolute for the increment x_next - x.
    A non-finite state then gives non-finite rows for its instance alone."""
    integ, M = EDGE[config]
    code, opts, _ = INTEG[integ]
    n = len(entries)
    idx = E.grid(entries, n, 1, first=5)[:, 0]
    assert np.unique(idx).size == n
    X, U = E.arrays(entries)
    x, u = np.ascontiguousarray(X[idx]), np.ascontiguousarray(U[idx])
    s = _solver(track, n, 2, **opts)
    out = s.sim_step_sens(x, u, model=model, M_sim=M)
    xo, Ao, Bo = (a[idx] for a in _edge_reference(track, entries, model, code, M))
    names = np.array([e.name for e in entries])[idx]
    tol_ab = E.tolerances(entries, "AB", NAME[model], config)[idx]
    tol_b = E.tolerances(entries, "b", NAME[model], config)[idx]
    assert all(np.all(np.isfinite(out[k])) for k in ("x", "Sx", "Su"))
    errs = ((_col_err(out["Sx"], Ao).max(axis=(1, 2)), tol_ab, "S_x"), (_col_err(out["Su"], Bo).max(axis=(1, 2)), tol_ab, "S_u"),
            (np.abs((out["x"] - x) - (xo - x)).max(axis=1), tol_b, "x_next - x"))
    for err, tol, q in errs:
        w = int(np.argmax(err / tol))
        print(f"{NAME[model]} {config} {q}: worst {err[w]:.2e} of {tol[w]:.1e} at {names[w]}; largest error {err.max():.2e}")
    for err, tol, q in errs:
        bad = err >= tol
        assert not bad.any(), (q, [(a, float(f"{b:.3g}")) for a, b in zip(names[bad], err[bad])][:12])
    _assert_zeros(out["Sx"])
    i = 41
    for name, (xbad, _) in E.non_finite_states().items():
        xm = x.copy()
        xm[i] = xbad
        bad = s.sim_step_sens(xm, u, model=model, M_sim=M)
        assert not np.all(np.isfinite(bad["x"][i])) and not np.all(np.isfinite(bad["Sx"][i])), name
        keep = np.arange(n) != i
        for k in ("x", "Sx", "Su", "model_used"):
            np.testing.assert_array_equal(bad[k][keep], out[k][keep], err_msg=f"{name} {k}")
    s.free()


# ---- c. switched plants ----
@pytest.mark.parametrize("integ,M", [("ERK", 25), ("IRK_RADAU4", 4)])
@pytest.mark.parametrize("plant", [-1, -2])
def test_switched_plants_take_the_bits_of_the_branch(track, entries, plant, integ, M):
    """The edge table (its switch family sits 1e-6 on either side of the threshold) followed by warm-start states: model_used is the
    switch rule, and every instance has the bits of a call with that model fixed."""
    _, opts, _ = INTEG[integ]
    X, U = E.arrays(entries)
    xw, uw = _pairs(track, 9, seed=8)
    x, u = np.vstack([X, xw]), np.vstack([U, uw])
    B = len(x)
    dyn = 2 if plant == -2 else 1
    s = _solver(track, B, 2, **opts)
    out = s.sim_step_sens(x, u, model=plant, M_sim=M)
    want = np.where(E.switch_value(x) <= 3.0, 0, dyn).astype(np.int32)
    np.testing.assert_array_equal(out["model_used"], want)
    sw = np.array([e.family == "switch" for e in entries])
    assert (want[:len(entries)][sw] == 0).sum() == (want[:len(entries)][sw] == dyn).sum() == sw.sum() // 2
    for fixed in (0, dyn):
        ref = s.sim_step_sens(x, u, model=fixed, M_sim=M)
        m = want == fixed
        assert m.any()
        for k in ("x", "Sx", "Su"):
            np.testing.assert_array_equal(out[k][m], ref[k][m], err_msg=f"model {fixed} {k}")
    s.free()


# ---- d. consistency with what exists ----
@pytest.mark.parametrize("case", ["fkin6_ERK_batch", "fkin6_ERK_LAG", "fkin6_ERK_cols", "fdyn6u_ERK", "fkin6_IRK_GL", "fdyn6_IRK_GL"])
def test_equals_the_linearisation_records(track, case):
    """A handle whose plant integrates as its shooting intervals do: S_x, S_u on the pairs (x_k, u_k) of the iterate are the records'
    A, B -- the same bits where the same device function runs in the same mapping (dev_integrate_sens_fkin6 one lane per interval, i.e.
    no latency batch, and ERK_LAG), otherwise within the edge table's "AB" tolerance relative to the column scale (1e-10 for fkin6 with RK4: the
    column-parallel kernel of the small batches; 1e-9 for the dynamic models and collocation)."""
    model, integ = case.split("_", 1)
    B, N = (3, 40) if integ == "ERK_cols" else (5, 40)
    opts = {"ERK_batch": dict(M=25), "ERK_cols": dict(M=25), "ERK": dict(M=25), "ERK_LAG": dict(M=4, **LAG),
            "IRK_GL": dict(M=1, integrator_type="IRK", collocation_type="GAUSS_LEGENDRE", sim_integrator_type="IRK",
                           sim_collocation_type="GAUSS_LEGENDRE")}[integ]
    s = _solver(track, B, N, model=model, **opts)
    s.set_x0(sample_x0(track, B, seed=21)); s.init_guess(); s.linearize()
    kernel = s.get_launch_record()["linearize"]
    A, Bm, _ = s.get_linearization()
    X, U = s.get_x(), s.get_u()
    code = {"fkin6": 0, "fdyn6": 1, "fdyn6u": 2}[model]
    worst = 0.0
    for k in (0, 1, 17, N - 1):
        out = s.sim_step_sens(np.ascontiguousarray(X[:, k]), np.ascontiguousarray(U[:, k]), model=code, M_sim=opts["M"])
        if kernel in ("k_linearize", "k_linearize_lag"):
            np.testing.assert_array_equal(out["Sx"], A[:, k]); np.testing.assert_array_equal(out["Su"], Bm[:, k])
        else:
            worst = max(worst, _col_err(out["Sx"], A[:, k]).max(), _col_err(out["Su"], Bm[:, k]).max())
    print(f"{case}: records by {kernel}, worst gap {worst:.2e}")
    assert kernel == LC.names(s)[0] and (kernel == "k_linearize_cols") == (integ == "ERK_cols")
    assert worst < E.TOL["AB"][0 if integ == "ERK_cols" else 1]
    s.free()


@pytest.mark.parametrize("shape", ["B65", "B5_N40"])
@pytest.mark.parametrize("integ", ["ERK", "IRK_RADAU4"])
def test_x_next_against_sim_step(track, integ, shape):
    """x_next is sim_step's bit for bit where the launch record names the shared fkin6 integrator (plant code 1; code 4 is checked in
    test_erk_lag_matches_lag_ref).  Elsewhere -- the state-only rollouts, the dynamic models on four lanes, the collocation plants on
    sixteen -- the gap is measured and printed; both sides are within 1e-10 of the reference, so 2e-10 is what can be asserted."""
    _, opts, Ms = INTEG[integ]
    B, N = SHAPES[shape]
    s = _solver(track, B, N, **opts)
    x, u = _pairs(track, B)
    for model in (0, 1, 2, -1):
        xn = s.sim_step(x, u, model=model, M_sim=Ms[0])
        kernel = s.get_launch_record()["sim"]
        out = s.sim_step_sens(x, u, model=model, M_sim=Ms[0])
        gap = (np.abs(out["x"] - xn) / (1.0 + np.abs(xn))).max()
        print(f"{integ} {shape} model {model}: sim_step by {kernel}, gap {gap:.2e}")
        if kernel == "k_sim_step_kin":
            np.testing.assert_array_equal(out["x"], xn)
        assert gap < 2e-10
    s.free()


@pytest.mark.parametrize("integ", [i[0] for i in SC.INTEGRATORS])
@pytest.mark.parametrize("model", [0, 2])
def test_central_differences_of_sim_step(track, model, integ):
    """No oracle involved: S_x, S_u against central differences of ihm2mpc_sim_step on the same handle, at ten times the error of the
    difference quotient measured on the CPU (sim_sens_cases.FD_WORST, test_oracle_sim_sens.py)."""
    _, _, opts, M = next(i for i in SC.INTEGRATORS if i[0] == integ)
    x, u = SC.fd_cases(track)
    s = _solver(track, len(x), 2, **opts)
    out = s.sim_step_sens(x, u, model=model, M_sim=M)
    S = SC.central_differences(lambda xs, us: s.sim_step(xs, us, model=model, M_sim=M), x, u)
    err = SC.column_error(S, np.concatenate([out["Sx"], out["Su"]], axis=2))
    print(f"model {model} {integ}: central differences of sim_step against sim_step_sens, worst {err:.3e} (bound {SC.FD_BOUND:.1e})")
    assert err < SC.FD_BOUND
    s.free()


# ---- e. nothing else moves ----
def _everything(s):
    pi, lam = s.get_multipliers()
    sx, su = s.get_x0_sensitivities()
    return dict(x0=s.get_x0(), u0=s.get_u0(), x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), lin=s.get_linearization(),
                status=s.get_status(), qp_iter=s.get_qp_iter(), res=s.get_residuals(), sens_x=sx, sens_u=su)


def _assert_same(a, b, what):
    for k in a:
        if isinstance(a[k], tuple):
            for p, q in zip(a[k], b[k]):
                np.testing.assert_array_equal(p, q, err_msg=f"{what}: {k}")
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("integ", ["ERK", "IRK_RADAU4"])
def test_the_call_moves_nothing_else(track, integ):
    """After a solve with x0 sensitivities on: every getter returns the same bits before and after calls with each model, of the launch
    record only the plant code moves, two calls give the same bits and all outputs NULL is accepted."""
    from test_gpu_qp_layouts import _start

    _, opts, Ms = INTEG[integ]
    B = 5
    s = _solver(track, B, 40, **opts)
    _start(s, track, B, 5)
    s.set_x0_sensitivities(2)
    s.solve()
    s.sim_advance(model=0, M_sim=Ms[0])
    before = _everything(s)
    rec = s.get_launch_record()
    x, u = _pairs(track, B)
    first = {m: s.sim_step_sens(x, u, model=m, M_sim=Ms[0]) for m in (0, 1, 2, -1, -2)}
    _assert_same(before, _everything(s), "after sim_step_sens")
    rec2 = s.get_launch_record()
    assert rec2.pop("sim") == "k_sim_sens" and rec.pop("sim") is not None and rec2 == rec
    for m, a in first.items():
        _assert_same(a, s.sim_step_sens(x, u, model=m, M_sim=Ms[0]), f"second call, model {m}")
    from ihm2_amd import _lib
    from ihm2_amd.solver import _ptr

    _lib.check(s.lib.ihm2mpc_sim_step_sens(s._h, -1, Ms[0], _ptr(x), _ptr(u), None, None, None, None))
    _assert_same(before, _everything(s), "after the call without outputs")
    s.free()


@pytest.mark.parametrize("memory", ["device", "pinned"])
def test_device_variant_gives_the_host_variants_bits(track, memory):
    from ihm2_amd import _lib

    B = 65
    hip = C.CDLL("libamdhip64.so")       # the HIP runtime the product library is linked against
    x, u = _pairs(track, B)
    sizes = dict(x=x.nbytes, u=u.nbytes, xn=B * 64, Sx=B * 512, Su=B * 128, mu=B * 4)
    for integ, model in (("ERK", -2), ("ERK", 0), ("IRK_RADAU4", -1)):
        _, opts, Ms = INTEG[integ]
        s = _solver(track, B, 2, **opts)
        host = s.sim_step_sens(x, u, model=model, M_sim=Ms[0])
        buf = {}
        for k, n in sizes.items():
            p = C.c_void_p()
            if memory == "device":
                assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
            else:
                _lib.check(s.lib.ihm2mpc_host_alloc(n, C.byref(p)))
            buf[k] = p
        assert hip.hipMemcpy(buf["x"], C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 4) == 0      # hipMemcpyDefault
        assert hip.hipMemcpy(buf["u"], C.c_void_p(u.ctypes.data), C.c_size_t(u.nbytes), 4) == 0
        for with_model_used in (True, False):          # (False on a switched plant: the mask is local to the call)
            s.sim_step_sens_device(buf["x"].value, buf["u"].value, model=model, M_sim=Ms[0], x_next=buf["xn"].value, Sx=buf["Sx"].value,
                                   Su=buf["Su"].value, model_used=buf["mu"].value if with_model_used else 0)
            s.synchronize()
            got = dict(x=np.empty((B, 8)), Sx=np.empty((B, 8, 8)), Su=np.empty((B, 8, 2)), model_used=np.empty(B, dtype=np.int32))
            for k, a in (("xn", got["x"]), ("Sx", got["Sx"]), ("Su", got["Su"]), ("mu", got["model_used"])):
                assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), buf[k], C.c_size_t(a.nbytes), 4) == 0
            _assert_same(host, got, f"{integ} model {model} {memory}")
        for p in buf.values():
            if memory == "device":
                assert hip.hipFree(p) == 0
            else:
                _lib.check(s.lib.ihm2mpc_host_free(p))
        s.free()


@pytest.mark.parametrize("names", ["1", "sim_sens_work"])
def test_poisoned_workspace_gives_the_same_bits(track, names):
    from poison_cases import ENV, environ

    B = 65
    x, u = _pairs(track, B)
    for integ, model in (("ERK", -2), ("IRK_RADAU4", -1)):
        _, opts, Ms = INTEG[integ]
        res = []
        for value in (None, names):
            with environ(**{ENV: value}):
                s = _solver(track, B, 2, **opts)
            res.append(s.sim_step_sens(x, u, model=model, M_sim=Ms[0]))
            s.free()
        _assert_same(res[0], res[1], f"{integ} model {model} poisoned with {names}")
        assert all(np.all(np.isfinite(v)) for v in res[1].values())


def test_refusals(track):
    from ihm2_amd import _lib
    from ihm2_amd.solver import _ptr

    B = 3
    x, u = _pairs(track, B)
    s = _solver(track, B, 2)
    for model in (3, 4, -3, 5, -4):          # the Cartesian plants IHM2MPC_PLANT_KIN6 / _DYN6 / _ROS have no such entry; unknown numbers
        with pytest.raises(_lib.Ihm2mpcError, match=f"unknown plant model {model}"):
            s.sim_step_sens(x, u, model=model, M_sim=25)
    with pytest.raises(_lib.Ihm2mpcError, match="RK4 with M_sim = 5 sub-steps.*unstable on the actuator lags"):
        s.sim_step_sens(x, u, model=0, M_sim=5)
    with pytest.raises(_lib.Ihm2mpcError, match="M_sim must be >= 1"):
        s.sim_step_sens(x, u, model=0, M_sim=0)
    out = [np.empty((B, 8)), np.empty((B, 8, 8)), np.empty((B, 8, 2))]
    for args in ((None, _ptr(u)), (_ptr(x), None)):
        assert s.lib.ihm2mpc_sim_step_sens(s._h, 0, 25, *args, *[_ptr(o) for o in out], None) != 0
        assert s.lib.ihm2mpc_last_error().decode() == "null argument"
        assert s.lib.ihm2mpc_sim_step_sens_device(s._h, 0, 25, None, None, None, None, None, None) != 0
        assert s.lib.ihm2mpc_last_error().decode() == "null argument"
    s.free()
    s = _solver(track, B, 2, M=4, **LAG)
    for model in (1, 2, -1):
        with pytest.raises(_lib.Ihm2mpcError, match="plant integrator ERK_LAG.*kinematic plant \\(model 0\\) only"):
            s.sim_step_sens(x, u, model=model, M_sim=4)
    s.free()


# ---- f. the shim and the closed loop ----
@pytest.mark.parametrize("B", [1, 3, 65])
def test_shim_fields(track, B):
    from test_sim_sens_abi import _sim
    from ihm2_amd.sim import AcadosSimSolver

    x, u = _pairs(track, B)
    res = {}
    for on in (True, False):
        sim = AcadosSimSolver(_sim(sens_forw=on), batch_size=B)
        sim.set("p", np.concatenate([track.s_ref, track.kappa_ref]))
        sim.set("x", x if B > 1 else x[0]); sim.set("u", u if B > 1 else u[0])
        assert sim.solve() == 0
        res[on] = sim.get("x")
        if on:
            Sx, Su, Sf = sim.get("Sx"), sim.get("Su"), sim.get("S_forw")
            lead = () if B == 1 else (B,)
            assert Sx.shape == lead + (8, 8) and Su.shape == lead + (8, 2) and Sf.shape == lead + (8, 10)
            np.testing.assert_array_equal(Sf, np.concatenate([Sx, Su], axis=-1))
            xo, Ao, Bo = _reference(track, 0, 2, 4, B)
            assert _col_err(np.reshape(Sx, (B, 8, 8)), Ao).max() < 1e-9 and _col_err(np.reshape(Su, (B, 8, 2)), Bo).max() < 1e-9
        else:
            with pytest.raises(ValueError, match="sens_forw"):
                sim.get("S_forw")
        sim.free()
    assert (np.abs(res[True] - res[False]) / (1.0 + np.abs(res[False]))).max() < 2e-10


def test_closed_loop_matrix(track):
    """A_cl = Sx + Su K0 from the separate getters, NaN rows where K0 has them, refused without the x0 sensitivities; on the reference
    layout with the kinematic plant the spectral radius is finite for every solved instance (printed: no threshold)."""
    from test_gpu_qp_layouts import _start

    from ihm2_amd import _lib

    B = 64
    s = _solver(track, B, 40)
    _start(s, track, B, 31)
    s.solve()
    with pytest.raises(_lib.Ihm2mpcError) as off:
        s.closed_loop_matrix(model=0, M_sim=25)
    with pytest.raises(_lib.Ihm2mpcError) as getter:
        s.get_x0_sensitivities()
    assert str(off.value) == str(getter.value)
    s.set_x0_sensitivities(1)
    st = s.solve()
    ok = (st == 0) | (st == 2)
    assert ok.mean() > 0.5
    for model in (0, 2):
        Acl = s.closed_loop_matrix(model=model, M_sim=25)
        _, K0 = s.get_x0_sensitivities()
        out = s.sim_step_sens(s.get_x0(), s.get_u0(), model=model, M_sim=25)
        np.testing.assert_array_equal(Acl, out["Sx"] + out["Su"] @ K0)
        assert np.all(np.isfinite(Acl[ok])) and np.all(np.isnan(Acl[~ok]).any(axis=(1, 2)))
        rho = np.abs(np.linalg.eigvals(Acl[ok])).max(axis=1)
        assert np.all(np.isfinite(rho))
        print(f"closed-loop spectral radius over {int(ok.sum())} solved instances, plant {NAME[model]}: {rho.min():.4f} .. {rho.max():.4f}; "
              f"open loop (S_x alone): {np.abs(np.linalg.eigvals(out['Sx'][ok])).max(axis=1).max():.4f}")
    s.free()
