"""GPU: the device spline fit (k_track_fit through ihm2mpc_fit_tracks) and the track tables (k_track_seglen, k_track_cumsum, k_track_sample
through ihm2mpc_build_tracks) on the synthetic centre lines of tests/track_cases.py -- the smallest and the largest systems the header allows,
ragged batches, clockwise lines, uneven chords, far-away coordinates, the range of curvature weights, table shapes that end on and one past a
wave, more than one wave of tracks, the rows the header calls ignored, and the failure contract.  tests/test_gpu_tracks.py runs the same
kernels on the product's seven centre lines at one shape; tests/test_track_cases.py shows on the CPU that the reference is well inside the
tolerances used here (two CPU methods agree to 7e-12 x extent at worst, where the device is asked for 1e-9 x extent)."""
import numpy as np
import pytest

import track_cases as TC
from conftest import make_ocp

pytestmark = pytest.mark.gpu

C = TC.CASES
FIT_TOL = 1e-9          # x extent, against fit_spline_nullspace
FEAS_TOL, STAT_TOL = 1e-9, 1e-8          # x extent: tests/test_gpu_tracks.py's bounds on kkt_residuals


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def handles():
    """handles(ntracks, n_samples): a solver with B = 1 (ihm2mpc_create accepts every batch >= 1, whatever ntracks), made on first use and
    shared; handles(..., fresh=True): one more of the same.  All are freed with the module."""
    from ihm2_amd.solver import BatchedOcpSolver

    ocp = make_ocp()
    shared, every = {}, []

    def get(ntracks, ns, fresh=False):
        if fresh or (ntracks, ns) not in shared:
            dummy = np.tile(np.linspace(0.0, 1.0, 3 * ns), (ntracks, 1))
            s = BatchedOcpSolver(ocp, 1, dummy, np.zeros_like(dummy))
            every.append(s)
            if fresh:
                return s
            shared[(ntracks, ns)] = s
        return shared[(ntracks, ns)]

    yield get
    for s in every:
        s.free()


def _fit_abi(s, lines, curv_weight=2.0):
    """ihm2mpc_fit_tracks as the C ABI returns it (tests/test_gpu_workspace_poison.py::_fit_tracks_padded): the status, and (ntracks, max_pts, 4)
    twice, the host arrays filled with a sentinel first."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import _ptr

    npts = np.array([len(c) for c in lines], dtype=np.int32)
    mx = int(npts.max())
    xy = np.zeros((len(lines), mx, 2))
    for t, c in enumerate(lines):
        xy[t, :npts[t]] = np.asarray(c, dtype=np.float64)
    cX = np.full((len(lines), mx, 4), 7.0); cY = np.full((len(lines), mx, 4), 7.0)
    rc = s.lib.ihm2mpc_fit_tracks(s._h, mx, npts.ctypes.data_as(_lib.c_int32_p), _ptr(xy), float(curv_weight), _ptr(cX), _ptr(cY))
    return rc, npts, cX, cY


def _fit(s, lines, curv_weight=2.0):
    """Per track (cX, cY) of a call that must succeed; the rows past a track's points come back as exactly 0 (include/ihm2mpc.h)."""
    from ihm2_amd import _lib

    rc, npts, cX, cY = _fit_abi(s, lines, curv_weight)
    _lib.check(rc)
    for t in range(len(lines)):
        assert (cX[t, npts[t]:] == 0.0).all() and (cY[t, npts[t]:] == 0.0).all(), f"track {t}: rows past npts = {npts[t]} are not 0"
    return [(cX[t, :npts[t]].copy(), cY[t, :npts[t]].copy()) for t in range(len(lines))]


def _build_abi(s, coeffs, pad=0.0):
    """ihm2mpc_build_tracks + get_tracks, the coefficient rows past nseg[t] filled with ``pad``."""
    from ihm2_amd import _lib
    from ihm2_amd.solver import _ptr

    nseg = np.array([len(c[0]) for c in coeffs], dtype=np.int32)
    mx = int(nseg.max())
    cX = np.full((len(coeffs), mx, 4), pad); cY = np.full((len(coeffs), mx, 4), pad)
    for t, (x, y) in enumerate(coeffs):
        cX[t, :nseg[t]] = x; cY[t, :nseg[t]] = y
    _lib.check(s.lib.ihm2mpc_build_tracks(s._h, mx, nseg.ctypes.data_as(_lib.c_int32_p), _ptr(cX), _ptr(cY)))
    return s.get_tracks()


def _check_fit(name, points, curv_weight, cX, cY, tol=FIT_TOL):
    from oracle import track_np as OT

    oX, oY = TC.oracle_fit(points, curv_weight)
    ext = float(np.ptp(points, axis=0).max())
    assert cX.shape == oX.shape and cY.shape == oY.shape
    err = max(np.max(np.abs(cX - oX)), np.max(np.abs(cY - oY)))
    feas, stat = OT.kkt_residuals(points, cX, cY, curv_weight)
    print(f"{name}: device vs oracle {err / ext:.2e} x extent, feas {feas / ext:.2e}, stat {stat / ext:.2e}")
    assert np.isfinite(cX).all() and np.isfinite(cY).all(), name
    assert err < tol * ext, (name, err / ext)
    assert feas < FEAS_TOL * ext and stat < STAT_TOL * ext, (name, feas / ext, stat / ext)


def _check_tables(tab, t, points, coeffs, ns, tag):
    """Against the oracle's sampling of the same coefficients, at tests/test_gpu_tracks.py's tolerances for 'same coefficients in'."""
    from oracle import track_np as OT

    mp = OT.motion_plan(points, np.full((len(points), 2), 1.5), n_samples=ns, coeffs=coeffs)
    s_ref, kappa, X, Y, phi = (a[t] for a in tab)
    L = mp["lap_length"]
    assert s_ref.shape == (3 * ns,)
    assert np.max(np.abs(s_ref - mp["s_ref"])) < 1e-9 * L, (tag, t)
    assert np.max(np.abs(X - mp["X_ref"])) < 1e-9 * L and np.max(np.abs(Y - mp["Y_ref"])) < 1e-9 * L, (tag, t)
    assert np.max(np.abs(kappa - mp["kappa_ref"])) < 1e-9 * max(1.0, np.max(np.abs(mp["kappa_ref"]))), (tag, t)
    assert np.max(np.abs(np.angle(np.exp(1j * (phi - mp["phi_ref"]))))) < 1e-9, (tag, t)
    assert np.all(np.diff(s_ref) > 0), (tag, t)


# ---- a, b: the ragged fit, and what a track's result may depend on ----

@pytest.fixture(scope="module")
def ragged(handles):
    """The eight tracks of TC.RAGGED in one call (max_pts = 182: slabs of 1274 x 1276 doubles, of which n3 uses 21 x 23)."""
    return _fit(handles(8, 64), [C[n].points for n in TC.RAGGED])


def test_ragged_fit_in_one_call(ragged):
    for n, (cX, cY) in zip(TC.RAGGED, ragged):
        _check_fit(n, C[n].points, 2.0, cX, cY)


def test_fit_is_independent_of_neighbours_position_and_max_pts(handles, ragged):
    """Bitwise: the elimination updates each entry once per pivot whatever order the LDS lists were filled in, the reductions have a fixed
    order, and the leading dimension is the track's own 7 n + 2."""
    rev = _fit(handles(8, 64), [C[n].points for n in reversed(TC.RAGGED)])[::-1]
    for n, a, b in zip(TC.RAGGED, ragged, rev):
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]), f"{n}: depends on its position in the batch"
    one = handles(1, 64)
    for n in ("n3", "n17"):
        alone = _fit(one, [C[n].points])[0]          # max_pts = the track's own n
        a = ragged[TC.RAGGED.index(n)]
        assert _same_bits(a[0], alone[0]) and _same_bits(a[1], alone[1]), f"{n}: depends on max_pts or on the batch"


SIXTEEN = ("n64", "n65_cw", "n17", "ratio10", "n5_cw", "n4", "n3", "n6", "n3", "ratio10", "n7", "n8", "n4", "n5_cw", "n17", "n6")


def test_sixteen_tracks_fit_as_each_does_alone(handles):
    """More workgroups than the device has dies (XCDs).  Measured with a slab stride taken from the track's own n instead of max_pts: the
    eight-track tests above pass, both orders, bit for bit, although in the reversed order three small slabs then lie inside ratio10's and
    n64's begins inside n65_cw's -- presumably because eight workgroups go to eight dies, each with an L2 of its own that keeps the slab for
    the length of the kernel, so that none sees another's stores.  From the ninth on, workgroups share an L2.  With such a stride the slab
    of track 8 here (n3) lies inside that of track 0 (n64) and that of track 9 (ratio10) across the end of track 1's (n65_cw), and this
    test fails."""
    got = _fit(handles(16, 64), [C[n].points for n in SIXTEEN])
    one = handles(1, 64)
    alone = {n: _fit(one, [C[n].points])[0] for n in sorted(set(SIXTEEN))}
    for t, n in enumerate(SIXTEEN):
        assert _same_bits(got[t][0], alone[n][0]) and _same_bits(got[t][1], alone[n][1]), f"track {t} ({n}): depends on the batch"


# ---- c: weights and conditioning ----

@pytest.mark.parametrize("name", ["w0", "w1e-6", "w1e4", "offset", "ratio50"])
def test_weights_and_conditioning(handles, name):
    c = C[name]
    cX, cY = _fit(handles(1, 64), [c.points], c.curv_weight)[0]
    _check_fit(name, c.points, c.curv_weight, cX, cY)


# ---- d: symmetries of the fit, no oracle involved ----

def test_fit_commutes_with_mirroring_and_a_quarter_turn(handles):
    """Only hypot's argument order (and the sign of its arguments) differs between the three systems."""
    s, p = handles(1, 64), C["n17"].points
    tol = 1e-12 * C["n17"].extent
    cX, cY = _fit(s, [p])[0]
    mX, mY = _fit(s, [TC.mirrored(p)])[0]
    assert np.max(np.abs(mX - cX)) < tol and np.max(np.abs(mY + cY)) < tol
    qX, qY = _fit(s, [TC.quarter_turn(p)])[0]
    assert np.max(np.abs(qX + cY)) < tol and np.max(np.abs(qY - cX)) < tol


# ---- e: tables at small and ragged shapes ----

def _ragged_coeffs():
    return [TC.oracle_fit(C[n].points, 2.0) for n in TC.RAGGED]


def test_tables_of_one_track_at_five_samples(handles):
    s = handles(1, 5)
    for n, co in zip(TC.RAGGED, _ragged_coeffs()):
        _check_tables(_build_abi(s, [co]), 0, C[n].points, co, 5, n)


@pytest.mark.parametrize("ns", [64, 65])
def test_tables_of_the_ragged_batch(handles, ns):
    """8 x 64 samples end on a wave, 8 x 65 run 8 lanes into the next; 8 x 182 segments are 22.75 waves.  At 64 the rows past nseg[t] are
    NaN in a second call: 'the rest of its rows is ignored' (include/ihm2mpc.h), so the tables are the same bits."""
    s, co = handles(8, ns), _ragged_coeffs()
    tab = _build_abi(s, co)
    for t, n in enumerate(TC.RAGGED):
        _check_tables(tab, t, C[n].points, co[t], ns, n)
    if ns == 64:
        tab_nan = _build_abi(s, co, pad=np.nan)
        for a, b, what in zip(tab, tab_nan, ("s_ref", "kappa_ref", "X_ref", "Y_ref", "phi_ref")):
            assert _same_bits(a, b), f"{what} depends on the coefficient rows past nseg[t]"


def test_tables_of_65_tracks_at_five_samples(handles):
    """k_track_cumsum's second wave (one lane per track); 65 x 5 = 325 samples and 65 x 8 = 520 segments end ragged."""
    lines = TC.many_tracks()
    co = [TC.oracle_fit(p, 2.0) for p in lines]
    tab = _build_abi(handles(TC.N_MANY, 5), co)
    for t, p in enumerate(lines):
        _check_tables(tab, t, p, co[t], 5, "ring")


def test_circle_pipeline_has_constant_curvature_and_the_right_length(handles):
    """Fit and tables on the device, against the closed form (tests/test_oracle_track.py::test_circle_has_constant_curvature_and_the_right_length)."""
    s, R, ns = handles(1, 64), 25.0, 64
    s_ref, kappa, X, Y, phi = _build_abi(s, _fit(s, [C["circle"].points]))
    L = s_ref[0, ns] - s_ref[0, 0]
    assert abs(L - 2 * np.pi * R) < 2e-3 * R
    np.testing.assert_allclose(kappa[0], 1.0 / R, rtol=2e-3)
    assert np.all(np.diff(s_ref[0]) > 0)


def test_clockwise_and_counter_clockwise_differ_in_sign_only(handles):
    s, p = handles(1, 64), C["n5_cw"].points
    s_a, k_a, X_a, Y_a, p_a = _build_abi(s, _fit(s, [p]))
    s_b, k_b, X_b, Y_b, p_b = _build_abi(s, _fit(s, [TC.mirrored(p)]))
    assert np.max(k_a) < 0.0 < np.min(k_b)          # clockwise: the curvature of this convex line is negative throughout
    assert np.max(np.abs(s_a - s_b)) < 1e-10 and np.max(np.abs(X_a - X_b)) < 1e-10
    assert np.max(np.abs(Y_a + Y_b)) < 1e-10 and np.max(np.abs(k_a + k_b)) < 1e-10
    assert np.max(np.abs(np.angle(np.exp(1j * (p_a + p_b))))) < 1e-10


# ---- f: the failure contract ----

def _bad_lines(kind):
    p = C["n17"].points.copy()
    if kind == "consecutive_equal":
        p[9] = p[8]
    elif kind == "last_repeats_first":
        p[-1] = p[0]
    else:
        p[4, 1] = np.nan
    return [C["n17"].points, p]


VALID_PAIR = ("n17", "n5_cw")


@pytest.fixture(scope="module")
def fresh_pair(handles):
    """What a handle that has seen nothing else returns for the valid pair."""
    return _fit(handles(2, 64, fresh=True), [C[n].points for n in VALID_PAIR])


@pytest.mark.parametrize("kind", ["consecutive_equal", "last_repeats_first", "nan_coordinate"])
def test_bad_centre_line_is_refused_and_leaves_the_handle_usable(handles, fresh_pair, kind):
    """Track 1 is bad, track 0 valid.  Every index of k_track_fit comes from n and loop counters, every loop is bounded by 7 n, and a NaN
    never wins the pivot comparison: bad points can make NaNs, not faults.  The call must not return 0."""
    s = handles(2, 64)
    rc, npts, cX, cY = _fit_abi(s, _bad_lines(kind))
    msg = s.lib.ihm2mpc_last_error().decode() if rc else ""
    print(f"{kind}: status {rc}, message {msg!r}, coefficients of track 1 finite: {bool(np.isfinite(cX[1]).all() and np.isfinite(cY[1]).all())}")
    assert rc != 0, f"{kind}: ihm2mpc_fit_tracks returned success"
    if kind != "nan_coordinate":
        assert "singular" in msg and "track 1 " in msg, msg
    again = _fit(s, [C[n].points for n in VALID_PAIR])
    for n, a, b in zip(VALID_PAIR, again, fresh_pair):
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]), f"{n} after a failed call differs from a fresh handle's"


def test_non_adjacent_repeated_point_is_solved(handles):
    c = C["crossing"]
    cX, cY = _fit(handles(1, 64), [c.points])[0]
    _check_fit("crossing", c.points, 2.0, cX, cY)
