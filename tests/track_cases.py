"""Synthetic closed centre lines for the spline fit and the track tables (tests/test_track_cases.py on the CPU, tests/test_gpu_track_shapes.py
on the device): the sizes, orientations, chord ratios, offsets and curvature weights that the seven product tracks of data/ do not have.

The base curve is (R cos th + 0.2 R cos 3 th + ox, 0.7 R sin th + oy), R = 30: a rounded triangle, 0.7 : 1, with curvature between 0.01 and 0.19
per metre at R = 30 (l_R kappa <= 0.15: far from asin's edge).  th is a uniform grid jittered by +-0.3 of a grid step from a fixed seed, and
reversed for a clockwise line.  Host only: nothing here touches the device."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle import track_np as OT

R0 = 30.0


@dataclass(frozen=True)
class Case:
    name: str
    points: np.ndarray          # (n, 2), closed: the last point is not the first again
    curv_weight: float = 2.0

    @property
    def n(self) -> int:
        return self.points.shape[0]

    @property
    def extent(self) -> float:
        """ptp of the points, the scale tests/test_gpu_tracks.py uses for the coefficients."""
        return float(np.ptp(self.points, axis=0).max())


def base_curve(th, R=R0, ox=0.0, oy=0.0):
    th = np.asarray(th, dtype=np.float64)
    return np.column_stack((R * np.cos(th) + 0.2 * R * np.cos(3 * th) + ox, 0.7 * R * np.sin(th) + oy))


def _jittered(name, n, R=R0, ox=0.0, oy=0.0, cw=False):
    rng = np.random.default_rng(zlib.crc32(name.encode()))          # a fixed seed per case
    th = 2 * np.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    return base_curve(th[::-1] if cw else th, R, ox, oy)


def _chord_pattern(n, pattern):
    """n points on the base curve whose consecutive distances ALONG the curve repeat ``pattern`` (the chords follow it to the curve's
    bending over one step: the ratio of neighbouring chords, which enters the continuity rows up to squared, is the pattern's)."""
    th = np.linspace(0.0, 2 * np.pi, 20001)
    dense = base_curve(th)
    arc = np.concatenate(([0.0], np.cumsum(np.linalg.norm(np.diff(dense, axis=0), axis=1))))
    w = np.resize(np.asarray(pattern, dtype=np.float64), n)
    at = np.concatenate(([0.0], np.cumsum(w)[:-1])) / w.sum() * arc[-1]
    return base_curve(np.interp(at, arc, th))


def _circle(n, R):
    th = 2 * np.pi * np.arange(n) / n
    return np.column_stack((R * np.cos(th), R * np.sin(th)))


def _crossing():
    """A 12-point ellipse with point 7 moved onto point 2: a repeated point that is NOT adjacent (a figure-eight crossing).  No chord is
    zero, so the programme is as regular as any: it must solve.  The line turns sharply into and out of the moved point; the ellipse is
    200 x 140 so that l_R kappa stays below 0.5 there too (at 30 x 21 it reaches 2.2 and asin leaves its domain)."""
    th = 2 * np.pi * np.arange(12) / 12
    p = np.column_stack((200.0 * np.cos(th), 140.0 * np.sin(th)))
    p[7] = p[2]
    return p


def _make():
    cs = [Case("n3", _jittered("n3", 3)), Case("n4", _jittered("n4", 4)), Case("n5_cw", _jittered("n5_cw", 5, cw=True)),
          Case("n17", _jittered("n17", 17)), Case("n64", _jittered("n64", 64)), Case("n65_cw", _jittered("n65_cw", 65, cw=True)),
          Case("n182", _jittered("n182", 182, R=120.0)),
          Case("ratio10", _chord_pattern(30, (1, 10, 10))), Case("ratio50", _chord_pattern(30, (1, 50))),
          Case("offset", _jittered("offset", 40, ox=1e4, oy=-2e4)),
          Case("w0", _jittered("w", 40), 0.0), Case("w1e-6", _jittered("w", 40), 1e-6), Case("w1e4", _jittered("w", 40), 1e4),
          Case("circle", _circle(60, 25.0)), Case("crossing", _crossing()),
          # the small rings of the 65-track table shape
          Case("n6", _jittered("n6", 6)), Case("n7", _jittered("n7", 7)), Case("n8", _jittered("n8", 8))]
    for c in cs:
        c.points.setflags(write=False)
    return {c.name: c for c in cs}


CASES = _make()
RAGGED = ("n3", "n4", "n5_cw", "n17", "n64", "n65_cw", "n182", "ratio10")         # one fit_tracks call: max_pts = 182
RINGS = ("n3", "n4", "n5_cw", "n6", "n7", "n8")
N_MANY = 65


def many_tracks():
    """65 centre lines cycling through RINGS, track k scaled by 1 + k / 64 (no two alike: a table built from a neighbour's segments shows)."""
    return [CASES[RINGS[k % len(RINGS)]].points * (1.0 + k / 64.0) for k in range(N_MANY)]


def mirrored(points):
    """Y -> -Y (turns a clockwise line into a counter-clockwise one)."""
    return np.asarray(points) * np.array([1.0, -1.0])


def quarter_turn(points):
    """(X, Y) -> (-Y, X)."""
    p = np.asarray(points)
    return np.column_stack((-p[:, 1], p[:, 0]))


def fit_spline_kkt(points, curv_weight):
    """The programme of oracle/track_np.py solved as one dense KKT system [[P, A'], [A, 0]] (numpy.linalg.solve): a second CPU method beside
    ``fit_spline_nullspace``, from the oracle's own matrices."""
    path = np.asarray(points, dtype=np.float64)
    n = path.shape[0]
    A, ds = OT.continuity_matrix(path)
    P, q = OT.spline_cost(path, ds, curv_weight)
    K = np.block([[P, A.T], [A, np.zeros((3 * n, 3 * n))]])
    sol = np.linalg.solve(K, np.vstack((-q, np.zeros((3 * n, 2)))))
    return sol[:4 * n, 0].reshape(n, 4), sol[:4 * n, 1].reshape(n, 4)


_ORACLE: dict = {}


def oracle_fit(points, curv_weight):
    """``fit_spline_nullspace``, computed once per (points, weight) and shared (read-only) among the tests."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    key = (pts.tobytes(), float(curv_weight))
    if key not in _ORACLE:
        cX, cY = OT.fit_spline_nullspace(pts, curv_weight)
        cX.setflags(write=False); cY.setflags(write=False)
        _ORACLE[key] = (cX, cY)
    return _ORACLE[key]
