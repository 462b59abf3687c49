"""Two-track cases: one handle (and one OracleProblem) that holds the tables of two tracks, instance b on track b mod 2, with widths
that differ per track.  A helper: tests/test_oracle_multi_track.py carries the conditions on these inputs without a GPU,
tests/test_gpu_multi_track.py runs every kernel that reads track_id on them.

With one track track_id[b] is 0 for every instance, and an index written as b, 0 or trk without its * 2, a widths pointer of another
launch or the lap length of the wrong track all give the right answer.  Here they do not: the two lap lengths differ by 122 m, the
curvature tables are those of two different circuits, and the corridor widths differ in both columns and are not symmetric, so that
[trk * 2 + 1] of one track is no entry of the other.

    TRACKS    fsds_competition_1 (L = 340.209 m) and fsds_competition_2 (L = 462.351 m), both tables of 1500 knots: they stack
    W_SOFT    (right, left) per track on the layouts with soft track rows; row 0 is layouts.track_widths of those layouts (width 1.2)
    W_HARD    the same on the layouts with hard track rows; row 0 is layouts.track_widths at the default width 1.6
    x0        per track t: drive.clipped_start(plan_t, n_t, 900 + layout seed + t)
    yref      the ramp of tests/test_gpu_qp_layouts.py::_start"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import drive
import layouts as L

TRACKS = ("fsds_competition_1", "fsds_competition_2")
W_SOFT = np.array([[1.2, 1.1], [0.9, 1.4]])
W_HARD = np.array([[1.6, 1.5], [1.0, 1.8]])
BLIND_FACTOR = 10.0                     # the blind reference (track_id = 0 for everybody) must be this many tolerances away


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    layout: str         # key of layouts.TABLE
    B: int
    block: str          # IHM2MPC_BLOCK_QP of the handle
    kernel: str         # the launch record's qp

    @property
    def lay(self):
        return L.TABLE[self.layout][0]

    @property
    def track_id(self):
        return track_ids(self.B)

    @property
    def widths(self):
        return widths(self.lay)

    @property
    def seed(self):
        return 900 + self.lay.seed


# The catalogue has no four-wave kernel with track rows (csrc/qp_catalogue.hpp: QP_KEY_BLOCK has PATH = 0, and qp_select.hpp finds no
# entry), so path_hard with IHM2MPC_BLOCK_QP=1 at B <= CU count stays on k_qp_wave<8,0,1,1>: the case is kept with the name the selection
# gives, and k_qp_block itself runs on per-instance track ids on the all-hard table it takes (block_hard: the linearisation in front of it
# reads each instance's curvature table).
CASES = {c.name: c for c in (
    Case("path_hard", "path_hard", 8, "0", "k_qp_wave<8,0,1,1>"),
    Case("path_soft_both_sides", "path_soft_both_sides", 8, "0", "k_qp_wave<10,4,1,1>"),
    Case("path_soft_4_per_lane", "path_soft_4_per_lane", 8, "0", "k_qp_wave<10,4,1,1>"),
    Case("alat_soft", "alat_soft", 8, "0", "k_qp_wave<10,4,2,1>"),
    Case("alat_hard", "alat_hard", 8, "0", "k_qp_wave<8,0,2,1>"),
    Case("path_hard_block_qp", "path_hard", 8, "1", "k_qp_wave<8,0,1,1>"),
    Case("block_hard", "block_hard", 8, "1", "k_qp_block<2,1,4>"),
    Case("path_soft_both_sides_ragged", "path_soft_both_sides", 67, "0", "k_qp_wave<10,4,1,1>"),
)}
TRACK_ROW_CASES = [n for n, c in CASES.items() if c.lay.path]
SOFT_CASES = [n for n in TRACK_ROW_CASES if CASES[n].lay.path_soft]


@functools.lru_cache(maxsize=None)
def plans():
    from ihm2_amd.track import track_table

    return tuple(track_table(n) for n in TRACKS)


def tables():
    """(s_ref, kappa_ref), each (2, nknots)."""
    p = plans()
    return np.stack([t.s_ref for t in p]), np.stack([t.kappa_ref for t in p])


def lap_lengths():
    return np.array([t.lap_length for t in plans()])


def track_ids(B):
    return (np.arange(B) % 2).astype(np.int32)


def widths(lay):
    return None if not lay.path else (W_SOFT if lay.path_soft else W_HARD).copy()


def start_arrays(lay, B, seed, lead=40.0, tid=None):
    """(x0, yref, yref_e): per track the clipped start of that track's own table, seed + t; the ramp of test_gpu_qp_layouts._start."""
    tid = track_ids(B) if tid is None else np.asarray(tid)
    x0 = np.zeros((B, 8))
    for t, plan in enumerate(plans()):
        sel = tid == t
        if sel.any():
            x0[sel] = drive.clipped_start(plan, int(sel.sum()), seed + t)
    N = lay.N
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + lead * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = x0[:, 0] + lead
    return x0, yref, yref_e


def oracle_problem(data, lay, w=None):
    """The OracleProblem of a handle's (or a flattened OCP's) data on both tables, with both rows of the widths."""
    from oracle import oracle as orc

    s_ref, k_ref = tables()
    return orc.OracleProblem(data.as_dict(s_ref, k_ref, track_widths=widths(lay) if w is None else w))


def flat_data(lay):
    """The OcpData of the layout without a handle (the CPU tests)."""
    data = L.make_ocp(lay).flatten()
    L.apply(data, lay)
    return data


def stanley_guess(data, lay, x0, tid):
    """orc.stanley_guess per track, each on a problem that holds that track's table alone."""
    from oracle import oracle as orc

    s_ref, k_ref = tables()
    B, N = x0.shape[0], lay.N
    x = np.zeros((B, N + 1, 8)); u = np.zeros((B, N, 2))
    w = widths(lay)
    for t in range(2):
        sel = tid == t
        if sel.any():
            P = orc.OracleProblem(data.as_dict(s_ref[t], k_ref[t], track_widths=None if w is None else w[t:t + 1]))
            x[sel], u[sel] = orc.stanley_guess(P, s_ref[t], k_ref[t], x0[sel], N)
    return x, u


def solver(case, build="default", track_id=None, **opts):
    """A BatchedOcpSolver on both tables with track_id= and track_widths= of shape (2, 2), the layout applied as
    tests/test_gpu_qp_layouts.py::_solver does.  ``opts`` go to layouts.make_ocp."""
    from ihm2_amd.solver import BatchedOcpSolver
    from test_gpu_configs import _build
    from test_gpu_qp_layouts import _block_qp

    lay = case.lay
    s_ref, k_ref = tables()
    with _build(build), _block_qp(case.block):
        s = BatchedOcpSolver(L.make_ocp(lay, **opts), case.B, s_ref, k_ref, track_id=case.track_id if track_id is None else track_id,
                             track_widths=widths(lay))
    arr = L.apply(s.data, lay)
    if arr["W"] is not None:
        s._push_weights()
    s._push_bounds()
    return s


def start(s, case, x0=None, yref=None, yref_e=None):
    """x0, the device's guess, the ramp and zero multipliers, as test_gpu_qp_layouts._start sets them; given arrays are used as they are."""
    if x0 is None:
        x0, yref, yref_e = start_arrays(case.lay, case.B, case.seed)
    s.set_x0(x0); s.init_guess()
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
    return x0, yref, yref_e


def blind_rows(qp, P, xbar, ubar, x0, yref, yref_e):
    """The QP with its track rows (and a_lat row) as a reference that took track 0's widths for every instance would have them."""
    other = P.build_qp(xbar, ubar, x0, yref, yref_e, track_id=0)
    blind = dict(qp)
    for k in ("R", "dl", "du"):
        blind[k] = np.array(qp[k]); blind[k][:, 12:] = other[k][:, 12:]
    return blind


def sens_distance(ax, au, bx, bu, rx, ru):
    """(stage 0, horizon): the distance of the sensitivity results a and b in the measure of
    test_gpu_sensitivity._check_against_reference -- of the largest entry of the instance's own (true) reference r, whichever two are compared."""
    scale = max(np.abs(rx).max(), np.abs(ru).max())
    return float(np.abs(bu[0] - au[0]).max() / scale), float(max(np.abs(bu - au).max(), np.abs(bx - ax).max()) / scale)


def discriminates(d0, d):
    """A (stage 0, horizon) distance that the comparison of test_gpu_sensitivity._check_against_reference could not miss."""
    from test_gpu_sensitivity import TOL_HORIZON, TOL_STAGE0

    return d0 >= BLIND_FACTOR * TOL_STAGE0 and d >= BLIND_FACTOR * TOL_HORIZON


# ---- the lap wrap: starts on the two tables ----
WRAP_B, WRAP_VX, WRAP_STEPS = 8, 10.0, 24
# (track, distance in front of that track's own lap length) of the cars that cross; (track, distance behind L0) of the cars on the longer
# track that sit between the two lap lengths and must never wrap; two cars on the shorter track in mid-lap fill the batch
WRAP_CROSS = ((0, 4.0), (0, 9.0), (1, 4.0), (1, 9.0))
WRAP_BETWEEN = (30.0, 60.0)
WRAP_MID = (100.0, 150.0)


def wrap_start():
    """(x0, track_id): rows 0..3 cross their own L_t, rows 4, 5 are on track 1 at L0 + 30 and L0 + 60, rows 6, 7 on track 0 in mid-lap."""
    from ihm2_amd.constants import l_R

    Ls = lap_lengths()
    tid = np.array([t for t, _ in WRAP_CROSS] + [1, 1, 0, 0], dtype=np.int32)
    s0 = np.array([Ls[t] - d for t, d in WRAP_CROSS] + [Ls[0] + d for d in WRAP_BETWEEN] + list(WRAP_MID))
    s_ref, k_ref = tables()
    kap = np.array([np.interp(s, s_ref[t], k_ref[t]) for s, t in zip(s0, tid)])
    x0 = np.zeros((WRAP_B, 8))
    x0[:, 0], x0[:, 3] = s0, WRAP_VX
    x0[:, 5] = WRAP_VX * kap
    x0[:, 7] = np.arctan(2 * np.tan(np.arcsin(np.clip(kap * l_R, -0.9, 0.9))))
    return x0, tid
