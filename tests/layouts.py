"""Seeded constraint layouts of the bicycle OCP, an independent numpy assembly of its RTI QP and a KKT report with soft slacks.

A layout writes the dense arrays of an ``OcpData`` (``lbx/ubx (N+1,8)``, ``lbu/ubu``, per-stage ``C/D/lg/ug``, ``soft_z/soft_Z (N+1,28)``
with ``soft_Z < 0`` for a hard side, optionally a stage-varying ``W``) directly, so that the product (``BatchedOcpSolver._push_bounds``)
and the oracle (``OracleProblem(data.as_dict(...))``) read the same problem.  What it varies is what the QP kernel's slot table
(``csrc/qp_tables.hpp: lay_out_slots``, called by ``api.hip::rebuild_slots``) packs differently: which rows exist per stage, one-sided rows and ``|v| >= 1e20`` as an absent side,
narrow boxes, stage-varying rows and weights, soft sides that are lower / upper only, L1 / L2 only, asymmetric, soft on one side and
hard on the other, track rows, the lateral-acceleration row, and the empty table.

The QP assembly here shares no code with the oracle or the product: H and g from ``cost_scale_stage``, the output selectors and the
weights; R, dl, du from the bounds minus the linearisation point; A, B, b from the caller (the linearisation of either side).  Only
the two nonlinear track rows (and the a_lat row) are taken from ``OracleProblem.build_qp``."""
from __future__ import annotations

import dataclasses

import numpy as np

NX, NU, NZ, NY, NC = 8, 2, 10, 12, 14
BIG = 1e20      # |v| >= 1e20: the side is absent (ihm2mpc_set_bounds, orc_build_qp)

# (lower, upper) of each state box when present: wide enough that a hard box keeps the RTI QPs of sample_x0 feasible
STATE_BOX = ((-50.0, 1e4), (-2.0, 2.0), (-0.9, 0.9), (0.0, 31.0), (-4.0, 4.0), (-4.0, 4.0), (-500.0, 500.0), (-0.5, 0.5))
SOFT_STATE_BOX = ((-50.0, 1e4), (-0.3, 0.3), (-0.05, 0.05), (3.0, 9.0), (-0.2, 0.2), (-0.3, 0.3), (-100.0, 150.0), (-0.1, 0.1))
U_BOX = ((-500.0, 500.0), (-0.5, 0.5))
RATE = ((-1e-3 * 5000.0, 1e-3 * 5000.0), (-0.02 * 1.0, 0.02 * 1.0))      # u - x[6:8] per step: t_T * T_dot_max, t_delta * delta_dot_max


@dataclasses.dataclass
class Layout:
    """Which rows exist per stage and how their sides are treated.  Every random choice comes from ``seed``.

    xbox      "ref" (the reference's [1,3,6,7], terminal [1,3,4,5]), "all", "none", "random" (a random subset per stage) or a tuple of indices
    ubox      input boxes on the stages 0..N-1
    grows     general rows: "ref" (the two rate rows), "none", "stagevary" (the rate rows scaled per stage: C, D differ by stage), "narrow"
              (the torque rate row pinned to a 1e-6 wide band)
    one_sided probability that a present hard row loses one (random) side, written as +-1e20, +-1e25 or +-inf
    soft      rows with soft sides ((row, stage set) pairs are drawn per stage with this probability), 0 = none
    soft_rows the rows that may get soft sides (0..13)
    soft_kind "random" (per side: L1 only, L2 only, both, asymmetric lower / upper, soft lower + hard upper, ...), or one of
              "l1", "l2", "both", "lower", "upper", "mixed"
    stage_W   stage-varying weights (the QP kernel's UNI = 0)
    path      the two track rows (lh = -1e3, uh = 0) on stages 1..N, ``path_soft``: both sides soft (True) or the upper one ("upper")
    alat      the lateral-acceleration row (needs ``path``), +-alat_max, soft with ``alat_soft``"""
    name: str
    N: int = 40
    seed: int = 0
    xbox: object = "ref"
    ubox: bool = True
    grows: str = "ref"
    one_sided: float = 0.0
    soft: float = 0.0
    soft_rows: tuple = (1, 3, 11)
    soft_kind: str = "random"
    stage_W: bool = False
    path: bool = False
    path_soft: bool = False
    alat: bool = False
    alat_soft: bool = False
    alat_max: float = 3.0
    width: float = 1.6


REF_X = (1, 3, 6, 7)
REF_X_E = (1, 3, 4, 5)


def _sides(rng, lo, hi, p_one):
    """(lower, upper) with a side dropped with probability p_one, the absent side written in one of three ways."""
    if rng.random() >= p_one:
        return lo, hi
    absent = (BIG, 1e25, np.inf)[rng.integers(3)]
    return (-absent, hi) if rng.random() < 0.5 else (lo, absent)


def _soft_pen(rng, kind):
    """(z_l, Z_l, z_u, Z_u) of a row; Z < 0 = hard side."""
    a, b, c, d = rng.uniform(5.0, 200.0, 4)
    kinds = ("l1", "l2", "both", "lower", "upper", "mixed", "asym")
    k = kinds[rng.integers(len(kinds))] if kind == "random" else kind
    if k == "l1":
        return a, 0.0, a, 0.0
    if k == "l2":
        return 0.0, b, 0.0, b
    if k == "both":
        return a, b, a, b
    if k == "lower":            # soft lower, upper side hard
        return a, b, 0.0, -1.0
    if k == "upper":
        return 0.0, -1.0, c, d
    if k == "mixed":            # L1-only lower, L2-only upper
        return a, 0.0, 0.0, d
    return a, b, c, d           # asymmetric penalties


def make_arrays(lay: Layout) -> dict:
    """The OcpData arrays of the layout: lbx, ubx, lbu, ubu, C, D, lg, ug, soft_z, soft_Z (None for an all-hard table) and W (None:
    keep the OCP's)."""
    rng = np.random.default_rng(lay.seed)
    N = lay.N
    lbx = np.full((N + 1, NX), -BIG); ubx = np.full((N + 1, NX), BIG)
    lbu = np.full((N, NU), -BIG); ubu = np.full((N, NU), BIG)
    C = np.zeros((N, 2, NX)); D = np.zeros((N, 2, NU)); lg = np.full((N, 2), -BIG); ug = np.full((N, 2), BIG)
    z = np.zeros((N + 1, 2 * NC)); Z = np.full((N + 1, 2 * NC), -1.0)
    soft_any = False
    for k in range(1, N + 1):
        if lay.xbox == "ref":
            idx = REF_X if k < N else REF_X_E
        elif lay.xbox == "all":
            idx = range(NX)
        elif lay.xbox == "none":
            idx = ()
        elif lay.xbox == "random":
            idx = np.flatnonzero(rng.random(NX) < 0.5)
        else:
            idx = lay.xbox
        for i in idx:
            soft_row = lay.soft > 0 and i in lay.soft_rows and rng.random() < lay.soft
            lo, hi = STATE_BOX[i]
            if soft_row:        # a soft side is tight (its slack is used), a hard side keeps the wide value (the QP stays feasible)
                z[k, i], Z[k, i], z[k, NC + i], Z[k, NC + i] = _soft_pen(rng, lay.soft_kind)
                lo = SOFT_STATE_BOX[i][0] if Z[k, i] >= 0 else lo
                hi = SOFT_STATE_BOX[i][1] if Z[k, NC + i] >= 0 else hi
                soft_any = True
            lbx[k, i], ubx[k, i] = _sides(rng, lo, hi, lay.one_sided)
    for k in range(N):
        if lay.ubox:
            for i in range(NU):
                lbu[k, i], ubu[k, i] = _sides(rng, *U_BOX[i], lay.one_sided)
        if lay.grows != "none":
            scale = 1.0 + 0.25 * (k % 3) if lay.grows == "stagevary" else 1.0
            for i in range(2):
                C[k, i, 6 + i] = -scale; D[k, i, i] = scale
                lo, hi = RATE[i]
                if lay.grows == "narrow" and i == 0:
                    lo, hi = 0.0, 1e-6
                lg[k, i], ug[k, i] = _sides(rng, scale * lo, scale * hi, lay.one_sided)
                c = 10 + i
                if lay.soft > 0 and c in lay.soft_rows and rng.random() < lay.soft:
                    z[k, c], Z[k, c], z[k, NC + c], Z[k, NC + c] = _soft_pen(rng, lay.soft_kind)
                    soft_any = True
    if lay.path and lay.path_soft:
        for k in range(1, N + 1):
            for c in (12, 13):
                z[k, NC + c], Z[k, NC + c] = 100.0, 100.0
                if lay.path_soft != "upper":
                    z[k, c], Z[k, c] = 100.0, 100.0
        soft_any = True
    W = None
    if lay.stage_W:
        from ihm2_amd import ocp as O

        W0, _ = O.default_weights()
        d = np.exp(rng.uniform(-0.5, 0.5, (N, NY)))
        W = d[:, :, None] * W0[None] * d[:, None, :]
    return dict(lbx=lbx, ubx=ubx, lbu=lbu, ubu=ubu, C=C, D=D, lg=lg, ug=ug,
                soft_z=z if soft_any else None, soft_Z=Z if soft_any else None, W=W)


# The layouts of tests/test_gpu_qp_layouts.py (which runs them) and tests/test_slot_table.py (which checks their slot tables on the CPU), each
# named for the table it is meant to give.
# name -> (layout, batch size, IHM2MPC_BLOCK_QP); B > 256 (the CU count) or BLOCK_QP = 0 keeps the all-hard tables on k_qp_wave
TABLE = {
    # all-hard tables without track rows: 8 rows per stage (reference layout) -> 8 N slots; 12 per stage with every state box
    "hard_5_per_lane": (Layout("hard_5_per_lane", N=40), 300, "1"),                                   # 320 slots
    "hard_5_per_lane_stage_W": (Layout("hard_5_per_lane_stage_W", N=40, stage_W=True, seed=1), 300, "1"),
    "hard_6_per_lane": (Layout("hard_6_per_lane", N=41), 96, "0"),                                    # 328 slots
    "hard_8_per_lane_stage_rows": (Layout("hard_8_per_lane_stage_rows", N=64, grows="stagevary"), 96, "0"),   # 512
    "hard_9_per_lane": (Layout("hard_9_per_lane", N=65), 65, "0"),                                    # 520
    "hard_10_per_lane_all_boxes": (Layout("hard_10_per_lane_all_boxes", N=53, xbox="all"), 96, "0"),          # 636
    "hard_10_per_lane_stage_W": (Layout("hard_10_per_lane_stage_W", N=53, xbox="all", stage_W=True, seed=2), 96, "0"),
    "hard_random_one_sided": (Layout("hard_random_one_sided", N=40, xbox="random", one_sided=0.5, seed=3), 130, "0"),
    "hard_narrow_rate_row": (Layout("hard_narrow_rate_row", N=40, grows="narrow", seed=4), 96, "0"),
    "empty_table": (Layout("empty_table", N=40, xbox="none", ubox=False, grows="none"), 70, "0"),
    # the four-wave kernel: B <= CU count, BLOCK_QP on; B = 1
    "block_hard": (Layout("block_hard", N=40), 64, "1"),
    "block_hard_B1": (Layout("block_hard_B1", N=40), 1, "1"),
    "block_hard_stage_W": (Layout("block_hard_stage_W", N=40, stage_W=True, seed=5), 33, "1"),
    # soft tables without track rows: <8,2,0> up to 2 soft sides per lane, <10,4,0> up to 4
    "soft_2_per_lane": (Layout("soft_2_per_lane", N=40, soft=1.0, soft_rows=(1,), soft_kind="both", seed=6), 96, "1"),        # 80 soft sides
    "soft_2_per_lane_stage_W": (Layout("soft_2_per_lane_stage_W", N=40, soft=1.0, soft_rows=(1,), soft_kind="lower", stage_W=True, seed=7), 96, "1"),
    # two rows soft on one side and hard on the other in one lane: their soft halves must lead the lane ([s, s, h, h], not [s, h, s, h])
    "soft_2_per_lane_split_rows": (Layout("soft_2_per_lane_split_rows", N=40, soft=1.0, soft_rows=(1, 3), soft_kind="lower", seed=17), 96, "1"),
    "soft_3_per_lane_asym": (Layout("soft_3_per_lane_asym", N=40, soft=1.0, soft_rows=(1, 3), soft_kind="asym", seed=8), 96, "1"),   # 160
    "soft_4_per_lane_mixed": (Layout("soft_4_per_lane_mixed", N=40, soft=1.0, soft_rows=(1, 3, 11), soft_kind="random", seed=9), 130, "1"),
    "soft_4_per_lane_stage_rows": (Layout("soft_4_per_lane_stage_rows", N=40, soft=1.0, soft_rows=(1, 3), grows="stagevary", seed=10), 96, "1"),
    "soft_one_sided_rows_padding": (Layout("soft_one_sided_rows_padding", N=40, xbox="all", one_sided=0.6, soft=0.4, soft_rows=(1, 4), seed=11), 96, "1"),
    # track rows: <8,0,1> all hard, <8,3,1> up to 3 soft sides per lane, <10,4,1> up to 4
    "path_hard": (Layout("path_hard", N=40, path=True), 96, "1"),
    "path_hard_stage_W": (Layout("path_hard_stage_W", N=40, path=True, stage_W=True, seed=12), 96, "1"),
    "path_soft_3_per_lane": (Layout("path_soft_3_per_lane", N=40, path=True, path_soft="upper", ubox=False, width=1.2), 96, "1"),       # 80
    "path_soft_3_per_lane_stage_W": (Layout("path_soft_3_per_lane_stage_W", N=40, path=True, path_soft="upper", ubox=False, width=1.2, stage_W=True, seed=13), 96, "1"),
    "path_soft_both_sides": (Layout("path_soft_both_sides", N=40, path=True, path_soft=True, width=1.2), 96, "1"),       # 160
    "path_soft_4_per_lane": (Layout("path_soft_4_per_lane", N=40, path=True, path_soft=True, soft=1.0, soft_rows=(3,), soft_kind="lower", width=1.2, seed=14), 96, "1"),
    "path_soft_4_per_lane_stage_W": (Layout("path_soft_4_per_lane_stage_W", N=40, path=True, path_soft=True, soft=1.0, soft_rows=(3,), soft_kind="upper", width=1.2, stage_W=True, seed=15), 96, "1"),
    # the lateral-acceleration row
    "alat_hard": (Layout("alat_hard", N=40, path=True, alat=True, alat_max=4.5), 96, "1"),
    "alat_soft": (Layout("alat_soft", N=40, path=True, alat=True, path_soft=True, alat_soft=True, alat_max=2.5, width=1.2), 96, "1"),
}
# past a limit: refused by ready() (reported by the first call that needs the table)
REFUSED = {
    "hard_11_per_lane": Layout("hard_11_per_lane", N=54, xbox="all"),                                   # 648 slots
    "soft_5_per_lane": Layout("soft_5_per_lane", N=40, soft=1.0, soft_rows=(1, 3, 6, 7), soft_kind="both", seed=16),      # 320 soft sides: 5 per lane
    # all-hard tables with track rows: <8,0,1> and <8,0,2> take at most 8 slots per lane
    "path_hard_9_per_lane": Layout("path_hard_9_per_lane", N=40, path=True, xbox="all"),                 # 560 slots
    "alat_hard_10_per_lane": Layout("alat_hard_10_per_lane", N=40, path=True, alat=True, alat_max=10.0, xbox="all"),    # 599 slots
}


def make_ocp(lay: Layout, **opts):
    """The OCP the layout edits: the reference's (conftest.make_ocp), with the track rows / a_lat row switched on as asked.  ``opts``
    go to conftest.make_ocp: ``model``, ``M`` and the solver options (integrator, SQP mode, line search)."""
    from conftest import make_ocp as base

    ocp = base(N=lay.N, **opts)
    if lay.path:
        ocp.model.con_h_expr = "track+a_lat" if lay.alat else "track"
        c = ocp.constraints
        c.lh = np.array([-1e3, -1e3, -lay.alat_max][:2 + lay.alat]); c.uh = np.array([0.0, 0.0, lay.alat_max][:2 + lay.alat])
        c.lh_e = np.array([-1e3, -1e3]); c.uh_e = np.array([0.0, 0.0])
        if lay.alat and lay.alat_soft:
            c.idxsh = np.array([2])
            ocp.cost.zl = ocp.cost.zu = ocp.cost.Zl = ocp.cost.Zu = np.array([100.0])
    return ocp


def apply(data, lay: Layout) -> dict:
    """Writes the layout's arrays onto an OcpData (``solver.data`` or ``ocp.flatten()``) in place; returns them."""
    arr = make_arrays(lay)
    for name in ("lbx", "ubx", "lbu", "ubu", "C", "D", "lg", "ug"):
        setattr(data, name, arr[name])
    data.soft_z, data.soft_Z = arr["soft_z"], arr["soft_Z"]
    if arr["W"] is not None:
        data.W = arr["W"]
    return arr


def track_widths(lay: Layout):
    return np.array([[lay.width, lay.width - 0.1]]) if lay.path else None


# ---- independent assembly of the RTI QP ----

def selectors():
    """y = Vx x + Vu u = [x; u; x[6:8] - u] (the reference's LINEAR_LS output), as one (12, 10) matrix on z = (x, u)."""
    V = np.zeros((NY, NZ))
    V[:NX, :NX] = np.eye(NX)
    V[NX:NX + NU, NX:] = np.eye(NU)
    V[NX + NU:, 6:8] = np.eye(NU); V[NX + NU:, NX:] = -np.eye(NU)
    return V


def assemble_qp(data, x, u, x0, yref, yref_e, A, Bm, b, nonlinear=None):
    """The RTI QP of one instance at the linearisation point (x, u): H, g, A, Bm, b, dx0, R (N+1,14,10), dl, du (bounds minus the row's
    value; -+inf = absent).  ``nonlinear``: a build_qp dict whose rows 12.. (track rows, a_lat row) are copied in -- those rows are
    nonlinear in x and are not restated here."""
    N = data.N
    V = selectors()
    cs = data.cost_scale_stage
    W = np.asarray(data.W)
    H = np.zeros((N + 1, NZ, NZ)); g = np.zeros((N + 1, NZ))
    for k in range(N):
        zk = np.concatenate([x[k], u[k]])
        H[k] = cs * V.T @ W[k] @ V
        g[k] = cs * V.T @ W[k] @ (V @ zk - yref[k])
    H[N, :NX, :NX] = data.W_e; H[N, NX:, NX:] = np.eye(NU)
    g[N, :NX] = np.asarray(data.W_e) @ (x[N] - yref_e)
    nc = NC if nonlinear is None else nonlinear["R"].shape[1]
    R = np.zeros((N + 1, nc, NZ)); dl = np.full((N + 1, nc), -np.inf); du = np.full((N + 1, nc), np.inf)

    def side(v, val, lower):
        if abs(v) >= BIG:
            return -np.inf if lower else np.inf
        return v - val

    for k in range(N + 1):
        if k >= 1:
            for i in range(NX):
                R[k, i, i] = 1.0
                dl[k, i] = side(data.lbx[k, i], x[k, i], True); du[k, i] = side(data.ubx[k, i], x[k, i], False)
        if k < N:
            for i in range(NU):
                R[k, 8 + i, 8 + i] = 1.0
                dl[k, 8 + i] = side(data.lbu[k, i], u[k, i], True); du[k, 8 + i] = side(data.ubu[k, i], u[k, i], False)
            for i in range(2):
                R[k, 10 + i, :NX] = data.C[k, i]; R[k, 10 + i, NX:] = data.D[k, i]
                val = data.C[k, i] @ x[k] + data.D[k, i] @ u[k]
                dl[k, 10 + i] = side(data.lg[k, i], val, True); du[k, 10 + i] = side(data.ug[k, i], val, False)
    if nonlinear is not None:
        R[:, 12:] = nonlinear["R"][:, 12:]; dl[:, 12:] = nonlinear["dl"][:, 12:]; du[:, 12:] = nonlinear["du"][:, 12:]
    return dict(H=H, g=g, A=A, Bm=Bm, b=b, dx0=x0 - x[0], R=R, dl=dl, du=du)


def soft_arrays(data, nc=NC, alat_soft=None):
    """(soft_z, soft_Z) as (N+1, 2 nc) with the sides of the a_lat row appended (nc = 15) where present."""
    N = data.N
    z = np.zeros((N + 1, 2 * NC)) if data.soft_z is None else np.asarray(data.soft_z, dtype=np.float64)
    Z = np.full((N + 1, 2 * NC), -1.0) if data.soft_Z is None else np.asarray(data.soft_Z, dtype=np.float64)
    if nc == NC:
        return z, Z
    az = np.zeros((N + 1, 2)); aZ = np.full((N + 1, 2), -1.0)
    if alat_soft is not None:
        az[1:N], aZ[1:N] = alat_soft
    return (np.concatenate([z[:, :NC], az[:, :1], z[:, NC:], az[:, 1:]], 1),
            np.concatenate([Z[:, :NC], aZ[:, :1], Z[:, NC:], aZ[:, 1:]], 1))


def kkt_report(qp, dz, pi, lam, sl, soft_z, soft_Z):
    """KKT residuals of the QP with soft sides at (dz, pi, lam, sl), each an inf-norm:

    stat  H z + g + [A B]' pi_{k+1} - pi_k - R' (lam_l - lam_u) on the free components (not x_0, not u_N)
    eq    z_0 = dx0 and [A B] z_k + b_k = x_{k+1}
    ineq  violation of R z + s >= dl, du + s >= R z (s = 0 for a hard side) and of s >= 0
    comp  |lam (R z + s - dl)| over the sides, |(z + Z s - lam) s| over the soft sides (the slack's own multiplier times the slack)
    dual  violation of lam >= 0 and, on soft sides, of lam <= z + Z s (the slack's stationarity z + Z s - lam - lam_s = 0, lam_s >= 0)
    lam_min  the smallest multiplier of a present side (an interior point keeps them >= 0)
    absent the largest |lam| of a side that does not exist (must be exactly 0)
    Sides are the columns of lam: nc lower then nc upper."""
    N = qp["A"].shape[0]
    nc = qp["R"].shape[1]
    stat = 0.0; eq = float(np.max(np.abs(dz[0, :NX] - qp["dx0"]))); ineq = 0.0; comp = 0.0; dual = 0.0
    lam_l, lam_u = lam[:, :nc], lam[:, nc:]
    for k in range(N + 1):
        r = qp["H"][k] @ dz[k] + qp["g"][k] - qp["R"][k].T @ (lam_l[k] - lam_u[k])
        if k < N:
            AB = np.hstack([qp["A"][k], qp["Bm"][k]])
            r += AB.T @ pi[k + 1]
            eq = max(eq, float(np.max(np.abs(AB @ dz[k] + qp["b"][k] - dz[k + 1, :NX]))))
        r[:NX] -= pi[k]
        lo, hi = (NX if k == 0 else 0), (NZ if k < N else NX)
        stat = max(stat, float(np.max(np.abs(r[lo:hi]))))
    Rz = np.einsum("kcj,kj->kc", qp["R"], dz)
    gap = np.concatenate([Rz - qp["dl"], qp["du"] - Rz], 1)          # >= 0 where the side holds without slack
    present = np.isfinite(gap)
    soft = present & (soft_Z >= 0.0)
    s = np.where(soft, sl, 0.0)
    g2 = np.where(present, gap, 0.0) + s
    ineq = max(ineq, float(np.max(np.where(present, -g2, 0.0), initial=0.0)), float(np.max(np.where(soft, -s, 0.0), initial=0.0)))
    comp = max(comp, float(np.max(np.abs(np.where(present, lam * g2, 0.0)), initial=0.0)))
    cap = soft_z + soft_Z * s
    comp = max(comp, float(np.max(np.abs(np.where(soft, (cap - lam) * s, 0.0)), initial=0.0)))
    dual = max(float(np.max(np.where(present, -lam, 0.0), initial=0.0)), float(np.max(np.where(soft, lam - cap, 0.0), initial=0.0)))
    lam_min = float(np.min(np.where(present, lam, 0.0), initial=0.0))
    absent = float(np.max(np.abs(np.where(present, 0.0, lam)), initial=0.0))
    return dict(stat=stat, eq=eq, ineq=ineq, comp=comp, dual=dual, lam_min=lam_min, absent=absent)


def scales(qp):
    """(sg, sb): the scales the interior-point tolerances are relative to -- gradient for stationarity / complementarity, dynamics
    data for equality / inequality (test_oracle_qp.py::test_nmpc_qp_kkt_and_iteration_count)."""
    N = qp["A"].shape[0]
    g = qp["g"].copy(); g[N, NX:] = 0.0
    sg = max(1.0, float(np.abs(g).max())); sb = max(1.0, float(np.abs(qp["b"]).max()), float(np.abs(qp["dx0"]).max()))
    return sg, sb
