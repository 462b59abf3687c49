"""float64 reference of the Stanley warm start (``ihm2mpc_init_guess``) and of the recovery of failed instances
(``ihm2mpc_reinit_failed``), and the recovery contract as a function.

Both entry points run ``kernels_misc.hip::k_init_guess``; this module restates what its comments and the reference's controller
(``python/main.py:139-163``: ``StanleyController.compute_control``, torque P-term only) say, not its arithmetic:

* feedback at stage ``k`` from the rolled-out state ``x_k``:  ``u_T = 90 (v_ref - v_x)`` with ``v_ref = v_ref_scale * x0[3]``, and
  ``u_delta = atan(2 tan(asin(clip(kappa(s) l_R, +-0.9)))) - 1.8 psi - atan(5.5 n / (2 + v_x))``;
* each input clamped to the intersection of its box ``[lbu, ubu]`` and its rate row ``[x_act + lg, x_act + ug]`` around the current
  actuator state (``T`` for ``u_T``, ``delta`` for ``u_delta``), with the instance's own tables when per-instance bounds are set;
* normal mode: RK4 of the OCP's model where it is usable as a simulator (``fdyn6u``), of ``fkin6`` otherwise (``fkin6``, and ``fdyn6`` as
  written, open-loop unstable over the horizon), with ``M`` sub-steps for ERK and ``max(25, ceil(dt / 2 ms))`` for IRK -- the step is
  the C oracle's RK4 (``OracleProblem.sim_step``);
* recovery: ``fkin6`` whatever the OCP's model, ``max(4, ceil(dt / 12.5 ms))`` sub-steps, RK4 on the first six states and the two
  actuator lags in closed form (numpy on ``oracle/models_np.fkin6``, independent of the C oracle);
* recovery contract: the instances whose status is neither 0 nor 2 get that rollout from their current ``x0`` and zero ``pi``, ``lam``,
  ``slk`` and a_lat multipliers / slacks; every other instance keeps all of it."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from oracle import models_np as mnp

NX, NU = 8, 2
MODEL_FKIN6, MODEL_FDYN6, MODEL_FDYN6U = 0, 1, 2          # IHM2MPC_MODEL_*
INTEG_ERK = 0                                            # IHM2MPC_INTEG_ERK; anything else is an IRK
KEEP_STATUS = (0, 2)                                     # solved, and SQP max-iter (python/main.py:326): not re-initialised
LAG_TAU = (mnp.t_T, mnp.t_delta)                         # the two actuator lags T' = (u_T - T) / t_T, delta' = (u_delta - delta) / t_delta
RK4_STAGES = ((0.0, 1.0 / 6.0), (0.5, 2.0 / 6.0), (0.5, 2.0 / 6.0), (1.0, 1.0 / 6.0))     # (c, b) of the classical tableau


@dataclasses.dataclass
class RolloutProblem:
    """What the rollout of one batch reads.  ``lbu, ubu, lg, ug``: ``(N, 2)`` batch-shared or ``(B, N, 2)`` per instance."""
    N: int
    dt: float
    M: int
    integrator: int
    model: int
    s_ref: np.ndarray           # (ntracks, nknots)
    kappa_ref: np.ndarray
    track_id: np.ndarray        # (B,)
    lbu: np.ndarray
    ubu: np.ndarray
    lg: np.ndarray
    ug: np.ndarray

    @classmethod
    def from_data(cls, data, s_ref, kappa_ref, track_id, inst_bounds=None):
        """From an ``OcpData`` (shared bounds), or with ``inst_bounds`` = the dict given to ``set_instance_bounds``."""
        s_ref, kappa_ref = np.atleast_2d(s_ref), np.atleast_2d(kappa_ref)
        src = data.__dict__ if inst_bounds is None else inst_bounds
        return cls(N=data.N, dt=data.dt, M=data.M, integrator=data.integrator, model=data.model, s_ref=s_ref, kappa_ref=kappa_ref,
                   track_id=np.asarray(track_id, dtype=np.int32),
                   **{k: np.asarray(src[k], dtype=np.float64) for k in ("lbu", "ubu", "lg", "ug")})

    def clamp_tables(self, idx, k):
        """``(lbu, ubu, lg, ug)`` of stage ``k`` for the instances ``idx``, ``(len(idx), 2)`` each."""
        out = []
        for a in (self.lbu, self.ubu, self.lg, self.ug):
            out.append(np.broadcast_to(a[k], (len(idx), NU)) if a.ndim == 2 else a[idx, k])
        return out


def substeps(P: RolloutProblem, recovery: bool) -> int:
    if recovery:
        return max(4, math.ceil(P.dt / 12.5e-3))
    return P.M if P.integrator == INTEG_ERK else max(25, math.ceil(P.dt / 2e-3))


def rollout_model(P: RolloutProblem, recovery: bool) -> int:
    return MODEL_FDYN6U if (P.model == MODEL_FDYN6U and not recovery) else MODEL_FKIN6


def kappa(s, s_ref, kappa_ref):
    """The curvature table as the models read it: linear between knots, linearly extrapolated outside (``models_np.kappa_interp``)."""
    return mnp.kappa_interp(s, s_ref, kappa_ref)


def feedback(x, x0, v_ref_scale, kap, lbu, ubu, lg, ug):
    """Stanley inputs ``(B, 2)`` at states ``x (B, 8)``, clamped to box and rate row."""
    u_T = 90.0 * (v_ref_scale * x0[:, 3] - x[:, 3])
    u_d = (np.arctan(2.0 * np.tan(np.arcsin(np.clip(kap * mnp.l_R, -0.9, 0.9)))) - 1.8 * x[:, 2]
           - np.arctan(5.5 * x[:, 1] / (2.0 + x[:, 3])))
    u = np.stack([u_T, u_d], 1)
    lo = np.maximum(lbu, x[:, 6:8] + lg)
    hi = np.minimum(ubu, x[:, 6:8] + ug)
    return np.minimum(np.maximum(u, lo), hi)


def lag_exact(x_act, u, t):
    """The actuator states after time ``t`` on a constant input: the exact solution of ``a' = (u - a) / tau`` (``x_act, u``: (B, 2))."""
    return u + (x_act - u) * np.exp(-t / np.asarray(LAG_TAU))


def _fkin6(X, U, s_ref, kappa_ref):
    return mnp.fkin6(X.T, U.T, s_ref, kappa_ref).T


def rk4_substep(x, u, h, s_ref, kappa_ref, exact_lags):
    """One RK4 sub-step of ``fkin6`` for a batch on one track.  ``exact_lags``: the stages and the result take the two actuator states in
    closed form at the stage times ``c h``, and RK4 integrates the first six states only."""
    K = np.zeros_like(x)
    acc = x.copy()
    for c, b in RK4_STAGES:
        X = x + (c * h) * K
        if exact_lags:
            X[:, 6:8] = lag_exact(x[:, 6:8], u, c * h)
        K = _fkin6(X, u, s_ref, kappa_ref)
        acc = acc + (b * h) * K
    if exact_lags:
        acc[:, 6:8] = lag_exact(x[:, 6:8], u, h)
    return acc


def _stanley_at(P, idx, k, xk, x0, v_ref_scale):
    kap = np.empty(len(idx))
    for t in np.unique(P.track_id[idx]):
        m = P.track_id[idx] == t
        kap[m] = kappa(xk[m, 0], P.s_ref[t], P.kappa_ref[t])
    return feedback(xk, x0, v_ref_scale, kap, *P.clamp_tables(idx, k))


def stanley_input(P: RolloutProblem, x, x0, v_ref_scale=1.0, idx=None, k=0):
    """``u_k`` of the instances ``idx`` from their states ``x`` (``(len(idx), 8)``) at stage ``k``."""
    idx = np.arange(len(x)) if idx is None else np.asarray(idx)
    return _stanley_at(P, idx, k, np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64), v_ref_scale)


def interval(P: RolloutProblem, x, u, recovery, idx=None, oracle=None):
    """``x_{k+1}`` from ``x_k`` under ``u_k`` over one shooting interval.  Normal mode: the C oracle's RK4 (``oracle`` = an
    ``OracleProblem`` of the same ``dt``); recovery: the closed-form-lag RK4 in numpy."""
    idx = np.arange(len(x)) if idx is None else np.asarray(idx)
    x = np.ascontiguousarray(x, dtype=np.float64); u = np.ascontiguousarray(u, dtype=np.float64)
    M = substeps(P, recovery)
    if not recovery:
        return oracle.sim_step(x, u, rollout_model(P, False), M, track_id=P.track_id[idx])
    out = np.empty_like(x)
    h = P.dt / M
    for t in np.unique(P.track_id[idx]):
        m = P.track_id[idx] == t
        xm, um = x[m], u[m]
        for _ in range(M):
            xm = rk4_substep(xm, um, h, P.s_ref[t], P.kappa_ref[t], True)
        out[m] = xm
    return out


def rollout(P: RolloutProblem, x0, v_ref_scale=1.0, recovery=False, idx=None, oracle=None):
    """The whole warm start of the instances ``idx`` (default: all) from their ``x0 (n, 8)`` alone: ``x (n, N+1, 8)``, ``u (n, N, 2)``."""
    x0 = np.asarray(x0, dtype=np.float64)
    idx = np.arange(len(x0)) if idx is None else np.asarray(idx)
    assert len(idx) == len(x0)
    x = np.zeros((len(idx), P.N + 1, NX)); u = np.zeros((len(idx), P.N, NU))
    x[:, 0] = x0
    for k in range(P.N):
        u[:, k] = _stanley_at(P, idx, k, x[:, k], x0, v_ref_scale)
        x[:, k + 1] = interval(P, x[:, k], u[:, k], recovery, idx, oracle)
    return x, u


def rk4_rollout_plain(P: RolloutProblem, x0, u, M, idx=None):
    """Classical RK4 of all eight ``fkin6`` states, ``M`` sub-steps per interval, under the given inputs ``u (n, N, 2)``."""
    idx = np.arange(len(x0)) if idx is None else np.asarray(idx)
    x = np.zeros((len(idx), u.shape[1] + 1, NX)); x[:, 0] = x0
    h = P.dt / M
    for t in np.unique(P.track_id[idx]):
        m = P.track_id[idx] == t
        for k in range(u.shape[1]):
            xm = x[m, k]
            for _ in range(M):
                xm = rk4_substep(xm, u[m, k], h, P.s_ref[t], P.kappa_ref[t], False)
            x[m, k + 1] = xm
    return x


def regular(P: RolloutProblem, x, idx=None, margin=0.5):
    """Per instance: the rollout ``x (n, N+1, 8)`` stays where the Frenet frame is regular, ``|kappa(s) n| <= margin`` at every stage.
    A car that leaves it (a Stanley rollout can run off the track; ``s' = ... / (1 + kappa n)`` then crosses its pole) turns every
    rounding difference into an O(1) one: its comparison says nothing about the kernel."""
    idx = np.arange(len(x)) if idx is None else np.asarray(idx)
    kn = np.empty(x.shape[:2])
    for t in np.unique(P.track_id[idx]):
        m = P.track_id[idx] == t
        kn[m] = kappa(x[m, :, 0], P.s_ref[t], P.kappa_ref[t]) * x[m, :, 1]
    return np.all(np.abs(kn) <= margin, axis=1)


def well_posed(P: RolloutProblem, x0, xr, v_ref_scale=1.0, recovery=False, idx=None, oracle=None, gain_max=1e6):
    """Per instance: its reference rollout ``xr`` is ``regular`` and amplifies a relative change of 1e-10 in ``x0`` by at most
    ``gain_max`` -- a rollout that spins or runs off the track amplifies rounding alike, and two correct statements of it differ in
    O(1) digits there."""
    x1, _ = rollout(P, np.asarray(x0) * (1.0 + 1e-10), v_ref_scale, recovery, idx, oracle)
    gain = np.max(np.abs(x1 - xr) / (1.0 + np.abs(xr)), axis=(1, 2)) / 1e-10
    return regular(P, xr, idx) & (gain <= gain_max)


def tight_bounds(data, B, seed):
    """Per-instance tables (``set_instance_bounds`` arguments) whose clamps bind: narrow input boxes and rate rows, the shared table's
    finite sides kept, the state boxes the shared ones."""
    rng = np.random.default_rng(seed)
    lbu = np.tile(data.lbu, (B, 1, 1)); ubu = np.tile(data.ubu, (B, 1, 1))
    lg = np.tile(data.lg, (B, 1, 1)); ug = np.tile(data.ug, (B, 1, 1))
    lbu[:, :, 0] = -rng.uniform(20, 200, (B, 1)); ubu[:, :, 0] = rng.uniform(20, 200, (B, 1))
    lbu[:, :, 1] = -rng.uniform(0.2, 0.45, (B, 1)); ubu[:, :, 1] = rng.uniform(0.2, 0.45, (B, 1))
    lg[:, :, 0] = -rng.uniform(5, 60, (B, data.N)); ug[:, :, 0] = rng.uniform(5, 60, (B, data.N))
    lg[:, :, 1] = -rng.uniform(0.008, 0.02, (B, data.N)); ug[:, :, 1] = rng.uniform(0.008, 0.02, (B, data.N))
    return dict(lbx=np.tile(data.lbx, (B, 1, 1)), ubx=np.tile(data.ubx, (B, 1, 1)), lbu=lbu, ubu=ubu, lg=lg, ug=ug)


STATE_FIELDS = ("x", "u", "pi", "lam", "slk", "lam_a", "slk_a")
CLEARED_FIELDS = ("pi", "lam", "slk", "lam_a", "slk_a")


def recovered(status):
    """The instances ``ihm2mpc_reinit_failed`` re-initialises: status neither 0 nor 2."""
    return ~np.isin(np.asarray(status), KEEP_STATUS)


def expected_after_recovery(P: RolloutProblem, before: dict, status, x0, v_ref_scale=1.0):
    """The recovery contract: the batch state after ``reinit_failed`` from the state ``before`` (``STATE_FIELDS`` -> ``(B, ...)``)
    and the statuses of the last solve.  Returns ``(expected, sel)``: kept instances hold ``before`` bit for bit, the selected ones
    (``sel``) the recovery rollout from their ``x0`` and zeros in ``CLEARED_FIELDS``."""
    sel = recovered(status)
    exp = {f: np.array(before[f], copy=True) for f in STATE_FIELDS}
    idx = np.flatnonzero(sel)
    if len(idx):
        x, u = rollout(P, np.asarray(x0)[idx], v_ref_scale, recovery=True, idx=idx)
        exp["x"][idx], exp["u"][idx] = x, u
        for f in CLEARED_FIELDS:
            exp[f][idx] = 0.0
    return exp, sel
