"""Batched NMPC solver on MI355X behind the reference's ``AcadosOcpSolver`` call surface.

Reference call sites this mirrors (tudoroancea/ihm2):
  * construction ``AcadosOcpSolver(ocp, json_file=..., verbose=False)`` -- ``python/mpc.py:104-113``
  * ``solver.set(stage, field, value)`` with fields ``"p","lbx","ubx","yref","x","u"``
    -- ``python/main.py:252,299-322``
  * ``solver.cost_set(stage, "W", W[, api="new"])`` -- ``python/main.py:253-295``, ``dpc/main.py:263-281``
  * ``solver.constraints_set(stage, "lbx"/"ubx"/"C"..., v)`` -- ``dpc/main.py:226-227,259-261``
  * ``status = solver.solve()`` -- ``python/main.py:325``; status codes ``dpc/main.py:287-293``
  * ``solver.get(stage, "x"/"u")`` -- ``python/main.py:331-334``

Two layers: :class:`BatchedOcpSolver` owns one ``ihm2mpc`` handle (B instances on one GPU) and speaks
``(B, ...)`` C-contiguous float64 arrays; :class:`AcadosOcpSolver` is the per-instance shim
(``view = batch[i]``, or a batch of one when built from an OCP like the reference does).
Host code is NumPy + ctypes only; all arithmetic runs in ``libihm2mpc.so`` (HIP, gfx950).
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from .constants import NG, NLAM, NU, NX, NY
from .ocp import AcadosOcp, AcadosOcpOptions, OcpData

_SOLVER_TYPE = {"SQP_RTI": 0, "SQP": 1}
_GLOBALIZATION = {"FIXED_STEP": 0, "MERIT_BACKTRACKING": 1}


def _f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {a.shape}")
    return a


def _ptr(a):
    return a.ctypes.data_as(_lib.c_double_p)


def decode_launch_record(rec) -> dict:
    """The dictionary of ``BatchedOcpSolver.get_launch_record`` from the sixteen integers of ``ihm2mpc_get_launch_record``
    (``csrc/qp_select.hpp``: ``encode_launch``, ``note_lin``, ``note_sim`` write them)."""
    r = [int(v) for v in rec]
    qp = None
    if r[0] == 1:
        qp = "k_qp_wave<%d,%d,%d,%d>" % tuple(r[1:5])
    elif r[0] == 2:
        qp = "k_qp_block<%d,%d,4>" % (r[1], r[4])
    steps, fallback = None, None
    if r[5] == 1:
        steps = "k_steps<%d,%d,%d,%d,%d,%d,%d>" % tuple(r[6:13]) if r[14] == 0 else "k_steps<%d,%d,%d,%d,%d,%d,%d,1>" % tuple(r[6:13])
    elif r[5] == 2:
        steps, fallback = "per_step", {1: "no_instantiation", 2: "not_resident"}.get(r[13])
    lin = (None, "k_linearize", "k_linearize_dyn", "k_linearize_cols", "k_linearize_irk", "k_linearize_lag")[r[15] & 15]
    sim = (None, "k_sim_step_kin", "k_sim_step", "k_sim_irk", "k_sim_step_kin_lag", "k_sim_sens")[(r[15] >> 4) & 15]
    forms = ("general", "plain", "plain_n40", None)
    slots = ("general", "full")
    return {"qp": qp, "steps": steps, "steps_fallback": fallback, "linearize": lin, "sim": sim,
            "qp_form": forms[(r[15] >> 8) & 3] if qp else None, "steps_form": forms[(r[15] >> 12) & 3] if r[5] == 1 else None,
            "qp_slots": slots[(r[15] >> 10) & 1] if qp else None, "steps_slots": slots[(r[15] >> 14) & 1] if r[5] == 1 else None}


class BatchedOcpSolver:
    """B independent instances of the bicycle NMPC on one MI355X."""

    def __init__(self, ocp: AcadosOcp, batch_size: int, s_ref, kappa_ref, track_id=None, device: int = 0, track_widths=None):
        self.lib = _lib.load()
        self.ocp = ocp
        self.data: OcpData = ocp.flatten()
        d = self.data
        self.B, self.N, self.device = int(batch_size), d.N, int(device)
        s_ref = np.atleast_2d(_f64(s_ref)); kappa_ref = np.atleast_2d(_f64(kappa_ref))
        if s_ref.shape != kappa_ref.shape:
            raise ValueError("s_ref and kappa_ref must have the same shape (ntracks, nknots)")
        self.ntracks, self.nknots = s_ref.shape
        cfg = _lib.Config(
            batch=self.B, N=d.N, M=d.M, model=d.model, ntracks=self.ntracks, nknots=self.nknots, device=device,
            nlp_solver_type=_SOLVER_TYPE[d.nlp_solver_type], nlp_solver_max_iter=d.nlp_solver_max_iter,
            ipm_iter_max=d.ipm_iter_max, dt=d.dt, cost_scale_stage=d.cost_scale_stage, ipm_tol=d.ipm_tol,
            ipm_mu0=d.ipm_mu0, ipm_tau0=d.ipm_tau0, nlp_tol=d.nlp_tol, integrator_type=d.integrator, sim_integrator_type=d.sim_integrator)
        self._h = C.c_void_p()
        _lib.check(self.lib.ihm2mpc_create(C.byref(cfg), C.byref(self._h)))
        self._sens_mode = 0
        self._s_ref, self._kappa_ref = s_ref.copy(), kappa_ref.copy()
        self._track_widths = None if track_widths is None else np.atleast_2d(_f64(track_widths))
        self._push_tracks()
        self.set_track_id(np.zeros(self.B, dtype=np.int32) if track_id is None else track_id)
        self._push_weights()
        self._push_bounds()
        if d.nlp_solver_type == "SQP":
            self.set_sqp_options(d.globalization, d.alpha_min, d.alpha_reduction, d.eps_sufficient_descent, d.use_sufficient_descent,
                                 d.full_step_dual, d.sqp_tol)

    # ---- lifetime ----
    def free(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            # ihm2_amd/torch_layer.py: a tensor that was marked as used on the handle's stream makes its allocator record an event on that
            # stream when the tensor is released -- the stream must outlive it, and the stream goes with the handle
            alive = sum(r() is not None for r in getattr(self, "_stream_users", ()))
            if alive:
                raise RuntimeError(f"the memory of {alive} tensors that went through rti_solve is still alive: their allocator records an event on the "
                                   "solver's stream when they are released, so release them (and the graph that holds them) before the solver")
            self.lib.ihm2mpc_synchronize(self._h)
            for ptr in getattr(self, "_pinned", []):
                self.lib.ihm2mpc_host_free(ptr)
            self._pinned = []
            self.lib.ihm2mpc_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            # A handle whose stream ihm2_amd/torch_layer.py has used is never freed from here: it is left to the process's end.  free()'s guard
            # counts weak references, and when the solver and the tensors die in one garbage collection (a cycle: the frames of a
            # traceback that hold both, say) the collector clears the weak references before it calls this, while the tensors' memory
            # is still held -- the guard would see nothing alive, the stream would go, and the allocator would record its event on a
            # destroyed stream when the tensors follow (the segmentation fault of NOTES.md R28, by another way: R30).
            if getattr(self, "_stream_users", None):
                return
            self.free()
        except Exception:
            pass

    def __len__(self):
        return self.B

    def __getitem__(self, i: int) -> "AcadosOcpSolver":
        if not -self.B <= i < self.B:
            raise IndexError(i)
        return AcadosOcpSolver._view(self, i % self.B)

    # ---- shared problem data ----
    def _push_tracks(self):
        _lib.check(self.lib.ihm2mpc_set_tracks(self._h, _ptr(self._s_ref), _ptr(self._kappa_ref)))

    def _push_weights(self):
        d = self.data
        d.W = _f64(d.W, (self.N, NY, NY), "W"); d.W_e = _f64(d.W_e, (NX, NX), "W_e")
        _lib.check(self.lib.ihm2mpc_set_weights(self._h, _ptr(d.W), _ptr(d.W_e)))

    def _push_bounds(self):
        d = self.data
        arrs = [_f64(getattr(d, n)) for n in ("lbx", "ubx", "lbu", "ubu", "C", "D", "lg", "ug")]
        _lib.check(self.lib.ihm2mpc_set_bounds(self._h, *[_ptr(a) for a in arrs]))
        self._push_path()
        self._push_soft()

    def _push_path(self):
        d = self.data
        if not d.path_on:
            _lib.check(self.lib.ihm2mpc_set_path_constraints(self._h, 0, 0.0, 0.0, None, None, None))
            return
        if self._track_widths is None or self._track_widths.shape != (self.ntracks, 2):
            raise ValueError(f"the track rows (model.con_h_expr) need track_widths of shape ({self.ntracks}, 2) = (right, left)")
        lh, uh = _f64(d.lh, (2,), "lh"), _f64(d.uh, (2,), "uh")
        _lib.check(self.lib.ihm2mpc_set_path_constraints(self._h, 1, float(d.car_L), float(d.car_W), _ptr(self._track_widths),
                                                         _ptr(lh), _ptr(uh)))
        self._push_alat()

    def _push_alat(self):
        """The lateral-acceleration row of the kinematic constraint set (``old/generate_acaods_interface.py:198-209``)."""
        d = self.data
        if not getattr(d, "alat_on", 0):
            _lib.check(self.lib.ihm2mpc_set_alat_constraint(self._h, 0, 0.0, 0.0, None, None))
            return
        z = None if d.alat_soft_z is None else _f64(d.alat_soft_z, (2,), "alat_soft_z")
        Z = None if d.alat_soft_Z is None else _f64(d.alat_soft_Z, (2,), "alat_soft_Z")
        _lib.check(self.lib.ihm2mpc_set_alat_constraint(self._h, 1, float(d.alat_lb), float(d.alat_ub), None if z is None else _ptr(z),
                                                        None if Z is None else _ptr(Z)))

    def _push_soft(self):
        d = self.data
        if getattr(d, "soft_Z", None) is None or not np.any(np.asarray(d.soft_Z) >= 0.0):
            _lib.check(self.lib.ihm2mpc_set_soft(self._h, None, None))
            return
        z = _f64(d.soft_z, (self.N + 1, NLAM), "soft_z"); Z = _f64(d.soft_Z, (self.N + 1, NLAM), "soft_Z")
        _lib.check(self.lib.ihm2mpc_set_soft(self._h, _ptr(z), _ptr(Z)))

    def set_soft(self, soft_z=None, soft_Z=None):
        """Soft constraint sides, ``(N+1, 28)`` each (14 lower then 14 upper; ``soft_Z < 0`` = hard); ``None`` = all hard."""
        self.data.soft_z = None if soft_z is None else np.asarray(soft_z, dtype=np.float64)
        self.data.soft_Z = None if soft_Z is None else np.asarray(soft_Z, dtype=np.float64)
        self._push_soft()

    def set_tracks(self, s_ref, kappa_ref):
        self._s_ref = _f64(np.atleast_2d(s_ref), (self.ntracks, self.nknots), "s_ref")
        self._kappa_ref = _f64(np.atleast_2d(kappa_ref), (self.ntracks, self.nknots), "kappa_ref")
        self._push_tracks()

    def set_track_id(self, track_id):
        tid = np.ascontiguousarray(track_id, dtype=np.int32)
        if tid.shape != (self.B,):
            raise ValueError(f"track_id must have shape ({self.B},)")
        self._track_id = tid
        _lib.check(self.lib.ihm2mpc_set_track_id(self._h, tid.ctypes.data_as(_lib.c_int32_p)))

    def set_weights(self, W=None, W_e=None):
        """W: (12,12) for all stages or (N,12,12); W_e: (8,8).  Shared by the batch."""
        if W is not None:
            W = np.asarray(W, dtype=np.float64)
            self.data.W = np.tile(W[None], (self.N, 1, 1)) if W.ndim == 2 else W
        if W_e is not None:
            self.data.W_e = np.asarray(W_e, dtype=np.float64)
        self._push_weights()

    # ---- per-instance tuning ----
    def set_instance_weights(self, W=None, W_e=None):
        """One weight set per instance: W ``(B,12,12)`` for every stage, W_e ``(B,8,8)``.  Instance b then gives what a
        batch whose shared weights are ``(W[b], W_e[b])`` gives, bit for bit.  ``None, None``: the shared weights again."""
        if W is None and W_e is None:
            self._inst_W = None
            _lib.check(self.lib.ihm2mpc_set_instance_weights(self._h, None, None))
            return
        if W is None or W_e is None:
            raise ValueError("W and W_e must both be given, or both be None")
        W = _f64(W, (self.B, NY, NY), "W"); W_e = _f64(W_e, (self.B, NX, NX), "W_e")
        _lib.check(self.lib.ihm2mpc_set_instance_weights(self._h, _ptr(W), _ptr(W_e)))
        self._inst_W = (W, W_e)

    def set_instance_bounds(self, lbx=None, ubx=None, lbu=None, ubu=None, lg=None, ug=None):
        """Bound values per instance: lbx/ubx ``(B,N+1,8)`` (stage 0 unused), lbu/ubu ``(B,N,2)``, lg/ug ``(B,N,2)``.  The finite
        sides must be the shared table's; C, D, soft penalties, track rows and the a_lat row stay shared.  All ``None``: shared again."""
        arrs = (lbx, ubx, lbu, ubu, lg, ug)
        if all(a is None for a in arrs):
            _lib.check(self.lib.ihm2mpc_set_instance_bounds(self._h, None, None, None, None, None, None))
            return
        if any(a is None for a in arrs):
            raise ValueError("lbx, ubx, lbu, ubu, lg, ug must all be given, or all be None")
        B, N = self.B, self.N
        shapes = ((B, N + 1, NX), (B, N + 1, NX), (B, N, NU), (B, N, NU), (B, N, 2), (B, N, 2))
        arrs = [_f64(a, sh, n) for a, sh, n in zip(arrs, shapes, ("lbx", "ubx", "lbu", "ubu", "lg", "ug"))]
        _lib.check(self.lib.ihm2mpc_set_instance_bounds(self._h, *[_ptr(a) for a in arrs]))

    def set_instance_soft(self, soft_z=None, soft_Z=None):
        """Slack penalties per instance, ``(B,N+1,28)`` each in the layout of :meth:`set_soft`.  A side must be soft (``soft_Z >= 0``)
        exactly where the shared table (:meth:`set_soft`, called first) holds it soft; the values are the instance's own.  Instance b
        then gives what a batch whose shared penalties are ``(soft_z[b], soft_Z[b])`` gives, bit for bit -- the QP, the SQP mode's
        merit, the cost and every gradient.  The bounds of the a_lat row, the track rows' ``lh`` / ``uh``, the widths and C, D stay
        shared.  ``None, None``: the shared penalties again."""
        self._set_instance_penalties(self.lib.ihm2mpc_set_instance_soft, soft_z, soft_Z, (self.B, self.N + 1, NLAM))

    def set_instance_alat_soft(self, soft_z=None, soft_Z=None):
        """Slack penalties of the lateral-acceleration row per instance, ``(B,2)`` each = lower / upper side; the row's shared
        penalties (``ihm2mpc_set_alat_constraint`` with soft sides) give the pattern.  ``None, None``: shared again."""
        self._set_instance_penalties(self.lib.ihm2mpc_set_instance_alat_soft, soft_z, soft_Z, (self.B, 2))

    def _set_instance_penalties(self, entry, soft_z, soft_Z, shape):
        if soft_z is None and soft_Z is None:
            _lib.check(entry(self._h, None, None))
            return
        if soft_z is None or soft_Z is None:
            raise ValueError("soft_z and soft_Z must both be given, or both be None")
        z = _f64(soft_z, shape, "soft_z"); Z = _f64(soft_Z, shape, "soft_Z")
        _lib.check(entry(self._h, _ptr(z), _ptr(Z)))

    # ---- per-instance data, batched ----
    def set_x0(self, x0):
        _lib.check(self.lib.ihm2mpc_set_x0(self._h, _ptr(_f64(x0, (self.B, NX), "x0"))))

    def set_x(self, x):
        _lib.check(self.lib.ihm2mpc_set_x(self._h, _ptr(_f64(x, (self.B, self.N + 1, NX), "x"))))

    def set_u(self, u):
        _lib.check(self.lib.ihm2mpc_set_u(self._h, _ptr(_f64(u, (self.B, self.N, NU), "u"))))

    def set_yref(self, yref):
        _lib.check(self.lib.ihm2mpc_set_yref(self._h, _ptr(_f64(yref, (self.B, self.N, NY), "yref"))))

    def set_yref_e(self, yref_e):
        _lib.check(self.lib.ihm2mpc_set_yref_e(self._h, _ptr(_f64(yref_e, (self.B, NX), "yref_e"))))

    def set_multipliers(self, pi=None, lam=None):
        pi_a = None if pi is None else _f64(pi, (self.B, self.N + 1, NX), "pi")
        lam_a = None if lam is None else _f64(lam, (self.B, self.N + 1, NLAM), "lam")
        _lib.check(self.lib.ihm2mpc_set_multipliers(self._h, None if pi_a is None else _ptr(pi_a),
                                                    None if lam_a is None else _ptr(lam_a)))

    # ---- the hot path ----
    def init_guess(self, v_ref_scale: float = 1.0):
        _lib.check(self.lib.ihm2mpc_init_guess(self._h, float(v_ref_scale)))

    def reinit_failed(self, v_ref_scale: float = 1.0):
        """Re-roll the warm start of the instances whose last solve failed (status not 0 and not 2) from their current ``x0``: the
        kinematic rollout (``fkin6`` whatever the OCP's model) with the actuator lags in closed form, and zero multipliers and slacks
        (``pi``, ``lam``, ``slk`` and the a_lat row's pair).  The other instances keep everything."""
        _lib.check(self.lib.ihm2mpc_reinit_failed(self._h, float(v_ref_scale)))

    def prepare_step(self, s_target: float):
        """Reference ramp + warm-start shift of ``compute_control`` (``python/main.py:303-322``) on device."""
        _lib.check(self.lib.ihm2mpc_prepare_step(self._h, float(s_target)))

    def solve_async(self, n_iter: int = 0):
        _lib.check(self.lib.ihm2mpc_solve(self._h, int(n_iter)))

    def solve(self, n_iter: int = 0) -> np.ndarray:
        """Runs the RTI iteration(s); returns the per-instance acados status codes, int32[B]."""
        self.solve_async(n_iter)
        return self.get_status()

    def compute_control(self, x0, s_target: float):
        """``IHM2Controller.compute_control`` (``python/main.py:297-334``) for the whole batch in one call: returns ``(u0, status)``."""
        u0 = np.empty((self.B, NU)); st = np.empty(self.B, dtype=np.int32)
        _lib.check(self.lib.ihm2mpc_compute_control(self._h, _ptr(_f64(x0, (self.B, NX), "x0")), float(s_target), _ptr(u0),
                                                    st.ctypes.data_as(_lib.c_int32_p)))
        return u0, st

    def reserve_history(self, n_steps: int):
        """Device room for the histories of ``run_steps`` calls of up to ``n_steps`` steps."""
        _lib.check(self.lib.ihm2mpc_reserve_history(self._h, int(n_steps)))

    def run_steps(self, s_target: float, n_steps: int, model: int = 0, M_sim: int = 25, freeze: bool = False, lap_stop: float = np.inf,
                  u0_hist=None, x0_hist=None, status_hist=None, qp_iter_hist=None, wait: bool = True, sens_u0_hist=None):
        """``n_steps`` control steps (plant + ``compute_control``) in one launch, every instance running ahead on its own
        wavefront (``ihm2mpc_run_steps``).  Histories are written into the given arrays -- ``(n_steps, B, 2)``, ``(n_steps, B, 8)``,
        ``(n_steps, B)`` int32 twice -- or, for ``True``, into fresh ones; returns a dict of those that were asked for.
        ``sens_u0_hist`` (an array or ``True``): the loop with x0 sensitivities (``ihm2mpc_run_steps_sens``, needs
        ``set_x0_sensitivities(1 or 2)``), ``out["sens_u0"]`` ``(n_steps, B, 2, 8)`` = ``du_0/dx_0`` of every step's solve; afterwards
        ``get_x0_sensitivities`` reads the last step's."""
        n = int(n_steps)
        out = {}
        def buf(v, shape, dtype, name):
            if v is None or v is False:
                return None
            a = np.empty(shape, dtype=dtype) if v is True else v
            if a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
            out[name] = a
            return a
        u = buf(u0_hist, (n, self.B, NU), np.float64, "u0"); x = buf(x0_hist, (n, self.B, NX), np.float64, "x0")
        st = buf(status_hist, (n, self.B), np.int32, "status"); it = buf(qp_iter_hist, (n, self.B), np.int32, "qp_iter")
        hists = (None if u is None else _ptr(u), None if x is None else _ptr(x),
                 None if st is None else st.ctypes.data_as(_lib.c_int32_p), None if it is None else it.ctypes.data_as(_lib.c_int32_p))
        if sens_u0_hist is None or sens_u0_hist is False:
            _lib.check(self.lib.ihm2mpc_run_steps(self._h, int(model), int(M_sim), float(s_target), n, int(bool(freeze)), float(lap_stop), *hists))
        else:
            k = buf(sens_u0_hist, (n, self.B, NU, NX), np.float64, "sens_u0")
            _lib.check(self.lib.ihm2mpc_run_steps_sens(self._h, int(model), int(M_sim), float(s_target), n, int(bool(freeze)), float(lap_stop),
                                                       *hists, _ptr(k)))
        if wait:
            self.synchronize()
        return out

    def set_sqp_options(self, globalization="MERIT_BACKTRACKING", alpha_min=0.05, alpha_reduction=0.7, eps_sufficient_descent=1e-4,
                        use_sufficient_descent=False, full_step_dual=False, tol=None):
        """Line search and tolerances of the SQP mode (``python/main.py:230-237``); ``tol`` = (stat, eq, ineq, comp) or a scalar."""
        t = None if tol is None else np.ascontiguousarray(np.broadcast_to(_f64(tol), (4,)))
        _lib.check(self.lib.ihm2mpc_set_sqp_options(self._h, _GLOBALIZATION[globalization], float(alpha_min), float(alpha_reduction),
                                                     float(eps_sufficient_descent), int(bool(use_sufficient_descent)), int(bool(full_step_dual)),
                                                     None if t is None else _ptr(t)))

    def get_sqp_stats(self):
        """QP solves made (B) and last step length (B) of the last SQP-mode solve."""
        it = np.empty(self.B, dtype=np.int32); alpha = np.empty(self.B)
        _lib.check(self.lib.ihm2mpc_get_sqp_stats(self._h, it.ctypes.data_as(_lib.c_int32_p), _ptr(alpha)))
        return {"sqp_iter": it, "alpha": alpha}

    def get_sqp_merit(self):
        """(B,4) merit values of the last line search of the last SQP-mode solve: m(0), m at the last trial step (the accepted step length,
        or the last one tried when the step fell to ``alpha_min``), D, the infeasibility part of m(0); zeros where no line search ran."""
        m = np.empty((self.B, 4))
        _lib.check(self.lib.ihm2mpc_get_sqp_merit(self._h, _ptr(m)))
        return m

    def synchronize(self):
        _lib.check(self.lib.ihm2mpc_synchronize(self._h))

    def linearize(self):
        _lib.check(self.lib.ihm2mpc_linearize(self._h))

    def get_linearization(self):
        A = np.empty((self.B, self.N, NX, NX)); Bm = np.empty((self.B, self.N, NX, NU)); b = np.empty((self.B, self.N, NX))
        _lib.check(self.lib.ihm2mpc_get_linearization(self._h, _ptr(A), _ptr(Bm), _ptr(b)))
        return A, Bm, b

    def _get(self, fn, shape):
        out = np.empty(shape, dtype=np.float64)
        _lib.check(fn(self._h, _ptr(out)))
        return out

    def get_x(self):
        return self._get(self.lib.ihm2mpc_get_x, (self.B, self.N + 1, NX))

    def get_u(self):
        return self._get(self.lib.ihm2mpc_get_u, (self.B, self.N, NU))

    def get_u0(self):
        return self._get(self.lib.ihm2mpc_get_u0, (self.B, NU))

    def get_x0(self):
        return self._get(self.lib.ihm2mpc_get_x0, (self.B, NX))

    def get_residuals(self):
        return self._get(self.lib.ihm2mpc_get_residuals, (self.B, 4))

    def build_tracks(self, coeffs_X, coeffs_Y):
        """Track tables on the device from the centre lines' spline coefficients (``python/motion_planning.py:139-428``): ``coeffs_X``,
        ``coeffs_Y`` are lists of ``(nseg_t, 4)`` arrays, one per track (``track.py::fit_spline``).  Replaces ``set_tracks`` +
        ``set_track_geometry``; ``nknots`` of this solver = 3 x samples per lap."""
        if len(coeffs_X) != self.ntracks or len(coeffs_Y) != self.ntracks:
            raise ValueError(f"{self.ntracks} tracks expected")
        nseg = np.array([len(c) for c in coeffs_X], dtype=np.int32)
        mx = int(nseg.max())
        cX = np.zeros((self.ntracks, mx, 4)); cY = np.zeros((self.ntracks, mx, 4))
        for t in range(self.ntracks):
            cX[t, :nseg[t]] = coeffs_X[t]; cY[t, :nseg[t]] = coeffs_Y[t]
        _lib.check(self.lib.ihm2mpc_build_tracks(self._h, mx, nseg.ctypes.data_as(_lib.c_int32_p), _ptr(cX), _ptr(cY)))
        s_ref = np.empty((self.ntracks, self.nknots)); kappa = np.empty((self.ntracks, self.nknots))
        _lib.check(self.lib.ihm2mpc_get_tracks(self._h, _ptr(s_ref), _ptr(kappa), None, None, None))
        self._s_ref, self._kappa_ref = s_ref, kappa          # the host copies the per-instance shim compares "p" against

    def fit_tracks(self, center_lines, curv_weight: float = 2.0):
        """Closed cubic-spline fit of every track's centre line on the device (``fit_spline``, ``python/motion_planning.py:28-124``; the
        weight 2.0 is ``offline_motion_plan``'s, ``:358``).  ``center_lines``: one ``(npts_t, 2)`` array per track.  Returns two lists of
        ``(npts_t, 4)`` coefficient arrays -- what :meth:`build_tracks` takes."""
        if len(center_lines) != self.ntracks:
            raise ValueError(f"{self.ntracks} tracks expected")
        npts = np.array([len(c) for c in center_lines], dtype=np.int32)
        mx = int(npts.max())
        xy = np.zeros((self.ntracks, mx, 2))
        for t, c in enumerate(center_lines):
            xy[t, :npts[t]] = np.asarray(c, dtype=np.float64)
        cX = np.zeros((self.ntracks, mx, 4)); cY = np.zeros((self.ntracks, mx, 4))
        _lib.check(self.lib.ihm2mpc_fit_tracks(self._h, mx, npts.ctypes.data_as(_lib.c_int32_p), _ptr(xy), float(curv_weight), _ptr(cX), _ptr(cY)))
        return [cX[t, :npts[t]].copy() for t in range(self.ntracks)], [cY[t, :npts[t]].copy() for t in range(self.ntracks)]

    def get_tracks(self):
        """``(s_ref, kappa_ref, X_ref, Y_ref, phi_ref)``, each ``(ntracks, nknots)``, as they are on the device."""
        out = [np.empty((self.ntracks, self.nknots)) for _ in range(5)]
        _lib.check(self.lib.ihm2mpc_get_tracks(self._h, *[_ptr(a) for a in out]))
        return tuple(out)

    def sim_step_dyn10(self, x, u, M_sim: int = 100):
        """Plant step of the 15-state model ``fdyn10`` (python/models.py:609-801): ``x`` (B, 15), ``u`` (B, 5) -> (B, 15)."""
        xn = np.empty((self.B, 15))
        _lib.check(self.lib.ihm2mpc_sim_step_dyn10(self._h, int(M_sim), _ptr(_f64(x, (self.B, 15), "x")), _ptr(_f64(u, (self.B, 5), "u")), _ptr(xn)))
        return xn

    def get_qp_residuals(self):
        """(B, 4) relative KKT residuals of the QP at the returned point (stationarity, dynamics, inequalities, complementarity)."""
        return self._get(self.lib.ihm2mpc_get_qp_residuals, (self.B, 4))

    def get_multipliers(self):
        pi = np.empty((self.B, self.N + 1, NX)); lam = np.empty((self.B, self.N + 1, NLAM))
        _lib.check(self.lib.ihm2mpc_get_multipliers(self._h, _ptr(pi), _ptr(lam)))
        return pi, lam

    def get_alat_multipliers(self):
        """Multipliers and slack values of the lateral-acceleration row, ``(B, N+1, 2)`` each: lower side, upper side."""
        lam = np.empty((self.B, self.N + 1, 2)); slk = np.empty((self.B, self.N + 1, 2))
        _lib.check(self.lib.ihm2mpc_get_alat_multipliers(self._h, _ptr(lam), _ptr(slk)))
        return lam, slk

    def set_alat_multipliers(self, lam=None, slk=None):
        la = None if lam is None else _f64(lam, (self.B, self.N + 1, 2), "lam")
        sa = None if slk is None else _f64(slk, (self.B, self.N + 1, 2), "slk")
        _lib.check(self.lib.ihm2mpc_set_alat_multipliers(self._h, None if la is None else _ptr(la), None if sa is None else _ptr(sa)))

    def set_slacks(self, sl=None):
        """Slack values the next SQP-mode solve starts from, ``(B, N+1, 28)``; ``None`` = zeros."""
        _lib.check(self.lib.ihm2mpc_set_slacks(self._h, None if sl is None else _ptr(_f64(sl, (self.B, self.N + 1, NLAM), "sl"))))

    def get_slacks(self):
        """Slack of each soft constraint side after the last QP, ``(B, N+1, 28)`` (0 for hard sides)."""
        return self._get(self.lib.ihm2mpc_get_slacks, (self.B, self.N + 1, NLAM))

    def get_status(self):
        out = np.empty(self.B, dtype=np.int32)
        _lib.check(self.lib.ihm2mpc_get_status(self._h, out.ctypes.data_as(_lib.c_int32_p)))
        return out

    def get_qp_iter(self):
        out = np.empty(self.B, dtype=np.int32)
        _lib.check(self.lib.ihm2mpc_get_qp_iter(self._h, out.ctypes.data_as(_lib.c_int32_p)))
        return out

    def get_timings(self):
        ms = np.zeros(3)
        _lib.check(self.lib.ihm2mpc_get_timings(self._h, _ptr(ms), 3))
        return {"total_ms": ms[0], "linearize_ms": ms[1], "qp_ms": ms[2]}

    def get_launch_record(self):
        """Which instantiations the launchers last launched (``ihm2mpc_get_launch_record``), as they launched them:

        ``qp``: the last per-step QP launch, e.g. ``"k_qp_wave<8,2,0,1>"`` (NSLOT, NSOFT, PATH, UNI) or ``"k_qp_block<2,1,4>"``
        (slots per thread, UNI, wavefronts); ``steps``: the last ``run_steps``, ``"k_steps<...>"`` (NSLOT, NSOFT, PATH, UNI, SQP, IRK,
        DYN, and an eighth 1 for the loop with x0 sensitivities) or ``"per_step"`` with ``steps_fallback`` ``"no_instantiation"`` /
        ``"not_resident"``; ``linearize`` / ``sim``: the kernel of the last linearisation / plant launch outside ``k_steps``
        (``"k_linearize"``, ``"k_linearize_dyn"``, ``"k_linearize_cols"``, ``"k_linearize_irk"``, ``"k_linearize_lag"``; ``"k_sim_step_kin"``,
        ``"k_sim_step"``, ``"k_sim_irk"``, ``"k_sim_step_kin_lag"``, ``"k_sim_sens"`` (``sim_step_sens``); ``_lag``: the integrator ``"ERK_LAG"``); ``qp_form`` / ``steps_form``: the form of the factor sweep in those two launches, ``"general"``,
        ``"plain"`` (straight-line stage, run-time horizon) or ``"plain_n40"`` (the horizon 40 compiled in) -- same results, so the
        kernel names above do not tell them apart; ``qp_slots`` / ``steps_slots``: the form of the slot phases alike, ``"general"`` or
        ``"full"`` (a table of 64 x 5 hard two-sided rows at the horizon 40: no validity or side test per slot).  ``None`` where nothing
        was launched yet."""
        rec = np.zeros(16, dtype=np.int32)
        _lib.check(self.lib.ihm2mpc_get_launch_record(self._h, rec.ctypes.data_as(_lib.c_int32_p)))
        return decode_launch_record(rec)

    # ---- device-pointer variants (zero copy; dptr = integer device address, instance-major layout) ----
    def set_x0_device(self, dptr: int):
        _lib.check(self.lib.ihm2mpc_set_x0_device(self._h, C.c_void_p(dptr)))

    def get_u0_device(self, dptr: int):
        _lib.check(self.lib.ihm2mpc_get_u0_device(self._h, C.c_void_p(dptr)))

    def get_x_device(self, dptr: int):
        _lib.check(self.lib.ihm2mpc_get_x_device(self._h, C.c_void_p(dptr)))

    def get_u_device(self, dptr: int):
        _lib.check(self.lib.ihm2mpc_get_u_device(self._h, C.c_void_p(dptr)))

    def get_status_device(self, dptr: int):
        _lib.check(self.lib.ihm2mpc_get_status_device(self._h, C.c_void_p(dptr)))

    def get_stream(self) -> int:
        """The handle's HIP stream as an integer (``ihm2mpc_get_stream``): what every ``*_device`` entry is ordered on."""
        stream = C.c_void_p()
        _lib.check(self.lib.ihm2mpc_get_stream(self._h, C.byref(stream)))
        return int(stream.value or 0)

    def set_yref_device(self, dptr: int):
        """``yref`` ``(B,N,12)`` from device memory, stream-ordered (``ihm2mpc_set_yref_device``)."""
        _lib.check(self.lib.ihm2mpc_set_yref_device(self._h, C.c_void_p(dptr)))

    def set_yref_e_device(self, dptr: int):
        """``yref_e`` ``(B,8)`` from device memory, stream-ordered (``ihm2mpc_set_yref_e_device``)."""
        _lib.check(self.lib.ihm2mpc_set_yref_e_device(self._h, C.c_void_p(dptr)))

    def set_instance_weights_device(self, W_dptr: int, W_e_dptr: int, check: bool = True):
        """:meth:`set_instance_weights` with ``W (B,12,12)`` and ``W_e (B,8,8)`` in device memory: the tables are expanded by a kernel,
        bit for bit what the host setter uploads.  ``check=True`` validates as the host setter does (NaN, symmetry) and blocks;
        ``check=False`` reads nothing back and does not block -- the caller vouches for symmetric weights without NaN.  ``0, 0``: the
        shared weights again (``ihm2mpc_set_instance_weights_device``)."""
        _lib.check(self.lib.ihm2mpc_set_instance_weights_device(self._h, C.c_void_p(int(W_dptr)) if W_dptr else None,
                                                                C.c_void_p(int(W_e_dptr)) if W_e_dptr else None, int(bool(check))))
        self._inst_W = None

    def get_instance_weight_tables(self):
        """``dict(Hs=(B,2,10,10), Gy=(B,2,10,12), Wd=(B,208))``: the per-instance weight tables as the QP reads them, stage then
        terminal (``ihm2mpc_get_instance_weight_tables``; refused while the per-instance weights are off)."""
        out = dict(Hs=np.empty((self.B, 2, 10, 10)), Gy=np.empty((self.B, 2, 10, NY)), Wd=np.empty((self.B, NY * NY + NX * NX)))
        _lib.check(self.lib.ihm2mpc_get_instance_weight_tables(self._h, *[_ptr(v) for v in out.values()]))
        return out

    def eval_adjoint_weight_sensitivities_device(self, n_seeds: int, seed_x: int = 0, seed_u: int = 0, grad_x0: int = 0, grad_yref: int = 0,
                                                 grad_yref_e: int = 0, grad_W: int = 0, grad_W_e: int = 0):
        """:meth:`eval_adjoint_weight_sensitivities` on device memory, stream-ordered and without a wait: addresses as integers, 0 for
        NULL (a zero seed, an output that is not wanted; both seeds 0 with ``n_seeds = 2``: the unit seeds on ``u_0``).  Seeds
        ``(B,n_seeds,N+1,8)`` / ``(B,n_seeds,N,2)``, gradients ``(B,n_seeds,...)``; everything must stay alive, the seeds unchanged,
        until the handle's stream has passed (``ihm2mpc_eval_adjoint_sensitivities_w_device``)."""
        ptr = [C.c_void_p(int(a)) if a else None for a in (seed_x, seed_u, grad_x0, grad_yref, grad_yref_e, grad_W, grad_W_e)]
        _lib.check(self.lib.ihm2mpc_eval_adjoint_sensitivities_w_device(self._h, int(n_seeds), *ptr))

    def set_instance_soft_device(self, soft_z_dptr: int, soft_Z_dptr: int, check: bool = True):
        """:meth:`set_instance_soft` with ``soft_z``, ``soft_Z`` ``(B,N+1,28)`` in device memory: a kernel writes the penalty halves of
        the per-instance constraint tables, bit for bit what the host setter uploads.  ``check=True`` validates as the host setter does
        (its message for the first offending instance, stage and side) and blocks; ``check=False`` reads nothing back -- the caller
        vouches.  The solver keeps no host copy: a later ``set_soft`` (for the a_lat pair: ``set_alat_constraint``) that changes which
        sides are soft makes the next solve refuse until the penalties are set again; shared setters that leave those flags alone keep
        the values.  ``0, 0``: the shared penalties again (``ihm2mpc_set_instance_soft_device``)."""
        _lib.check(self.lib.ihm2mpc_set_instance_soft_device(self._h, C.c_void_p(int(soft_z_dptr)) if soft_z_dptr else None,
                                                             C.c_void_p(int(soft_Z_dptr)) if soft_Z_dptr else None, int(bool(check))))

    def set_instance_alat_soft_device(self, soft_z_dptr: int, soft_Z_dptr: int, check: bool = True):
        """:meth:`set_instance_alat_soft` with the ``(B,2)`` pairs in device memory; otherwise as :meth:`set_instance_soft_device`
        (``ihm2mpc_set_instance_alat_soft_device``)."""
        _lib.check(self.lib.ihm2mpc_set_instance_alat_soft_device(self._h, C.c_void_p(int(soft_z_dptr)) if soft_z_dptr else None,
                                                                  C.c_void_p(int(soft_Z_dptr)) if soft_Z_dptr else None, int(bool(check))))

    def get_instance_penalty_tables(self):
        """``dict(slot_z, slot_Z (B,640), stage_z, stage_Z (B,N+1,28), alat_z, alat_Z (B,2))``: the penalty halves of the per-instance
        constraint tables as the kernels read them -- the slot table's entries in table order, padded with ``(0, -1)`` to 640
        (``ihm2mpc_get_instance_penalty_tables``; refused while no per-instance bounds or penalties are on)."""
        B, N = self.B, self.N
        out = dict(slot_z=np.empty((B, 640)), slot_Z=np.empty((B, 640)), stage_z=np.empty((B, N + 1, NLAM)), stage_Z=np.empty((B, N + 1, NLAM)),
                   alat_z=np.empty((B, 2)), alat_Z=np.empty((B, 2)))
        _lib.check(self.lib.ihm2mpc_get_instance_penalty_tables(self._h, *[_ptr(v) for v in out.values()]))
        return out

    def get_slacks_device(self, slk_dptr: int = 0, slk_alat_dptr: int = 0):
        """:meth:`get_slacks` ``(B,N+1,28)`` and the slacks of :meth:`get_alat_multipliers` ``(B,N+1,2)`` into device memory,
        stream-ordered; 0 = not wanted (``ihm2mpc_get_slacks_device``)."""
        _lib.check(self.lib.ihm2mpc_get_slacks_device(self._h, C.c_void_p(int(slk_dptr)) if slk_dptr else None,
                                                      C.c_void_p(int(slk_alat_dptr)) if slk_alat_dptr else None))

    def eval_adjoint_penalty_sensitivities_device(self, n_seeds: int, seed_x: int = 0, seed_u: int = 0, seed_s: int = 0, seed_sa: int = 0,
                                                  grad_x0: int = 0, grad_yref: int = 0, grad_yref_e: int = 0, grad_W: int = 0, grad_W_e: int = 0,
                                                  grad_z: int = 0, grad_Z: int = 0, grad_za: int = 0, grad_Za: int = 0, zeta: int = 0):
        """:meth:`eval_adjoint_penalty_sensitivities` on device memory, stream-ordered and without a wait: addresses as integers, 0 for
        NULL (a zero seed, an output that is not wanted; all four seeds 0 with ``n_seeds = 2``: the unit seeds on ``u_0``).  Seeds
        ``(B,n_seeds,N+1,8)``, ``(B,n_seeds,N,2)``, ``(B,n_seeds,N+1,28)``, ``(B,n_seeds,N+1,2)``; the penalty gradients
        ``(B,n_seeds,N+1,28)`` and ``(B,n_seeds,N+1,2)``, ``zeta (B,n_seeds,N+1,10)``; everything must stay alive, the seeds unchanged,
        until the handle's stream has passed (``ihm2mpc_eval_adjoint_sensitivities_p_device``)."""
        ptr = [C.c_void_p(int(a)) if a else None for a in (seed_x, seed_u, seed_s, seed_sa, grad_x0, grad_yref, grad_yref_e, grad_W, grad_W_e,
                                                           grad_z, grad_Z, grad_za, grad_Za, zeta)]
        _lib.check(self.lib.ihm2mpc_eval_adjoint_sensitivities_p_device(self._h, int(n_seeds), *ptr))

    # ---- sensitivities of the solution with respect to x0 (acados: eval_param_sens(j, 0, "ex"); get(k, "sens_x" / "sens_u")) ----
    def set_x0_sensitivities(self, mode: int = 2):
        """0 off; 1 ``du_0/dx_0`` only (the feedback gain K0); 2 the whole horizon.  Every later RTI ``solve`` /
        ``compute_control`` / ``step`` computes them after its QP (refused in the SQP mode; ``run_steps`` computes none unless it is
        given ``sens_u0_hist``)."""
        _lib.check(self.lib.ihm2mpc_set_x0_sensitivities(self._h, int(mode)))
        self._sens_mode = int(mode)

    def get_x0_sensitivities(self):
        """``(sens_x, sens_u)`` of the last solve: mode 2 ``(B,N+1,8,8)``, ``(B,N,2,8)`` with ``sens_x[b,k,i,j] = dx_k,i/dx0_j``;
        mode 1 ``(None, (B,2,8))``.  NaN rows for instances whose status is neither 0 nor 2."""
        full = self._sens_mode == 2
        sx = np.empty((self.B, self.N + 1, NX, NX)) if full else None
        su = np.empty((self.B, self.N, NU, NX)) if full else np.empty((self.B, NU, NX))
        _lib.check(self.lib.ihm2mpc_get_x0_sensitivities(self._h, _ptr(sx) if full else None, _ptr(su)))
        return sx, su

    def get_sens_u0_device(self, dptr: int):
        """``du_0/dx_0`` ``(B,2,8)`` into device memory, stream-ordered."""
        _lib.check(self.lib.ihm2mpc_get_sens_u0_device(self._h, C.c_void_p(dptr)))

    # ---- adjoint sensitivities of the same solution (acados: eval_adjoint_solution_sensitivity(seed_x, seed_u)) ----
    def eval_adjoint_sensitivities(self, seed_x=None, seed_u=None):
        """Gradients of scalar functions ``L`` of the last RTI solution with respect to what the solve was fed: ``seed_x``
        ``(B,S,N+1,8)`` = ``dL/dx_k``, ``seed_u`` ``(B,S,N,2)`` = ``dL/du_k`` for ``S <= 8`` functions at once (``(B,N+1,8)`` /
        ``(B,N,2)``: one, and the outputs drop that axis; one of the two may be ``None`` = zero).  Both ``None``: the two unit seeds on
        ``u_0``, i.e. the Jacobians of the first control.  Returns ``dict(x0=(B,S,8), yref=(B,S,N,12), yref_e=(B,S,8))``, NaN rows for
        instances whose status is neither 0 nor 2.  Needs ``set_x0_sensitivities(1 or 2)`` before the solve and must follow the solve
        directly (``ihm2mpc_eval_adjoint_sensitivities``)."""
        return self._eval_adjoint(seed_x, seed_u, False)

    def _eval_adjoint(self, seed_x, seed_u, weights: bool):
        B, N = self.B, self.N
        given = seed_x if seed_x is not None else seed_u
        if given is None:
            S, squeeze = 2, False
        else:
            squeeze = np.ndim(given) == 3
            S = 1 if squeeze else int(np.shape(given)[1])
        sx = None if seed_x is None else _f64(np.asarray(seed_x, dtype=np.float64).reshape(B, S, N + 1, NX), (B, S, N + 1, NX), "seed_x")
        su = None if seed_u is None else _f64(np.asarray(seed_u, dtype=np.float64).reshape(B, S, N, NU), (B, S, N, NU), "seed_u")
        out = dict(x0=np.empty((B, S, NX)), yref=np.empty((B, S, N, NY)), yref_e=np.empty((B, S, NX)))
        if weights:
            out.update(W=np.empty((B, S, NY, NY)), W_e=np.empty((B, S, NX, NX)))
        fn = self.lib.ihm2mpc_eval_adjoint_sensitivities_w if weights else self.lib.ihm2mpc_eval_adjoint_sensitivities
        _lib.check(fn(self._h, S, None if sx is None else _ptr(sx), None if su is None else _ptr(su), *[_ptr(v) for v in out.values()]))
        return {k: v[:, 0] for k, v in out.items()} if squeeze else out

    def eval_adjoint_weight_sensitivities(self, seed_x=None, seed_u=None):
        """``eval_adjoint_sensitivities`` with the gradients in the cost weights: ``dict(x0, yref, yref_e, W=(B,S,12,12),
        W_e=(B,S,8,8))``, the first three the same bits.  ``W = -c_s sum_k sym((V zeta_k) e_k')`` with ``e_k = V z_k - yref_k`` at the
        returned solution and ``W_e = -sym(zeta_N (x_N - yref_e)')``: the gradients on the symmetric matrices, ``dL = <W, dW> +
        <W_e, dW_e>`` for a symmetric change ``dW`` common to all stages (the diagonal entry is ``dL/dq_i`` of a diagonal weight).  Same
        seed shapes, squeeze rule, preconditions and NaN rows as ``eval_adjoint_sensitivities``
        (``ihm2mpc_eval_adjoint_sensitivities_w``).  Bounds are not differentiated."""
        return self._eval_adjoint(seed_x, seed_u, True)

    def du0_dW(self):
        """``dict(W=(B,2,12,12), W_e=(B,2,8,8))``: the derivative of the first control of the last solve in the cost weights (the two
        unit seeds on ``u_0``)."""
        out = dict(W=np.empty((self.B, 2, NY, NY)), W_e=np.empty((self.B, 2, NX, NX)))
        _lib.check(self.lib.ihm2mpc_eval_adjoint_sensitivities_w(self._h, 2, None, None, None, None, None, _ptr(out["W"]), _ptr(out["W_e"])))
        return out

    # ---- the objective and its total gradient (acados: get_cost, eval_and_get_optimal_value_gradient) ----
    def get_cost(self, stagewise: bool = False):
        """The objective at the current iterate (after a solve: at the returned solution), as acados documents ``get_cost`` with the
        stage terms scaled by ``cost_scale_stage``: ``J = sum_k (c_s/2) e_k' W_k e_k + 1/2 e_N' W_e e_N`` plus the slack penalties
        ``z s + 1/2 Z s^2`` of the soft sides.  ``(B,)``, or with ``stagewise`` the terms of the stages ``(B, N+1)``, whose sum it is.
        Works in both solver modes, on every constraint table and at any time (``ihm2mpc_eval_cost``)."""
        out = np.empty((self.B, self.N + 1)) if stagewise else np.empty(self.B)
        _lib.check(self.lib.ihm2mpc_eval_cost(self._h, None if stagewise else _ptr(out), _ptr(out) if stagewise else None, None))
        return out

    def get_slack_cost(self):
        """``(B,)``: the part of :meth:`get_cost` that comes from the slack penalties of the soft sides."""
        out = np.empty(self.B)
        _lib.check(self.lib.ihm2mpc_eval_cost(self._h, None, None, _ptr(out)))
        return out

    def eval_cost_gradient(self):
        """The cost of the last RTI solve and its total derivative through the QP-solution map: ``dict(cost=(B,), x0=(B,8),
        yref=(B,N,12), yref_e=(B,8), W=(B,12,12), W_e=(B,8,8), seed_x=(B,N+1,8), seed_u=(B,N,2))``.  ``seed_x``, ``seed_u`` are
        ``dJ/dx_k``, ``dJ/du_k`` -- the seeds ``eval_adjoint_weight_sensitivities`` would be given -- and the five gradients are its
        outputs for them plus the explicit partials of ``J`` (``x0``: the value-function gradient of the RTI step, no explicit part).
        ``W`` is the derivative in a change common to all stages; ``W`` and ``W_e`` are exactly symmetric.  NaN gradients for
        instances whose status is neither 0 nor 2.  Preconditions of ``eval_adjoint_sensitivities``; all-hard constraint tables only
        (``ihm2mpc_eval_cost_gradient``)."""
        B, N = self.B, self.N
        out = dict(cost=np.empty(B), x0=np.empty((B, NX)), yref=np.empty((B, N, NY)), yref_e=np.empty((B, NX)), W=np.empty((B, NY, NY)),
                   W_e=np.empty((B, NX, NX)), seed_x=np.empty((B, N + 1, NX)), seed_u=np.empty((B, N, NU)))
        _lib.check(self.lib.ihm2mpc_eval_cost_gradient(self._h, *[_ptr(v) for v in out.values()]))
        return out

    def eval_cost_gradient_soft(self):
        """:meth:`eval_cost_gradient` on every constraint table: the slack penalties' own seed ``dJ/ds_i = z_i + Z_i s_i`` is folded
        onto the stage seeds before the adjoint runs, so ``seed_x``, ``seed_u`` come back as the seeds the adjoint saw.  The same dict;
        on a table without a soft side the same bits (``ihm2mpc_eval_cost_gradient_soft``)."""
        B, N = self.B, self.N
        out = dict(cost=np.empty(B), x0=np.empty((B, NX)), yref=np.empty((B, N, NY)), yref_e=np.empty((B, NX)), W=np.empty((B, NY, NY)),
                   W_e=np.empty((B, NX, NX)), seed_x=np.empty((B, N + 1, NX)), seed_u=np.empty((B, N, NU)))
        _lib.check(self.lib.ihm2mpc_eval_cost_gradient_soft(self._h, *[_ptr(v) for v in out.values()]))
        return out

    def eval_adjoint_slack_sensitivities(self, seed_x=None, seed_u=None, seed_s=None, seed_sa=None):
        """``eval_adjoint_weight_sensitivities`` for functions ``L`` that also depend on the soft slacks: ``seed_s`` ``(B,S,N+1,28)`` =
        ``dL/ds`` in the layout of ``get_slacks`` (14 lower sides, 14 upper sides), ``seed_sa`` ``(B,S,N+1,2)`` for the slacks of the
        lateral-acceleration row (``get_alat_multipliers``); the ``S`` axis may be dropped on all of them, as there.  A seed on a side
        without a slack is ignored.  Any seed may be ``None`` = zero; all four ``None``: the two unit seeds on ``u_0``.  Returns the
        dict of ``eval_adjoint_weight_sensitivities``; without slack seeds the same bits (``ihm2mpc_eval_adjoint_sensitivities_s``)."""
        B, N = self.B, self.N
        S, squeeze, ptrs = self._slack_seed_args(seed_x, seed_u, seed_s, seed_sa)
        out = dict(x0=np.empty((B, S, NX)), yref=np.empty((B, S, N, NY)), yref_e=np.empty((B, S, NX)), W=np.empty((B, S, NY, NY)),
                   W_e=np.empty((B, S, NX, NX)))
        _lib.check(self.lib.ihm2mpc_eval_adjoint_sensitivities_s(self._h, S, *[None if p is None else _ptr(p) for p in ptrs],
                                                                 *[_ptr(v) for v in out.values()]))
        return {k: v[:, 0] for k, v in out.items()} if squeeze else out

    def _slack_seed_args(self, seed_x, seed_u, seed_s, seed_sa):
        """``(S, squeeze, the four seed arrays or None)`` of the entries that take seeds on the slacks."""
        B, N = self.B, self.N
        shapes = dict(seed_x=(N + 1, NX), seed_u=(N, NU), seed_s=(N + 1, 28), seed_sa=(N + 1, 2))
        seeds = dict(seed_x=seed_x, seed_u=seed_u, seed_s=seed_s, seed_sa=seed_sa)
        given = next((v for v in seeds.values() if v is not None), None)
        if given is None:
            S, squeeze = 2, False
        else:
            squeeze = np.ndim(given) == 3
            S = 1 if squeeze else int(np.shape(given)[1])
        ptrs = []
        for name, v in seeds.items():
            shape = (B, S) + shapes[name]
            ptrs.append(None if v is None else _f64(np.asarray(v, dtype=np.float64).reshape(shape), shape, name))
        return S, squeeze, ptrs

    # ---- gradients in the slack penalties of the soft sides ----
    def eval_adjoint_penalty_sensitivities(self, seed_x=None, seed_u=None, seed_s=None, seed_sa=None):
        """``eval_adjoint_slack_sensitivities`` with the gradients in the slack penalties: its dict (the same bits) plus ``soft_z``,
        ``soft_Z`` ``(B,S,N+1,28)`` in the layout of ``set_soft`` / ``get_slacks``, ``alat_soft_z``, ``alat_soft_Z`` ``(B,S,N+1,2)`` for
        the two sides of the lateral-acceleration row, and ``zeta`` ``(B,S,N+1,10)``, the adjoint solution ``(zeta_x,k, zeta_u,k)``.
        ``soft_z = -zeta_s``, ``soft_Z = -s zeta_s`` with ``zeta_s`` the slack component of the adjoint; 0 on a side without a slack or
        with a zero multiplier, so the sum over the batch is the gradient in the shared table.  With per-instance penalties
        (:meth:`set_instance_soft`, :meth:`set_instance_alat_soft`) the rows are each instance's own: row ``b`` is the gradient in
        instance ``b``'s penalties, at its values.  Bounds are not differentiated (``ihm2mpc_eval_adjoint_sensitivities_p``)."""
        B, N = self.B, self.N
        S, squeeze, ptrs = self._slack_seed_args(seed_x, seed_u, seed_s, seed_sa)
        out = dict(x0=np.empty((B, S, NX)), yref=np.empty((B, S, N, NY)), yref_e=np.empty((B, S, NX)), W=np.empty((B, S, NY, NY)),
                   W_e=np.empty((B, S, NX, NX)), soft_z=np.empty((B, S, N + 1, NLAM)), soft_Z=np.empty((B, S, N + 1, NLAM)),
                   alat_soft_z=np.empty((B, S, N + 1, 2)), alat_soft_Z=np.empty((B, S, N + 1, 2)), zeta=np.empty((B, S, N + 1, NX + NU)))
        _lib.check(self.lib.ihm2mpc_eval_adjoint_sensitivities_p(self._h, S, *[None if p is None else _ptr(p) for p in ptrs],
                                                                 *[_ptr(v) for v in out.values()]))
        return {k: v[:, 0] for k, v in out.items()} if squeeze else out

    def eval_cost_gradient_penalties(self):
        """:meth:`eval_cost_gradient_soft` with the total derivative of the cost in the slack penalties: the same dict (the same bits)
        plus ``soft_z``, ``soft_Z`` ``(B,N+1,28)`` and ``alat_soft_z``, ``alat_soft_Z`` ``(B,N+1,2)``: ``dJ/dz = s - zeta_s``,
        ``dJ/dZ = s^2 / 2 - s zeta_s``; with per-instance penalties (:meth:`set_instance_soft`) the cost and the gradient rows are
        each instance's own (``ihm2mpc_eval_cost_gradient_penalties``)."""
        B, N = self.B, self.N
        out = dict(cost=np.empty(B), x0=np.empty((B, NX)), yref=np.empty((B, N, NY)), yref_e=np.empty((B, NX)), W=np.empty((B, NY, NY)),
                   W_e=np.empty((B, NX, NX)), soft_z=np.empty((B, N + 1, NLAM)), soft_Z=np.empty((B, N + 1, NLAM)),
                   alat_soft_z=np.empty((B, N + 1, 2)), alat_soft_Z=np.empty((B, N + 1, 2)), seed_x=np.empty((B, N + 1, NX)),
                   seed_u=np.empty((B, N, NU)))
        _lib.check(self.lib.ihm2mpc_eval_cost_gradient_penalties(self._h, *[_ptr(v) for v in out.values()]))
        return out

    def du0_dsoft(self):
        """``dict(soft_z, soft_Z (B,2,N+1,28), alat_soft_z, alat_soft_Z (B,2,N+1,2))``: the derivative of the first control of the last
        solve in the slack penalties (the two unit seeds on ``u_0``).  With per-instance penalties (:meth:`set_instance_soft`) row
        ``b`` is the derivative in instance ``b``'s own penalties: one launch differentiates a whole penalty sweep."""
        g = self.eval_adjoint_penalty_sensitivities()
        return {k: g[k] for k in ("soft_z", "soft_Z", "alat_soft_z", "alat_soft_Z")}

    def du0_ds_target(self):
        """``(B,2)``: the reaction of the first control of the last solve to ``prepare_step``'s ``s_target`` -- the reference ramp puts
        ``(j / N) s_target`` into ``yref_j[0]`` and ``s_target`` into ``yref_e[0]``, so it is
        ``sum_j (j / N) du_0/dyref_j[0] + du_0/dyref_e[0]``."""
        g = self.eval_adjoint_sensitivities()
        ramp = np.arange(self.N) / self.N
        return g["yref"][:, :, :, 0] @ ramp + g["yref_e"][:, :, 0]

    # ---- plant ----
    def sim_step(self, x, u, model: int = 0, M_sim: int = 100):
        x = _f64(x, (self.B, NX), "x"); u = _f64(u, (self.B, NU), "u")
        out = np.empty((self.B, NX))
        _lib.check(self.lib.ihm2mpc_sim_step(self._h, int(model), int(M_sim), _ptr(x), _ptr(u), _ptr(out)))
        return out

    def sim_step_sens(self, x, u, model: int = 0, M_sim: int = 100):
        """Plant step with forward sensitivities (acados: ``AcadosSimSolver.solve()`` with ``sens_forw``): ``dict(x=(B,8), Sx=(B,8,8),
        Su=(B,8,2), model_used=(B,) int32)`` with ``Sx[b,i,j] = dx_next,i/dx_j``, ``Su[b,i,j] = dx_next,i/du_j`` -- the exact derivative
        of the handle's plant integrator with ``M_sim`` steps -- and the model that integrated instance ``b`` (for the switched plants
        ``model = -1 / -2`` the branch taken, whose derivative it is: the rule is piecewise).  ``ihm2mpc_sim_step_sens``; nothing else of
        the solver changes."""
        x = _f64(x, (self.B, NX), "x"); u = _f64(u, (self.B, NU), "u")
        out = dict(x=np.empty((self.B, NX)), Sx=np.empty((self.B, NX, NX)), Su=np.empty((self.B, NX, NU)), model_used=np.empty(self.B, dtype=np.int32))
        _lib.check(self.lib.ihm2mpc_sim_step_sens(self._h, int(model), int(M_sim), _ptr(x), _ptr(u), _ptr(out["x"]), _ptr(out["Sx"]), _ptr(out["Su"]),
                                                  out["model_used"].ctypes.data_as(_lib.c_int32_p)))
        return out

    def sim_step_sens_device(self, x_dptr: int, u_dptr: int, model: int = 0, M_sim: int = 100, x_next: int = 0, Sx: int = 0, Su: int = 0,
                             model_used: int = 0):
        """The same on device (or pinned host) memory, stream-ordered: addresses as integers, 0 = that output is not wanted."""
        ptr = [C.c_void_p(int(a)) if a else None for a in (x_next, Sx, Su, model_used)]
        _lib.check(self.lib.ihm2mpc_sim_step_sens_device(self._h, int(model), int(M_sim), C.c_void_p(int(x_dptr)), C.c_void_p(int(u_dptr)), *ptr))

    def closed_loop_matrix(self, model: int = 0, M_sim: int = 100):
        """``A_cl = Sx + Su @ K0`` ``(B,8,8)``: the plant's Jacobian at the handle's ``(x0, u0)`` closed with the gain ``K0 = du_0/dx_0`` of
        the last solve -- the linearised closed loop of one control period, whose spectral radius says whether a tuning is linearly
        stable on that plant.  Needs ``set_x0_sensitivities(1 or 2)`` before the solve (refused otherwise, as ``get_x0_sensitivities``
        is); NaN rows where ``K0`` has them (status neither 0 nor 2)."""
        _, su = self.get_x0_sensitivities()
        K0 = su[:, 0] if su.ndim == 4 else su
        s = self.sim_step_sens(self.get_x0(), self.get_u0(), model=model, M_sim=M_sim)
        return s["Sx"] + s["Su"] @ K0

    # ---- Cartesian side of the ROS stack (plants of sim_node.cpp, Track::project) ----
    def set_track_geometry(self, X_ref, Y_ref, phi_ref):
        """Centre line on the ``s_ref`` grid, ``(ntracks, nknots)`` each (the track-file columns of ``tracks.cpp:132-181``)."""
        arrs = [_f64(np.atleast_2d(a), (self.ntracks, self.nknots), n) for a, n in ((X_ref, "X_ref"), (Y_ref, "Y_ref"), (phi_ref, "phi_ref"))]
        _lib.check(self.lib.ihm2mpc_set_track_geometry(self._h, *[_ptr(a) for a in arrs]))

    def sim_step_cart(self, x, u, model: int = -3, M_sim: int = 10, dt_sim: float = 0.01, n_steps: int = 5, v_dyn: float = 3.0):
        """``n_steps`` plant steps of ``dt_sim`` under a constant ``u``; model 3 = kin6, 4 = dyn6, -3 = the node's switch."""
        x = _f64(x, (self.B, NX), "x"); u = _f64(u, (self.B, NU), "u")
        out = np.empty((self.B, NX))
        _lib.check(self.lib.ihm2mpc_sim_step_cart(self._h, int(model), int(M_sim), float(dt_sim), int(n_steps), float(v_dyn), _ptr(x), _ptr(u), _ptr(out)))
        return out

    def project(self, x_cart, s_guess, s_tol: float = 2.0):
        """Cartesian states ``(B,8)`` -> Frenet states ``(B,8)`` and the next projection guess ``(B,)``."""
        xc = _f64(x_cart, (self.B, NX), "x_cart"); sg = _f64(s_guess, (self.B,), "s_guess").copy()
        out = np.empty((self.B, NX))
        _lib.check(self.lib.ihm2mpc_project(self._h, _ptr(xc), _ptr(sg), float(s_tol), _ptr(out)))
        return out, sg

    def set_cart_state(self, x_cart, s_guess):
        _lib.check(self.lib.ihm2mpc_set_cart_state(self._h, _ptr(_f64(x_cart, (self.B, NX), "x_cart")), _ptr(_f64(s_guess, (self.B,), "s_guess"))))

    def get_cart_state(self):
        xc = np.empty((self.B, NX)); sg = np.empty(self.B)
        _lib.check(self.lib.ihm2mpc_get_cart_state(self._h, _ptr(xc), _ptr(sg)))
        return xc, sg

    def sim_advance_cart(self, model: int = -3, M_sim: int = 10, dt_sim: float = 0.01, n_steps: int = 5, v_dyn: float = 3.0, s_tol: float = 2.0):
        """On device: x_cart <- plant(x_cart, u0 of the last solve); x0 <- project(x_cart)."""
        _lib.check(self.lib.ihm2mpc_sim_advance_cart(self._h, int(model), int(M_sim), float(dt_sim), int(n_steps), float(v_dyn), float(s_tol)))

    def sim_advance(self, model: int = 0, M_sim: int = 100):
        """x0 <- plant(x0, u0 of the last solve), on device."""
        _lib.check(self.lib.ihm2mpc_sim_advance(self._h, int(model), int(M_sim)))

    def alloc_pinned(self, shape):
        """float64 array in pinned host memory (for :meth:`get_u0_async`); freed with the solver."""
        n = int(np.prod(shape))
        ptr = C.c_void_p()
        _lib.check(self.lib.ihm2mpc_host_alloc(C.c_uint64(n * 8), C.byref(ptr)))
        self._pinned = getattr(self, "_pinned", []) + [ptr]
        return np.ctypeslib.as_array(C.cast(ptr, _lib.c_double_p), shape=(n,)).reshape(shape)

    def get_u0_async(self, out):
        """Enqueue the copy of ``u0`` (B,2) into the pinned array ``out``; valid after :meth:`synchronize`."""
        if out.shape != (self.B, NU) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 (B, 2) array from alloc_pinned")
        _lib.check(self.lib.ihm2mpc_get_u0_async(self._h, _ptr(out)))

    def set_lap_wrap(self, enable: bool = True):
        """Keep endless closed loops inside the three-lap track tables: cars past ``s = L`` are moved back by one lap."""
        _lib.check(self.lib.ihm2mpc_set_lap_wrap(self._h, int(bool(enable))))

    def set_active(self, active=None):
        """Plant mask for ``sim_advance`` / ``step``: instances with ``active[b] == 0`` keep their ``x0``; ``None`` = all.
        ``run_steps(freeze=True)`` clears entries of this mask as cars stop; without a mask from here it keeps one of its own, which
        only later ``run_steps(freeze=True)`` calls read (``step`` / ``sim_advance`` / ``freeze=False`` do not), until ``set_active(None)``."""
        if active is None:
            _lib.check(self.lib.ihm2mpc_set_active(self._h, None))
        else:
            a = np.ascontiguousarray(active, dtype=np.int32)
            if a.shape != (self.B,):
                raise ValueError(f"active must have shape ({self.B},)")
            _lib.check(self.lib.ihm2mpc_set_active(self._h, a.ctypes.data_as(_lib.c_int32_p)))

    def step(self, s_target: float, model: int = 0, M_sim: int = 100):
        """One MiL iteration on the device: ``sim_advance`` + ``prepare_step`` + one RTI iteration, with the plant step
        overlapped with the linearisation.  Asynchronous; read results with ``get_u0`` / ``get_status``."""
        _lib.check(self.lib.ihm2mpc_step(self._h, int(model), int(M_sim), float(s_target)))

    # ---- single stage of a single instance ----
    def _set_stage(self, i, stage, field, value):
        v = _f64(np.ravel(value))
        _lib.check(self.lib.ihm2mpc_set_stage(self._h, i, stage, field.encode(), _ptr(v), v.size))

    def _get_stage(self, i, stage, field, n):
        out = np.empty(n)
        _lib.check(self.lib.ihm2mpc_get_stage(self._h, i, stage, field.encode(), _ptr(out), n))
        return out


# The serial number of a solver: every solving call and every setter advances it.  The adjoint entries differentiate the last solve and must
# follow it directly (include/ihm2mpc.h), which the library does not detect; a caller that keeps the serial of its solve can
# (ihm2_amd/torch_layer.py: backward refuses when it has moved).  Getters and the eval_* entries leave it alone.
_ADVANCES_SERIAL = ("init_guess", "reinit_failed", "prepare_step", "solve_async", "compute_control", "run_steps", "linearize", "build_tracks",
                    "fit_tracks", "sim_advance", "sim_advance_cart", "step", "_set_stage")


def _advancing(fn):
    @functools.wraps(fn)
    def wrapped(self, *args, **kw):
        self._serial += 1
        return fn(self, *args, **kw)
    return wrapped


BatchedOcpSolver._serial = 0
for _name, _fn in list(vars(BatchedOcpSolver).items()):
    if callable(_fn) and (_name.startswith(("set_", "_push_")) or _name in _ADVANCES_SERIAL):
        setattr(BatchedOcpSolver, _name, _advancing(_fn))
del _name, _fn


class AcadosOcpSolver:
    """Per-instance shim with the method names and semantics of ``acados_template.AcadosOcpSolver`` as
    the reference uses them.  Built from an OCP it owns a batch of one; ``batch[i]`` gives a view."""

    def __init__(self, ocp: AcadosOcp, json_file: str | None = None, verbose: bool = False, *, s_ref=None, kappa_ref=None,
                 device: int = 0):
        n_half = ocp.dims.np // 2
        if s_ref is None:           # placeholder table until set(i, "p", p) arrives (python/main.py:249-252)
            s_ref = np.arange(n_half, dtype=np.float64)
            kappa_ref = np.zeros(n_half)
        self.batch = BatchedOcpSolver(ocp, 1, s_ref, kappa_ref, device=device)
        self.i = 0
        self._owner = True

    @classmethod
    def _view(cls, batch: BatchedOcpSolver, i: int) -> "AcadosOcpSolver":
        self = cls.__new__(cls)
        self.batch, self.i, self._owner = batch, i, False
        return self

    @property
    def N(self):
        return self.batch.N

    # -- set -------------------------------------------------------------------------------------
    def set(self, stage: int, field: str, value) -> None:
        b = self.batch
        if field == "p":
            p = _f64(np.ravel(value))
            if p.size != 2 * b.nknots:
                raise ValueError(f"p must have {2 * b.nknots} entries [s_ref; kappa_ref], got {p.size}")
            t = int(b._track_id[self.i])       # the table is per track, not per stage: same p for all stages
            if not (np.array_equal(b._s_ref[t], p[:b.nknots]) and np.array_equal(b._kappa_ref[t], p[b.nknots:])):
                b._s_ref[t], b._kappa_ref[t] = p[:b.nknots], p[b.nknots:]
                b._push_tracks()
        elif field in ("lbx", "ubx"):
            self.constraints_set(stage, field, value)
        elif field in ("x", "u", "pi", "lam"):
            b._set_stage(self.i, stage, field, value)
        elif field in ("yref", "y_ref"):
            v = np.ravel(value)
            if stage == b.N:
                # the C++ node hands a 12-vector at the terminal stage too (quirk Q8): keep the first 8
                b._set_stage(self.i, 0, "yref_e", v[:NX])
            else:
                b._set_stage(self.i, stage, "yref", v)
        else:
            raise Exception(f"AcadosOcpSolver.set(): '{field}' is not a valid argument.")

    def cost_set(self, stage: int, field: str, value, api: str = "warn") -> None:
        """Writes the batch-SHARED weight table (every instance of the batch sees it); per-instance weights go through
        ``BatchedOcpSolver.set_instance_weights``."""
        if field != "W":
            raise Exception(f"AcadosOcpSolver.cost_set(): '{field}' is not a valid argument.")
        b = self.batch
        W = np.asarray(value, dtype=np.float64)
        if stage == b.N:
            if W.shape != (NX, NX):
                raise Exception(f"terminal W must be {NX}x{NX}")
            b.data.W_e = W.copy()
        else:
            if W.shape != (NY, NY):
                raise Exception(f"stage W must be {NY}x{NY}")
            b.data.W[stage] = W
        b._push_weights()

    def constraints_set(self, stage: int, field: str, value, api: str = "warn") -> None:
        """Stage 0's lbx/ubx set this instance's x0; every other field writes the batch-SHARED bound table.  Per-instance
        bounds go through ``BatchedOcpSolver.set_instance_bounds``."""
        b, d, c = self.batch, self.batch.data, self.batch.ocp.constraints
        v = np.asarray(value, dtype=np.float64)
        if field in ("lbx", "ubx") and stage == 0:
            b._set_stage(self.i, 0, field, v)      # initial-state equality (python/main.py:299-300)
            return
        if field in ("lbx", "ubx"):
            idx = np.asarray(c.idxbx_e if stage == b.N else c.idxbx, dtype=int)
            getattr(d, field)[stage, idx] = v
        elif field in ("lbu", "ubu"):
            getattr(d, field)[stage, np.asarray(c.idxbu, dtype=int)] = v
        elif field in ("C", "D"):
            getattr(d, field)[stage, :v.shape[0]] = v
        elif field in ("lg", "ug"):
            getattr(d, field)[stage, :v.size] = v
        else:
            raise Exception(f"AcadosOcpSolver.constraints_set(): '{field}' is not a valid argument.")
        b._push_bounds()

    # -- solve / get -----------------------------------------------------------------------------
    def solve(self) -> int:
        """Runs the solver (for a view: the whole batch) and returns this instance's status."""
        return int(self.batch.solve()[self.i])

    def eval_param_sens(self, index: int, stage: int = 0, field: str = "ex") -> None:
        """acados' ``eval_param_sens``: the sensitivities of the last solution with respect to ``x0[index]``, read afterwards by
        ``get(k, "sens_x")`` / ``get(k, "sens_u")``.  Only ``field = "ex"`` at stage 0 exists here; the batch computes them in its
        solves once ``BatchedOcpSolver.set_x0_sensitivities`` is on (mode 1: ``get(0, "sens_u")`` only)."""
        if field != "ex":
            raise Exception(f"AcadosOcpSolver.eval_param_sens(): field '{field}' is not supported (only 'ex', the initial state)")
        if stage != 0:
            raise Exception("AcadosOcpSolver.eval_param_sens(): the initial state is a parameter of stage 0 only")
        if not 0 <= int(index) < NX:
            raise Exception(f"AcadosOcpSolver.eval_param_sens(): index {index} out of range [0, {NX})")
        if self.batch._sens_mode == 0:
            raise Exception("AcadosOcpSolver.eval_param_sens(): x0 sensitivities are off -- call set_x0_sensitivities(1 or 2) on the "
                            "batch before solve()")
        sx, su = self.batch.get_x0_sensitivities()
        j = int(index)
        self._sens = (None if sx is None else sx[self.i, :, :, j].copy(), su[self.i, ..., j].copy())

    def eval_adjoint_solution_sensitivity(self, seed_x, seed_u, with_respect_to: str = "x0", sanity_checks: bool = True) -> np.ndarray:
        """acados' ``eval_adjoint_solution_sensitivity``: ``seed_x`` / ``seed_u`` lists of ``(stage, array (nx | nu, n_seeds))`` (either may
        be ``None`` or empty), the gradient of ``sum_k seed_x[k]' x_k + seed_u[k]' u_k`` of this instance's last solution, one row per
        seed: ``with_respect_to`` ``"x0"`` ``(n_seeds, 8)``, ``"yref"`` ``(n_seeds, N, 12)`` or ``"yref_e"`` ``(n_seeds, 8)``.  acados
        differentiates in ``"p_global"``; this OCP has no global parameters (the track tables are data of the batch), so that raises."""
        if with_respect_to == "p_global":
            raise Exception("AcadosOcpSolver.eval_adjoint_solution_sensitivity(): this OCP has no p_global (the track tables are batch data, "
                            "not parameters); the solve's inputs are with_respect_to = 'x0', 'yref' or 'yref_e'")
        if with_respect_to not in ("x0", "yref", "yref_e"):
            raise Exception(f"AcadosOcpSolver.eval_adjoint_solution_sensitivity(): with_respect_to '{with_respect_to}' is not supported "
                            "('x0', 'yref', 'yref_e')")
        sx, su = self._adjoint_seeds(seed_x, seed_u, "eval_adjoint_solution_sensitivity")
        return self.batch.eval_adjoint_sensitivities(sx, su)[with_respect_to][self.i].copy()

    def _adjoint_seeds(self, seed_x, seed_u, who: str):
        """The batch's seed arrays (B,S,N+1,8), (B,S,N,2) from acados' lists of ``(stage, array (nx | nu, n_seeds))``: this instance's
        rows, zero elsewhere."""
        pairs = [(st, np.asarray(v, dtype=np.float64), n, nm) for lst, n, nm in ((seed_x, NX, "seed_x"), (seed_u, NU, "seed_u"))
                 for st, v in (lst or [])]
        if not pairs:
            raise Exception(f"AcadosOcpSolver.{who}(): seed_x and seed_u are both empty")
        b = self.batch
        S = pairs[0][1].shape[1] if pairs[0][1].ndim == 2 else 0
        sx, su = np.zeros((b.B, S, b.N + 1, NX)), np.zeros((b.B, S, b.N, NU))
        for st, v, n, nm in pairs:
            if v.shape != (n, S) or not 0 <= int(st) <= (b.N if n == NX else b.N - 1):
                raise Exception(f"AcadosOcpSolver.{who}(): {nm} entries are (stage, array ({n}, n_seeds)) "
                                f"with one n_seeds, got stage {st}, shape {v.shape}")
            (sx if n == NX else su)[self.i, :, int(st), :] += v.T
        return sx, su

    def eval_adjoint_weight_sensitivity(self, seed_x, seed_u):
        """The gradient of ``sum_k seed_x[k]' x_k + seed_u[k]' u_k`` of this instance's last solution in the cost weights: seeds as for
        ``eval_adjoint_solution_sensitivity``, returns ``(grad_W (n_seeds, 12, 12), grad_W_e (n_seeds, 8, 8))``
        (``BatchedOcpSolver.eval_adjoint_weight_sensitivities``).  acados has no counterpart."""
        sx, su = self._adjoint_seeds(seed_x, seed_u, "eval_adjoint_weight_sensitivity")
        g = self.batch.eval_adjoint_weight_sensitivities(sx, su)
        return g["W"][self.i].copy(), g["W_e"][self.i].copy()

    def eval_adjoint_penalty_sensitivity(self, seed_x, seed_u):
        """The gradient of ``sum_k seed_x[k]' x_k + seed_u[k]' u_k`` of this instance's last solution in the slack penalties: seeds as for
        ``eval_adjoint_solution_sensitivity``, returns ``dict(soft_z, soft_Z (n_seeds, N+1, 28), alat_soft_z, alat_soft_Z
        (n_seeds, N+1, 2))`` (``BatchedOcpSolver.eval_adjoint_penalty_sensitivities``).  acados has no counterpart."""
        sx, su = self._adjoint_seeds(seed_x, seed_u, "eval_adjoint_penalty_sensitivity")
        g = self.batch.eval_adjoint_penalty_sensitivities(sx, su)
        return {k: g[k][self.i].copy() for k in ("soft_z", "soft_Z", "alat_soft_z", "alat_soft_Z")}

    def get_cost(self) -> float:
        """acados' ``get_cost``: the objective at this instance's current iterate, stage terms scaled by ``cost_scale_stage``
        (``BatchedOcpSolver.get_cost``)."""
        return float(self.batch.get_cost()[self.i])

    def eval_and_get_optimal_value_gradient(self, with_respect_to: str = "initial_state") -> np.ndarray:
        """acados' ``eval_and_get_optimal_value_gradient``: ``(8,)``, the gradient of this instance's cost in the initial state.  Named
        difference: acados differentiates the optimal value of a converged NLP, this is the derivative of the cost of the last RTI
        step's solution through that step's QP (``BatchedOcpSolver.eval_cost_gradient``)."""
        if with_respect_to == "p_global":
            raise Exception("AcadosOcpSolver.eval_and_get_optimal_value_gradient(): this OCP has no p_global (the track tables are batch "
                            "data, not parameters); with_respect_to = 'initial_state' is supported")
        if with_respect_to != "initial_state":
            raise Exception(f"AcadosOcpSolver.eval_and_get_optimal_value_gradient(): with_respect_to '{with_respect_to}' is not supported "
                            "('initial_state')")
        return self.batch.eval_cost_gradient()["x0"][self.i].copy()

    def eval_and_get_optimal_value_gradient_soft(self, with_respect_to: str = "initial_state") -> np.ndarray:
        """:meth:`eval_and_get_optimal_value_gradient` on every constraint table, soft sides included
        (``BatchedOcpSolver.eval_cost_gradient_soft``)."""
        if with_respect_to != "initial_state":
            return self.eval_and_get_optimal_value_gradient(with_respect_to)        # raises
        return self.batch.eval_cost_gradient_soft()["x0"][self.i].copy()

    def get(self, stage: int, field: str) -> np.ndarray:
        if field in ("sens_x", "sens_u"):
            sens = getattr(self, "_sens", None)
            if sens is None:
                raise Exception(f"AcadosOcpSolver.get(): '{field}' needs eval_param_sens() first")
            sx, su = sens
            if field == "sens_x":
                if sx is None:
                    raise Exception("AcadosOcpSolver.get(): 'sens_x' needs x0 sensitivity mode 2 (mode 1 holds du_0/dx_0 only)")
                return sx[stage].copy()
            if su.ndim == 1:            # mode 1: stage 0 only
                if stage != 0:
                    raise Exception("AcadosOcpSolver.get(): x0 sensitivity mode 1 holds 'sens_u' of stage 0 only")
                return su.copy()
            return su[stage].copy()
        sizes = {"x": NX, "u": NU, "pi": NX, "lam": NLAM}
        if field not in sizes:
            raise Exception(f"AcadosOcpSolver.get(): '{field}' is not a valid argument.")
        return self.batch._get_stage(self.i, stage, field, sizes[field])

    def get_stats(self, field: str):
        if field == "residuals":
            return self.batch.get_residuals()[self.i]
        if field == "qp_iter":
            return int(self.batch.get_qp_iter()[self.i])
        if field in ("sqp_iter", "alpha"):
            if self.batch.data.nlp_solver_type != "SQP":
                return 1 if field == "sqp_iter" else 1.0
            return self.batch.get_sqp_stats()[field][self.i].item()
        if field == "time_tot":
            return self.batch.get_timings()["total_ms"] * 1e-3
        raise Exception(f"AcadosOcpSolver.get_stats(): '{field}' is not a valid argument.")

    def get_status(self) -> int:
        return int(self.batch.get_status()[self.i])


def get_acados_solver(ocp: AcadosOcp, opts: AcadosOcpOptions, gen_code_dir: str | None = None, **kw) -> AcadosOcpSolver:
    """``python/mpc.py:104-113``; nothing is generated or compiled, ``gen_code_dir`` is accepted and ignored."""
    ocp.solver_options = opts
    return AcadosOcpSolver(ocp, json_file=None, verbose=False, **kw)
