"""One RTI step of the batched NMPC as a differentiable PyTorch function.

``rti_solve(solver, x0, yref, yref_e, W, W_e)`` feeds device tensors to a :class:`~ihm2_amd.solver.BatchedOcpSolver` through the
library's ``*_device`` entries, runs one RTI solve and returns ``(x, u, status)`` as tensors; ``backward`` is one call of
``ihm2mpc_eval_adjoint_sensitivities_w_device``.  Nothing passes through host memory and nothing waits for the GPU: the handle's stream
and torch's current stream are ordered against each other with events.

``rti_solve_soft`` is the same step with the soft constraints' side of it: per-instance slack penalties go in, the slack values come out,
and ``backward`` (one call of ``ihm2mpc_eval_adjoint_sensitivities_p_device``) also returns the gradients in the penalties.
``plant_step`` is the plant's step with its exact Jacobians as a differentiable function, so that a closed loop
``x_next = plant_step(solver, x, rti_solve_soft(solver, x, ...)[1][:, 0])`` can be written in torch and differentiated.

This module is the only one of the package that imports torch; ``import ihm2_amd`` stays torch-free.
"""
from __future__ import annotations

import weakref

import torch

from .constants import NLAM, NU, NX, NY

__all__ = ["rti_solve", "rti_solve_soft", "plant_step", "check_rti_inputs"]


def check_rti_inputs(B: int, N: int, device, x0, yref, yref_e, W=None, W_e=None, *, soft_z=None, soft_Z=None, alat_z=None, alat_Z=None) -> None:
    """The argument check of :func:`rti_solve` and :func:`rti_solve_soft`, before any GPU call: every tensor a contiguous float64 tensor
    on ``device`` with the shape ``x0 (B,8)``, ``yref (B,N,12)``, ``yref_e (B,8)``, ``W (B,12,12)``, ``W_e (B,8,8)``, ``soft_z``,
    ``soft_Z (B,N+1,28)``, ``alat_z``, ``alat_Z (B,2)``; ``W`` and ``W_e`` together or not at all, and so each penalty pair
    (keyword-only).  Raises ``TypeError`` (not a tensor, not float64) or ``ValueError`` (device, shape, layout, a pair given by
    halves), each naming the argument."""
    device = torch.device(device)
    for (na, a), (nb, b), what in ((("W", W), ("W_e", W_e), "W and W_e"), (("soft_z", soft_z), ("soft_Z", soft_Z), "soft_z and soft_Z"),
                                   (("alat_z", alat_z), ("alat_Z", alat_Z), "alat_z and alat_Z")):
        if (a is None) != (b is None):
            missing, given = (nb, na) if b is None else (na, nb)
            raise ValueError(f"{missing} is missing: {what} are given together or not at all ({given} was given)")
    shapes = {"x0": (B, NX), "yref": (B, N, NY), "yref_e": (B, NX), "W": (B, NY, NY), "W_e": (B, NX, NX), "soft_z": (B, N + 1, NLAM),
              "soft_Z": (B, N + 1, NLAM), "alat_z": (B, 2), "alat_Z": (B, 2)}
    for name, t in (("x0", x0), ("yref", yref), ("yref_e", yref_e), ("W", W), ("W_e", W_e), ("soft_z", soft_z), ("soft_Z", soft_Z),
                    ("alat_z", alat_z), ("alat_Z", alat_Z)):
        if t is None and name not in ("x0", "yref", "yref_e"):
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float64:
            raise TypeError(f"{name} must be float64, got {t.dtype}")
        if t.device != device:
            raise ValueError(f"{name} must be on {device} (the solver's device), it is on {t.device}")
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{name} must have shape {shapes[name]}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")


def _handle_stream(solver, device):
    return torch.cuda.ExternalStream(solver.get_stream(), device=device)


def _used_on(hs, solver, tensors):
    """The tensors the handle's stream touched: marked for the allocator (a block released while the stream still works on it is not
    handed out again before the stream has passed), and noted on the solver, whose ``free()`` refuses while the memory of one of them is alive -- the
    allocator records an event on the stream when it releases such a tensor, so the stream has to outlive it."""
    for t in tensors:
        t.record_stream(hs)
    # (the storages, not the tensors: a view keeps the block alive after the tensor it was taken from has gone)
    solver._stream_users = [r for r in getattr(solver, "_stream_users", ()) if r() is not None] + \
                           [weakref.ref(t.untyped_storage()) for t in tensors]


class _RtiSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, zero_failed, x0, yref, yref_e, W, W_e):
        B, N = solver.B, solver.N
        device = x0.device
        weights = W is not None
        cur = torch.cuda.current_stream(device)
        hs = _handle_stream(solver, device)
        if weights:     # the point the weights are taken at is the symmetric part: the setter is not asked to check (no read-back)
            Ws = ((W + W.transpose(1, 2)) * 0.5).contiguous()
            Wes = ((W_e + W_e.transpose(1, 2)) * 0.5).contiguous()
        x = torch.empty((B, N + 1, NX), dtype=torch.float64, device=device)
        u = torch.empty((B, N, NU), dtype=torch.float64, device=device)
        status = torch.empty((B,), dtype=torch.int32, device=device)
        hs.wait_stream(cur)
        solver.set_x0_device(x0.data_ptr())
        solver.set_yref_device(yref.data_ptr())
        solver.set_yref_e_device(yref_e.data_ptr())
        if weights:
            solver.set_instance_weights_device(Ws.data_ptr(), Wes.data_ptr(), check=False)
        solver.solve_async()
        solver.get_x_device(x.data_ptr())
        solver.get_u_device(u.data_ptr())
        solver.get_status_device(status.data_ptr())
        cur.wait_stream(hs)
        _used_on(hs, solver, [x0, yref, yref_e, x, u, status] + ([Ws, Wes] if weights else []))
        ctx.solver, ctx.serial, ctx.zero_failed, ctx.weights = solver, solver._serial, bool(zero_failed), weights
        ctx.save_for_backward(status)
        ctx.mark_non_differentiable(status)
        return x, u, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x, grad_u, _grad_status):
        solver = ctx.solver
        if solver._serial != ctx.serial:
            raise RuntimeError("rti_solve: the solver was used between this solve and its backward (a solve or a setter came in between): "
                               "the adjoint entry differentiates the last solve and must follow it directly")
        (status,) = ctx.saved_tensors
        B, N = solver.B, solver.N
        device = status.device
        kw = dict(dtype=torch.float64, device=device)
        sx = torch.zeros((B, 1, N + 1, NX), **kw) if grad_x is None else grad_x.reshape(B, 1, N + 1, NX).contiguous()
        su = torch.zeros((B, 1, N, NU), **kw) if grad_u is None else grad_u.reshape(B, 1, N, NU).contiguous()
        need = list(ctx.needs_input_grad[2:7])
        if not ctx.weights:
            need[3] = need[4] = False
        shapes = ((B, NX), (B, N, NY), (B, NX), (B, NY, NY), (B, NX, NX))
        grads = [torch.empty(sh, **kw) if nd else None for sh, nd in zip(shapes, need)]
        cur = torch.cuda.current_stream(device)
        hs = _handle_stream(solver, device)
        hs.wait_stream(cur)
        solver.eval_adjoint_weight_sensitivities_device(1, sx.data_ptr(), su.data_ptr(), *[0 if g is None else g.data_ptr() for g in grads])
        cur.wait_stream(hs)
        _used_on(hs, solver, [sx, su] + [g for g in grads if g is not None])
        if ctx.zero_failed:
            ok = (status == 0) | (status == 2)
            grads = [None if g is None else torch.where(ok.reshape((B,) + (1,) * (g.dim() - 1)), g, torch.zeros((), **kw)) for g in grads]
        # grad_W, grad_W_e are exactly symmetric (include/ihm2mpc.h): the derivative through the forward's (W + W') / 2 is themselves
        return (None, None, *grads)


def rti_solve(solver, x0, yref, yref_e, W=None, W_e=None, zero_failed: bool = False):
    """One RTI step of ``solver`` (a :class:`~ihm2_amd.solver.BatchedOcpSolver`) on device tensors, differentiable:
    ``(x (B,N+1,8), u (B,N,2), status (B,) int32)`` from ``x0 (B,8)``, ``yref (B,N,12)``, ``yref_e (B,8)`` and, optionally, per-instance
    weights ``W (B,12,12)``, ``W_e (B,8,8)`` (taken at their symmetric parts; without them the solver's weights stay as they are).  All
    tensors are contiguous float64 on the solver's device (:func:`check_rti_inputs`).  The solver must have
    ``set_x0_sensitivities(1 or 2)`` on, else the library's refusal is raised.

    What the derivative is: that of ONE RTI step -- the QP at the handle's current linearisation point (the iterate the solver holds
    when the call comes), solved by the interior point method, whose smoothing of the active set is part of the derivative.  The warm
    start (iterate, multipliers, slacks) is state of the solver, not an input: nothing is differentiated through it, and two calls
    with the same tensors differ if the solver's state does.  Bounds are not differentiated.  ``status`` is not differentiable.

    ``backward`` (once differentiable) is one call of the library's adjoint entry and must be the next use of the solver after its
    forward: it raises ``RuntimeError`` if a solve or a setter of the solver came in between.  Instances whose status is neither 0 nor
    2 have NaN gradient rows; ``zero_failed=True`` gives them zero rows instead (on the device, from the status).

    Lifetime: every tensor that goes in or comes out is marked as used on the solver's stream (``record_stream``), and PyTorch's
    allocator records an event on that stream when it releases such a tensor.  The solver must therefore outlive them:
    ``solver.free()`` raises ``RuntimeError`` while one is alive.  A solver that is garbage-collected without ``free()`` after it went
    through the layer keeps its handle to the process's end: in a collection the weak references the guard counts are cleared before
    the solver's finaliser runs, so it cannot tell whether the tensors have gone."""
    device = torch.device("cuda", solver.device)
    check_rti_inputs(solver.B, solver.N, device, x0, yref, yref_e, W, W_e)
    if not solver._sens_mode:
        solver.get_x0_sensitivities()       # raises the library's refusal: the mode is off
    return _RtiSolve.apply(solver, zero_failed, x0, yref, yref_e, W, W_e)


class _RtiSolveSoft(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, zero_failed, x0, yref, yref_e, W, W_e, soft_z, soft_Z, alat_z, alat_Z):
        B, N = solver.B, solver.N
        device = x0.device
        weights, soft, alat = W is not None, soft_z is not None, alat_z is not None
        cur = torch.cuda.current_stream(device)
        hs = _handle_stream(solver, device)
        if weights:
            Ws = ((W + W.transpose(1, 2)) * 0.5).contiguous()
            Wes = ((W_e + W_e.transpose(1, 2)) * 0.5).contiguous()
        kw = dict(dtype=torch.float64, device=device)
        x = torch.empty((B, N + 1, NX), **kw)
        u = torch.empty((B, N, NU), **kw)
        s = torch.empty((B, N + 1, NLAM), **kw)
        sa = torch.empty((B, N + 1, 2), **kw)
        status = torch.empty((B,), dtype=torch.int32, device=device)
        hs.wait_stream(cur)
        solver.set_x0_device(x0.data_ptr())
        solver.set_yref_device(yref.data_ptr())
        solver.set_yref_e_device(yref_e.data_ptr())
        if weights:
            solver.set_instance_weights_device(Ws.data_ptr(), Wes.data_ptr(), check=False)
        if soft:        # (the setters are not asked to check: no read-back)
            solver.set_instance_soft_device(soft_z.data_ptr(), soft_Z.data_ptr(), check=False)
        if alat:
            solver.set_instance_alat_soft_device(alat_z.data_ptr(), alat_Z.data_ptr(), check=False)
        solver.solve_async()
        solver.get_x_device(x.data_ptr())
        solver.get_u_device(u.data_ptr())
        solver.get_slacks_device(s.data_ptr(), sa.data_ptr())
        solver.get_status_device(status.data_ptr())
        cur.wait_stream(hs)
        _used_on(hs, solver, [x0, yref, yref_e, x, u, s, sa, status] + ([Ws, Wes] if weights else []) + ([soft_z, soft_Z] if soft else []) +
                 ([alat_z, alat_Z] if alat else []))
        ctx.solver, ctx.serial, ctx.zero_failed = solver, solver._serial, bool(zero_failed)
        ctx.given = (weights, soft, alat)
        ctx.set_materialize_grads(False)    # an output the loss does not use is no seed: without a slack seed no fold runs
        ctx.save_for_backward(status)
        ctx.mark_non_differentiable(status)
        return x, u, s, sa, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x, grad_u, grad_s, grad_sa, _grad_status):
        solver = ctx.solver
        if solver._serial != ctx.serial:
            raise RuntimeError("rti_solve_soft: the solver was used between this solve and its backward (a solve or a setter came in between): "
                               "the adjoint entry differentiates the last solve and must follow it directly")
        (status,) = ctx.saved_tensors
        B, N = solver.B, solver.N
        device = status.device
        kw = dict(dtype=torch.float64, device=device)
        sx = torch.zeros((B, 1, N + 1, NX), **kw) if grad_x is None else grad_x.reshape(B, 1, N + 1, NX).contiguous()
        su = torch.zeros((B, 1, N, NU), **kw) if grad_u is None else grad_u.reshape(B, 1, N, NU).contiguous()
        ss = None if grad_s is None else grad_s.reshape(B, 1, N + 1, NLAM).contiguous()
        ssa = None if grad_sa is None else grad_sa.reshape(B, 1, N + 1, 2).contiguous()
        weights, soft, alat = ctx.given
        need = list(ctx.needs_input_grad[2:11])
        for i, on in ((3, weights), (4, weights), (5, soft), (6, soft), (7, alat), (8, alat)):
            need[i] = need[i] and on
        shapes = ((B, NX), (B, N, NY), (B, NX), (B, NY, NY), (B, NX, NX), (B, N + 1, NLAM), (B, N + 1, NLAM), (B, N + 1, 2), (B, N + 1, 2))
        grads = [torch.empty(sh, **kw) if nd else None for sh, nd in zip(shapes, need)]
        cur = torch.cuda.current_stream(device)
        hs = _handle_stream(solver, device)
        hs.wait_stream(cur)
        solver.eval_adjoint_penalty_sensitivities_device(1, sx.data_ptr(), su.data_ptr(), 0 if ss is None else ss.data_ptr(),
                                                         0 if ssa is None else ssa.data_ptr(), *[0 if g is None else g.data_ptr() for g in grads])
        cur.wait_stream(hs)
        _used_on(hs, solver, [sx, su] + [t for t in (ss, ssa) if t is not None] + [g for g in grads if g is not None])
        if ctx.zero_failed:
            ok = (status == 0) | (status == 2)
            grads = [None if g is None else torch.where(ok.reshape((B,) + (1,) * (g.dim() - 1)), g, torch.zeros((), **kw)) for g in grads]
        # the a_lat row's pair is one pair for all stages: its gradient is the sum of the per-stage ones
        grads[7:9] = [None if g is None else g.sum(dim=1) for g in grads[7:9]]
        return (None, None, *grads)


def rti_solve_soft(solver, x0, yref, yref_e, W=None, W_e=None, soft_z=None, soft_Z=None, alat_z=None, alat_Z=None, zero_failed: bool = False):
    """:func:`rti_solve` with the soft constraints' side of the step: ``(x, u, s, sa, status)`` with ``s (B,N+1,28)`` the slack values of
    the soft sides (the layout of ``get_slacks``: 14 lower, then 14 upper sides per stage; 0 on a hard side) and ``sa (B,N+1,2)`` those of
    the lateral-acceleration row (the ``slk`` of ``get_alat_multipliers``; the slack values are per stage, the row's penalties one pair
    for all stages), from the inputs of :func:`rti_solve` and, optionally, per-instance slack penalties ``soft_z``, ``soft_Z (B,N+1,28)``
    (``set_instance_soft``) and ``alat_z``, ``alat_Z (B,2)`` (``set_instance_alat_soft``), each pair given together or not at all;
    without a pair the solver's penalties of those rows stay as they are.  The penalties go in unchecked (no read-back): the caller
    vouches that a side is soft (``soft_Z >= 0``) exactly where the solver's shared table holds it soft, with ``soft_z >= 0`` and
    ``soft_z + soft_Z > 0`` there and no NaN (``BatchedOcpSolver.set_instance_soft_device(..., check=True)`` checks a pair once).

    ``backward`` seeds ``x``, ``u``, ``s`` and ``sa`` -- an output the loss does not use is no seed -- and returns the gradients in
    ``x0``, ``yref``, ``yref_e``, ``W``, ``W_e`` and in ``soft_z``, ``soft_Z``, ``alat_z``, ``alat_Z`` through one call of
    ``ihm2mpc_eval_adjoint_sensitivities_p_device``: a penalty gradient is 0 on a side without a slack or with a zero multiplier, the
    a_lat pair's is the sum over the stages.  Bounds are not differentiated.  What the derivative is, the stream ordering, the lifetime
    rule, the serial guard (``backward`` must be the solver's next use after its forward; :func:`plant_step` does not count as one) and
    ``zero_failed`` are :func:`rti_solve`'s.  Without penalties ``x``, ``u``, ``status`` and the five old gradients are
    :func:`rti_solve`'s bits.

    Chains: the adjoint entry differentiates the solver's LAST solve, so a graph with several RTI steps -- a closed loop
    ``x0 -> rti -> plant -> rti -> loss`` -- takes one solver per RTI step (backward reaches the steps in reverse order, and each must
    still find its own solve on its solver); a second solve on the same solver before the first one's backward trips the serial guard."""
    device = torch.device("cuda", solver.device)
    check_rti_inputs(solver.B, solver.N, device, x0, yref, yref_e, W, W_e, soft_z=soft_z, soft_Z=soft_Z, alat_z=alat_z, alat_Z=alat_Z)
    if not solver._sens_mode:
        solver.get_x0_sensitivities()       # raises the library's refusal: the mode is off
    return _RtiSolveSoft.apply(solver, zero_failed, x0, yref, yref_e, W, W_e, soft_z, soft_Z, alat_z, alat_Z)


class _PlantStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, model, M_sim, x, u):
        B = solver.B
        device = x.device
        kw = dict(dtype=torch.float64, device=device)
        x_next, Sx, Su = torch.empty((B, NX), **kw), torch.empty((B, NX, NX), **kw), torch.empty((B, NX, NU), **kw)
        model_used = torch.empty((B,), dtype=torch.int32, device=device)
        cur = torch.cuda.current_stream(device)
        hs = _handle_stream(solver, device)
        hs.wait_stream(cur)
        solver.sim_step_sens_device(x.data_ptr(), u.data_ptr(), model=model, M_sim=M_sim, x_next=x_next.data_ptr(), Sx=Sx.data_ptr(),
                                    Su=Su.data_ptr(), model_used=model_used.data_ptr())
        cur.wait_stream(hs)
        _used_on(hs, solver, [x, u, x_next, Sx, Su, model_used])
        ctx.save_for_backward(Sx, Su)
        ctx.mark_non_differentiable(model_used)
        return x_next, model_used

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_next, _grad_model):
        Sx, Su = ctx.saved_tensors
        if grad_next is None:
            return None, None, None, None, None
        g = grad_next.unsqueeze(2)
        gx = torch.bmm(Sx.transpose(1, 2), g).squeeze(2) if ctx.needs_input_grad[3] else None
        gu = torch.bmm(Su.transpose(1, 2), g).squeeze(2) if ctx.needs_input_grad[4] else None
        return None, None, None, gx, gu


def plant_step(solver, x, u, model: int = 0, M_sim: int = 100):
    """One plant step of ``solver`` on device tensors, differentiable: ``(x_next (B,8), model_used (B,) int32)`` from ``x (B,8)``,
    ``u (B,2)`` (contiguous float64 on the solver's device) -- the handle's plant integrator with ``M_sim`` steps over ``dt`` on
    ``model`` (0, 1, 2, or the switched plants -1, -2), one call of ``ihm2mpc_sim_step_sens_device``, whose exact Jacobians
    ``S_x = dx_next/dx``, ``S_u = dx_next/du`` are kept for ``backward`` (once differentiable): ``S_x' g`` and ``S_u' g`` by ``torch.bmm``.

    The derivative of a switched plant is piecewise: the rule that chooses the kinematic or the dynamic model is evaluated once per
    instance (``model_used``, not differentiable), and the instance gets the derivative of the branch taken; on the switching surface
    ``x_next`` jumps and the Jacobians say nothing about the jump.

    The call changes nothing of the solver and does not advance its serial number: it may stand between :func:`rti_solve_soft` (or
    :func:`rti_solve`) and that solve's backward.  Stream ordering and the lifetime rule are :func:`rti_solve`'s."""
    device = torch.device("cuda", solver.device)
    for name, t, shape in (("x", x, (solver.B, NX)), ("u", u, (solver.B, NU))):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float64:
            raise TypeError(f"{name} must be float64, got {t.dtype}")
        if t.device != device:
            raise ValueError(f"{name} must be on {device} (the solver's device), it is on {t.device}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return _PlantStep.apply(solver, int(model), int(M_sim), x, u)
