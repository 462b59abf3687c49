"""One RTI step of the batched NMPC as a differentiable PyTorch function.

``rti_solve(solver, x0, yref, yref_e, W, W_e)`` feeds device tensors to a :class:`~ihm2_amd.solver.BatchedOcpSolver` through the
library's ``*_device`` entries, runs one RTI solve and returns ``(x, u, status)`` as tensors; ``backward`` is one call of
``ihm2mpc_eval_adjoint_sensitivities_w_device``.  Nothing passes through host memory and nothing waits for the GPU: the handle's stream
and torch's current stream are ordered against each other with events.

This module is the only one of the package that imports torch; ``import ihm2_amd`` stays torch-free.
"""
from __future__ import annotations

import weakref

import torch

from .constants import NU, NX, NY

__all__ = ["rti_solve", "check_rti_inputs"]


def check_rti_inputs(B: int, N: int, device, x0, yref, yref_e, W=None, W_e=None) -> None:
    """The argument check of :func:`rti_solve`, before any GPU call: every tensor a contiguous float64 tensor on ``device`` with the
    shape ``x0 (B,8)``, ``yref (B,N,12)``, ``yref_e (B,8)``, ``W (B,12,12)``, ``W_e (B,8,8)``; ``W`` and ``W_e`` together or not at all.
    Raises ``TypeError`` (not a tensor, not float64) or ``ValueError`` (device, shape, layout, one weight without the other), each
    naming the argument."""
    device = torch.device(device)
    if (W is None) != (W_e is None):
        missing, given = ("W_e", "W") if W_e is None else ("W", "W_e")
        raise ValueError(f"{missing} is missing: W and W_e are given together or not at all ({given} was given)")
    shapes = {"x0": (B, NX), "yref": (B, N, NY), "yref_e": (B, NX), "W": (B, NY, NY), "W_e": (B, NX, NX)}
    for name, t in (("x0", x0), ("yref", yref), ("yref_e", yref_e), ("W", W), ("W_e", W_e)):
        if t is None and name in ("W", "W_e"):
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
    ``solver.free()`` raises ``RuntimeError`` while one is alive."""
    device = torch.device("cuda", solver.device)
    check_rti_inputs(solver.B, solver.N, device, x0, yref, yref_e, W, W_e)
    if not solver._sens_mode:
        solver.get_x0_sensitivities()       # raises the library's refusal: the mode is off
    return _RtiSolve.apply(solver, zero_failed, x0, yref, yref_e, W, W_e)
