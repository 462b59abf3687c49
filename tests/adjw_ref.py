"""Independent numpy reference of the adjoint gradients in the cost weights W, W_e ("gradients in the weights").

The stationarity row of the RTI QP reads H_k dz_k + g_k = c_s V' W_k (V z+_k - yref_k) with z+ = zbar + dz the returned solution
(terminal: W_e (x+_N - yref_e)), so a symmetric change dW common to all stages k < N moves the stage gradients by c_s V' dW e_k,
e_k = V z+_k - yref_k, and with dL = -zeta' dg of adj_ref.py
    dL/dW = -c_s sum_{k<N} sym((V zeta_k) e_k'),    dL/dW_e = -sym(zeta_N[:8] (x+_N - yref_e)'),    sym(X) = (X + X') / 2.
zeta is adj_ref.adjoint's; V is layouts.selectors().  No code is shared with the kernel."""
from __future__ import annotations

import numpy as np

import layouts as L


def _sym(X):
    return 0.5 * (X + np.swapaxes(X, -1, -2))


def stage_terms(data, zeta, zplus, yref):
    """(N,12,12): the contribution -c_s sym((V zeta_k) e_k') of every stage k < N and its cancellation-free magnitude
    c_s |V zeta_k| |e_k|' (the scale rounding errors of the sum are relative to)."""
    V = L.selectors()
    N = yref.shape[0]
    a = zeta[:N] @ V.T                      # (N,12) V zeta_k
    e = zplus[:N] @ V.T - yref              # (N,12) e_k
    cs = data.cost_scale_stage
    return -cs * _sym(a[:, :, None] * e[:, None, :]), cs * np.abs(a)[:, :, None] * np.abs(e)[:, None, :]


def weight_gradients(data, zeta, zplus, yref, yref_e):
    """zeta (N+1,10) of adj_ref.adjoint, zplus (N+1,10) the returned solution (x+_k, u+_k; the input part of row N is ignored),
    yref (N,12), yref_e (8).  Returns grad_W (12,12), grad_W_e (8,8)."""
    terms, _ = stage_terms(data, zeta, zplus, yref)
    N = yref.shape[0]
    return terms.sum(0), -_sym(np.outer(zeta[N, :8], zplus[N, :8] - yref_e))
