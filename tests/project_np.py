"""Independent NumPy restatement of Track::project (src/ihm2/src/common/tracks.cpp:183-288) and of the Frenet states of the control
node (src/ihm2/src/mpc_control_node.cpp:142-157), shared by test_oracle_cart.py and test_oracle_cart_edge_states.py.  It restates the
source, not the oracle: searchsorted for the window, argmin for the nearest knot, modular indices for the wrap inside the window."""
import numpy as np


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def _project_np(s_ref, X_ref, Y_ref, phi_ref, X, Y, s_guess, s_tol, margins=None):
    """Independent NumPy restatement of tracks.cpp:183-288.  A NaN guess falls out of std::max / std::min as fmax / fmin drop it (the
    window is the whole table); a window of one knot divides 0 by 0.  ``margins``: a dict that receives the relative margins of the two
    decisions -- nearest knot (best against the second-best squared distance, knots at the same place of another lap apart: the first
    wins on both sides) and angle_prev against angle_next (no decision where both are the same knot)."""
    n = len(s_ref)
    lo = max(np.searchsorted(s_ref, np.fmax(s_guess - s_tol, s_ref[0]), side="right") - 1, 0)
    up = np.searchsorted(s_ref, np.fmin(s_guess + s_tol, s_ref[-1]), side="right") - 1
    lo = lo - 1 if lo > 0 else lo
    up = up + 1 if up < n - 1 else up
    P = np.stack([X_ref[lo:up + 1], Y_ref[lo:up + 1]], 1)
    car = np.array([X, Y])
    d2 = ((P - car) ** 2).sum(1)
    i = int(np.argmin(d2)) if np.all(np.isfinite(d2)) else 0          # NaN never wins a "<": the first knot stays
    ip, inx = (i - 1) % len(P), (i + 1) % len(P)
    ang = lambda a, b, c: abs(_wrap(np.arctan2(c[1] - b[1], c[0] - b[0]) - np.arctan2(a[1] - b[1], a[0] - b[0])))
    a_prev, a_next = ang(P[i], car, P[ip]), ang(P[i], car, P[inx])
    if margins is not None:
        other = d2[np.any(P != P[i], axis=1)]
        margins["nearest"] = np.inf if other.size == 0 else (other.min() - d2[i]) / other.min()
        margins["angle"] = np.inf if ip == inx else abs(a_prev - a_next) / max(a_prev, a_next, 1e-300)
    if a_prev > a_next:
        a, b, sa, sb = P[ip], P[i], s_ref[lo + ip], s_ref[lo + i]
    else:
        a, b, sa, sb = P[i], P[inx], s_ref[lo + i], s_ref[lo + inx]
    with np.errstate(invalid="ignore", divide="ignore"):
        lam = np.dot(car - a, b - a) / np.dot(b - a, b - a)
    s = sa + lam * (sb - sa)
    ind = min(lo + i, n - 2)
    phi = phi_ref[ind] + (phi_ref[ind + 1] - phi_ref[ind]) / (s_ref[ind + 1] - s_ref[ind]) * (s - s_ref[ind])
    return s, a[0] + lam * (b[0] - a[0]), a[1] + lam * (b[1] - a[1]), phi


def cart_to_frenet_np(s_ref, X_ref, Y_ref, phi_ref, xc, s_guess, s_tol, margins=None):
    """mpc_control_node.cpp:142-157 on one Cartesian state (8): (Frenet state (8), next guess).  ``margins`` also receives the distance
    of the three wrapped angles from +-pi and of s + 0.05 v_x from the non-zero multiples of the lap length, relative to it."""
    s, Xp, Yp, phi_p = _project_np(s_ref, X_ref, Y_ref, phi_ref, xc[0], xc[1], s_guess, s_tol, margins)
    rho = _wrap(phi_p)
    w0 = _wrap(xc[2])
    psi = _wrap(w0 - rho)
    e = np.hypot(Xp - xc[0], Yp - xc[1])
    tpr = (xc[1] - Yp) * np.cos(rho) - (xc[0] - Xp) * np.sin(rho)
    L = -s_ref[0]
    nxt = np.fmod(s + 0.05 * xc[3], L)
    if margins is not None:
        fin = [v for v in (rho, w0, psi) if np.isfinite(v)]
        margins["wrap"] = min([np.pi - abs(v) for v in fin], default=np.inf)
        q = (s + 0.05 * xc[3]) / L
        margins["fmod"] = np.inf if not np.isfinite(q) or abs(q) < 0.5 else abs(q - np.round(q))
    return np.array([s, e * (1.0 if tpr > 0.0 else -1.0), psi, *xc[3:]]), nxt
