"""The per-step partner of run_steps, the gain read-back and the clipped start: what every "the loop equals step by step" test shares."""
import numpy as np
from conftest import sample_x0

HIST = ("u0", "x0", "status", "qp_iter")


def gain(s):
    """du_0/dx_0 of the last solve as (B, 2, 8), whichever sensitivity mode the handle is in."""
    su = s.get_x0_sensitivities()[1]
    return su if su.ndim == 3 else su[:, 0]


def per_step(s, s_target, n, model, M_sim, sens=False, after=None):
    """n step() calls: the dict run_steps(..., u0_hist=True, x0_hist=True, status_hist=True, qp_iter_hist=True) returns (with sens, its
    sens_u0 as well); after(s) is called behind every step."""
    h = {k: [] for k in HIST + (("sens_u0",) if sens else ())}
    for _ in range(n):
        s.step(s_target, model=model, M_sim=M_sim)
        h["u0"].append(s.get_u0()); h["x0"].append(s.get_x0()); h["status"].append(s.get_status()); h["qp_iter"].append(s.get_qp_iter())
        if sens:
            h["sens_u0"].append(gain(s))
        if after is not None:
            after(s)
    return {k: np.array(v) for k, v in h.items()}


def clipped_start(track, B, seed):
    """conftest.sample_x0 with v_x clipped to [4, 12] m/s."""
    x0 = sample_x0(track, B, seed=seed)
    x0[:, 3] = np.clip(x0[:, 3], 4.0, 12.0)
    return x0
