"""The cases of the per-instance slack penalties, shared by tests/test_oracle_instance_penalties.py (CPU: the inputs tell the tunings
apart) and tests/test_gpu_instance_penalties.py (GPU: a mixed batch against homogeneous handles).  Nothing here reads a result.

Four penalty tunings (z, Z); z = 0 is the edge where nu_i = max(Z s - lam, 0) alone carries the slack.  The same x0 for all of them,
with n pushed beyond the soft bound so that every instance pays for a slack from the first stage on."""
from __future__ import annotations

import numpy as np
from conftest import sample_x0

N = 40
PENALTIES = ((100.0, 100.0), (10.0, 1000.0), (1000.0, 10.0), (0.0, 500.0))
K = len(PENALTIES)
LIMITS = dict(n_max=2.0, v_x_max=31.0, T_max=500.0, delta_max=0.5, T_dot_max=1e6, delta_dot_max=1.0)
WIDTHS = np.array([[1.2, 1.1]])

# kind: which sides carry the tuning's penalty -- "state": the soft state boxes (n, v_x, the terminal box), "track": the two track rows
# on both sides (and the a_lat row, which follows them).  push: |n| of x0
CASES = {
    "soft_state": dict(kind="state", limits=dict(n_max=0.5), push=0.8),
    "track_rows_soft": dict(kind="track", push=0.8),
    "alat_soft": dict(kind="track", alat=True, a_lat_max=2.0, push=0.8),
    "fdyn6u": dict(kind="track", model="fdyn6u", push=0.8),
    "live": dict(kind="state", limits=dict(n_max=0.5), push=0.8,
                 opts=dict(nlp_solver_type="SQP", nlp_solver_max_iter=2, globalization="MERIT_BACKTRACKING", integrator_type="IRK",
                           sim_method_num_steps=1)),
}


def ocp_of(case, pen, nknots, Nf=N):
    """The OCP of a case with the penalty tuning pen = (z, Z) on its soft sides."""
    from ihm2_amd import ocp as O
    from ihm2_amd.controller import controller_ocp

    c = CASES[case]
    lim = {**LIMITS, **c.get("limits", {})}
    if c.get("model", "fkin6") == "fkin6":
        if c["kind"] == "state":
            _, ocp = controller_ocp(nknots, Nf, lim, terminal_bounds="stage", soft_state_bounds=pen)
        else:
            _, ocp = controller_ocp(nknots, Nf, lim, a_lat_max=c.get("a_lat_max", 5.0), track_rows=True, track_rows_penalty=pen,
                                    lateral_acceleration_row=c.get("alat", False))
    else:       # the dynamic model with the soft track rows of old/generate_acaods_interface.py:380-395 (tests/test_gpu_parity.py: _path_setup)
        mdl = O.get_acados_model_from_explicit_dynamics("ihm2_" + c["model"], O.fdyn6u_model, 8, 2, 2 * nknots)
        ocp = O.get_acados_ocp(mdl, Nf, *lim.values())
        ocp.model.con_h_expr = "track"
        k = ocp.constraints
        k.lh = k.lh_e = np.array([-1e3, -1e3]); k.uh = k.uh_e = np.array([0.0, 0.0])
        k.idxsh, k.idxsh_e = np.arange(2), np.arange(2)
        ocp.cost.zl = ocp.cost.zu = ocp.cost.zl_e = ocp.cost.zu_e = np.full(2, pen[0])
        ocp.cost.Zl = ocp.cost.Zu = ocp.cost.Zl_e = ocp.cost.Zu_e = np.full(2, pen[1])
    ocp.cost.W, ocp.cost.W_e = O.default_weights()
    ocp.solver_options.tf = Nf * 0.05
    ocp.solver_options.sim_method_num_steps = 25
    for name, v in c.get("opts", {}).items():
        setattr(ocp.solver_options, name, v)
    return ocp


def widths(case):
    return WIDTHS if CASES[case]["kind"] == "track" else None


def x0_of(track, case, B, seed=7):
    x0 = sample_x0(track, B, seed=seed)
    x0[:, 3] = np.clip(x0[:, 3], 4.0, 9.0)
    x0[:, 6] = np.clip(x0[:, 6], -150.0, 150.0)
    x0[:, 1] = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * CASES[case]["push"]      # beyond the soft bound, either side
    return x0


def instance_tables(flats, assign):
    """((soft_z, soft_Z) (B,N+1,28), (alat z, Z) (B,2) or None) of the flattened OCPs of the tunings for the instances `assign`."""
    soft = tuple(np.stack([np.asarray(getattr(flats[j], k), dtype=np.float64) for j in assign]) for k in ("soft_z", "soft_Z"))
    if flats[0].alat_soft_Z is None:
        return soft, None
    return soft, tuple(np.stack([np.asarray(getattr(flats[j], k), dtype=np.float64) for j in assign]) for k in ("alat_soft_z", "alat_soft_Z"))
