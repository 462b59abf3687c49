"""CPU: the per-instance tuning's interface -- the C ABI declares both setters and the bindings list them; the expansion of (B,) controller
arguments gives, instance by instance, the weight and bound tables the scalar path builds from that instance's values."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 40


def test_header_declares_and_bindings_list_the_setters():
    from ihm2_amd import _lib

    with open(os.path.join(ROOT, "include", "ihm2mpc.h")) as f:
        hdr = f.read()
    assert re.search(r"int ihm2mpc_set_instance_weights\(ihm2mpc_handle \*h, const double \*W, const double \*W_e\);", hdr)
    assert re.search(r"int ihm2mpc_set_instance_bounds\(ihm2mpc_handle \*h, const double \*lbx, const double \*ubx, const double \*lbu,\s*"
                     r"const double \*ubu, const double \*lg, const double \*ug\);", hdr)
    assert len(_lib.SYMBOLS["ihm2mpc_set_instance_weights"][1]) == 3
    assert len(_lib.SYMBOLS["ihm2mpc_set_instance_bounds"][1]) == 7


def _scalar_tables(weights, limits, nk, **kw):
    from ihm2_amd.controller import WEIGHT_NAMES, controller_ocp
    from ihm2_amd.ocp import default_weights

    W, W_e = default_weights(*(weights[k] for k in WEIGHT_NAMES))
    d = controller_ocp(nk, N, limits, **kw)[1].flatten()
    return W, W_e, {k: getattr(d, k) for k in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")}


@pytest.mark.parametrize("kw", [{}, dict(terminal_bounds="stage", soft_state_bounds=(10.0, 20.0), track_rows=True)])
def test_expansion_matches_the_scalar_path_per_instance(kw):
    from ihm2_amd.controller import LIMIT_NAMES, WEIGHT_NAMES, instance_tuning

    B, nk = 6, 50
    rng = np.random.default_rng(1)
    weights = {k: 1.0 for k in WEIGHT_NAMES}
    weights["q_n"] = rng.uniform(0.5, 5.0, B)
    weights["q_delta_dot"] = rng.uniform(100.0, 900.0, B)
    limits = dict(n_max=rng.uniform(1.0, 2.5, B), v_x_max=31.0, T_max=np.array([500.0, 300.0] * 3), delta_max=0.5, T_dot_max=1e6,
                  delta_dot_max=rng.uniform(0.5, 1.5, B))
    inst_w, inst_b = instance_tuning(B, weights, limits, nk, N, **kw)
    assert inst_w[0].shape == (B, 12, 12) and inst_w[1].shape == (B, 8, 8)
    assert inst_b["lbx"].shape == (B, N + 1, 8) and inst_b["lbu"].shape == (B, N, 2) and inst_b["ug"].shape == (B, N, 2)
    for b in range(B):
        wb = {k: float(np.broadcast_to(v, (B,))[b]) for k, v in weights.items()}
        lb = {k: float(np.broadcast_to(v, (B,))[b]) for k, v in limits.items()}
        W, W_e, tab = _scalar_tables(wb, lb, nk, **kw)
        np.testing.assert_array_equal(inst_w[0][b], W)
        np.testing.assert_array_equal(inst_w[1][b], W_e)
        for k, v in tab.items():
            np.testing.assert_array_equal(inst_b[k][b], v, err_msg=k)
    assert set(LIMIT_NAMES) == set(limits)


def test_scalars_expand_to_nothing_and_bad_shapes_are_refused():
    from ihm2_amd.controller import LIMIT_NAMES, WEIGHT_NAMES, instance_tuning

    weights = {k: 1.0 for k in WEIGHT_NAMES}
    limits = dict(zip(LIMIT_NAMES, (2.0, 31.0, 500.0, 0.5, 1e6, 1.0)))
    assert instance_tuning(4, weights, limits, 50, N) == (None, None)
    with pytest.raises(ValueError):
        instance_tuning(4, {**weights, "q_s": np.ones(3)}, limits, 50, N)
    with pytest.raises(ValueError):
        instance_tuning(4, weights, {**limits, "T_max": np.ones((4, 1))}, 50, N)


def test_array_a_lat_max_is_refused():
    from ihm2_amd.controller import IHM2Controller

    s_ref = np.linspace(0.0, 100.0, 50)
    with pytest.raises(ValueError, match="a_lat_max"):
        IHM2Controller(s_ref, 0 * s_ref, batch_size=4, a_lat_max=np.full(4, 5.0))
