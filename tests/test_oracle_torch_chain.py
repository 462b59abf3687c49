"""The two-step closed loop x0 -> rti -> plant -> rti -> u_0 on the CPU oracle (no GPU): the start and the directions of
tests/test_gpu_torch_chain.py::test_chain_against_central_differences, chosen by the reference and not by the code under test.  The
solves are the oracle's interior point on the RTI QP, the plant step is the oracle's RK4 with sensitivities, the gradient is the NumPy
references (adj_ref, penalty_grad_ref, adjw_ref) composed by tests/chain_ref.py::backward, and it is compared with central differences
of whole oracle chains."""
import types

import numpy as np

import chain_ref as CR
from test_gpu_penalty_device import LAY, _penalties
from test_gpu_qp_layouts import _widen

B = 64


def _run(track, drop_sx=False):
    ch = CR.OracleChain(track, LAY, B)
    N = LAY.N
    z, Z, az, aZ = CR.fd_penalties(*_penalties(types.SimpleNamespace(data=ch.data), B))
    wide = lambda a28, a2: _widen(a28, np.broadcast_to(a2, (N + 1, 2)))  # noqa: E731
    dirs = CR.directions(z, Z, ch.W0, ch.We0)
    pred, fd = ({k: np.zeros((B, 2)) for k in dirs} for _ in range(2))
    ok = {k: np.ones(B, dtype=bool) for k in dirs}
    for i in range(B):
        pen = (wide(z[i], az[i]), wide(Z[i], aZ[i]))
        r = ch.chain(i, ch.x0[i], pen, pen)
        if not r["solved"] or ch.weakly_active(r):
            for k in dirs:
                ok[k][i] = False
            continue
        g = ch.reference(i, r, drop_sx=drop_sx)
        for name, (eps, d) in dirs.items():
            if name == "x0":
                pred[name][i] = g["x0"] @ d["x0"][i]
                moved = lambda sign: ch.chain(i, ch.x0[i] + sign * eps * d["x0"][i], pen, pen)  # noqa: E731
            elif name == "penalties":
                dz, dZ = wide(d["soft_z"][i], np.zeros(2)), wide(d["soft_Z"][i], np.zeros(2))
                pred[name][i] = (g["soft_z"] * dz).sum((1, 2)) + (g["soft_Z"] * dZ).sum((1, 2))
                moved = lambda sign: ch.chain(i, ch.x0[i], (pen[0] + sign * eps * dz, pen[1] + sign * eps * dZ), pen)  # noqa: E731
            else:
                pred[name][i] = (g["W"] * d["W"][i]).sum((1, 2)) + (g["W_e"] * d["W_e"][i]).sum((1, 2))
                moved = lambda sign: ch.chain(i, ch.x0[i], pen, pen, W=ch.W0 + sign * eps * d["W"][i], We=ch.We0 + sign * eps * d["W_e"][i])  # noqa: E731
            up, um = moved(1.0), moved(-1.0)
            ok[name][i] = up["solved"] and um["solved"]
            fd[name][i] = (up["u2"] - um["u2"]) / (2 * eps)
    return {name: (pred[name], fd[name], np.flatnonzero(ok[name])) for name in dirs}


def test_reference_chain_against_central_differences_of_oracle_chains(track):
    """On the start of the GPU test (tests/chain_ref.py::fd_start: tests/cost_cases.py::start, every car below the soft lower bound on
    v_x, the table LAY of tests/test_gpu_penalty_device.py with that file's per-instance penalties, B = 64) and its three directions
    (x0; step 1's (soft_z, soft_Z); step 1's (W, W_e)): the skip rule (a QP not solved in one of the three evaluations, or weakly
    active in one of the two solves) keeps at least 48 of 64 instances, the composed reference meets tests/cost_cases.py::profile
    (median <= 1e-6, 75 % <= 1e-5, 95 % <= 1e-3) in the measure of tests/chain_ref.py::measure, and the zero prediction does not.

    Chosen: the directions as named; the start changed (tests/chain_ref.py::fd_start, fd_penalties, where the choice and its rule are
    written down): the instances of seed 900, v_x from 2.5 to 2.9, every heading 0.06 rad off, the quadratic penalties of the soft
    sides times 80.  On the start of _Start(..., slow=True) the reference misses the bars (64 of 64 kept; penalties median 6.5e-3,
    12.5 % <= 1e-5; weights median 1.0e-2): the rate rows pin u_0 of step 1 on two instances in three, the batch's median |fd| is
    1e-7, noise.  Measured on the chosen start, 64 of 64 kept in every direction:
      x0:        median 2.8e-10, 100 % <= 1e-5, 100 % <= 1e-3, 7.2e-7 at worst; zero prediction median 0.98
      penalties: median 3.1e-8, 95.3 % <= 1e-5, 100 % <= 1e-3, 8.3e-5 at worst; zero prediction median 0.97, 28 % <= 1e-5
      weights:   median 2.1e-7, 89.1 % <= 1e-5, 98.4 % <= 1e-3, 1.1e-3 at worst; zero prediction median 0.99, 25 % <= 1e-5
    With the plant's S_x' g dropped from the composition (_run(track, drop_sx=True)) the x0 direction fails: NOTES.md R30."""
    res = _run(track)
    for name, (pred, fd, keep) in res.items():
        CR.verdict("ORACLE-CHAIN-FD", name, pred, fd, keep, B)
