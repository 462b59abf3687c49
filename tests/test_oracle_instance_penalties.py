"""The inputs of tests/test_gpu_instance_penalties.py can tell the penalty tunings apart -- shown with the oracle alone, without a GPU.

For each case, the same x0 under the four tunings of instance_penalty_cases.PENALTIES, one oracle RTI step each from the same guess:
every instance has a slack above 1e-6, and for every pair of tunings u_0 differs by more than 1e-6 relative on at least half of the
instances.  The slack is read off the step: at the QP's solution the slack of a soft side covers the violation of its linearised row,
s_i >= dl_i - r_i dz (lower) or r_i dz - du_i (upper), so the largest such violation over the soft sides is a lower bound of the
instance's largest slack.  A kernel that ignored the per-instance values could then not pass the GPU test's bit-for-bit comparison."""
import itertools

import numpy as np
import pytest

import instance_penalty_cases as IP
import layouts as L

B = 9
CASES = ("soft_state", "track_rows_soft", "alat_soft")


@pytest.mark.parametrize("case", CASES)
def test_inputs_tell_the_tunings_apart(track, case):
    from oracle import oracle as orc

    nk = track.s_ref.shape[-1]
    x0 = IP.x0_of(track, case, B)
    w = IP.widths(case)
    u0, slack = [], []
    guess = None
    for pen in IP.PENALTIES:
        d = IP.ocp_of(case, pen, nk).flatten()
        P = orc.OracleProblem(d.as_dict(track.s_ref, track.kappa_ref, track_widths=w))
        if guess is None:       # the same guess and references for every tuning (the guess does not read the penalties)
            x, u = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, IP.N)
            yref, yref_e = orc.prepare_step(IP.N, x0, 40.0, x, u)
            guess = (x, u, yref, yref_e)
        xb, ub, yref, yref_e = guess
        x, u = xb.copy(), ub.copy()
        out = P.rti_step(x, u, x0, yref, yref_e)
        assert np.all(out["status"] == 0), out["status"]
        _, Z = L.soft_arrays(d, P.nc, alat_soft=None if d.alat_soft_Z is None else (d.alat_soft_z, d.alat_soft_Z))
        s = np.zeros(B)
        for b in range(B):
            qp = P.build_qp(xb[b], ub[b], x0[b], yref[b], yref_e[b])
            dz = np.concatenate([x[b] - xb[b], np.concatenate([u[b] - ub[b], np.zeros((1, 2))])], 1)
            Rz = np.einsum("kcj,kj->kc", qp["R"], dz)
            viol = np.concatenate([qp["dl"] - Rz, Rz - qp["du"]], 1)
            soft = np.isfinite(viol) & (Z >= 0.0)
            s[b] = np.max(np.where(soft, viol, 0.0))
        u0.append(u[:, 0].copy()); slack.append(s)
    for j, s in enumerate(slack):
        print(f"{case} tuning {j}: smallest of the instances' largest slacks {s.min():.3e}")
        assert np.all(s > 1e-6), (j, s)
    for i, j in itertools.combinations(range(IP.K), 2):
        rel = np.max(np.abs(u0[i] - u0[j]) / np.maximum(1.0, np.abs(u0[j])), axis=1)
        print(f"{case} tunings {i}, {j}: u0 differs by more than 1e-6 on {int((rel > 1e-6).sum())} of {B}")
        assert (rel > 1e-6).sum() >= (B + 1) // 2, (i, j, rel)
