"""The cases of the checks of adjoint seeds on the soft slacks, shared by tests/test_oracle_slack_seeds.py (CPU: the NumPy references
against each other and against central differences of whole QP solves) and tests/test_gpu_slack_seeds.py (GPU): the soft layouts, the
instances, and the solve of one RTI QP by the oracle's interior point with the slacks returned.  The start, the directions, the step
lengths and the acceptance profile are those of tests/cost_cases.py.  Nothing here reads a result."""
from __future__ import annotations

import ctypes as C

import numpy as np

import layouts as L

# (layout, batch size, seed of the instances) of the whole-solve check: two tables of the horizon 40, a short horizon at B = 67
CASES = {
    "soft_2_per_lane": (L.TABLE["soft_2_per_lane"][0], 40, 1234),
    "path_soft_both_sides": (L.TABLE["path_soft_both_sides"][0], 40, 1234),
    "soft_n10_asym": (L.Layout("soft_n10_asym", N=10, soft=1.0, soft_rows=(1, 3), soft_kind="asym", seed=8), 67, 4321),
}
# the layouts of the reference-against-reference check (B = 3 each); alat_soft takes the fifteen-row build of the oracle
REF_LAYOUTS = ("soft_2_per_lane", "soft_4_per_lane_mixed", "path_soft_both_sides", "soft_one_sided_rows_padding", "alat_soft")
SLACK_COST_MIN = 1e-6       # an instance whose slack cost is above this exercises the fold


def soft_arrays(data, lay):
    """(nc, soft_z, soft_Z) of the layout's table: 14 rows, or 15 with the lateral-acceleration row."""
    nc = 15 if lay.alat else L.NC
    z, Z = L.soft_arrays(data, nc, (data.alat_soft_z, data.alat_soft_Z) if lay.alat and data.alat_soft_Z is not None else None)
    return nc, z, Z


def qp_solve(qp, data, z, Z, tol, iter_max=200):
    """oracle.qp_solve on a build_qp dict with the soft penalties (N+1, 2 nc); nc = 15: the same entry of the fifteen-row build, which
    oracle.qp_solve does not reach (it sizes lam, t and sl for 14 rows)."""
    from oracle import oracle as orc

    nc = qp["R"].shape[1]
    if nc == L.NC:
        return orc.qp_solve(**qp, iter_max=iter_max, tol=tol, mu0=data.ipm_mu0, tau0=data.ipm_tau0, soft_z=z, soft_Z=Z)
    N = qp["A"].shape[0]
    dp = C.POINTER(C.c_double)
    keep = [np.ascontiguousarray(qp[k], dtype=np.float64) for k in ("H", "g", "A", "Bm", "b", "dx0", "R", "dl", "du")]
    keep += [np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(Z, dtype=np.float64)]
    assert keep[6].shape == (N + 1, nc, 10) and keep[9].shape == (N + 1, 2 * nc)
    dz, pi = np.zeros((N + 1, 10)), np.zeros((N + 1, 8))
    lam, t, sl = (np.zeros((N + 1, 2 * nc)) for _ in range(3))
    stats, iters = np.zeros(8), C.c_int(0)
    fn = orc.lib15().orc_qp_solve_soft
    fn.restype = C.c_int
    st = fn(C.c_int(N), *[a.ctypes.data_as(dp) for a in keep], C.c_int(iter_max), C.c_double(tol), C.c_double(data.ipm_mu0),
            C.c_double(data.ipm_tau0), *[a.ctypes.data_as(dp) for a in (dz, pi, lam, t, sl, stats)], C.byref(iters))
    return dict(status=st, dz=dz, pi=pi, lam=lam, t=t, sl=sl, stats=stats, iters=iters.value)


def split_slacks(sl, nc):
    """(slk (N+1,28), slk_a (N+1,2) or None) of get_slacks / get_alat_multipliers from the QP's (N+1, 2 nc)."""
    if nc == L.NC:
        return sl, None
    return np.concatenate([sl[:, :L.NC], sl[:, nc:nc + L.NC]], 1), np.stack([sl[:, L.NC], sl[:, nc + L.NC]], 1)
