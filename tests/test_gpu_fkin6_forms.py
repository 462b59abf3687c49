"""fkin6's linearisation records after the rewrite of its arithmetic (the steering block without the tangent; rows 2 and 5 of the Jacobian
applied in factored form by the batch kernels, csrc/model.hpp and csrc/device_steps.hpp), at N = 5 on two tracks with M = 1, 4, 25
sub-steps: the batch kernel (B = 67: 335 intervals, a ragged sixth wave) and the small-batch path (B = 3: the column kernel for ERK) of
the integrators ERK and ERK_LAG against the reference, and against each other on the same three instances.

States: the steering and heading entries of tests/edge_states.py and 40 ``random_state`` draws.  Interval (b, k) with k even starts from
state ((3 b + k / 2) * 37) mod 80, so the 201 even intervals of the large batch hold every state and the first three instances -- the
small batch -- hold nine of them from all three groups; node k + 1 is the reference's successor of node k plus OFFSET, so that the defect
b_k is small and its absolute bound holds as it stands (tests/test_gpu_edge_states.py).  Only those intervals are compared.

Reference: the oracle's linearisation (``OracleProblem.linearize``) for ERK; for ERK_LAG tests/lag_ref.py, which evaluates the oracle's
model and Jacobian (the oracle has no such integrator; tests/test_gpu_lag_integrator.py compares with it as well).  Tolerances: A and B 1e-10
relative to the column scale and b 1e-11, or the entry's own where it carries one (``Entry.tolerance``); the two kernels against each
other 1e-13, as tests/test_gpu_parity.py::test_small_batch_linearisation_matches_the_batch_kernel.

ERK over dt = 0.002 M (RK4 with fewer than 18 sub-steps of 0.05 is refused as unstable on the torque lag), ERK_LAG over dt = 0.05."""
import numpy as np
import pytest
from conftest import make_ocp, random_state

import edge_states as E
import lag_ref
import launch_cases as LC

pytestmark = pytest.mark.gpu

N, B_BIG, B_SMALL = 5, 67, 3
OFFSET = 1e-3 * np.array([1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0])
KS = np.arange(0, N, 2)          # the compared intervals


def _states(track):
    """(x (80, 8), u (80, 2), tolerance AB (80), tolerance b (80), names)"""
    entries = [e for e in E.table(track.s_ref, track.kappa_ref) if e.family in ("steering", "heading")]
    assert len(entries) == 40
    x, u = E.arrays(entries)
    rng = np.random.default_rng(606)
    draws = [random_state(rng) for _ in range(40)]
    x = np.concatenate([x, np.stack([d[0] for d in draws])]); u = np.concatenate([u, np.stack([d[1] for d in draws])])
    tol_ab = np.concatenate([E.tolerances(entries, "AB", "fkin6", "ERK"), np.full(40, E.TOL["AB"][0])])
    tol_b = np.concatenate([E.tolerances(entries, "b", "fkin6", "ERK"), np.full(40, E.TOL["b"][0])])
    assert E.TOL["AB"][0] == 1e-10 and E.TOL["b"][0] == 1e-11
    return x, u, tol_ab, tol_b, [e.name for e in entries] + [f"random_{i}" for i in range(40)]


@pytest.fixture(scope="module", params=[("ERK", 1), ("ERK", 4), ("ERK", 25), ("ERK_LAG", 1), ("ERK_LAG", 4), ("ERK_LAG", 25)], ids=lambda p: f"{p[0]}-M{p[1]}")
def case(request, track):
    """Both batches' records and launch records, and the reference's (computed once for the large batch; the small one is its first rows)."""
    from ihm2_amd.solver import BatchedOcpSolver
    from ihm2_amd.track import track_table
    from oracle import oracle as orc

    integ, M = request.param
    dt = 0.05 if integ == "ERK_LAG" else 0.002 * M
    second = track_table("fsds_competition_2")
    s_ref, k_ref = np.stack([track.s_ref, second.s_ref]), np.stack([track.kappa_ref, second.kappa_ref])
    tid = (np.arange(B_BIG) % 2).astype(np.int32)
    xs, us, tol_ab, tol_b, names = _states(track)
    idx = ((3 * np.arange(B_BIG)[:, None] + np.arange(KS.size)[None, :]) * E.STRIDE) % len(xs)          # (B, 3)
    assert np.unique(idx).size == len(xs)
    groups = np.minimum(idx[:B_SMALL].ravel() // 12, 3)          # 0: steering, 1, 2: heading, 3: random
    assert {0, 3} <= set(groups.tolist()) and ({1, 2} & set(groups.tolist()))
    x = np.zeros((B_BIG, N + 1, 8)); u = np.zeros((B_BIG, N, 2))
    x[:, KS] = xs[idx]; u[:, KS] = us[idx]
    opts = dict(integrator_type="ERK_LAG", sim_integrator_type="ERK_LAG") if integ == "ERK_LAG" else {}
    ocp = make_ocp(N=N, M=M, tf=N * dt, **opts)
    if integ == "ERK":
        P = orc.OracleProblem(ocp.flatten().as_dict(s_ref, k_ref))
        assert P.M == M and abs(P.p.dt - dt) < 1e-15
        succ = P.sim_step(x[:, KS].reshape(-1, 8), u[:, KS].reshape(-1, 2), 0, M, track_id=np.repeat(tid, KS.size)).reshape(B_BIG, KS.size, 8)
    else:
        succ = np.stack([[lag_ref.lag_step(x[b, k], u[b, k], s_ref[tid[b]], k_ref[tid[b]], dt, M) for k in KS] for b in range(B_BIG)])
    x[:, KS + 1] = succ + OFFSET
    u[:, KS[:-1] + 1] = u[:, KS[:-1]]          # the odd intervals start from the successors: run, not compared
    ref = P.linearize(x, u, track_id=tid) if integ == "ERK" else lag_ref.linearize(x, u, s_ref, k_ref, dt, M, track_id=tid)
    got = {}
    for B in (B_BIG, B_SMALL):
        s = BatchedOcpSolver(ocp, B, s_ref, k_ref, track_id=tid[:B])
        s.set_x0(x[:B, 0]); s.set_x(x[:B]); s.set_u(u[:B])
        s.linearize()
        got[B] = (s.get_linearization(), s.get_launch_record(), LC.names(s)[0])
        s.free()
    return dict(integ=integ, M=M, idx=idx, tol_ab=tol_ab, tol_b=tol_b, names=np.array(names), ref=ref, got=got)


def _errors(got, ref):
    (A, Bm, b), (Ao, Bo, bo) = got, ref
    err_a = (np.abs(A - Ao) / np.maximum(np.abs(Ao).max(axis=2, keepdims=True), 1e-30)).max(axis=(2, 3))
    err_b = (np.abs(Bm - Bo) / np.maximum(np.abs(Bo).max(axis=2, keepdims=True), 1e-30)).max(axis=(2, 3))
    return err_a, err_b, np.abs(b - bo).max(axis=2)


@pytest.mark.parametrize("B", [B_BIG, B_SMALL])
def test_records_match_the_reference(case, B):
    (A, Bm, b), rec, kernel = case["got"][B]
    assert rec["linearize"] == kernel and (kernel == "k_linearize_cols") == (case["integ"] == "ERK" and B == B_SMALL)
    ref = tuple(r[:B] for r in case["ref"])
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(Bm)) and np.all(np.isfinite(b))
    assert np.abs(ref[2][:, KS]).max() < 0.01          # the defects are the offset
    idx = case["idx"][:B]
    for err, tol, q in zip(_errors((A, Bm, b), ref), (case["tol_ab"], case["tol_ab"], case["tol_b"]), "ABb"):
        err, tol = err[:, KS], tol[idx]
        w = np.unravel_index(np.argmax(err / tol), err.shape)
        print(f"{case['integ']} M={case['M']} B={B} {q}: worst {err[w]:.2e} of {tol[w]:.1e} at {case['names'][idx][w]}; largest error {err.max():.2e}")
        bad = err >= tol
        assert not bad.any(), (q, sorted({(n, float(f"{e:.3g}")) for n, e in zip(case["names"][idx][bad], err[bad])})[:12])
    assert np.all(A[:, :, 3:, :3] == 0) and np.all(A[:, :, 6:, :6] == 0) and np.all(A[:, :, 3:5, 5] == 0)          # structural zeros are exact


def test_small_batch_matches_the_batch_kernel(case):
    """The first three instances alone (ERK: the column kernel, whose Jacobian is dense) and inside the large batch (factored rows)."""
    (A, Bm, b), rec_big, kernel_big = case["got"][B_BIG]
    (As, Bms, bs), rec_small, kernel_small = case["got"][B_SMALL]
    assert (rec_big["linearize"], rec_small["linearize"]) == (kernel_big, kernel_small)
    assert (kernel_big == kernel_small) == (case["integ"] == "ERK_LAG")
    ea, eb, ec = _errors((As, Bms, bs), (A[:B_SMALL], Bm[:B_SMALL], b[:B_SMALL]))
    print(f"{case['integ']} M={case['M']}: small batch against the batch kernel A {ea.max():.2e} B {eb.max():.2e} b {ec.max():.2e}")
    assert ea.max() < 1e-13 and eb.max() < 1e-13 and ec.max() < 1e-13
    if case["integ"] == "ERK_LAG":          # one kernel at both sizes
        np.testing.assert_array_equal(As, A[:B_SMALL]); np.testing.assert_array_equal(Bms, Bm[:B_SMALL]); np.testing.assert_array_equal(bs, b[:B_SMALL])
