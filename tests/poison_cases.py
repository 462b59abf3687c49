"""Helpers and case tables of tests/test_gpu_workspace_poison.py (the GPU runs) and tests/test_poison_starts.py (the oracle-side check of
their starts, without a GPU).

The instrument: IHM2MPC_POISON_WORKSPACE=1, read by ihm2mpc_create, fills every workspace buffer of doubles of that handle with NaN
(0xFF bytes) instead of zeros, at allocation and at every regrowth (csrc/ihm2mpc_internal.h: WorkBuf).  A kernel that reads a workspace
word before anything wrote it -- a term times a zero coefficient, a prefetched row that leaks into a sum, an output written in part --
sees 0.0 on every fresh handle, and so in every other test; here it sees NaN on one of two handles.

``run_twin`` builds a clean and a poisoned handle of one configuration, gives both the same start and the same calls, and compares
everything the getters return for equality of bits.  Then each handle gets its starting state back explicitly and repeats the calls:
the second pass, on a workspace that holds the first pass's leftovers, must equal the first.  No tolerance anywhere.

A developer narrows a finding to a buffer by running the module with IHM2MPC_POISON_WORKSPACE set to a list of member names: the
poisoned handle is then created with that list instead of 1."""
from __future__ import annotations

import contextlib
import os

import numpy as np

import layouts as L

ENV = "IHM2MPC_POISON_WORKSPACE"
Lay = L.Layout


@contextlib.contextmanager
def environ(**kv):
    """Environment variables set (a string) or removed (None) inside; the handle-creation switches are read in ihm2mpc_create."""
    saved = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def poison_value() -> str:
    """What the poisoned handle is created with: 1, or the list of buffer names the caller's environment narrows it to."""
    v = os.environ.get(ENV, "")
    return v if v not in ("", "0") else "1"


def assert_equal(a, b, path="out"):
    """Equality of bits of two nested results (dicts, lists, arrays); equal NaN positions count as equal."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            assert_equal(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            assert_equal(x, y, f"{path}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, path
    else:
        np.testing.assert_array_equal(a, b, err_msg=path)


def iterate(s) -> dict:
    """The state a pass starts from, as the getters give it."""
    pi, lam = s.get_multipliers()
    lam_a, slk_a = s.get_alat_multipliers()
    return dict(x0=s.get_x0(), x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(), lam_a=lam_a, slk_a=slk_a)


def set_iterate(s, it, yref=None, yref_e=None):
    """tests/test_gpu_regrowth.py::_set_iterate, with the a_lat row's pair and the references."""
    s.set_x0(it["x0"]); s.set_x(it["x"]); s.set_u(it["u"]); s.set_multipliers(it["pi"], it["lam"]); s.set_slacks(it["slk"])
    s.set_alat_multipliers(it["lam_a"], it["slk_a"])
    if yref is not None:
        s.set_yref(yref); s.set_yref_e(yref_e)


def adjoint_seeds(B, N, S=2):
    rng = np.random.default_rng(4711)
    return rng.standard_normal((B, S, N + 1, 8)), rng.standard_normal((B, S, N, 2))


def outputs(s, sqp=False, sens=False, adjoint=False) -> dict:
    """Everything a getter returns after a solve / step.  sens: the x0 sensitivities are readable (mode 1 or 2, the last call computed
    them); adjoint: the five gradients with given seeds, with a NULL seed_u and with the two unit seeds on u_0 (first, so that they follow
    the solve directly)."""
    adj = {}
    if adjoint:
        sx, su = adjoint_seeds(s.B, s.N)
        adj["adj_seeds"] = s.eval_adjoint_weight_sensitivities(sx, su)
        adj["adj_null_seed_u"] = s.eval_adjoint_sensitivities(sx, None)
        adj["adj_unit_u0"] = s.eval_adjoint_weight_sensitivities()
    pi, lam = s.get_multipliers()
    lam_a, slk_a = s.get_alat_multipliers()
    A, Bm, b = s.get_linearization()
    # (status and iteration count first: they are what a failing comparison should name first)
    out = dict(status=s.get_status(), qp_iter=s.get_qp_iter(), x0=s.get_x0(), x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks(),
               lam_a=lam_a, slk_a=slk_a, u0=s.get_u0(), res=s.get_residuals(), qp_res=s.get_qp_residuals(), lin_A=A, lin_B=Bm, lin_b=b, **adj)
    if sqp:
        out.update(s.get_sqp_stats())
    if sens:
        sx, su = s.get_x0_sensitivities()
        out["sens_u"] = su
        if sx is not None:
            out["sens_x"] = sx
    return out


def final_status(res):
    """The statuses the last call of a pass left (the guard's input): the last `status` entry of a nested result, depth first."""
    found = None
    if isinstance(res, dict):
        if "status" in res:
            st = np.asarray(res["status"])
            found = st if st.ndim == 1 else st[-1]
        for k, v in res.items():
            if k != "status" and isinstance(v, (dict, list, tuple)):
                f = final_status(v)
                found = f if f is not None else found
    elif isinstance(res, (list, tuple)):
        for v in res:
            f = final_status(v)
            found = f if f is not None else found
    return found


def run_twin(make, start, calls, accepted=(0,), share=0.6, restore=None):
    """make(): a fresh handle of the case's configuration (created inside the environment this function sets); start(s): puts the
    starting state in and returns (yref, yref_e) as it set them, or None where the calls form or need no reference; calls(s, tag):
    the compared calls, returning everything they leave (tag: "clean" or "poisoned").  share: the part of the clean handle's
    instances whose last status must be accepted, None where the calls solve nothing; restore(s): sets again, before the replay, state
    the calls overwrite beyond the iterate and the references.  Returns the clean handle's first pass."""
    value = poison_value()
    with environ(**{ENV: None}):
        clean = make()
    with environ(**{ENV: value}):
        pois = make()
    if value == "1" or "lin" in value.split(","):
        # the switch took effect: ihm2mpc_get_linearization has no precondition and reads `lin`, which nothing has written yet
        assert all(np.isnan(a).all() for a in pois.get_linearization()), "the poisoned handle's workspace is not NaN"
        assert all((a == 0.0).all() for a in clean.get_linearization()), "the clean handle's workspace is not zero"
    res = {}
    for tag, s in (("clean", clean), ("poisoned", pois)):
        ref = start(s)
        it = iterate(s)
        first = calls(s, tag)
        if restore is not None:
            restore(s)
        set_iterate(s, it, *(ref if ref is not None else ()))
        res[tag] = (first, calls(s, tag))
    clean.free(); pois.free()
    assert_equal(res["poisoned"][0], res["clean"][0], "poisoned vs clean")
    for tag in ("clean", "poisoned"):
        assert_equal(res[tag][1], res[tag][0], f"{tag}: replay vs first pass")
    if share is not None:
        st = final_status(res["clean"][0])
        ok = np.isin(st, accepted)
        assert ok.mean() >= share, ("too few instances solved for the comparison to mean much", st.tolist())
    return res["clean"][0]


# ---- the per-step QP cases: one per entry of layouts.TABLE, the LDS classes at the shortest horizons, the horizons around the ring depth ----
# (id, layout, B, IHM2MPC_BLOCK_QP, sample_x0 seed, the kernel the launch record must name)

def qp_name(table_name, lay, block_kernel):
    """The instantiation a layout of layouts.TABLE is named for (tests/test_slot_table.py: NAMED_FOR; UNI = 0 with stage-varying
    weights or general rows), or the four-wave kernel of its 5-slot table."""
    from test_slot_table import NAMED_FOR

    nslot, nsoft, path = NAMED_FOR[table_name]
    uni = 0 if (lay.stage_W or lay.grows == "stagevary") else 1
    if block_kernel:
        assert (nslot, nsoft, path) == (5, 0, 0)
        return "k_qp_block<2,%d,4>" % uni
    return "k_qp_wave<%d,%d,%d,%d>" % (nslot, nsoft, path, uni)


# sample_x0 seeds moved from the ones the layouts were chosen with (900 + the layout's seed at B = 65 .. 300), where the oracle solves fewer
# than 60 % of the smaller batch from them over three iterations: (id) -> seed.  tests/test_poison_starts.py asserts every start.
# (empty_table: nothing bounds the iterates of an unconstrained OCP after its first Newton step; from 923 three of five stay solved)
QP_SEEDS: dict = {"empty_table-B5": 923}

# the LDS classes of tests/test_gpu_qp_layouts.py::SHORT and the horizons of tests/test_gpu_factor_sweep_forms.py::SEEDS (N >= 2), at their
# batch size 8 and with their seeds
SHORT = {
    "hard_stage_W": (dict(stage_W=True, seed=21), "k_qp_wave<5,0,0,0>", {2: 4, 4: 1}),
    "path_hard": (dict(path=True), "k_qp_wave<8,0,1,1>", {2: 4, 4: 1}),
    "alat_hard": (dict(path=True, alat=True, alat_max=4.5), "k_qp_wave<8,0,2,1>", {2: 4, 4: 4}),
}
RING = {2: 4, 3: 1, 4: 1, 5: 0, 7: 0, 9: 0}


def qp_cases():
    out = []
    for name, (lay, B_table, block) in L.TABLE.items():
        # B = 5: 200 intervals at N = 40, a ragged wave.  The table keeps its two 300-instance layouts on k_qp_wave by their batch size
        # (more instances than compute units) with the switch on; at B = 5 the switch itself has to say so.
        block = "0" if B_table > 256 else block
        blk = name.startswith("block_")
        for B in ((5, 1, 3) if blk else (5,)):
            cid = f"{name}-B{B}"
            out.append((cid, lay, B, block, QP_SEEDS.get(cid, 900 + lay.seed), qp_name(name, lay, blk)))
    for cls, (kw, kernel, seeds) in SHORT.items():
        for N in (2, 4):
            cid = f"short_{cls}-N{N}"
            out.append((cid, Lay(f"short_{cls}", N=N, **kw), 8, "0", seeds[N], kernel))
    for N, seed in RING.items():
        cid = f"ring-N{N}"
        out.append((cid, Lay(f"ring_N{N}", N=N), 8, "0", seed, "k_qp_wave<5,0,0,1>"))
    return out


QP_CASES = {c[0]: c for c in qp_cases()}


def qp_start(track, lay, B, seed):
    """(x0, yref, yref_e) of tests/test_gpu_qp_layouts.py::_start."""
    import drive

    N = lay.N
    x0 = drive.clipped_start(track, B, seed)
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = x0[:, 0:1] + 40.0 * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = x0[:, 0] + 40.0
    return x0, yref, yref_e


QP_SOLVES = 3
# the reference layout at B = 5: the handle of the cases that are about something else than the QP's table
MISC_LAYOUT, MISC_B, MISC_SEED = Lay("misc_ref", N=40), 5, 900

# The SQP mode's line search with the collocation integrator and alpha_reduction = 0.9: a ladder of 29 step lengths.  api.hip::sqp_iterations
# splits it into two pairs of launches (rollouts of the first three lengths for everybody, the rest only for the instances the first
# line-search launch leaves pending) when n_alpha B N > 16384: B = 16 at N = 40.  From this seed and steering perturbation the oracle
# shortens the step past the third rung for some instances and not for others (tests/test_poison_starts.py), so the masked rollout runs
# beside rows of ls_phi nobody writes.
SQP_B, SQP_SEED, SQP_PERTURB, SQP_ALPHA_RED = 16, 905, 0.2, 0.9
SQP_DEEP = SQP_ALPHA_RED ** 2 - 1e-9        # a step length below it was settled by the second pair of launches


def perturb_steering(u, amount=SQP_PERTURB):
    """A poor steering guess: full steps overshoot and the ladder is walked (tests/test_gpu_sqp.py::_setup)."""
    u = u.copy()
    u[:, :, 1] = np.clip(u[:, :, 1] + amount * np.sin(np.arange(u.shape[1]))[None], -0.5, 0.5)
    return u


# the two tracks of the Cartesian / track-kernel case, and its Frenet start: instance b drives on track b % 2
TWO_TRACKS = ("fsds_competition_1", "short_skidpad")


def two_track_start(plans, B=MISC_B):
    """(track_id, x0, yref, yref_e) on the reference layout."""
    from conftest import sample_x0

    tid = np.arange(B, dtype=np.int32) % 2
    xf = np.zeros((B, 8))
    for t, p in enumerate(plans):
        xf[tid == t] = sample_x0(p, int((tid == t).sum()), seed=30 + t)
    xf[:, 3] = np.clip(xf[:, 3], 4.0, 12.0)
    N = MISC_LAYOUT.N
    yref = np.zeros((B, N, 12)); yref[:, :, 0] = xf[:, 0:1] + 40.0 * np.arange(N)[None] / N
    yref_e = np.zeros((B, 8)); yref_e[:, 0] = xf[:, 0] + 40.0
    return tid, xf, yref, yref_e


# per-instance tuning on layouts.TABLE["soft_one_sided_rows_padding"]: instance b has the layout's finite bounds scaled by TUNING_BOUNDS[b % 3]
# (tests/test_gpu_qp_layouts.py::_variant) and both weights scaled by 1 + 0.1 b
TUNING_LAYOUT = "soft_one_sided_rows_padding"
TUNING_BOUNDS = (1.0, 0.9, 0.8)


def tuning_bounds(lay, b):
    arr = L.make_arrays(lay)
    out = {}
    for n in ("lbx", "ubx", "lbu", "ubu", "lg", "ug"):
        a = arr[n].copy()
        fin = np.abs(a) < L.BIG
        a[fin] *= TUNING_BOUNDS[b % 3]
        out[n] = a
    return out


def tuning_weight_factor(b):
    return 1.0 + 0.1 * b
