"""GPU: the penalty side of the device-pointer entries and of the torch layer -- ihm2mpc_set_instance_soft_device / _alat_soft_device
(kernels_penalties.hip: k_penalty_tables, k_penalty_check), ihm2mpc_get_instance_penalty_tables, ihm2mpc_get_slacks_device,
ihm2mpc_eval_adjoint_sensitivities_p_device, ihm2_amd/torch_layer.py: rti_solve_soft and plant_step.

One table throughout (LAY, N = 5): a soft lower side with a hard upper side on the state row v_x and on the second general row, both
sides of the two track rows soft, both sides of the a_lat row soft, every other row hard -- so every stage has hard sides, soft slots of
rows 0..13 on either side, the a_lat row's slots, and the slot table (78 slots, 38 of them soft, over 64 lanes: _slot_count) has
padding.  B = 8 for the tables and the bits, B = 64 for the one statistical test."""
import gc

import numpy as np
import pytest
import torch

import bitcmp
import cost_cases as C
import layouts as L
import penalty_grad_cases as PC
import poison_cases as PO
import sens_ref as S
from devmem import DevMem
from test_gpu_adjoint import _seeds
from test_gpu_qp_layouts import _start, _widen
from test_gpu_sensitivity import _outputs

pytestmark = pytest.mark.gpu

LAY = L.Layout("penalty_device", N=5, soft=1.0, soft_rows=(3, 11), soft_kind="lower", path=True, path_soft=True, alat=True, alat_soft=True,
               alat_max=2.5, width=1.2, seed=21)
HARD = L.Layout("penalty_device_hard", N=5)        # the reference's rows, every side hard: ihm2mpc_eval_adjoint_sensitivities_p_device's other branch
N, B = LAY.N, 8
TABLES = ("slot_z", "slot_Z", "stage_z", "stage_Z", "alat_z", "alat_Z")
ADJ = ("x0", "yref", "yref_e", "W", "W_e")
PEN = ("soft_z", "soft_Z", "alat_soft_z", "alat_soft_Z")


def _solver(track, Bn=B, tight=False, lay=LAY, **opts):
    from ihm2_amd.solver import BatchedOcpSolver

    ocp = L.make_ocp(lay, **opts)
    if tight:       # the re-solves of the central differences (tests/cost_cases.py)
        ocp.solver_options.qp_tol = C.QP_TOL
        ocp.solver_options.qp_solver_iter_max = 200
    s = BatchedOcpSolver(ocp, Bn, track.s_ref, track.kappa_ref, track_widths=L.track_widths(lay))
    L.apply(s.data, lay)
    s._push_bounds()
    return s


def _penalties(s, Bn=B, seed=5):
    """Random admissible penalties per instance: the shared table's on its soft sides times a factor in (0.5, 2); on the hard sides
    anything with soft_Z < 0, which the slot images must not take over."""
    rng = np.random.default_rng(seed)
    z0, Z0 = L.soft_arrays(s.data)
    soft = Z0 >= 0.0
    z = np.where(soft, z0 * rng.uniform(0.5, 2.0, (Bn,) + z0.shape), rng.uniform(0.0, 9.0, (Bn,) + z0.shape))
    Z = np.where(soft, Z0 * rng.uniform(0.5, 2.0, (Bn,) + z0.shape), -rng.uniform(1.0, 3.0, (Bn,) + z0.shape))
    az = np.asarray(s.data.alat_soft_z)[None] * rng.uniform(0.5, 2.0, (Bn, 2))
    aZ = np.asarray(s.data.alat_soft_Z)[None] * rng.uniform(0.5, 2.0, (Bn, 2))
    return z, Z, az, aZ


def _instance_bounds(Bn=B):
    arr = L.make_arrays(LAY)
    fac = 1.0 - 0.02 * np.arange(Bn)
    return {n: np.stack([np.where(np.abs(arr[n]) < L.BIG, arr[n] * f, arr[n]) for f in fac]) for n in ("lbx", "ubx", "lbu", "ubu", "lg", "ug")}


def _slot_count():
    """(slots, soft slots) of LAY's table from its arrays: a row without a soft side is one slot, a row with one is a slot per finite
    side (csrc/qp_tables.hpp: Lane::take); the a_lat row is on at the stages 1..N-1, both sides soft."""
    arr = L.make_arrays(LAY)
    Z = arr["soft_Z"]
    lo, up = np.full((N + 1, 14), -np.inf), np.full((N + 1, 14), np.inf)
    lo[1:, :8], up[1:, :8] = arr["lbx"][1:], arr["ubx"][1:]
    lo[:N, 8:10], up[:N, 8:10], lo[:N, 10:12], up[:N, 10:12] = arr["lbu"], arr["ubu"], arr["lg"], arr["ug"]
    lo[1:, 12:], up[1:, 12:] = -1e3, 0.0
    fl, fu = np.abs(lo) < L.BIG, np.abs(up) < L.BIG
    sl, su = fl & (Z[:, :14] >= 0.0), fu & (Z[:, 14:] >= 0.0)
    assert all(((fl & ~sl) | (fu & ~su))[k].any() and (sl | su)[k].any() for k in range(N + 1)), "a stage without a hard or without a soft side"
    slots = np.where(sl | su, fl.astype(int) + fu, (fl | fu).astype(int)).sum() + 2 * (N - 1)
    return int(slots), int(sl.sum() + su.sum() + 2 * (N - 1))


def _same_bits(a, b, what=""):
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint64), np.ascontiguousarray(b[k]).view(np.uint64)), (what, k)


def _put_start(s, track, fail0):
    """tests/test_gpu_qp_layouts.py::_start; fail0: instance 0 far outside the hard box on n -- an infeasible QP, reported by its status
    (the instance of tests/test_gpu_adjoint.py), so that the NaN rows are there to be compared."""
    x0, yref, yref_e = C.start(track, s.B, 900, s.N)
    if fail0:
        x0[0, 1] = 5.0
    s.set_x0(x0); s.init_guess()
    s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
    return x0, yref, yref_e


def _solve_outputs(s, track, fail0=False):
    _put_start(s, track, fail0)
    s.set_x0_sensitivities(1)
    st = s.solve()
    o = _outputs(s, alat=True)
    return dict(status=st, x=o["x"], u=o["u"], lam=o["lam"], slk=o["slk"], lam_a=o["lam_a"], slk_a=o["slk_a"])


# ---- 1. the tables ----

@pytest.mark.parametrize("bounds", [False, True])
@pytest.mark.parametrize("pairs", ["state", "alat", "both"])
def test_tables_equal_the_host_setters(track, pairs, bounds):
    """get_instance_penalty_tables after the device setter (checked and unchecked) against the same call after the host setter, bits of
    all six arrays; then one RTI solve on each handle, bit for bit."""
    dm = DevMem()
    res = []
    for how in ("host", "device", "device_unchecked"):
        s = _solver(track)
        z, Z, az, aZ = _penalties(s)
        if bounds:
            s.set_instance_bounds(**_instance_bounds())
        if pairs != "alat":
            if how == "host":
                s.set_instance_soft(z, Z)
            else:
                s.set_instance_soft_device(dm.up(z), dm.up(Z), check=how == "device")
        if pairs != "state":
            if how == "host":
                s.set_instance_alat_soft(az, aZ)
            else:
                s.set_instance_alat_soft_device(dm.up(az), dm.up(aZ), check=how == "device")
        t = s.get_instance_penalty_tables()
        out = _solve_outputs(s, track)
        s.free()
        res.append((t, out))
        # what the images must hold, independently of the host setter: the values as given per (stage, side); on the slots the
        # instance's values exactly on the soft slots -- every hard slot and the padding is (0, -1)
        if pairs != "alat":
            assert np.array_equal(t["stage_z"], z) and np.array_equal(t["stage_Z"], Z)
        if pairs != "state":
            assert np.array_equal(t["alat_z"], az) and np.array_equal(t["alat_Z"], aZ)
        hard = t["slot_Z"] < 0.0
        assert np.array_equal(hard, np.broadcast_to(hard[0], hard.shape)) and (t["slot_z"][hard] == 0.0).all() and (t["slot_Z"][hard] == -1.0).all()
        assert (~hard[0]).sum() == _slot_count()[1] and not np.array_equal(t["slot_Z"][0], t["slot_Z"][1])
    dm.free()
    (t0, o0) = res[0]
    assert np.isin(o0["status"], (0, 2)).mean() > 0.7 and o0["slk"].max() > 1e-6 and o0["slk_a"].max() > 1e-6, o0["status"]
    for t, o in res[1:]:
        for k in TABLES:
            assert np.array_equal(t[k].view(np.uint64), t0[k].view(np.uint64)), k
        for k in o0:
            np.testing.assert_array_equal(o[k], o0[k], err_msg=k)


def test_table_has_padding_and_every_kind_of_slot(track):
    """The slot table of LAY: its slots are no multiple of 64, so the table of 64 lanes has padding entries; a hard and a soft side at
    every stage (_slot_count); the a_lat row's slots beside those of the rows 0..13."""
    slots, soft = _slot_count()
    assert (slots, soft) == (78, 38) and slots % 64 != 0
    s = _solver(track)
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft(z, Z); s.set_instance_alat_soft(az, aZ)
    t = s.get_instance_penalty_tables()
    rec_soft = int((t["slot_Z"][0] >= 0).sum())
    s.free()
    assert rec_soft == soft
    # the a_lat row's slots carry the a_lat pair: 2 sides on each of the stages 1..N-1
    assert sum(int(np.isin(t["slot_Z"][0], aZ[0, m]).sum()) for m in range(2)) == 2 * (N - 1)


# ---- 2. check ----

def _with(a, idx, v):
    a = a.copy(); a[idx] = v
    return a


@pytest.mark.parametrize("kind", ["flag_hard", "flag_soft", "negative", "nan", "no_penalty", "alat_flag", "alat_negative", "alat_nan", "alat_no_penalty"])
def test_check_refuses_with_the_host_setters_message(track, kind):
    """One offence at a known (instance, stage, side) with a second one later in the scan order: check=1 refuses with the host
    setter's message for the same arrays, and the tables and the mode are what they were."""
    from ihm2_amd._lib import Ihm2mpcError

    s = _solver(track)
    dm = DevMem()
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft_device(dm.up(z), dm.up(Z), check=True)
    s.set_instance_alat_soft_device(dm.up(az), dm.up(aZ), check=True)
    before = s.get_instance_penalty_tables()
    alat = kind.startswith("alat")
    # sides: 3 = lbx[3] soft, 17 = ubx[3] hard, 26 = uh[0] soft (stages >= 1)
    bad_z, bad_Z, where = {
        "flag_hard": (z, _with(_with(Z, (2, 3, 3), -1.0), (2, 4, 17), 5.0), r"instance 2, stage 3, side 3 \(lbx\[3\]\): the side is hard"),
        "flag_soft": (z, _with(_with(Z, (1, 2, 17), 5.0), (6, 1, 3), -1.0), r"instance 1, stage 2, side 17 \(ubx\[3\]\): the side is soft"),
        "negative": (_with(_with(z, (4, 5, 26), -1.0), (4, 5, 27), -1.0), Z, r"instance 4, stage 5, side 26 \(uh\[0\]\): soft_z < 0"),
        "nan": (_with(z, (3, 1, 26), np.nan), _with(Z, (7, 0, 0), np.nan), r"instance 3, stage 1, side 26 \(uh\[0\]\): slack penalty is NaN"),
        "no_penalty": (_with(_with(z, (5, 2, 3), 0.0), (5, 3, 3), 0.0), _with(_with(Z, (5, 2, 3), 0.0), (5, 3, 3), 0.0),
                       r"instance 5, stage 2, side 3 \(lbx\[3\]\): the soft side has neither"),
        "alat_flag": (az, _with(_with(aZ, (5, 1), -1.0), (6, 0), -1.0), r"instance 5, stage 0, side 29 \(a_lat upper\): the side is hard"),
        "alat_negative": (_with(_with(az, (4, 0), -0.5), (4, 1), -0.5), aZ, r"instance 4, stage 0, side 28 \(a_lat lower\): soft_z < 0"),
        "alat_nan": (_with(az, (7, 1), np.nan), _with(aZ, (7, 0), np.nan), r"instance 7, stage 0, side 28 \(a_lat lower\): slack penalty is NaN"),
        "alat_no_penalty": (_with(_with(az, (0, 1), 0.0), (3, 0), 0.0), _with(_with(aZ, (0, 1), 0.0), (3, 0), 0.0),
                            r"instance 0, stage 0, side 29 \(a_lat upper\): the soft side has neither"),
    }[kind]
    host, dev = (s.set_instance_alat_soft, s.set_instance_alat_soft_device) if alat else (s.set_instance_soft, s.set_instance_soft_device)
    with pytest.raises(Ihm2mpcError, match=where) as eh:
        host(bad_z, bad_Z)
    with pytest.raises(Ihm2mpcError, match=where) as ed:
        dev(dm.up(bad_z), dm.up(bad_Z), check=True)
    assert str(ed.value) == str(eh.value)
    after = s.get_instance_penalty_tables()
    _same_bits(before, after, kind)
    _start(s, track, B, 900)
    assert np.isin(s.solve(), (0, 2)).mean() > 0.7         # the mode is on and fits: the solve is not refused
    dm.free()
    s.free()


# ---- 3. a pattern change behind a device set ----

def test_pattern_change_makes_the_next_solve_refuse(track):
    from ihm2_amd._lib import Ihm2mpcError

    s = _solver(track)
    dm = DevMem()
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft_device(dm.up(z), dm.up(Z), check=False)
    _start(s, track, B, 900)
    s.solve()
    z0, Z0 = (a.copy() for a in L.soft_arrays(s.data))
    Z1 = Z0.copy(); Z1[:, 12:14] = -1.0            # the lower sides of the track rows hard
    s.set_soft(z0, Z1)
    with pytest.raises(Ihm2mpcError, match=r"per-instance penalties do not fit the batch-shared constraint pattern any more: set them again, or pass NULL"):
        s.solve()
    # per-instance bounds coming behind it change nothing of that
    s.set_instance_bounds(**_instance_bounds())
    with pytest.raises(Ihm2mpcError, match=r"do not fit the batch-shared constraint pattern any more"):
        s.solve()
    s.set_instance_bounds()
    # set again in the new pattern: solves, and holds what the host setter gives on a fresh handle with that pattern
    Zn = np.where(Z1[None] >= 0.0, Z, -1.0)
    s.set_instance_soft_device(dm.up(z), dm.up(Zn), check=True)
    t = s.get_instance_penalty_tables()
    assert np.isin(s.solve(), (0, 2)).mean() > 0.7
    s.set_instance_soft_device(0, 0)               # NULL, NULL: the shared penalties again
    s.solve()
    s.free()
    f = _solver(track)
    f.set_soft(z0, Z1)
    f.set_instance_soft(z, Zn)
    _same_bits(t, f.get_instance_penalty_tables(), "after the pattern change")
    f.free()
    dm.free()


def test_shared_setters_that_keep_the_soft_flags_keep_device_set_values(track):
    """Behind a device set of both pairs: every shared setter again (set_bounds with other numbers on the same sides, the track rows,
    the a_lat row and set_soft with other shared values -- the soft flags as they were) keeps the device-set values, as it keeps
    host-set ones: tables and one solve are those of a handle that got the same shared table and then the host setters."""
    dm = DevMem()

    def change(h):
        d = h.data
        d.lbu, d.ubu = d.lbu * 0.9, d.ubu * 0.9
        d.soft_z = np.where(d.soft_Z >= 0.0, 1.5 * d.soft_z, d.soft_z)
        d.alat_soft_z = 0.5 * np.asarray(d.alat_soft_z)
        h._push_bounds()

    s = _solver(track)
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft_device(dm.up(z), dm.up(Z), check=False)
    s.set_instance_alat_soft_device(dm.up(az), dm.up(aZ), check=False)
    change(s)
    got, out = s.get_instance_penalty_tables(), _solve_outputs(s, track)
    s.free()
    f = _solver(track)
    change(f)
    f.set_instance_soft(z, Z); f.set_instance_alat_soft(az, aZ)
    want, ref = f.get_instance_penalty_tables(), _solve_outputs(f, track)
    f.free()
    dm.free()
    _same_bits(got, want)
    assert np.isin(ref["status"], (0, 2)).mean() > 0.7
    for k in ref:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


def test_a_failure_behind_the_check_puts_the_previous_penalties_back(track):
    """The device setter has to build the images first (the host-held pair stopped fitting), and that fails on per-instance bounds
    whose finite sides the shared table has lost: the call is refused with that text and the pair's previous host values are back --
    still not fitting, as before the call -- where dropping them would have left the handle without per-instance penalties."""
    from ihm2_amd._lib import Ihm2mpcError

    dm = DevMem()
    s = _solver(track)
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft(z, Z)
    s.set_instance_bounds(**_instance_bounds())
    z0, Z0 = (a.copy() for a in L.soft_arrays(s.data))
    Z1 = Z0.copy(); Z1[:, 12:14] = -1.0
    s.set_soft(z0, Z1)                             # the host-held pair does not fit any more
    s.data.ubu = s.data.ubu.copy(); s.data.ubu[:, 0] = 1e20
    with pytest.raises(Ihm2mpcError, match="the finite sides .* differ from the batch-shared table's"):
        s._push_bounds()                           # ... and neither do the per-instance bounds
    Zn = np.where(Z1[None] >= 0.0, Z, -1.0)
    with pytest.raises(Ihm2mpcError, match="the finite sides .* differ from the batch-shared table's"):
        s.set_instance_soft_device(dm.up(z), dm.up(Zn), check=True)
    s.set_instance_bounds()                        # the bounds dropped: what is left is the penalties' state
    with pytest.raises(Ihm2mpcError, match=r"per-instance penalties do not fit the batch-shared constraint pattern any more"):
        _put_start(s, track, False)                # (the initial guess is the first call that needs the tables)
    s.set_instance_soft_device(dm.up(z), dm.up(Zn), check=True)
    _put_start(s, track, False)
    assert np.isin(s.solve(), (0, 2)).mean() > 0.7
    dm.free()
    s.free()


def test_device_set_behind_a_refused_shared_setter_rebuilds_or_refuses(track):
    """A device-set pair that fits, per-instance bounds, then a shared set_bounds with more finite sides: it is refused for the
    per-instance bounds -- after the handle's slot table has been replaced, so the per-instance images on the device are the previous
    table's (of another length, when the table grows).  The next device set must not scatter into them on the strength of what the
    handle believed before: it rebuilds, which is refused with the bounds' text, and the getter refuses too; with the bounds dropped it
    rebuilds and holds what a fresh handle with the new shared table and the host setters holds."""
    from ihm2_amd._lib import Ihm2mpcError

    dm = DevMem()

    def more_sides(h):
        d = h.data
        d.lbx, d.ubx = d.lbx.copy(), d.ubx.copy()
        for i in (2, 4, 5):
            d.lbx[1:, i], d.ubx[1:, i] = L.STATE_BOX[i]
        h._push_bounds()

    s = _solver(track)
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft_device(dm.up(z), dm.up(Z), check=False)
    s.set_instance_alat_soft_device(dm.up(az), dm.up(aZ), check=False)
    s.set_instance_bounds(**_instance_bounds())
    with pytest.raises(Ihm2mpcError, match="the finite sides .* differ from the batch-shared table's"):
        more_sides(s)
    for check in (False, True):
        with pytest.raises(Ihm2mpcError, match="the finite sides .* differ from the batch-shared table's"):
            s.set_instance_soft_device(dm.up(z), dm.up(Z), check=check)
    with pytest.raises(Ihm2mpcError, match="are not those of the current constraint rows"):
        s.get_instance_penalty_tables()
    s.set_instance_bounds()
    s._push_bounds()                               # (the shared setters that the refusal cut short: track rows, a_lat row, penalties)
    s.set_instance_soft_device(dm.up(z), dm.up(Z), check=False)
    s.set_instance_alat_soft_device(dm.up(az), dm.up(aZ), check=False)
    got, out = s.get_instance_penalty_tables(), _solve_outputs(s, track)
    s.free()
    f = _solver(track)
    more_sides(f)
    f.set_instance_soft(z, Z); f.set_instance_alat_soft(az, aZ)
    want, ref = f.get_instance_penalty_tables(), _solve_outputs(f, track)
    f.free()
    dm.free()
    _same_bits(got, want)
    assert np.isin(ref["status"], (0, 2)).mean() > 0.7
    for k in ref:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


def test_other_setters_leave_device_set_values_in_place(track):
    """Per-instance bounds, and the host setter of the other pair, behind a device set: the tables are those of a handle that got
    everything from the host."""
    dm = DevMem()
    s = _solver(track)
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft_device(dm.up(z), dm.up(Z), check=False)
    s.set_instance_bounds(**_instance_bounds())
    s.set_instance_alat_soft(az, aZ)
    got, out = s.get_instance_penalty_tables(), _solve_outputs(s, track)
    s.free()
    f = _solver(track)
    f.set_instance_bounds(**_instance_bounds())
    f.set_instance_soft(z, Z); f.set_instance_alat_soft(az, aZ)
    want, ref = f.get_instance_penalty_tables(), _solve_outputs(f, track)
    f.free()
    dm.free()
    _same_bits(got, want)
    for k in ref:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


# ---- 4., 5. the device adjoint entry and the slacks ----

def _solved(track, dm):
    s = _solver(track)
    z, Z, az, aZ = _penalties(s)
    s.set_instance_soft_device(dm.up(z), dm.up(Z), check=False)
    s.set_instance_alat_soft_device(dm.up(az), dm.up(aZ), check=False)
    out = _solve_outputs(s, track, fail0=True)
    ok = np.isin(out["status"], (0, 2))
    assert not ok[0] and ok.mean() > 0.7, out["status"]       # instance 0 failed: its rows are the NaN rows
    return s, out


def _p_device(s, dm, S_, seeds, want=ADJ + PEN + ("zeta",)):
    shapes = dict(x0=(B, S_, 8), yref=(B, S_, N, 12), yref_e=(B, S_, 8), W=(B, S_, 12, 12), W_e=(B, S_, 8, 8), soft_z=(B, S_, N + 1, 28),
                  soft_Z=(B, S_, N + 1, 28), alat_soft_z=(B, S_, N + 1, 2), alat_soft_Z=(B, S_, N + 1, 2), zeta=(B, S_, N + 1, 10))
    ptr = {k: (dm.alloc(8 * int(np.prod(sh)), fill=0x5A) if k in want else 0) for k, sh in shapes.items()}
    s.eval_adjoint_penalty_sensitivities_device(S_, *[0 if a is None else dm.up(a) for a in seeds], *ptr.values())
    s.synchronize()
    return {k: dm.down(p, shapes[k]) for k, p in ptr.items() if p}


@pytest.mark.parametrize("S_", [1, 3])
def test_p_device_gives_the_host_entrys_bits(track, S_):
    dm = DevMem()
    s, out = _solved(track, dm)
    assert np.isin(out["status"], (0, 2)).mean() > 0.7
    rng = np.random.default_rng(40 + S_)
    sx, su = _seeds(B, S_, N, 30 + S_)
    ss, ssa = rng.standard_normal((B, S_, N + 1, 28)), rng.standard_normal((B, S_, N + 1, 2))
    for seeds in ((sx, su, ss, ssa), (sx, su, None, None), (None, None, ss, None), (None, su, None, ssa)):
        host = s.eval_adjoint_penalty_sensitivities(*seeds)
        dev = _p_device(s, dm, S_, seeds)
        assert host.keys() == dev.keys()
        for k in host:
            assert np.array_equal(np.isnan(dev[k]), np.isnan(host[k])), k
            np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
            assert np.isnan(host[k][0]).all() and np.isfinite(host[k][1:][np.isin(out["status"][1:], (0, 2))]).all(), k
        assert any(np.nan_to_num(host[k]).any() for k in PEN)
    # the five old gradients alone: the bits of the _w_device entry
    first = _p_device(s, dm, S_, (sx, su, None, None), want=ADJ)
    shapes = {k: first[k].shape for k in ADJ}
    ptr = {k: dm.alloc(first[k].nbytes, fill=0x5A) for k in ADJ}
    s.eval_adjoint_weight_sensitivities_device(S_, dm.up(sx), dm.up(su), *ptr.values())
    s.synchronize()
    for k in ADJ:
        np.testing.assert_array_equal(first[k], dm.down(ptr[k], shapes[k]), err_msg=k)
    dm.free()
    s.free()


@pytest.mark.parametrize("S_", [1, 3])
def test_p_device_on_a_table_without_a_soft_side(track, S_):
    """No k_penalty_grad runs on an all-hard table: the host entry fills the four penalty gradients with zeros, NaN where the status is
    neither 0 nor 2, after reading the status back; the device entry has a kernel for it (k_penalty_fill).  All and some of the outputs,
    pre-filled with 0x5A, with and without slack seeds, one instance failed: the host entry's bits, NaN masks included."""
    dm = DevMem()
    s = _solver(track, lay=HARD)
    out = _solve_outputs(s, track, fail0=True)
    ok = np.isin(out["status"], (0, 2))
    assert not ok[0] and ok.mean() > 0.7, out["status"]
    rng = np.random.default_rng(50 + S_)
    sx, su = _seeds(B, S_, N, 60 + S_)
    ss, ssa = rng.standard_normal((B, S_, N + 1, 28)), rng.standard_normal((B, S_, N + 1, 2))
    cases = [(S_, (sx, su, None, None)), (S_, (sx, su, ss, ssa)), (S_, (None, None, ss, None)), (2, (None, None, None, None))]
    for n_seeds, seeds in cases:
        host = s.eval_adjoint_penalty_sensitivities(*seeds)
        for k in PEN:
            assert not host[k][ok].any() and np.isnan(host[k][~ok]).all(), k
        for want in (ADJ + PEN + ("zeta",), PEN, ("soft_Z", "alat_soft_z"), ("x0", "soft_z"), ("alat_soft_Z",)):
            dev = _p_device(s, dm, n_seeds, seeds, want=want)
            assert set(dev) == set(want)
            for k in dev:
                assert np.array_equal(np.isnan(dev[k]), np.isnan(host[k])), (k, want)
                np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
                live = ~np.isnan(host[k])
                assert np.array_equal(dev[k][live].view(np.uint64), host[k][live].view(np.uint64)), (k, want)      # (+0.0, not -0.0)
    dm.free()
    s.free()


def test_p_device_unit_seeds_and_refusals(track):
    from ihm2_amd._lib import Ihm2mpcError

    dm = DevMem()
    s, _ = _solved(track, dm)
    host = s.eval_adjoint_penalty_sensitivities()           # the two unit seeds on u_0
    dev = _p_device(s, dm, 2, (None, None, None, None))
    for k in host:
        np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
    for n, text in ((1, "needs n_seeds = 2"), (9, "takes 1 to 8 seeds")):
        with pytest.raises(Ihm2mpcError, match=text):
            s.eval_adjoint_penalty_sensitivities_device(n)
    s.set_x0_sensitivities(0)
    with pytest.raises(Ihm2mpcError, match="x0 sensitivities are off"):
        s.eval_adjoint_penalty_sensitivities_device(2)
    dm.free()
    s.free()


def test_get_slacks_device_equals_get_slacks(track):
    dm = DevMem()
    s, out = _solved(track, dm)
    p, pa = dm.alloc(8 * B * (N + 1) * 28, fill=0x5A), dm.alloc(8 * B * (N + 1) * 2, fill=0x5A)
    s.get_slacks_device(p, pa)
    s.synchronize()
    got, got_a = dm.down(p, (B, N + 1, 28)), dm.down(pa, (B, N + 1, 2))
    np.testing.assert_array_equal(got, s.get_slacks())
    np.testing.assert_array_equal(got_a, s.get_alat_multipliers()[1])
    assert got.max() > 1e-6 and got_a.max() > 1e-6
    dm.free()
    s.free()


# ---- 6. the layer's bits ----

def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0", requires_grad=grad)


def _free(s):
    gc.collect()
    s.free()


class _Start:
    """A handle of LAY with the state every solve starts from kept for restoring (the warm start is state of the solver)."""

    def __init__(self, track, Bn, tight=False, slow=False, fail0=False):
        self.s = s = _solver(track, Bn, tight=tight)
        self.x0, self.yref, self.yref_e = C.start(track, Bn, 1234, N)      # (test_gpu_qp_layouts._start's)
        if slow:        # every car below the soft lower bound on v_x (3 m/s): its slack is in use and moves u_0
            self.x0[:, 3] = np.linspace(1.6, 2.9, Bn)
        if fail0:       # instance 0 far outside the hard box on n: an infeasible QP, whose rows are the NaN rows
            self.x0[0, 1] = 5.0
        s.set_x0(self.x0); s.init_guess()
        s.set_yref(self.yref); s.set_yref_e(self.yref_e); s.set_multipliers(None, None)
        s.set_x0_sensitivities(1)
        self.x, self.u = s.get_x(), s.get_u()
        self.pi, self.lam = s.get_multipliers()
        self.slk = s.get_slacks()
        self.lam_a, self.slk_a = s.get_alat_multipliers()

    def restore(self):
        s = self.s
        s.set_x(self.x); s.set_u(self.u); s.set_multipliers(self.pi, self.lam); s.set_slacks(self.slk)
        s.set_alat_multipliers(self.lam_a, self.slk_a)


def test_layer_gradients_equal_the_host_entrys_bits(track):
    c = _Start(track, B, fail0=True)
    _layer_bits(c)
    _free(c.s)


def _layer_bits(c):
    from ihm2_amd.torch_layer import rti_solve, rti_solve_soft

    s = c.s
    rng = np.random.default_rng(11)
    z, Z, az, aZ = _penalties(s)
    W = (1.0 + 0.01 * np.arange(B))[:, None, None] * np.asarray(s.data.W[0], dtype=np.float64)[None]
    We = (1.0 + 0.01 * np.arange(B))[:, None, None] * np.asarray(s.data.W_e, dtype=np.float64)[None]
    cx, cu = rng.standard_normal((B, N + 1, 8)), rng.standard_normal((B, N, 2))
    cs, csa = rng.standard_normal((B, N + 1, 28)), rng.standard_normal((B, N + 1, 2))
    ins = [_t(a, grad=True) for a in (c.x0, c.yref, c.yref_e, W, We, z, Z, az, aZ)]
    c.restore()
    x, u, sl, sa, status = rti_solve_soft(s, *ins)
    assert sl.shape == (B, N + 1, 28) and sa.shape == (B, N + 1, 2) and sl.requires_grad and sa.requires_grad and not status.requires_grad
    loss = (_t(cx) * x).sum() + (_t(cu) * u).sum() + (_t(cs) * sl).sum() + (_t(csa) * sa).sum()
    grads = [g.cpu().numpy() for g in torch.autograd.grad(loss, ins)]
    layer = dict(zip(ADJ + ("soft_z", "soft_Z", "alat_z", "alat_Z"), grads))
    out = {k: v.detach().cpu().numpy() for k, v in dict(x=x, u=u, slk=sl, slk_a=sa, status=status).items()}
    # the same state through the host setters
    c.restore()
    s.set_instance_weights(W, We)
    s.set_instance_soft(z, Z); s.set_instance_alat_soft(az, aZ)
    s.set_x0(c.x0); s.set_yref(c.yref); s.set_yref_e(c.yref_e)
    st = s.solve()
    host = s.eval_adjoint_penalty_sensitivities(cx, cu, cs, csa)
    # (tests/bitcmp.py: a failure names the array, counts the differing entries and shows the first of them with both values)
    bitcmp.assert_all_same_bits("rti_solve_soft against the host setters and solve", out,
                                dict(status=st, x=s.get_x(), u=s.get_u(), slk=s.get_slacks(), slk_a=s.get_alat_multipliers()[1]), nan_equal=True)
    ok = (st == 0) | (st == 2)
    assert not ok[0] and ok.mean() > 0.7 and out["slk"].max() > 1e-6, st
    for k in ADJ + ("soft_z", "soft_Z"):
        bitcmp.assert_same_bits(f"gradient in {k}", layer[k], host[k], nan_equal=True)
        bitcmp.assert_same_bits(f"gradient in {k}, solved instances", layer[k], host[k], rows=ok)
    assert np.abs(layer["soft_z"][ok]).max() > 0.0 and np.abs(layer["soft_Z"][ok]).max() > 0.0
    # the a_lat pair is one pair for all stages: the layer sums the host entry's per-stage rows (N - 1 terms: the order of the sum is
    # the only difference, a few ulp of the sum of the absolute terms)
    for k, hk in (("alat_z", "alat_soft_z"), ("alat_Z", "alat_soft_Z")):
        want, mag = host[hk][ok].sum(1), np.abs(host[hk][ok]).sum(1)
        assert layer[k].shape == (B, 2) and np.abs(want).max() > 0.0
        assert (np.abs(layer[k][ok] - want) <= 8 * np.finfo(float).eps * mag).all(), k
        assert np.isnan(layer[k][~ok]).all()
    # without penalties: rti_solve's x, u, status and five gradients, bit for bit (the solver's penalties stay what they are)
    res = []
    for fn in (rti_solve, rti_solve_soft):
        c.restore()
        a = [_t(v, grad=True) for v in (c.x0, c.yref, c.yref_e, W, We)]
        o = fn(s, *a)
        g = torch.autograd.grad((_t(cx) * o[0]).sum() + (_t(cu) * o[1]).sum(), a)
        res.append([o[0].detach().cpu().numpy(), o[1].detach().cpu().numpy(), o[-1].cpu().numpy()] + [v.cpu().numpy() for v in g])
    for name, a, b in zip(("x", "u", "status") + tuple("gradient in " + k for k in ADJ), *res):
        bitcmp.assert_same_bits(f"rti_solve against rti_solve_soft without penalties: {name}", a, b, nan_equal=True)


# ---- 7. the layer against central differences of itself ----

def test_penalty_gradient_against_central_differences_of_the_layer(track):
    """tests/test_gpu_penalty_grad.py::test_gradient_against_whole_solves' quantity through the layer, B = 64: the gradient of u[:, 0, m]
    in (soft_z, soft_Z) from backward, contracted with a direction of the penalties' size (z N(0,1), Z N(0,1) per instance on the soft
    sides), against central differences of rti_solve_soft itself at +- 1e-4 of it; the measure of tests/penalty_grad_cases.py,
    |pred - fd| / max(|fd|, free), the skip rule of tests/test_gpu_torch_layer.py::_central_differences (weakly active or not solved) and
    the bars of that existing test (tests/cost_cases.py::profile: median <= 1e-6, 75 % <= 1e-5, 95 % <= 1e-3), at least 48 of 64 kept;
    the zero prediction does not meet them.  The start is tests/cost_cases.py::start with every car below the soft lower bound on v_x:
    from the unchanged start the slacks move u_0 on one instance in fifty and a zero gradient met the bars.  The CPU oracle keeps 64 of
    64 instances of this start (qp_solve + weakly_active on every instance's own penalties), and its reference gradient is above 1e-3
    of the measure's scale on a third of them.

    Measured: 64 of 64 instances kept, median 1.3e-9, 92 % below 1e-5, 98 % below 1e-3, 1.8e-3 at worst -- the existing test's bars,
    unwidened; the zero prediction has median 1.4e-8 with 66 % below 1e-5 and 72 % below 1e-3."""
    c = _Start(track, 64, tight=True, slow=True)
    _central_differences(c, track)
    _free(c.s)


def _central_differences(c, track):
    from ihm2_amd.torch_layer import rti_solve_soft
    from oracle import oracle as orc

    s, Bn, eps = c.s, 64, PC.EPS
    z, Z, az, aZ = _penalties(s, Bn)
    rng = np.random.default_rng(77)
    soft = Z >= 0.0
    dz = np.where(soft, z * rng.standard_normal(z.shape), 0.0)
    dZ = np.where(soft, Z * rng.standard_normal(Z.shape), 0.0)
    tx0, tyref, tyref_e, taz, taZ = _t(c.x0), _t(c.yref), _t(c.yref_e), _t(az), _t(aZ)

    def solve_at(sign, grad=False):
        c.restore()
        tz, tZ = _t(z + sign * eps * dz, grad), _t(Z + sign * eps * dZ, grad)
        o = rti_solve_soft(s, tx0, tyref, tyref_e, None, None, tz, tZ, taz, taZ)
        return tz, tZ, o[1], o[4]

    tz, tZ, us, st_t = solve_at(0.0, grad=True)
    pred = np.zeros((Bn, 2))
    for m in range(2):
        gz, gZ = torch.autograd.grad(us[:, 0, m].sum(), (tz, tZ), retain_graph=(m == 0))
        pred[:, m] = (gz.cpu().numpy() * dz).sum((1, 2)) + (gZ.cpu().numpy() * dZ).sum((1, 2))
    st = st_t.cpu().numpy()
    o = _outputs(s, alat=True)
    lam, slk = _widen(o["lam"], o["lam_a"]), _widen(o["slk"], o["slk_a"])
    P = orc.OracleProblem(s.data.as_dict(track.s_ref, track.kappa_ref, track_widths=L.track_widths(LAY)))
    A, Bm, b = s.get_linearization()
    wide = lambda a28, a2: _widen(a28, np.broadcast_to(a2, (N + 1, 2)))  # noqa: E731
    keep, free = [], np.zeros((Bn, 2))
    for i in np.flatnonzero(st == 0):
        args = (c.x[i], c.u[i], c.x0[i], c.yref[i], c.yref_e[i])
        qp = L.assemble_qp(s.data, *args, A[i], Bm[i], b[i], nonlinear=P.build_qp(*args))
        step = np.zeros((N + 1, 10)); step[:, :8] = o["x"][i] - c.x[i]; step[:N, 8:] = o["u"][i] - c.u[i]
        zi, Zi = wide(z[i], az[i]), wide(Z[i], aZ[i])
        if S.weakly_active(qp, step, lam[i], sl=slk[i], soft_z=zi, soft_Z=Zi):
            continue
        keep.append(i)
        sd = np.zeros((2, N + 1, 10)); sd[0, 0, 8] = sd[1, 0, 9] = 1.0
        free[i] = PC.free_scale(qp, step, lam[i], slk[i], zi, Zi, sd, wide(dz[i], np.zeros(2)), wide(dZ[i], np.zeros(2)))
    with torch.no_grad():
        _, _, up, stp = solve_at(1.0)
        up, stp = up[:, 0].cpu().numpy(), stp.cpu().numpy()
        _, _, um, stm = solve_at(-1.0)
        um, stm = um[:, 0].cpu().numpy(), stm.cpu().numpy()
    fd = (up - um) / (2 * eps)
    solved = (st == 0) & (stp == 0) & (stm == 0)
    keep = np.array([i for i in keep if solved[i]], dtype=int)
    errs, zero = PC.measure(pred, fd, free), PC.measure(0.0 * pred, fd, free)
    (med, s5, s3), met = C.profile(errs[keep])
    (med0, s50, s30), met0 = C.profile(zero[keep])
    print(f"LAYER-PENALTY-FD: kept {keep.size} of {Bn}, median {med:.2e} share<=1e-5 {s5:.3f} share<=1e-3 {s3:.3f} max {errs[keep].max():.2e}; "
          f"zero prediction median {med0:.2e} share<=1e-5 {s50:.3f} share<=1e-3 {s30:.3f}")
    assert keep.size >= 48, keep.size
    assert met, (med, s5, s3, np.sort(errs[keep])[-4:])
    assert not met0, (med0, s50, s30)


# ---- 8. the plant step ----

@pytest.mark.parametrize("model", [0, 1, -1])
def test_plant_step_bits_and_gradients(track, model):
    from ihm2_amd.torch_layer import plant_step

    s = _solver(track)

    def body():
        rng = np.random.default_rng(3 + model)
        x0 = _start(s, track, B, 900)[0]
        x0[:, 3], x0[:, 7] = np.linspace(2.0, 12.0, B), 0.2         # both branches of the switched plant (v^2 sin(beta) / l_R against 3)
        u = np.stack([rng.uniform(-100.0, 200.0, B), rng.uniform(-0.2, 0.2, B)], 1)
        g = rng.standard_normal((B, 8))
        host = s.sim_step_sens(x0, u, model=model, M_sim=25)
        tx, tu = _t(x0, True), _t(u, True)
        serial = s._serial
        xn, used = plant_step(s, tx, tu, model=model, M_sim=25)
        assert s._serial == serial and used.dtype == torch.int32 and not used.requires_grad and xn.requires_grad
        gx, gu = torch.autograd.grad((_t(g) * xn).sum(), (tx, tu))
        return host, g, xn.detach().cpu().numpy(), used.cpu().numpy(), gx.cpu().numpy(), gu.cpu().numpy()

    host, g, xn, used, gx, gu = body()
    _free(s)
    np.testing.assert_array_equal(xn, host["x"])
    np.testing.assert_array_equal(used, host["model_used"])
    if model == -1:
        assert len(set(used.tolist())) == 2, used
    # S' g: a dot product of eight terms per entry, the order of the sum is the only difference
    for got, Sm in ((gx, host["Sx"]), (gu, host["Su"])):
        want = np.einsum("bij,bi->bj", Sm, g)
        mag = np.einsum("bij,bi->bj", np.abs(Sm), np.abs(g))
        assert np.isfinite(got).all() and (np.abs(got - want) <= 1e-14 * mag).all(), np.abs(got - want).max()


def test_plant_step_between_a_solve_and_its_backward_and_a_closed_loop_chain(track):
    from ihm2_amd.torch_layer import plant_step, rti_solve_soft

    c = _Start(track, B)
    s = c.s
    z, Z, az, aZ = _penalties(s)

    def body():
        # the plant step does not count as a use of the solver: backward of the solve before it goes through
        c.restore()
        tx0, tZ = _t(c.x0, True), _t(Z, True)
        x, u, sl, sa, st = rti_solve_soft(s, tx0, _t(c.yref), _t(c.yref_e), None, None, _t(z), tZ, _t(az), _t(aZ), zero_failed=True)
        xn, _ = plant_step(s, tx0.detach(), u[:, 0].detach().contiguous(), model=0, M_sim=25)
        g = torch.autograd.grad(u.sum() + sl.sum(), (tx0, tZ))
        assert all(torch.isfinite(a).all() for a in g)
        # x0 -> rti -> plant -> rti -> loss: the second solve is the solver's last use when backward reaches it, the first solve's
        # backward would come after it -- so each step has a solver of its own, as a closed loop over a horizon of steps would.  The
        # two-step chain against its composition from the host entries (tests/test_gpu_torch_chain.py::compare_chain: the forward bit
        # for bit, every gradient of both steps to the reference's own rounding scale)
        import test_gpu_torch_chain as TC

        c2 = _Start(track, B)
        cs = [c, c2]
        _, grads, _, worst = TC.compare_chain(cs, c.x0, TC.chain_inputs(c, 2), TC.chain_seeds(2), model=0, zero_failed=True)
        print(f"CHAIN-HOST two steps: worst ratio {worst[0]:.3f} of 8 (step {worst[1]}, {worst[2]})")
        assert grads[0]["x0"].shape == (B, 8) and grads[0]["soft_Z"].shape == (B, N + 1, 28)
        assert np.isfinite(grads[0]["x0"]).all() and np.isfinite(grads[0]["soft_Z"]).all()          # (zero_failed)
        assert np.abs(grads[0]["x0"]).max() > 0.0 and np.abs(grads[0]["soft_Z"]).max() > 0.0
        return c2

    c2 = body()
    _free(c2.s)
    _free(s)


@pytest.mark.parametrize("subset", ["s", "sa", "u_sa"])
def test_layer_seed_subsets_equal_the_host_entry_with_zeros_for_the_absent_seeds(track, subset):
    """rti_solve_soft's backward with a loss on some of its outputs only (set_materialize_grads(False): an output the loss does not use
    reaches backward as None -- no x / u seed at all, a slack seed alone) against the host entry given zeros for the absent seeds: the
    bits on the solved rows, the NaN pattern on the failed one, B = 8."""
    from ihm2_amd.torch_layer import rti_solve_soft

    c = _Start(track, B, fail0=True)
    s = c.s

    def body():
        rng = np.random.default_rng(23)
        z, Z, az, aZ = _penalties(s)
        seeds = dict(x=None, u=rng.standard_normal((B, N, 2)), s=rng.standard_normal((B, N + 1, 28)), sa=rng.standard_normal((B, N + 1, 2)))
        used = {"s": ("s",), "sa": ("sa",), "u_sa": ("u", "sa")}[subset]
        ins = [_t(a, grad=True) for a in (c.x0, c.yref, c.yref_e, None, None, z, Z, az, aZ) if a is not None]
        c.restore()
        x, u, sl, sa, status = rti_solve_soft(s, *ins[:3], None, None, *ins[3:])
        out = dict(x=x, u=u, s=sl, sa=sa)
        loss = sum((_t(seeds[k]) * out[k]).sum() for k in used)
        grads = [g.cpu().numpy() for g in torch.autograd.grad(loss, ins)]
        st = status.cpu().numpy()
        zeros = dict(x=np.zeros((B, N + 1, 8)), u=np.zeros((B, N, 2)), s=np.zeros((B, N + 1, 28)), sa=np.zeros((B, N + 1, 2)))
        host = s.eval_adjoint_penalty_sensitivities(*[seeds[k] if k in used else zeros[k] for k in ("x", "u", "s", "sa")])
        return grads, st, host

    grads, st, host = body()
    _free(s)
    ok = (st == 0) | (st == 2)
    assert not ok[0] and ok.mean() > 0.7, st
    layer = dict(zip(("x0", "yref", "yref_e", "soft_z", "soft_Z", "alat_z", "alat_Z"), grads))
    for k in ("x0", "yref", "yref_e", "soft_z", "soft_Z"):
        bitcmp.assert_same_bits(f"seeds on {subset}: gradient in {k}", layer[k], host[k], nan_equal=True)
        bitcmp.assert_same_bits(f"seeds on {subset}: gradient in {k}, solved instances", layer[k], host[k], rows=ok)
        assert np.isnan(layer[k][~ok]).all() and np.isfinite(layer[k][ok]).all(), k
    assert any(np.abs(layer[k][ok]).max() > 0.0 for k in ("soft_z", "soft_Z"))
    for k, hk in (("alat_z", "alat_soft_z"), ("alat_Z", "alat_soft_Z")):     # the sum over the stages: test_layer_gradients_equal_the_host_entrys_bits' rule
        want, mag = host[hk][ok].sum(1), np.abs(host[hk][ok]).sum(1)
        assert (np.abs(layer[k][ok] - want) <= 8 * np.finfo(float).eps * mag).all(), k
        assert np.isnan(layer[k][~ok]).all()


# ---- 9. workspace poison ----

def test_workspace_poison(track):
    """The new kernels and the device adjoint entry on a handle created with IHM2MPC_POISON_WORKSPACE=1 give the bits of the
    zero-filled twin, on the first pass and on the replay (tests/poison_cases.py::run_twin): outputs that are asked for and outputs that
    land in the handle's workspace."""
    dm = DevMem()
    x0, yref, yref_e = C.start(track, B, 900, N)
    rng = np.random.default_rng(8)
    sx, su = _seeds(B, 2, N, 31)
    ss, ssa = rng.standard_normal((B, 2, N + 1, 28)), rng.standard_normal((B, 2, N + 1, 2))

    def make():
        s = _solver(track)
        s.set_x0_sensitivities(1)
        return s

    def start(s):
        s.set_x0(x0); s.init_guess()
        s.set_yref(yref); s.set_yref_e(yref_e); s.set_multipliers(None, None)
        return yref, yref_e

    def calls(s, tag):
        z, Z, az, aZ = _penalties(s)
        s.set_instance_soft_device(dm.up(z), dm.up(Z), check=True)
        s.set_instance_alat_soft_device(dm.up(az), dm.up(aZ), check=False)
        out = dict(tables=s.get_instance_penalty_tables(), status=s.solve())
        out["all"] = _p_device(s, dm, 2, (sx, su, ss, ssa))
        out["some"] = _p_device(s, dm, 2, (None, su, ss, None), want=("x0", "soft_Z", "alat_soft_z"))
        out["unit"] = _p_device(s, dm, 2, (None, None, None, None), want=PEN)
        p, pa = dm.alloc(8 * B * (N + 1) * 28, fill=0x5A), dm.alloc(8 * B * (N + 1) * 2, fill=0x5A)
        s.get_slacks_device(p, pa)
        s.synchronize()
        out["slk"], out["slk_a"] = dm.down(p, (B, N + 1, 28)), dm.down(pa, (B, N + 1, 2))
        return out

    PO.run_twin(make, start, calls, accepted=(0, 2), share=0.7)

    # the branch without a soft side (k_penalty_fill), one instance failed
    x0[0, 1] = 5.0

    def make_hard():
        s = _solver(track, lay=HARD)
        s.set_x0_sensitivities(1)
        return s

    def calls_hard(s, tag):
        out = dict(status=s.solve())
        assert out["status"][0] not in (0, 2)
        out["all"] = _p_device(s, dm, 2, (sx, su, ss, ssa))
        out["some"] = _p_device(s, dm, 2, (None, su, None, None), want=("yref", "soft_Z", "alat_soft_z"))
        out["unit"] = _p_device(s, dm, 2, (None, None, None, None), want=PEN)
        return out

    PO.run_twin(make_hard, start, calls_hard, accepted=(0, 2), share=0.7)
    dm.free()
