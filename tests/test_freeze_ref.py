"""tests/freeze_ref.py (the stop rules of ihm2mpc_run_steps(freeze != 0) in numpy) on hand-written histories, one car per cause, and
against the bookkeeping of ihm2_amd.closed_loop_sim.run_closed_loop on the same synthetic cars.  No GPU."""
import numpy as np
import pytest

import freeze_ref as F

T = 6
LAP_STOP = 10.0
INF = np.inf

# One synthetic car per line: start s, metres per step, the s above which its solves fail (status 4), the s above which its plant
# step gives a NaN.  The plant adds the speed to s, so after the plant of step t a car stands at s0 + v (t + 1).
CARS = {                 # s0,  v,   solve fails, plant NaN       what the rules must make of it over T = 6 steps
    "healthy":          (0.0, 1.0, INF, INF),                   # drives every step
    "slow":             (0.0, 0.5, INF, INF),
    "fails_row_2":      (0.0, 1.0, 2.5, INF),                   # the solve of step 2 (s = 3) fails: stops at step 3
    "nan_step_3":       (0.0, 1.0, INF, 2.5),                   # the plant of step 3 (from s = 3) is NaN: stops at step 3 at s = 3
    "lap_row_3":        (0.0, 3.0, INF, INF),                   # s = 12 > 10 after step 3: keeps row 3, stops at step 4
    "failed_before":    (0.0, 1.0, -1.0, INF),                  # the solve before the call failed: stops at step 0
    "fails_row_4":      (0.0, 1.0, 4.5, INF),                   # stops at step 5, the last one
    "nan_last_step":    (0.0, 1.0, INF, 4.5),                   # stops at step 5
    "lap_last_row":     (0.0, 1.8, INF, INF),                   # s = 10.8 after step 5: every row kept, mask 0 afterwards
    "fails_last_row":   (0.0, 1.0, 5.5, INF),                   # the solve of step 5 fails: nothing stops in this call, mask still 1
}
NAMES = list(CARS)
B = len(NAMES)


def _x_start():
    x = np.zeros((B, 8))
    for b, (s0, v, fail, nan) in enumerate(CARS.values()):
        x[b] = [s0, 0.1 * b, 0.0, v, 0.0, 0.0, fail, nan]           # (the two thresholds ride along in the state: constants of the car)
    return x


def _solve(x):
    """A time-invariant 'controller': (u (B,2), status (B), gain (B,2,8)) as functions of the state alone."""
    s = x[:, 0]
    u = np.stack([1.0 + 0.25 * s + x[:, 1], np.cos(s)], 1)
    with np.errstate(invalid="ignore"):
        status = np.where(s > x[:, 6], 4, np.where(np.floor(s) % 2 == 1, 2, 0)).astype(np.int32)        # 0 and 2 are both accepted
    gain = (s + 1.0)[:, None, None] * np.arange(1.0, 17.0).reshape(2, 8)[None]
    gain[~np.isin(status, F.ACCEPTED)] = np.nan          # as ihm2mpc_get_x0_sensitivities: NaN rows for a solve that was not accepted
    return u, status, gain


def _plant(x, u):
    xn = x.copy()
    xn[:, 0] += x[:, 3]
    xn[:, 2] = 0.01 * u[:, 0]           # (the input leaves a trace in the state)
    xn[x[:, 0] > x[:, 7], 4] = np.nan
    return xn


def _unfrozen():
    """The loop without any stop rule: plant, then solve, T times after a priming solve."""
    x = _x_start()
    u, st0, k0 = _solve(x)
    u_first = u
    h = dict(u0=[], x0=[], status=[], qp_iter=[], sens_u0=[])
    for _ in range(T):
        x = _plant(x, u)
        u, st, k = _solve(x)
        h["u0"].append(u); h["x0"].append(x); h["status"].append(st); h["qp_iter"].append(np.full(B, 7, dtype=np.int32)); h["sens_u0"].append(k)
    return {k: np.array(v) for k, v in h.items()}, st0, u_first, k0


@pytest.fixture(scope="module")
def world():
    hist, st0, u_first, k0 = _unfrozen()
    ref = F.apply(hist, st0, _x_start(), None, LAP_STOP)
    return dict(hist=hist, st0=st0, u_first=u_first, k0=k0, ref=ref)


def _car(name):
    return NAMES.index(name)


def _assert_rows(world, name, stop, cause, active, x_stop=None, status_stop=None):
    """Rows before `stop` are the unfrozen ones; rows from `stop` on hold u0 = 0, x0 = x_stop, the last status, qp_iter = 0, NaN gains."""
    h, r, b = world["hist"], world["ref"], _car(name)
    assert (r["stop_step"][b], r["cause"][b], r["active"][b]) == (stop, cause, active), name
    for k in ("u0", "x0", "status", "qp_iter", "sens_u0"):
        np.testing.assert_array_equal(r[k][:stop, b], h[k][:stop, b], err_msg=f"{name}: {k}")
    if stop < T:
        assert np.all(r["u0"][stop:, b] == 0.0) and np.all(r["qp_iter"][stop:, b] == 0) and np.isnan(r["sens_u0"][stop:, b]).all()
        assert np.all(r["status"][stop:, b] == status_stop)
        np.testing.assert_array_equal(r["x0"][stop:, b], np.broadcast_to(x_stop, (T - stop, 8)))
    np.testing.assert_array_equal(r["x0_final"][b], r["x0"][-1, b])


def test_a_healthy_car_keeps_every_row(world):
    _assert_rows(world, "healthy", T, F.NONE, 1)
    _assert_rows(world, "slow", T, F.NONE, 1)
    assert np.isfinite(world["ref"]["sens_u0"][:, _car("healthy")]).all()


def test_a_failed_solve_stops_the_car_at_the_next_step(world):
    h, b = world["hist"], _car("fails_row_2")
    assert h["status"][:, b].tolist() == [2, 0, 4, 4, 4, 4]
    _assert_rows(world, "fails_row_2", 3, F.STATUS, 0, x_stop=h["x0"][2, b], status_stop=4)      # row 2 itself is kept: it was driven and solved
    assert world["ref"]["x0"][3, b, 0] == 3.0


def test_a_nan_plant_state_stops_the_car_where_it_was(world):
    h, b = world["hist"], _car("nan_step_3")
    assert np.isnan(h["x0"][3, b]).any() and not np.isnan(h["x0"][:3, b]).any()
    _assert_rows(world, "nan_step_3", 3, F.NAN, 0, x_stop=h["x0"][2, b], status_stop=h["status"][2, b])
    assert not np.isnan(world["ref"]["x0"][:, b]).any()


def test_a_finished_lap_keeps_its_row_and_stops_the_car_afterwards(world):
    h, b = world["hist"], _car("lap_row_3")
    assert h["x0"][2, b, 0] <= LAP_STOP < h["x0"][3, b, 0]
    _assert_rows(world, "lap_row_3", 4, F.LAP, 0, x_stop=h["x0"][3, b], status_stop=h["status"][3, b])


def test_a_car_that_failed_before_the_call_never_moves(world):
    b = _car("failed_before")
    assert world["st0"][b] == 4
    _assert_rows(world, "failed_before", 0, F.STATUS, 0, x_stop=_x_start()[b], status_stop=4)
    np.testing.assert_array_equal(world["ref"]["x0_final"][b], _x_start()[b])


def test_cars_that_stop_on_the_last_step(world):
    h = world["hist"]
    b = _car("fails_row_4")
    _assert_rows(world, "fails_row_4", T - 1, F.STATUS, 0, x_stop=h["x0"][T - 2, b], status_stop=4)
    b = _car("nan_last_step")
    _assert_rows(world, "nan_last_step", T - 1, F.NAN, 0, x_stop=h["x0"][T - 2, b], status_stop=h["status"][T - 2, b])
    # rules that act on the last row change no row of this call; the lap rule clears the mask, the status rule waits for the next call
    _assert_rows(world, "lap_last_row", T, F.LAP, 0)
    _assert_rows(world, "fails_last_row", T, F.NONE, 1)
    assert world["ref"]["status"][-1, _car("fails_last_row")] == 4


def test_a_masked_car_stops_at_step_zero(world):
    h = world["hist"]
    mask = np.ones(B, dtype=np.int32); mask[_car("healthy")] = 0
    r = F.apply(h, world["st0"], _x_start(), mask, LAP_STOP)
    b = _car("healthy")
    assert (r["stop_step"][b], r["cause"][b], r["active"][b]) == (0, F.MASK, 0)
    assert np.all(r["u0"][:, b] == 0) and np.all(r["qp_iter"][:, b] == 0) and np.all(r["status"][:, b] == world["st0"][b])
    np.testing.assert_array_equal(r["x0"][:, b], np.broadcast_to(_x_start()[b], (T, 8)))
    assert np.isnan(r["sens_u0"][:, b]).all()
    others = np.arange(B) != b
    for k in ("u0", "x0", "status", "qp_iter", "sens_u0"):         # the other cars: as without the mask
        np.testing.assert_array_equal(r[k][:, others], world["ref"][k][:, others])


def test_the_input_is_left_alone_and_sens_is_optional(world):
    h = {k: v.copy() for k, v in world["hist"].items()}
    F.apply(h, world["st0"], _x_start(), None, LAP_STOP)
    for k in h:
        np.testing.assert_array_equal(h[k], world["hist"][k])
    del h["sens_u0"]
    r = F.apply(h, world["st0"], _x_start(), None, LAP_STOP)
    assert "sens_u0" not in r
    np.testing.assert_array_equal(r["x0"], world["ref"]["x0"])


@pytest.mark.parametrize("first", [1, 2, 4, 5])
def test_two_calls_in_a_row_give_what_one_call_gives(world, first):
    """The mask, the last statuses and x0 are all a second call needs: apply over `first` steps, then over the rest from what the
    first left, equals apply over all T steps -- whatever rule acted on the last row of the first piece."""
    h, one = world["hist"], world["ref"]
    a = F.apply({k: v[:first] for k, v in h.items()}, world["st0"], _x_start(), None, LAP_STOP)
    b = F.apply({k: v[first:] for k, v in h.items()}, a["status"][-1], a["x0_final"], a["active"], LAP_STOP)
    for k in ("u0", "x0", "status", "qp_iter", "sens_u0"):
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), one[k], err_msg=k)
    np.testing.assert_array_equal(b["active"], one["active"])
    np.testing.assert_array_equal(b["x0_final"], one["x0_final"])
    np.testing.assert_array_equal(np.where(a["stop_step"] < first, a["stop_step"], first + b["stop_step"]), one["stop_step"])


class _Controller:
    """What run_closed_loop asks of a controller, answered by _solve."""
    dt = 0.05
    x0_sensitivities = True

    def __init__(self):
        self.B = B

    def compute_control(self, x):
        u, self.last_status, self.feedback_gain = _solve(np.asarray(x))
        return u


class _Simulator:
    def simulate(self, x, u):
        return _plant(np.asarray(x), np.asarray(u))


def test_rules_agree_with_the_bookkeeping_of_run_closed_loop(world):
    """run_closed_loop solves, then drives; the persistent loop drives, then solves, after a priming solve.  So its iteration i holds
    the solve behind row i - 1 of the frozen histories and the plant step of row i: states, statuses, zeroed inputs, NaN gains, and
    the alive / finished flags must be those the rules give."""
    from ihm2_amd.closed_loop_sim import run_closed_loop

    r = world["ref"]
    res = run_closed_loop(_Controller(), _Simulator(), _x_start(), T, lap_length=LAP_STOP - 1.0)
    assert res.u.shape[0] == T          # (some car is alive to the end: the loop did not break off)
    np.testing.assert_array_equal(res.x[0], _x_start())
    np.testing.assert_array_equal(res.x[1:], r["x0"])
    np.testing.assert_array_equal(res.status, np.concatenate([world["st0"][None], r["status"][:-1]]))
    step = np.arange(T)[:, None]
    stop, cause = r["stop_step"][None], r["cause"][None]
    # alive at the start of iteration i: no stopped row yet, or the rule that stops the car at i acts inside the iteration
    alive_at_start = (stop > step) | ((stop == step) & np.isin(cause, (F.STATUS, F.NAN)))
    np.testing.assert_array_equal(res.alive_history, alive_at_start)
    # its input counts: the car still drives the plant step of iteration i (a car whose plant then gives a NaN did drive)
    drives = (stop > step) | ((stop == step) & (cause == F.NAN))
    u_raw = np.concatenate([world["u_first"][None], r["u0"][:-1]])
    np.testing.assert_array_equal(res.u, np.where(drives[:, :, None], u_raw, 0.0))
    k_raw = np.concatenate([world["k0"][None], r["sens_u0"][:-1]])
    np.testing.assert_array_equal(res.feedback_gain, np.where(drives[:, :, None, None], k_raw, np.nan))
    np.testing.assert_array_equal(res.alive, r["active"] != 0)
    np.testing.assert_array_equal(res.finished, r["cause"] == F.LAP)
    np.testing.assert_array_equal(np.isfinite(res.lap_time), r["cause"] == F.LAP)
    # every cause occurs in this batch
    assert {F.NONE, F.STATUS, F.NAN, F.LAP} == set(r["cause"].tolist())


def test_header_says_which_calls_read_the_mask_of_a_frozen_loop():
    """include/ihm2mpc.h on ihm2mpc_run_steps: what a stopped car's rows hold, and that without ihm2mpc_set_active the mask a frozen loop
    leaves is read by later calls with freeze != 0 only (tests/test_gpu_freeze_rules.py asserts that behaviour on the device)."""
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ihm2mpc.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ihm2mpc_run_steps\(", hdr, flags=re.S)
    assert m, "ihm2mpc_run_steps is not declared right after its comment"
    doc = " ".join(m.group(1).replace(" * ", " ").split())
    for words in ("u0 = 0", "last status repeated", "0 QP iterations", "until ihm2mpc_set_active(NULL)", "calls with freeze != 0 ONLY",
                  "ihm2mpc_step, ihm2mpc_sim_advance and freeze == 0 read a mask only after ihm2mpc_set_active(mask)"):
        assert words in doc, f"the comment of ihm2mpc_run_steps does not say {words!r}"
