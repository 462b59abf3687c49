"""The stop rules of the persistent control-step loop -- ihm2mpc_run_steps / ihm2mpc_run_steps_sens with freeze != 0 -- in every k_steps
instantiation, by name, against the rules in numpy (tests/freeze_ref.py) applied to launches per step.

include/ihm2mpc.h promises per car: a solve status other than 0 / 2 stops it where it is, a NaN plant state stops it where it was,
s > lap_stop ends its run; the mask is kept for later frozen calls until ihm2mpc_set_active(NULL); with sensitivities a stopped car's
gains are NaN.  k_steps implements that in a lambda, an early return out of the step loop and two tests inside the step, and is compiled
into one register allocation per instantiation (tests/test_gpu_steps_catalogue.py, which launches them all with freeze = 0): here each one
runs a batch in which every rule acts.

The cars of a batch do not see one another, so the reference is the loop WITHOUT freeze, as ihm2mpc_step calls from the same planted
start (that those equal run_steps(freeze = 0) bit for bit is the catalogue module's assertion), passed through freeze_ref.apply.  Every
comparison is bit for bit, NaN positions included.  NaN values here are input data of solves that must end with status 1.

The handles take the single-wave QP kernel (IHM2MPC_BLOCK_QP=0), as in the catalogue module."""
import dataclasses

import numpy as np
import pytest

import drive
import freeze_ref as F
import steps_cases as S
from test_gpu_steps_catalogue import _sens, _solver, _start

pytestmark = pytest.mark.gpu

B = 8               # x N >= 40: 320 intervals and more, no latency batch (launch_cases.latency_batch: k_linearize_cols and the state-only plant)
STEPS = 6
FAILED_CAR, NAN_CAR = 0, 1          # the cars the causes (a) and (b) are planted in; the lap rule acts among the cars 2 .. B - 1
MASKED = (3, 6)                     # the cars a user's mask stops in test_user_mask_without_freeze


@pytest.fixture(autouse=True)
def _single_wave_qp(monkeypatch):
    monkeypatch.setenv("IHM2MPC_BLOCK_QP", "0")          # read when a handle is created


# Starts (conftest.sample_x0 seeds) other than the case table's.  The dynamic OCP model loses cars by itself (status 4), and from the
# table's start of this case, drawn for 8 cars, the only two cars whose six solves all succeed are the two furthest along the track:
# any lap_stop that another car crosses stops both at step 0, so no lap_stop leaves two cars that never stop.
SEEDS = {"k_steps<8,2,0,1,0,0,1>": 1706}           # the table's seed + 1000


def _case(name, build):
    case = S.ILP_CASES.get(name, S.BY_NAME[name]) if build == "ilp" else S.BY_NAME[name]
    return dataclasses.replace(case, B=B, seed=SEEDS.get(name) or case.seed)


def _handle(track, case, build, plant):
    """A handle after the priming step(); plant = (poison, cars): with the stop causes planted through the setters,
    (a) one NaN in the iterate of every car of `cars` (car 0, see _reference) at an interior stage -- its next solve ends with status 1
        (poison "u": in its inputs instead),
    (b) a NaN steering angle in car 1's plant state -- its next plant step gives a NaN state."""
    s = _solver(track, case, build)
    s.set_lap_wrap(True)
    if case.sens:
        s.set_x0_sensitivities(case.sens)
    _start(s, track, case)
    s.step(_tgt(case), model=case.plant, M_sim=case.M_sim)
    if plant is not None:
        poison, cars = plant
        k = s.N // 2
        if poison == "x":
            x = s.get_x(); x[list(cars), k, 1] = np.nan; s.set_x(x)
        else:
            u = s.get_u(); u[list(cars), k, 1] = np.nan; s.set_u(u)
        x0 = s.get_x0(); x0[NAN_CAR, 7] = np.nan; s.set_x0(x0)
    return s


def _tgt(case):
    return S.s_target(S.LAYOUTS[case.layout])


def _state(s, case):
    pi, lam = s.get_multipliers()
    f = dict(x=s.get_x(), u=s.get_u(), pi=pi, lam=lam, slk=s.get_slacks())
    if case.sqp:
        f.update(s.get_sqp_stats())
    if case.sens:
        f.update(_sens(s, case))
    return f


def _per_step(s, case, n):
    """n step() calls: the histories, and the handle's state after every one of them."""
    states = []
    h = drive.per_step(s, _tgt(case), n, model=case.plant, M_sim=case.M_sim, sens=bool(case.sens), after=lambda s: states.append(_state(s, case)))
    return h, states


def _run(s, case, n, freeze, lap_stop=np.inf):
    return s.run_steps(_tgt(case), n, model=case.plant, M_sim=case.M_sim, freeze=freeze, lap_stop=lap_stop, u0_hist=True, x0_hist=True,
                       status_hist=True, qp_iter_hist=True, sens_u0_hist=True if case.sens else None)


def _cut(h, a, b):
    return {k: v[a:b] for k, v in h.items()}


def _choose_lap_stop(h, status0, x00, failed):
    """A lap_stop strictly between two s values of the reference's x0 history, such that one of the cars 2 .. B - 1 crosses it at a
    step 1 .. 4 (step 1 where possible: the last step of the first piece of test_in_pieces), the planted causes stop the cars 0 and 1
    before the lap rule does, and two cars never stop -- where possible two whose last solve is accepted as well (_survivors).
    (lap_stop, the rules' output) -- or None."""
    sh = h["x0"][:, :, 0]
    for count in (_survivors, _never_stopped):
        for t in (1, 2, 3, 4):
            for c in range(2, B):
                if not sh[t - 1, c] < sh[t, c]:
                    continue
                stop = 0.5 * (sh[t - 1, c] + sh[t, c])
                r = F.apply(h, status0, x00, None, stop)
                if (r["cause"][c] == F.LAP and r["stop_step"][c] == t + 1 and np.all(r["cause"][list(failed)] == F.STATUS) and r["cause"][NAN_CAR] == F.NAN
                        and len(count(r)) >= 2 and not np.any(sh == stop)):
                    return stop, r
    return None


def _never_stopped(rule):
    """The cars without a stopped row in the call whose mask entry is still 1."""
    return np.flatnonzero((rule["cause"] == F.NONE) & (rule["stop_step"] == STEPS))


def _survivors(rule):
    """The cars that drive every step of the call and would drive the next one."""
    return np.flatnonzero((rule["cause"] == F.NONE) & (rule["stop_step"] == STEPS) & np.isin(rule["status"][-1], F.ACCEPTED))


REFERENCES = {}         # name -> the reference run of a CLASSES case (default build), computed once and left unchanged


def _reference(track, name, build):
    """The planted start driven by STEPS + 1 step() calls (the last one for test_reset), and the rules applied to the first STEPS.
    Asserted here, on the reference: every cause occurs and two cars run to the end."""
    if build == "default" and name in REFERENCES:
        return REFERENCES[name]
    case = _case(name, build)
    # (a) goes into car 0; where car 0's priming solve failed by itself from this start (it then stops at step 0), into the last car as
    # well, so that a solve fails INSIDE the loop in every case: that car keeps the row of step 0 and stops at step 1
    for plant in (("x", (FAILED_CAR,)), ("x", (FAILED_CAR, B - 1)), ("u", (FAILED_CAR,)), ("u", (FAILED_CAR, B - 1))):
        s = _handle(track, case, build, plant)
        status0, x00, state0 = s.get_status(), s.get_x0(), _state(s, case)
        h7, states = _per_step(s, case, STEPS + 1)
        s.free()
        fails_inside = [c for c in plant[1] if status0[c] in F.ACCEPTED and h7["status"][0, c] not in F.ACCEPTED]
        if fails_inside:
            break
    poison, failed = plant
    h = _cut(h7, 0, STEPS)
    assert fails_inside, ("no poison makes a planted solve fail", status0, h["status"])
    assert np.isnan(h["x0"][0, NAN_CAR]).any()
    chosen = _choose_lap_stop(h, status0, x00, failed)
    assert chosen is not None, ("no lap_stop gives every cause and two survivors", status0, h["x0"][:, :, 0], h["status"])
    lap_stop, rule = chosen
    lap_cars = np.flatnonzero((rule["cause"] == F.LAP) & (rule["stop_step"] < STEPS))
    survivors, never = _survivors(rule), _never_stopped(rule)
    assert rule["stop_step"][NAN_CAR] == 0 and np.all(rule["stop_step"][fails_inside] == 1) and len(lap_cars) >= 1
    assert len(never) >= 2 and len(survivors) >= 1
    print(f"{name} [{build}]: poison {poison} in cars {list(failed)}, status before {status0.tolist()}, lap_stop {lap_stop:.3f}, cause {rule['cause'].tolist()}, stop_step {rule['stop_step'].tolist()}, "
          f"status {h['status'].tolist()}")
    ref = dict(case=case, plant=plant, status0=status0, x00=x00, hist=h, hist7=h7, states=[state0] + states, lap_stop=lap_stop, rule=rule,
               lap_cars=lap_cars, survivors=survivors, never_stopped=never)
    if build == "default" and name in CLASSES.values():         # the cases the contract tests below share
        REFERENCES[name] = ref
    return ref


def _assert_hist(got, want, msg=""):
    assert set(got) == {k for k in want if k in drive.HIST + ("sens_u0",)}
    for k in got:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{msg}{k}")


LOOPS = [(c.name, "default") for c in S.CASES] + [(c.name, "ilp") for c in S.CASES if c.qp_set in S.ILP_SETS]


@pytest.mark.parametrize("name,build", LOOPS)
def test_frozen_loop_follows_the_rules(track, name, build):
    """One frozen call over STEPS steps on a batch with a failing solve (car 0), a NaN plant state (car 1), a lap_stop that one of the
    other cars crosses on the way, and at least two cars that run to the end: the instantiation of the name ran; every history is the
    rules' output, stopped cars' rows included (u0 = 0, x0 and status repeated, qp_iter = 0, NaN gains); x0 is the rules'; the cars
    that never stopped end with the iterate, multipliers, slacks, SQP statistics and sensitivities of the last step() call, and the
    cars stopped by a failed solve or a finished lap with the iterate and multipliers of their last solved step."""
    ref = _reference(track, name, build)
    case, rule = ref["case"], ref["rule"]
    s = _handle(track, case, build, ref["plant"])
    got = _run(s, case, STEPS, True, ref["lap_stop"])
    rec = s.get_launch_record()
    assert rec["steps"] == name, rec
    assert (rec["steps_form"], rec["steps_slots"]) == case.form, rec
    _assert_hist(got, rule)
    np.testing.assert_array_equal(s.get_x0(), rule["x0_final"])
    fin = _state(s, case)
    s.free()
    ran = ~F.stopped_in_call(rule)
    for k, v in ref["states"][STEPS].items():
        np.testing.assert_array_equal(fin[k][ran], v[ran], err_msg=f"cars that never stopped: {k}")
    # (the iterate of the car with the NaN plant state is not asserted: when the rule finds the NaN, the step has already shifted it)
    for b in np.flatnonzero(~ran & np.isin(rule["cause"], (F.STATUS, F.LAP))):
        last = ref["states"][rule["stop_step"][b]]          # [t]: the state after step t - 1, [0] before the call
        for k in ("x", "u", "pi", "lam"):
            np.testing.assert_array_equal(fin[k][b], last[k][b], err_msg=f"car {b} stopped at step {rule['stop_step'][b]}: {k}")
    if case.sens:
        np.testing.assert_array_equal(np.isnan(got["sens_u0"]), np.isnan(rule["sens_u0"]))
        assert np.isnan(got["sens_u0"][rule["stop_step"][NAN_CAR]:, NAN_CAR]).all()
        for k in ("sens_x", "sens_u"):          # (mode 2: the whole horizon, mode 1: the gain)
            if k in fin:
                assert np.isnan(fin[k][~ran]).all(), k


# ---- the contracts around the rules, one case per class of loop ----
CLASSES = {
    "hard_rti": "k_steps<5,0,0,1,0,0,0>", "sqp": "k_steps<5,0,0,1,1,0,0>", "collocation": "k_steps<8,0,0,1,0,1,0>",
    "dynamic": "k_steps<5,0,0,1,0,0,1>", "soft": "k_steps<8,2,0,1,0,0,0>", "sens": "k_steps<5,0,0,1,0,0,0,1>", "erk_lag": "k_steps<5,0,0,1,0,2,0>",
}
assert S.BY_NAME[CLASSES["sens"]].sens == 2          # the whole horizon's read-back
classes = pytest.mark.parametrize("cls", list(CLASSES))


@classes
def test_in_pieces(track, cls):
    """A frozen call over 2 steps and one over 4 give what one call over 6 gives: the second call finds the mask and the statuses the
    first left.  A car that crosses lap_stop on the last step of the first piece does not move in the second."""
    ref = _reference(track, CLASSES[cls], "default")
    case, rule = ref["case"], ref["rule"]
    first = F.apply(_cut(ref["hist"], 0, 2), ref["status0"], ref["x00"], None, ref["lap_stop"])
    crossed = np.flatnonzero((first["cause"] == F.LAP) & (first["stop_step"] == 2))
    assert len(crossed) >= 1, "no car of the reference crosses lap_stop on step 1"
    s = _handle(track, case, "default", ref["plant"])
    a = _run(s, case, 2, True, ref["lap_stop"])
    x0_between = s.get_x0()
    b = _run(s, case, STEPS - 2, True, ref["lap_stop"])
    assert s.get_launch_record()["steps"] == case.name
    _assert_hist(a, first, "first piece: ")
    _assert_hist({k: np.concatenate([a[k], b[k]]) for k in a}, rule)
    np.testing.assert_array_equal(s.get_x0(), rule["x0_final"])
    fin = _state(s, case)
    s.free()
    assert np.all(b["x0"][:, crossed] == x0_between[crossed]) and np.all(b["qp_iter"][:, crossed] == 0) and np.all(b["u0"][:, crossed] == 0.0)
    ran = ~F.stopped_in_call(rule)
    for k, v in ref["states"][STEPS].items():
        np.testing.assert_array_equal(fin[k][ran], v[ran], err_msg=k)


@classes
def test_reset(track, cls):
    """ihm2mpc_set_active(NULL) forgets the mask a frozen loop left, not the reasons that hold by themselves: in one more frozen step
    without a lap_stop the cars a finished lap had stopped drive and solve again, the car whose solve failed still stands (its status is
    what it was), and so does the car whose plant state has a NaN.  The cars that never stopped take the step as if nothing had happened."""
    ref = _reference(track, CLASSES[cls], "default")
    case, rule = ref["case"], ref["rule"]
    s = _handle(track, case, "default", ref["plant"])
    _run(s, case, STEPS, True, ref["lap_stop"])
    x0 = s.get_x0()
    s.set_active(None)
    got = _run(s, case, 1, True)
    s.free()
    lap = ref["lap_cars"]
    assert np.all(got["qp_iter"][0, lap] > 0) and np.all(np.any(got["x0"][0, lap] != x0[lap], axis=1)), (got["qp_iter"], lap)
    for b in (FAILED_CAR, NAN_CAR):
        np.testing.assert_array_equal(got["x0"][0, b], x0[b])
        assert got["qp_iter"][0, b] == 0 and np.all(got["u0"][0, b] == 0.0) and got["status"][0, b] == rule["status"][-1, b]
        if case.sens:
            assert np.isnan(got["sens_u0"][0, b]).all()
    ran = ref["survivors"]
    for k in got:
        np.testing.assert_array_equal(got[k][0, ran], ref["hist7"][k][STEPS, ran], err_msg=k)


def _masked_start(track, case):
    s = _handle(track, case, "default", None)
    mask = np.ones(B, dtype=np.int32); mask[list(MASKED)] = 0
    s.set_active(mask)
    return s


@classes
def test_user_mask_without_freeze(track, cls):
    """freeze == 0 under ihm2mpc_set_active(mask): what step() calls give under the same mask, bit for bit -- the masked cars stand
    still (constant x0) and keep solving (qp_iter > 0)."""
    case = _case(CLASSES[cls], "default")
    s = _masked_start(track, case)
    x00 = s.get_x0()
    want, states = _per_step(s, case, STEPS)
    s.free()
    s = _masked_start(track, case)
    got = _run(s, case, STEPS, False)
    assert s.get_launch_record()["steps"] == case.name
    fin = _state(s, case)
    s.free()
    _assert_hist(got, want)
    for k, v in states[-1].items():
        np.testing.assert_array_equal(fin[k], v, err_msg=k)
    m = list(MASKED)
    assert np.all(got["x0"][:, m] == x00[m]) and np.all(got["qp_iter"][:, m] > 0)
    others = [b for b in range(B) if b not in MASKED]
    assert np.all(np.any(got["x0"][:, others] != x00[others], axis=2))


@classes
def test_user_mask_with_freeze(track, cls):
    """freeze != 0 under ihm2mpc_set_active(mask): the masked cars stop at step 0, the others follow the rules -- and the loop clears
    entries of the USER's mask, which ihm2mpc_step reads afterwards: a car stopped by a finished lap stands still in a following step()."""
    ref = _reference(track, CLASSES[cls], "default")
    case = ref["case"]
    # masked: two of the cars 2 .. B - 1, first those that would run to the end; a car the lap rule stops and a survivor stay unmasked
    keep = {int(ref["lap_cars"][0]), int(ref["survivors"][0])}
    free = [b for b in range(2, B) if b not in keep]
    masked = sorted(free, key=lambda b: b not in ref["never_stopped"])[:2]
    mask = np.ones(B, dtype=np.int32); mask[masked] = 0
    rule = F.apply(ref["hist"], ref["status0"], ref["x00"], mask, ref["lap_stop"])
    assert np.all(rule["stop_step"][masked] == 0) and np.all(rule["cause"][masked] == F.MASK)
    lap = np.flatnonzero((rule["cause"] == F.LAP) & (rule["stop_step"] < STEPS))
    drove = _survivors(rule)
    assert len(lap) >= 1 and len(drove) >= 1
    s = _handle(track, case, "default", ref["plant"])
    s.set_active(mask)
    got = _run(s, case, STEPS, True, ref["lap_stop"])
    _assert_hist(got, rule)
    x0 = s.get_x0()
    np.testing.assert_array_equal(x0, rule["x0_final"])
    s.step(_tgt(case), model=case.plant, M_sim=case.M_sim)
    x1 = s.get_x0()
    s.free()
    stands = masked + lap.tolist()
    np.testing.assert_array_equal(x1[stands], x0[stands])
    assert np.all(np.any(x1[drove] != x0[drove], axis=1))


def test_stopped_cars_leave_their_neighbours_alone(track):
    """The rows of the cars 2 .. B - 1, and what the handle holds for them afterwards, are the same bits whether or not the cars 0 and 1
    carry NaN data and stop."""
    ref = _reference(track, CLASSES["hard_rti"], "default")
    case = ref["case"]
    s = _handle(track, case, "default", None)
    clean = _run(s, case, STEPS, True, ref["lap_stop"])
    fin = _state(s, case)
    s.free()
    s = _handle(track, case, "default", ref["plant"])
    planted = _run(s, case, STEPS, True, ref["lap_stop"])
    fin_p = _state(s, case)
    s.free()
    assert not np.array_equal(planted["u0"][:, FAILED_CAR], clean["u0"][:, FAILED_CAR])          # (the two runs do differ in car 0)
    rest = [b for b in range(2, B) if b not in ref["plant"][1]]
    assert len(rest) >= 5
    for k in clean:
        np.testing.assert_array_equal(planted[k][:, rest], clean[k][:, rest], err_msg=k)
        np.testing.assert_array_equal(planted[k][:, rest], ref["rule"][k][:, rest], err_msg=k)
    for k in fin:
        np.testing.assert_array_equal(fin_p[k][rest], fin[k][rest], err_msg=k)


@classes
def test_only_frozen_calls_read_the_mask_a_frozen_loop_left(track, cls):
    """include/ihm2mpc.h: without ihm2mpc_set_active, the mask a frozen loop leaves is read by later calls with freeze != 0 only.
    After a frozen call that stopped a car at lap_stop, ihm2mpc_step moves that car again, ihm2mpc_run_steps(freeze = 0) moves it
    again, and a frozen call after those still finds its mask entry cleared: the car stands."""
    ref = _reference(track, CLASSES[cls], "default")
    case = ref["case"]
    lap = ref["lap_cars"]
    s = _handle(track, case, "default", ref["plant"])
    _run(s, case, STEPS, True, ref["lap_stop"])
    x0 = s.get_x0()
    s.step(_tgt(case), model=case.plant, M_sim=case.M_sim)
    x1, it1 = s.get_x0(), s.get_qp_iter()
    assert np.all(np.any(x1[lap] != x0[lap], axis=1)) and np.all(it1[lap] > 0)
    free = _run(s, case, 1, False)
    assert s.get_launch_record()["steps"] == case.name
    assert np.all(np.any(free["x0"][0, lap] != x1[lap], axis=1)) and np.all(free["qp_iter"][0, lap] > 0)
    x2 = s.get_x0()
    h = _run(s, case, 1, True, ref["lap_stop"])
    s.free()
    # the rules for this step: a car stands if the six-step call cleared its mask entry, or if its last solve (the step before) failed
    stands = (ref["rule"]["active"] == 0) | ~np.isin(free["status"][0], F.ACCEPTED)
    assert stands[lap].all()
    np.testing.assert_array_equal(h["x0"][0, stands], x2[stands])
    assert np.all(h["qp_iter"][0, stands] == 0) and np.all(h["u0"][0, stands] == 0.0)
    assert np.all(h["qp_iter"][0, ~stands] > 0) and np.all(np.any(h["x0"][0, ~stands] != x2[~stands], axis=1))
