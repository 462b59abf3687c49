"""Edge states of the Cartesian side of the ROS stack and of the 15-state plant: three tables of named entries, shared by the CPU
certification of the oracle (``test_oracle_cart_edge_states.py``) and the GPU comparison of ``k_sim_cart``, ``k_project``,
``ihm2mpc_sim_advance_cart`` and ``k_sim_dyn10`` with it (``test_gpu_cart_edge_states.py``).  ``csrc/kernels_cart.hip`` carries its own
model code (library sincos / tan / atan2, a hand-chained 2 x 2 load-transfer solve, the speed switch and the "no reversing" clamp, the
windowed projection), which the table of ``edge_states.py`` never reaches; the parity tests of it (``test_gpu_cart.py``,
``test_gpu_dyn10.py``) stay at |psi| <= 0.1, v_x in [2, 15], a guess within 1 m of the truth.

Cartesian plant entries ``(x (8), u (2))`` -- ``plant_table()``; everything that is not named is ``BASE_X``, ``BASE_U``:

heading      phi on both sides of the quadrant boundaries of sincos, and 6.3, 40, 1e3, +-1.1e5
steering     delta = u_delta = +-0.78 ... +-1.5, and sweeps of delta across 0 (tan(delta), q, beta_dot)
speed        v_x = 0, +-1e-12 ... +-0.5, 1, -3, 40 (tanh(10 v_x), tanh(1000 v_x), atan2 in every quadrant)
standstill   the car exactly at rest, with and without throttle: atan2(0, 0) (python/models.py:376-379)
wheels       v_x - track / 2 r < 0 for the left wheels and, with negative r, for the right: a backward contact velocity
sideways     |v_y| >> |v_x| with both signs of either: slip angles beyond +-pi/2
switch       hypot(v_x, v_y) at v_dyn (1 -+ 1.01e-6) and exactly v_dyn (hypot(3, 0) = 3, hypot(4, 3) = 5), for v_dyn = 3 and 5
clamp        results on both sides of v_x+ < 0, v_x+ < 0.01, T+ <= 0.1 (T = u_T = 0.1 stays 0.1 bit for bit: the "<=")
crossing     a car that passes v_dyn, in either direction, inside a call of n_steps = 5, and one that brakes to the clamp inside it
combo        a value of several families at once

Projection entries ``(x_cart (8), s_guess)`` -- ``projection_table()`` on the knots of one track, each compared under every window
half-width of ``S_TOLS``: the guess off by 0, +-1.9, +3.5, -10 m and by one lap; the car at the first and at the last knot of the
table; a guess below the table by less than the window (for s_tol = 2) and by more (the window of ONE knot: 0 / 0, NaN on both sides),
above it by more; a NaN guess (fmax / fmin drop it: the window is the whole table); the car on an interior knot, on the centre line
between two knots, 1 m to either side; on both sides of the lap seams s = 0 and s = L; the nearest knot as the first and as the last
of its window (the wrap of id_prev / id_next, src/ihm2/src/common/tracks.cpp:183-288 as written); headings +-3.1415, +-3.15 and 1e3
where the centre line's own heading is nearest to +-pi.

fdyn10 entries ``(x (15), u (5))`` -- ``dyn10_table()``: entry (x, u) of the Frenet table of ``edge_states.py`` becomes
(s, n, psi, v_x, v_y, r, omega_w = v_x / R_w * WHEEL_SLIP[w], tau_w = T / 4, delta), (u_T / 4 four times, u_delta) -- wheel speeds 2 %,
3 % above, 1 % below and 1 % above rolling in the order FL, FR, RL, RR, so that no two wheels agree --, plus entries of its own: one
wheel locked, one spinning at twice rolling, torques of both signs.

Tolerances are the project's own: 1e-11 relative to 1 + |x| for one Cartesian plant step, 1e-10 for five, 1e-11 absolute for the
projection, 1e-9 relative to max(1, |x|) for fdyn10 -- unless the ORACLE's sensitivity to one ulp of the input exceeds a tenth of
that: then 16 x the measured sensitivity, for that plant and configuration alone (``RAISED``, ``RAISED_DYN10``).
``test_oracle_cart_edge_states.py`` measures it, on the oracle only, and fails for an entry whose sensitivity exceeds a tenth of what
it carries.  Decisions (switch, clamp, nearest knot, segment choice, fmod and the three wraps) keep a margin of 1e-6 relative in the
oracle at every entry, or sit on the threshold with an exact input: no comparison is left out.

Measured one-ulp sensitivities of the oracle (fsds_competition_1), worst entry of a family; Cartesian plants relative to 1 + |x+|:

family          kin6 RK4_10  kin6 RK4_1 kin6 STEPS_5  dyn6 RK4_10  dyn6 RK4_1 dyn6 STEPS_5
base             1.0e-17     1.0e-17     1.0e-17     4.1e-17     1.0e-17     6.9e-17
heading          3.7e-13     7.5e-14     1.9e-12     3.7e-13     7.5e-14     1.9e-12
steering         1.8e-15     3.4e-16     9.4e-15     1.0e-16     4.1e-17     2.8e-16
speed            7.3e-17     2.4e-17     9.4e-17     2.3e-14     2.4e-17     2.6e-14
standstill       1.0e-17     1.0e-17     1.0e-17     4.3e-13     1.0e-17     1.6e-07
wheels           1.0e-17     1.0e-17     6.7e-17     9.6e-17     1.0e-17     7.1e-14
sideways         2.6e-17     1.0e-17     2.5e-17     1.0e-17     1.0e-17     2.4e-17
switch           4.1e-17     1.0e-17     3.9e-17     2.2e-17     1.0e-17     4.3e-17
clamp            5.6e-14     4.2e-16     5.7e-14     4.3e-13     4.2e-16     4.4e-05
crossing         1.4e-17     1.0e-17     2.0e-17     1.3e-17     1.0e-17     9.1e-14
combo            1.1e-15     2.2e-16     5.4e-15     2.2e-16     1.0e-17     3.1e-08
(1.0e-17 stands for "no move beyond the rounding grid of the result".)  The switched plant (-3) at v_dyn = 3 and 5 moves by no more
than the model it chose: 3.7e-13 for one step, 1.9e-12 for five (phi = +-1.1e5), with v_x, v_y unperturbed where the entry sits on the
switch, T where T+ = 0.1 decides the clamp, and the velocities of the car at rest (atan2(0, 0) = 0, atan2(5e-324, 0) = pi / 2); under
the forced models these last are perturbed after the first RK4 sub-step instead, where every evaluation rounds them.

Projection (absolute, worst over the three window half-widths and the two tracks): 1.1e-13 (s near 340 m;
psi less the move of phi itself, which at phi = -1.1e5 is the grid of phi + pi, 1.5e-11, on both sides alike)

fdyn10 (relative to max(1, |x+|)), worst entry of a family:

family           RK4_1    RK4_100  RADAU_100
base            1.1e-16    2.2e-16    3.3e-16
heading         2.2e-13    5.6e-12    5.6e-12
steering        1.1e-16    1.2e-15    1.5e-15
speed           5.3e-15    3.4e-01    1.3e-15
arc             1.7e-16    1.4e-15    2.6e-15
offset          1.8e-15    1.5e-15    1.2e-15
switch          2.0e-16    3.5e-16    4.3e-16
combo           3.6e-15    9.4e-02    1.0e-14
wheels          4.2e-16    3.8e-16    1.4e-15

Above a tenth of the tolerance (-> RAISED, 16 x the measured value) and the "single-step only" entries of fdyn10 (RK4 x 100 over 0.05 s
moves them by more than 1e-6 per ulp: the wheel-slip dynamics near standstill are chaotic over a whole plant step, and a comparison
there would say nothing about the kernel; one RK4 step over 0.002 s, four nearly bare model evaluations, is well conditioned at every
entry, and so is the Radau IIA plant, RADAU_100):
  standstill_no_throttle                       dyn6 STEPS_5   1.6e-07   (in v_x, v_y, r after the first RK4 sub-step, where they have
                                                                         left the exact 0 of the input; 1.0e-08 in the other five inputs)
  clamp_coast_below_T_low, clamp_T_falls_below dyn6 STEPS_5   4.4e-05, 3.2e-06   (forced dyn6 at v_x ~ 0.01: RK4 with h = 1e-3 is unstable on
  clamp_coast_below_T_high, _above_T_low       dyn6 STEPS_5   2.9e-08, 5.5e-08    the lateral tyre dynamics, ~ C / (m v_x), and amplifies rounding
  clamp_T_exactly_0p1, combo_crawl_far_heading dyn6 STEPS_5   5.3e-11, 3.1e-08    noise over the 50 sub-steps; the node never runs dyn6 there)
  fdyn10 single-step only (RK4_100: 7.5e-02 ... 3.4e-01): vx_0, vx_1em12, vx_m1em12, vx_0p001, vx_m0p001, vx_0p05, vx_m0p05,
  vx_0_nearly_at_rest, combo_crawl_at_table_end -- 9 of 92.  Under Radau IIA x 100, the reference's own plant integrator, none of
  them moves by more than 6.1e-16: every entry is compared there.
"""
from __future__ import annotations

import dataclasses

import numpy as np

BASE_X = (3.0, -2.0, 0.3, 8.0, 0.1, 0.3, 100.0, 0.1)          # X, Y, phi, v_x, v_y, r, T, delta
BASE_U = (150.0, 0.15)
_IX = dict(X=0, Y=1, phi=2, vx=3, vy=4, r=5, T=6, delta=7)
_IU = dict(uT=0, ud=1)
HALF_TRACK, R_W = 0.62, 0.20809          # python/constants.py: axle_track / 2, wheel radius (the CPU test compares them with the project's)

V_DYNS = (3.0, 5.0)
# configurations of a Cartesian plant call: (M_sim, dt_sim, n_steps, v_dyn)
PLANT_CONFIGS = {"RK4_10": (10, 0.01, 1, 3.0), "RK4_1": (1, 0.002, 1, 3.0), "STEPS_5": (10, 0.01, 5, 3.0), "VDYN_5": (10, 0.01, 1, 5.0)}
PLANT_TOL = {"RK4_10": 1e-11, "RK4_1": 1e-11, "STEPS_5": 1e-10, "VDYN_5": 1e-11}
PROJ_TOL = 1e-11
DYN10_TOL = 1e-9
DYN10_CONFIGS = {"RK4_1": (1, 0.002), "RK4_100": (100, 0.05), "RADAU_100": (100, 0.05)}          # (M_sim, dt); RADAU: Radau IIA collocation, 4 stages
S_TOLS = (2.0, 1e-3, 50.0)
WHEEL_SLIP = (1.02, 1.03, 0.99, 1.01)

# where the reference's sensitivity exceeds a tenth of the tolerance: (model the step integrates with, configuration) -> 16 x measured
RAISED = {
    "standstill_no_throttle": {("dyn6", "STEPS_5"): 2.6e-06},          # v_x, v_y, r perturbed after the first RK4 sub-step
    "clamp_coast_below_T_low": {("dyn6", "STEPS_5"): 0.00073},
    "clamp_coast_below_T_high": {("dyn6", "STEPS_5"): 4.8e-07},
    "clamp_coast_above_T_low": {("dyn6", "STEPS_5"): 9.1e-07},
    "clamp_T_exactly_0p1": {("dyn6", "STEPS_5"): 8.7e-10},
    "clamp_T_falls_below": {("dyn6", "STEPS_5"): 5.3e-05},
    "combo_crawl_far_heading": {("dyn6", "STEPS_5"): 5.2e-07},
}
RAISED_DYN10 = {
}
# fdyn10 entries compared in the one-step configuration only (see above); fixed by name, at most 15 % of the table
SINGLE_STEP_ONLY = (
    "vx_0", "vx_1em12", "vx_m1em12", "vx_0p001", "vx_m0p001", "vx_0p05", "vx_m0p05", "vx_0_nearly_at_rest", "combo_crawl_at_table_end",
)

HEADINGS = (0.78, 0.79, 1.57, 1.58, 2.35, 2.36, 3.14, 3.15, 4.8, 6.3, 40.0, 1e3, 1.1e5)
STEERINGS = (0.78, 0.79, 1.2, 1.5)
SPEEDS = (0.0, 1e-12, -1e-12, 1e-3, -1e-3, 0.05, -0.05, 0.5, -0.5, 1.0, -3.0, 40.0)


def _num(v):
    return ("m" if v < 0 else "") + f"{abs(v):g}".replace("e-", "em").replace("+", "").replace(".", "p")


@dataclasses.dataclass(frozen=True)
class PlantEntry:
    name: str
    family: str
    x: np.ndarray
    u: np.ndarray
    raised: dict
    exact_switch: tuple = ()          # the v_dyn this entry sits on exactly, with an exactly representable hypot
    exact: tuple = ()                 # (plant or "*", component) pairs: inputs that sit on a threshold bit for bit, not to be perturbed

    def tolerance(self, model: str, config: str) -> float:
        """model "kin6" or "dyn6": the one that integrates the step (under the switch, the one the reference chose)."""
        return self.raised.get((model, config), PLANT_TOL[config])


def plant_table():
    out, seen = [], set()

    def add(family, name, exact_switch=(), exact=(), **ch):
        x, u = np.array(BASE_X), np.array(BASE_U)
        for key, v in ch.items():
            if key in _IX:
                x[_IX[key]] = v
            else:
                u[_IU[key]] = v
        assert name not in seen, name
        seen.add(name)
        out.append(PlantEntry(name, family, x, u, dict(RAISED.get(name, {})), tuple(exact_switch), tuple(exact)))

    add("base", "base")
    for h in HEADINGS:
        for sg in (1.0, -1.0):
            add("heading", "phi_" + _num(sg * h), phi=sg * h)
    for d in STEERINGS:
        for sg in (1.0, -1.0):
            add("steering", "delta_" + _num(sg * d), delta=sg * d, ud=sg * d)
    add("steering", "delta_0p1_to_m0p79", ud=-0.79)                      # sweeps across 0 inside the step
    add("steering", "delta_m0p2_to_0p3", delta=-0.2, ud=0.3)
    add("steering", "delta_1p2_to_m1p2", delta=1.2, ud=-1.2)
    add("steering", "delta_m1p5_to_0p78", delta=-1.5, ud=0.78)
    add("steering", "delta_0_stays", delta=0.0, ud=0.0)
    add("steering", "delta_0_to_1p5", delta=0.0, ud=1.5)
    for v in SPEEDS:
        add("speed", "vx_" + _num(v), vx=v, vy=0.01, r=0.02)
    rest = (("*", 3), ("*", 4), ("*", 5))          # atan2(0, 0): the smallest v_y turns a slip angle by pi / 2
    add("standstill", "standstill_no_throttle", exact=rest, vx=0.0, vy=0.0, r=0.0, T=0.0, uT=0.0)
    # (with T = delta = 0 as well f is 0 bit for bit on both sides, and the smallest T or delta sets a wheel off along atan2(5e-324, 0))
    add("standstill", "standstill_throttle", exact=rest, vx=0.0, vy=0.0, r=0.0, T=100.0, uT=150.0)
    add("standstill", "standstill_straight_wheels", exact=rest + (("*", 6), ("*", 7)), vx=0.0, vy=0.0, r=0.0, T=0.0, uT=0.0, delta=0.0, ud=0.0)
    add("wheels", "wheels_left_backward", vx=0.5, r=1.0)                 # 0.5 - 0.62 < 0
    add("wheels", "wheels_right_backward", vx=0.5, r=-1.0)
    add("wheels", "wheels_left_backward_fast", vx=4.0, vy=-0.5, r=7.0)
    for vx in (0.1, -0.1):
        for vy in (5.0, -5.0):
            add("sideways", f"sideways_vx_{_num(vx)}_vy_{_num(vy)}", vx=vx, vy=vy, r=0.05)
    for vd in V_DYNS:
        for side, f in (("kin", 1.0 - 1.01e-6), ("dyn", 1.0 + 1.01e-6)):
            vy = 0.1
            add("switch", f"switch_{_num(vd)}_{side}", vy=vy, vx=np.sqrt((vd * f) ** 2 - vy * vy))
    add("switch", "switch_3_exact", exact_switch=(3.0,), vx=3.0, vy=0.0)                     # hypot(3, 0) = 3: not < v_dyn, dynamic
    add("switch", "switch_5_exact", exact_switch=(5.0,), vx=4.0, vy=3.0)                     # hypot(4, 3) = 5
    add("switch", "switch_5_exact_sideways", exact_switch=(5.0,), vx=3.0, vy=-4.0)
    # clamp (under the switch these are kinematic steps: T+ = u_T + 5.5e-5 (T - u_T), drag ~ -0.13 m/s^2 at v_x = 0.01)
    add("clamp", "clamp_braking_crawl", vx=0.05, vy=0.0, r=0.0, T=-200.0, uT=-400.0)                     # v_x+ < 0
    add("clamp", "clamp_coast_below_T_low", vx=0.0105, vy=0.0, r=0.0, T=0.05, uT=0.05)                   # v_x+ < 0.01, T+ <= 0.1: stopped
    add("clamp", "clamp_coast_below_T_high", vx=0.0105, vy=0.0, r=0.0, T=0.15, uT=0.15)                  # v_x+ < 0.01, T+ > 0.1: rolls on
    add("clamp", "clamp_coast_above_T_low", vx=0.013, vy=0.0, r=0.0, T=0.05, uT=0.05)                    # v_x+ > 0.01: rolls on
    add("clamp", "clamp_coast_above_T_high", vx=0.013, vy=0.0, r=0.0, T=0.15, uT=0.15)
    add("clamp", "clamp_T_exactly_0p1", exact=(("ros", 6),), vx=0.0105, vy=0.0, r=0.0, T=0.1, uT=0.1)                         # T_dot = 0: T+ = 0.1 bit for bit
    add("clamp", "clamp_reverse_by_steering", vx=0.05, vy=1.0, r=0.0, T=50.0, uT=50.0, delta=0.0, ud=0.4)   # -beta_dot v_y: v_x+ < 0, T+ > 0.1
    add("clamp", "clamp_T_falls_below", vx=0.001, vy=0.0, r=0.0, T=300.0, uT=0.0)                        # T+ = 0.0165 from T = 300
    # crossings inside n_steps = 5
    add("crossing", "crossing_accelerates_through_3", vx=2.85, vy=0.0, r=0.0, T=400.0, uT=400.0)
    add("crossing", "crossing_accelerates_through_5", vx=4.85, vy=0.0, r=0.0, T=400.0, uT=400.0)
    add("crossing", "crossing_brakes_through_3", vx=3.1, vy=0.0, r=0.0, T=-300.0, uT=-300.0)
    add("crossing", "crossing_brakes_to_the_clamp", vx=0.2, vy=0.0, r=0.0, T=-300.0, uT=-300.0)
    add("combo", "combo_reverse_steered_quadrant_3", phi=-4.8, vx=-3.0, vy=0.5, r=-1.0, delta=1.2, ud=-1.2)
    add("combo", "combo_crawl_far_heading", phi=1.1e5, vx=1e-3, vy=0.01, r=0.02, delta=0.78, ud=0.79, T=0.0, uT=20.0)
    add("combo", "combo_sideways_at_switch", phi=3.15, exact_switch=(5.0,), vx=0.0, vy=5.0, r=-7.0, delta=-1.5, ud=-1.5)
    return out


def plant_arrays(entries):
    return np.stack([e.x for e in entries]), np.stack([e.u for e in entries])


# ---- projection ----
@dataclasses.dataclass(frozen=True)
class ProjEntry:
    name: str
    x: np.ndarray          # Cartesian state (8)
    s_guess: float
    on_knot: int = -1          # the knot the car sits on bit for bit, if any


def projection_table(s_ref, X_ref, Y_ref, phi_ref):
    """The entries on the knots of one track (1-D arrays of the same length, three laps side by side)."""
    s_ref, X_ref, Y_ref, phi_ref = (np.asarray(a, dtype=np.float64) for a in (s_ref, X_ref, Y_ref, phi_ref))
    nk = s_ref.size
    lap = nk // 3
    L = -s_ref[0]
    out, seen = [], set()

    def point(s, n=0.0):
        """Cartesian point at arc length s (inside the table) and lateral offset n (left positive) of the knot polyline."""
        i = int(np.clip(np.searchsorted(s_ref, s, side="right") - 1, 0, nk - 2))
        lam = (s - s_ref[i]) / (s_ref[i + 1] - s_ref[i])
        tx, ty = X_ref[i + 1] - X_ref[i], Y_ref[i + 1] - Y_ref[i]
        nrm = np.hypot(tx, ty)
        return X_ref[i] + lam * tx - n * ty / nrm, Y_ref[i] + lam * ty + n * tx / nrm

    def add(name, s, n=0.0, guess_off=0.0, phi=0.2, XY=None, guess=None, on_knot=-1, vx=6.0):
        X, Y = point(s, n) if XY is None else XY
        x = np.array([X, Y, phi, vx, 0.2, -0.1, 50.0, 0.05])
        assert name not in seen, name
        seen.add(name)
        out.append(ProjEntry(name, x, float(s + guess_off if guess is None else guess), on_knot))

    k = lap + lap // 3 + 7          # an interior knot of the middle lap
    d = s_ref[k + 1] - s_ref[k]
    sm = s_ref[k] + 0.3 * d         # between two knots, nearer to the first
    for tag, off in (("0", 0.0), ("1p9", 1.9), ("m1p9", -1.9), ("3p5", 3.5), ("m10", -10.0), ("one_lap", L), ("minus_one_lap", -L)):
        add("guess_off_" + tag, sm, n=0.4, guess_off=off)
        add("guess_off_" + tag + "_right", s_ref[k + 9] + 0.6 * d, n=-0.4, guess_off=off)
    for lam in (0.01, 0.49, 0.51, 0.99):                                   # along one interval: the nearest knot changes at 0.5
        add("along_interval_" + _num(lam), s_ref[k + 20] + lam * (s_ref[k + 21] - s_ref[k + 20]), n=0.3, guess_off=-0.7)
    dphi = np.abs(np.diff(phi_ref[lap:2 * lap]))
    kt = lap + int(np.argmax(np.where(dphi < 1.0, dphi, 0.0)))              # the tightest bend of the middle lap (not a jump of atan2)
    for lam in (0.1, 0.45, 0.9):
        for n in (1.5, -1.5):                                              # inside and outside of it: the segment choice by the angles
            add(f"tight_bend_{_num(lam)}_n_{_num(n)}", s_ref[kt] + lam * (s_ref[kt + 1] - s_ref[kt]), n=n, guess_off=0.9)
    add("first_lap", s_ref[lap // 2] + 0.2, n=0.5, guess_off=-1.0)
    add("first_lap_guess_in_second", s_ref[lap // 2] + 0.2, n=-0.5, guess_off=L)
    add("last_lap", s_ref[2 * lap + lap // 2] + 0.2, n=0.5, guess_off=1.0)
    add("last_lap_guess_in_second", s_ref[2 * lap + lap // 2] + 0.2, n=-0.5, guess_off=-L)
    for ph in (1.57, -1.58, 40.0):
        add("phi_" + _num(ph), s_ref[k + 30] + 0.2 * d, n=-0.2, phi=ph)
    add("first_knot_left", s_ref[0] + 0.05, n=0.08)
    add("first_knot_right_behind", s_ref[0] + 0.02, n=-0.05, guess_off=-0.5)
    add("last_knot_left", s_ref[-1] - 0.05, n=0.08)
    add("last_knot_right_guess_beyond", s_ref[-1] - 0.02, n=-0.05, guess_off=0.7)
    add("guess_below_table_by_1", s_ref[0] + 0.2, n=0.3, guess=s_ref[0] - 1.0)
    add("guess_below_table_by_60", s_ref[0] + 0.2, n=-0.3, guess=s_ref[0] - 60.0)          # one knot for every s_tol of S_TOLS
    add("guess_below_table_by_3", s_ref[0] + 0.2, n=0.2, guess=s_ref[0] - 3.0)
    add("guess_above_table_by_60", s_ref[-1] - 0.2, n=0.3, guess=s_ref[-1] + 60.0)
    add("guess_above_table_by_3", s_ref[-1] - 0.2, n=-0.3, guess=s_ref[-1] + 3.0)
    add("guess_nan", sm, n=-0.4, guess=np.nan)
    add("guess_nan_on_last_lap", s_ref[2 * lap + 40] + 0.1, n=0.2, guess=np.nan)
    add("on_knot", s_ref[k], XY=(X_ref[k], Y_ref[k]), on_knot=k)
    add("on_knot_guess_off", s_ref[k + 5], XY=(X_ref[k + 5], Y_ref[k + 5]), guess_off=1.9, on_knot=k + 5)
    add("on_centre_line", sm)
    add("on_centre_line_late", s_ref[k + 2] + 0.8 * d)
    add("left_1m", sm, n=1.0)
    add("right_1m", sm, n=-1.0)
    for name, s0 in (("seam_0", s_ref[lap]), ("seam_L", s_ref[2 * lap])):
        add(name + "_before", s0 - 0.15, n=0.3)
        add(name + "_after", s0 + 0.15, n=-0.3)
        add(name + "_before_guess_after", s0 - 0.15, n=-0.2, guess_off=0.5)
    # the nearest knot as the first / the last of its window: the guess 2 1/3 intervals + s_tol away from the car, for s_tol = 2
    # (other half-widths see these as plain wrong guesses)
    add("nearest_is_first_of_window", sm, n=0.2, guess=s_ref[k] + 2.0 + 1.4 * d)
    add("nearest_is_last_of_window", sm, n=-0.2, guess=s_ref[k] - 2.0 - 1.4 * d)
    add("nearest_is_first_of_narrow_window", sm, n=0.2, guess=s_ref[k + 1] + 0.4 * d)            # s_tol = 1e-3: window k .. k + 2
    add("nearest_is_last_of_narrow_window", s_ref[k] + 0.7 * d, n=0.2, guess=s_ref[k] - 0.6 * d)   # window k - 2 .. k + 1... nearest k + 1
    # headings against a centre-line heading near +-pi
    w = lap + int(np.argmax(np.abs(phi_ref[lap:2 * lap - 1])))
    for ph in (3.1415, -3.1415, 3.15, -3.15, 1e3, 0.0):
        add("phi_" + _num(ph) + "_where_track_heads_pi", s_ref[w] + 0.3 * (s_ref[w + 1] - s_ref[w]), n=0.3, phi=ph)
    add("phi_m1e5", sm, n=0.1, phi=-1.1e5)
    add("fast_car_guess_wraps", s_ref[2 * lap] - 0.4, n=0.1, vx=40.0)                        # s + 0.05 v_x > L: the fmod
    add("reversing_car_near_0", s_ref[lap] + 0.3, n=0.1, vx=-20.0)                           # s + 0.05 v_x < 0
    return out


def projection_arrays(entries):
    return np.stack([e.x for e in entries]), np.array([e.s_guess for e in entries])


# ---- fdyn10 ----
@dataclasses.dataclass(frozen=True)
class Dyn10Entry:
    name: str
    family: str
    x: np.ndarray
    u: np.ndarray
    raised: dict
    single_step_only: bool

    def tolerance(self, config: str) -> float:
        assert config in DYN10_CONFIGS and not (self.single_step_only and config == "RK4_100"), (self.name, config)
        return self.raised.get(config, DYN10_TOL)


def dyn10_table(frenet_entries):
    """``frenet_entries``: the list ``edge_states.table(s_ref, kappa_ref)`` (anything with name, family, x (8), u (2))."""
    out = []

    def add(name, family, x8, u2, omega=None, tau=None, u_tau=None):
        x = np.zeros(15); u = np.zeros(5)
        x[:6] = x8[:6]
        x[6:10] = x8[3] / R_W * np.array(WHEEL_SLIP) if omega is None else omega
        x[10:14] = 0.25 * x8[6] if tau is None else tau
        x[14] = x8[7]
        u[:4] = 0.25 * u2[0] if u_tau is None else u_tau
        u[4] = u2[1]
        out.append(Dyn10Entry(name, family, x, u, dict(RAISED_DYN10.get(name, {})), name in SINGLE_STEP_ONLY))

    base = None
    for e in frenet_entries:
        add(e.name, e.family, e.x, e.u)
        if e.name == "base":
            base = e
    roll = base.x[3] / R_W
    add("wheel_FL_locked", "wheels", base.x, base.u, omega=roll * np.array([0.0, 1.03, 0.99, 1.01]))
    add("wheel_RR_spinning", "wheels", base.x, base.u, omega=roll * np.array([1.02, 1.03, 0.99, 2.0]))
    add("wheel_FR_backward", "wheels", base.x, base.u, omega=roll * np.array([1.02, -0.5, 0.99, 1.01]))
    add("torques_alternate", "wheels", base.x, base.u, tau=np.array([40.0, -40.0, -40.0, 40.0]), u_tau=np.array([-60.0, 60.0, 60.0, -60.0]))
    add("torques_all_brake", "wheels", base.x, base.u, tau=np.full(4, -50.0), u_tau=np.full(4, -80.0))
    assert len({e.name for e in out}) == len(out)
    return out


def dyn10_arrays(entries):
    return np.stack([e.x for e in entries]), np.stack([e.u for e in entries])


# ---- isolation: the non-finite slots of the GPU tests (named explicitly: they are compared with nothing) ----
def non_finite_cart_states():
    """name -> (x_cart (8), s_guess offset or NaN): NaN in X, NaN in phi, a NaN guess, inf in v_x."""
    out = {}
    for name, idx, v, g in (("nan_in_X", 0, np.nan, 0.0), ("nan_in_phi", 2, np.nan, 0.0), ("nan_guess", None, None, np.nan), ("inf_in_vx", 3, np.inf, 0.0)):
        x = np.array(BASE_X)
        if idx is not None:
            x[idx] = v
        out[name] = (x, g)
    return out
