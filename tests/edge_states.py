"""Edge states of the vehicle models: one table of named ``(x, u)`` pairs, shared by the CPU certification of the oracle
(``test_oracle_edge_states.py``) and the GPU comparison of every model-evaluating kernel with it (``test_gpu_edge_states.py``).

The parity tests evaluate the models at Stanley warm starts of ``sample_x0``: ``|psi| <= 0.1`` at the start and up to 1.1 along the
rollout (reduction index +-1 at 30 of the 3936 nodes of the parity batch, never beyond), ``|delta| < 0.5``, ``v_x`` in [1.4, 15], ``s``
inside the first lap and moving forward by centimetres per sub-step.  The hand-written model code (``csrc/model.hpp``) has branches
those states never reach; every family below is there for one of them:

heading      ``fast_sincos`` with a reduction index |n| >= 2: both sides of every quadrant boundary, n up to 6e4, and the library fallback
             beyond 1e5
steering     ``fast_sincos(delta)`` outside the first octant, fkin6's algebraic slip angle where cos(delta) is not ~1 (|delta| < pi/2)
speed        ``tanh_e(10 v_x)``, the drag derivative and the regularised slip angles at v_x = 0, near it and at negative v_x
arc length   ``TrackSeg``: s on knots and one ulp below, both extrapolation branches of ``init``, leaving the table inside an interval,
             several knots crossed per interval, the backward walk of ``seek``
track offset 1 + kappa n near 0.5 on the tightest curvature
plant switch both sides of (v_x^2 + v_y^2) sin(beta) / l_R = 3, 1e-6 relative apart (plants -1 and -2)
combination  a value of every family at once (a mask error that couples two of them)

Everything else of an entry is the benign base state ``BASE_X``, ``BASE_U``.  The table is data: it reads the knots of the track it is
built on and nothing else.

Tolerances.  An entry carries the tolerances it is compared with, ``entry.tolerance(quantity, model, configuration)``: ``AB`` for A and
B relative to the column scale, ``b`` absolute, ``plant`` for plant steps relative to 1 + |x|.  They are the project's own (``TOL`` =
(fkin6 with RK4, dynamic models and collocation), as ``test_gpu_parity.py`` and ``test_gpu_irk.py`` carry them) unless the ORACLE's
sensitivity to one ulp of the input state exceeds a tenth of that: then 16 x that sensitivity, for that model and integrator alone
(``RAISED``).  The sensitivity is measured
by ``test_oracle_edge_states.py::test_reference_is_well_conditioned`` on ``orc.rk4_sens`` over one shooting interval (dt = 0.05) and on
``orc.rk4`` for the plant steps of the GPU tests, never on a kernel; the same test fails for an entry whose sensitivity exceeds a tenth
of the tolerance it carries.

Measured one-ulp sensitivities of the oracle, worst over the entries of a family and over the three models (fsds_competition_1;
A, B relative to the column scale | increment x+ - x absolute):

family                          ERK                  IRK_GL               IRK_RADAU
base            2.8e-15 |  1.7e-16      1.9e-15 |  1.4e-14      6.2e-15 |  1.1e-16
heading         5.7e-12 |  5.7e-12      5.7e-12 |  5.7e-12      5.7e-12 |  5.7e-12
steering        7.0e-15 |  8.8e-15      5.3e-15 |  1.4e-14      1.2e-14 |  3.4e-15
speed           7.8e-10 |  2.8e-14      3.1e-13 |  2.8e-14      4.2e-13 |  2.5e-13
arc             2.8e-15 |  9.7e-16      1.9e-15 |  1.4e-14      6.2e-15 |  8.9e-16
offset          2.8e-15 |  1.2e-15      5.0e-15 |  1.4e-14      1.1e-14 |  1.6e-15
switch          2.7e-15 |  3.5e-16      4.3e-15 |  1.4e-14      5.8e-15 |  1.9e-16
combo           8.9e-12 |  4.4e-14      7.2e-13 |  9.2e-14      7.6e-13 |  1.1e-13

Above a tenth of the tolerance (-> RAISED):
  psi_99000, psi_m99000, psi_110000, psi_m110000   fkin6 ERK  b   4.7e-12, 5.1e-12, 5.6e-12, 5.7e-12   (ulp(1e5) v_x dt = 5.8e-12)
  vx_m0p05                                         fdyn6u ERK A   7.8e-10                              (regularised slip angles)
  vx_0p05, combo_crawl_at_table_end                fdyn6u plant, Radau IIA x 4   8.5e-11, 6.9e-11      (the same, three Newton iterations)
Plant steps (RK4 x 25, one RK4 step over 0.002, Radau IIA x 4; relative to 1 + |x+|) otherwise stay below 5.1e-12 (psi = +-1.1e5).
The heading family's 5.7e-12 is those four entries; every other heading stays below 1e-13.
"""
from __future__ import annotations

import dataclasses

import numpy as np

BASE_X = (50.0, 0.2, 0.05, 8.0, 0.1, 0.3, 100.0, 0.1)
BASE_U = (150.0, 0.15)
_IX = dict(s=0, n=1, psi=2, vx=3, vy=4, r=5, T=6, delta=7)
_IU = dict(uT=0, ud=1)

# (fkin6 with RK4, dynamic models and collocation)
TOL = {"AB": (1e-10, 1e-9), "b": (1e-11, 1e-10), "plant": (1e-10, 1e-10)}
# configurations: the integrators of a shooting interval and the plant steps of tests/test_gpu_edge_states.py
RK4_CONFIGS = ("ERK", "ERK_25", "ERK_1")
CONFIGS = {"AB": ("ERK", "IRK_GL", "IRK_RADAU"), "b": ("ERK", "IRK_GL", "IRK_RADAU"), "plant": ("ERK_25", "ERK_1", "RADAU_4")}
# where the reference's sensitivity exceeds a tenth of TOL: (quantity, model, configuration) -> 16 x the measured sensitivity (see the
# table above); every other model and integrator keeps TOL at that entry
RAISED = {
    "psi_99000": {("b", "fkin6", "ERK"): 7.6e-11},
    "psi_m99000": {("b", "fkin6", "ERK"): 8.2e-11},
    "psi_110000": {("b", "fkin6", "ERK"): 9.0e-11},
    "psi_m110000": {("b", "fkin6", "ERK"): 9.1e-11},
    "vx_m0p05": {("AB", "fdyn6u", "ERK"): 1.3e-8},
    "vx_0p05": {("plant", "fdyn6u", "RADAU_4"): 1.4e-9},
    "combo_crawl_at_table_end": {("plant", "fdyn6u", "RADAU_4"): 1.2e-9},
}

HEADINGS = (0.78, 0.79, 1.57, 1.58, 2.35, 2.36, 3.14, 3.15, 4.8, 6.3, 40.0, 1e3, 9.9e4, 1.1e5)
STEERINGS = (0.78, 0.79, 1.2, 1.5)
SPEEDS = (0.0, 1e-12, -1e-12, 1e-3, -1e-3, 0.05, -0.05, 0.5, -0.5, 1.0, -3.0, 40.0)
STRIDE = 37                     # coprime to 64 (the wavefront) and to the length of the table: see grid()
L_R, RWD = 0.7853, 0.5          # python/constants.py: l_R and the rear weight distribution l_R / wheelbase (the CPU test compares them
                                # with ihm2_amd.constants: this module stays data, it imports nothing of the project)


@dataclasses.dataclass(frozen=True)
class Entry:
    name: str
    family: str
    x: np.ndarray
    u: np.ndarray
    raised: dict

    def tolerance(self, quantity: str, model: str, config: str) -> float:
        """quantity "AB" / "b" with the integrator of the shooting interval ("ERK", "IRK_GL", "IRK_RADAU"), "plant" with the plant step
        ("ERK_25", "ERK_1", "RADAU_4"); model "fkin6", "fdyn6" or "fdyn6u"."""
        assert config in CONFIGS[quantity], (quantity, config)
        return self.raised.get((quantity, model, config), TOL[quantity][0 if (model == "fkin6" and config in RK4_CONFIGS) else 1])


def _num(v):
    return ("m" if v < 0 else "") + f"{abs(v):g}".replace("e-", "em").replace("+", "").replace(".", "p")


def switch_value(x):
    """Left-hand side of the plants' switch rule (python/main.py:482-489): kinematic where it is <= 3."""
    x = np.asarray(x)
    beta = np.arctan(RWD * np.tan(x[..., 7]))
    return (x[..., 3] ** 2 + x[..., 4] ** 2) * np.sin(beta) / L_R


def table(s_ref, kappa_ref):
    """The entries on the curvature table ``(s_ref, kappa_ref)`` (one track, 1-D arrays)."""
    s_ref, kappa_ref = np.asarray(s_ref, dtype=np.float64), np.asarray(kappa_ref, dtype=np.float64)
    nk = s_ref.size
    k, j = nk // 2 + 57, (3 * nk) // 4 + 11              # two interior knots
    kt = nk // 3 + int(np.argmax(np.abs(kappa_ref[nk // 3:2 * nk // 3])))      # tightest curvature of the middle lap
    n_half = -0.5 / kappa_ref[kt]                          # 1 + kappa n = 0.5 there
    out, seen = [], set()

    def add(family, name, **ch):
        x, u = np.array(BASE_X), np.array(BASE_U)
        for key, v in ch.items():
            if key in _IX:
                x[_IX[key]] = v
            else:
                u[_IU[key]] = v
        assert name not in seen, name
        seen.add(name)
        out.append(Entry(name, family, x, u, dict(RAISED.get(name, {}))))

    add("base", "base")
    for h in HEADINGS:
        for sg in (1.0, -1.0):
            add("heading", "psi_" + _num(sg * h), psi=sg * h)
    for d in STEERINGS:
        for sg in (1.0, -1.0):
            add("steering", "delta_" + _num(sg * d), delta=sg * d, ud=sg * d)                # stays there
    add("steering", "delta_0p1_to_1p5", ud=1.5)                                               # sweeps delta over the interval
    add("steering", "delta_0p1_to_m0p79", ud=-0.79)
    add("steering", "delta_1p2_to_m1p2", delta=1.2, ud=-1.2)
    add("steering", "delta_m1p5_to_0p78", delta=-1.5, ud=0.78)
    for v in SPEEDS:
        add("speed", "vx_" + _num(v), vx=v, vy=0.01, r=0.02)
    # (v_x = v_y = 0 exactly is a singular point of the dynamic models themselves, sqrt(v_x^2 + v_y^2) in the torque vectoring: not a state)
    add("speed", "vx_0_nearly_at_rest", vx=0.0, vy=1e-3, r=0.0, T=0.0, uT=0.0)
    add("speed", "vx_m0p05_braking", vx=-0.05, vy=-0.02, r=0.05, T=-200.0, uT=-300.0)
    # arc length
    add("arc", "s_first_knot", s=s_ref[0])
    add("arc", "s_last_knot", s=s_ref[-1])
    add("arc", "s_knot_k", s=s_ref[k])
    add("arc", "s_knot_j", s=s_ref[j])
    add("arc", "s_below_knot_k", s=np.nextafter(s_ref[k], -np.inf))
    add("arc", "s_below_knot_j", s=np.nextafter(s_ref[j], -np.inf))
    add("arc", "s_below_last_knot", s=np.nextafter(s_ref[-1], -np.inf))
    add("arc", "s_below_second_knot", s=np.nextafter(s_ref[1], -np.inf))
    add("arc", "s_0p1_before_table", s=s_ref[0] - 0.1)
    add("arc", "s_5_before_table", s=s_ref[0] - 5.0)
    add("arc", "s_0p1_after_table", s=s_ref[-1] + 0.1)
    add("arc", "s_5_after_table", s=s_ref[-1] + 5.0)
    add("arc", "s_leaves_table_forward", s=s_ref[-1] - 0.3, vx=30.0)
    add("arc", "s_leaves_table_backward", s=s_ref[0] + 0.3, vx=-20.0)
    add("arc", "s_enters_table_forward", s=s_ref[0] - 0.3, vx=30.0)
    add("arc", "s_crosses_2_knots", s=s_ref[k] - 1e-9, vx=30.0)
    add("arc", "s_crosses_3_knots", s=s_ref[j] - 1e-9, vx=40.0)
    add("arc", "s_back_2_knots", s=s_ref[j] + 0.1, vx=-20.0)
    add("arc", "s_back_2_knots_psi_pi", s=s_ref[k] + 0.1, vx=20.0, psi=3.14)
    # track offset
    add("offset", "n_half_denominator", s=s_ref[kt] + 0.2, n=n_half)
    add("offset", "n_half_denominator_slow", s=s_ref[kt] - 0.2, n=n_half, vx=0.5)
    add("offset", "n_outside_of_curve", s=s_ref[kt] + 0.2, n=-n_half)
    # plant switch: pairs 1e-6 relative on either side of the threshold
    for d in (0.1, 0.3, 0.45):
        sb = np.sin(np.arctan(RWD * np.tan(d)))
        for side, f in (("kin", 1.0 - 1e-6), ("dyn", 1.0 + 1e-6)):
            vy = 0.1
            add("switch", f"switch_delta_{_num(d)}_{side}", delta=d, ud=d, vy=vy, vx=np.sqrt(3.0 * f * L_R / sb - vy * vy))
    # combinations: a value of every family at once
    add("combo", "combo_back_over_tight_curve", s=s_ref[kt] + 0.05, n=n_half, psi=3.15, vx=1.0, delta=-0.79, ud=0.78)
    add("combo", "combo_slow_reverse_at_table_start", s=s_ref[0] + 0.1, n=0.5, psi=1e3, vx=-3.0, vy=0.01, r=0.02, delta=1.2, ud=-1.2)
    add("combo", "combo_crawl_at_table_end", s=s_ref[-1], n=-0.3, psi=-9.9e4, vx=1e-3, vy=0.01, r=0.02, delta=0.78, ud=0.79)
    add("combo", "combo_fast_quadrant_3", s=s_ref[j] - 1e-9, n=-0.4,
        psi=-4.8, vx=40.0, delta=-1.5, ud=-1.5)
    return out


def grid(entries, B, N, first=0):
    """Index (B, N + 1) of the entry at every node of a batch of horizons: interval k of instance b -- lane (b N + k) mod 64 of the
    interval-per-lane kernels, quad (b N + k) mod 16 of the collocation kernels -- takes entry (first + (b N + k) STRIDE) mod len, so that
    B N >= len intervals hold every entry and an entry that comes again lands on another lane.  Node N continues the cycle (it is the
    next instance's first entry): it only enters the defect of the last interval."""
    flat = np.arange(B)[:, None] * N + np.arange(N + 1)[None, :]
    return (first + flat * STRIDE) % len(entries)


def arrays(entries):
    """(x (n, 8), u (n, 2)) of a list of entries."""
    return np.stack([e.x for e in entries]), np.stack([e.u for e in entries])


def tolerances(entries, quantity, model, config):
    return np.array([e.tolerance(quantity, model, config) for e in entries])


# the three non-finite states of the isolation tests (named explicitly: they are compared with nothing)
def non_finite_states():
    out = {}
    for name, idx, v in (("nan_in_s", 0, np.nan), ("nan_in_psi", 2, np.nan), ("inf_in_s", 0, np.inf)):
        x = np.array(BASE_X)
        x[idx] = v
        out[name] = (x, np.array(BASE_U))
    return out
