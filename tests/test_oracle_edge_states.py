"""Certifies the inputs of tests/test_gpu_edge_states.py before a kernel sees them: at every entry of tests/edge_states.py and for
all three models the C oracle agrees with its NumPy mirror and with complex-step Jacobians, stays finite, and is so well conditioned
over one shooting interval that a disagreement beyond the entry's tolerance is the kernel's."""
import numpy as np
import pytest

import edge_states as E
from oracle import models_np as mnp
from oracle import oracle as orc

MODELS = [("fkin6", orc.MODEL_FKIN6, mnp.fkin6), ("fdyn6", orc.MODEL_FDYN6, mnp.fdyn6), ("fdyn6u", orc.MODEL_FDYN6U, mnp.fdyn6u)]
# the integrators of a shooting interval: RK4 x 25, Gauss-Legendre and Radau IIA (4 stages, one step)
INTEGRATORS = [("ERK", orc.INTEG_RK4, 25), ("IRK_GL", orc.INTEG_IRK_GL4, 1), ("IRK_RADAU", orc.INTEG_IRK_RADAU4, 1)]
# the plant steps of tests/test_gpu_edge_states.py: (integrator, sub-steps, dt)
PLANTS = [("ERK_25", orc.INTEG_RK4, 25, 0.05), ("ERK_1", orc.INTEG_RK4, 1, 0.002), ("RADAU_4", orc.INTEG_IRK_RADAU4, 4, 0.05)]
DT = 0.05


@pytest.fixture(scope="module")
def entries(track):
    return E.table(track.s_ref, track.kappa_ref)


def test_table_covers_the_families(entries, track):
    fam = {e.family for e in entries}
    assert fam == {"base", "heading", "steering", "speed", "arc", "offset", "switch", "combo"}
    assert len({e.name for e in entries}) == len(entries)
    x, _ = E.arrays(entries)
    assert np.all(np.isfinite(x)) and np.all(np.abs(x[:, 7]) < np.pi / 2)         # the domain fkin6_eval documents
    assert (np.abs(x[:, 2]) > 1e5).sum() >= 2 and (x[:, 3] == 0).any() and (x[:, 3] < 0).any()
    assert (x[:, 0] < track.s_ref[0]).any() and (x[:, 0] > track.s_ref[-1]).any()
    sw = np.array([E.switch_value(e.x) for e in entries if e.family == "switch"])
    assert np.all(np.abs(sw / 3.0 - 1.0) < 1.1e-6) and (sw <= 3.0).sum() == (sw > 3.0).sum() == sw.size // 2
    kap = np.interp(x[:, 0], track.s_ref, track.kappa_ref)
    assert np.min(1.0 + kap * x[:, 1]) < 0.55
    # the coprime stride of the GPU tests reaches every entry on every lane position
    assert np.gcd(len(entries), 64) == 1 and np.gcd(len(entries), E.STRIDE) == 1 and np.gcd(64, E.STRIDE) == 1
    # a raised tolerance is the exception, for one model and integrator, and never below the project's own
    assert set(E.RAISED) <= {e.name for e in entries} and sum(len(v) for v in E.RAISED.values()) == 7
    for e in entries:
        for q, cfgs in E.CONFIGS.items():
            for m, _, _ in MODELS:
                for cfg in cfgs:
                    assert e.tolerance(q, m, cfg) >= E.TOL[q][0 if (m == "fkin6" and cfg in E.RK4_CONFIGS) else 1]
    # the table is data and imports nothing of the project: its copies of the constants are the project's
    from ihm2_amd import constants as c

    assert E.L_R == c.l_R and E.RWD == c.l_R / c.wheelbase


@pytest.mark.parametrize("name,model,fnp", MODELS)
def test_f_matches_numpy_mirror_at_edge_states(track, entries, name, model, fnp):
    for e in entries:
        fc = orc.f(model, e.x, e.u, track.s_ref, track.kappa_ref)
        fn = fnp(e.x, e.u, track.s_ref, track.kappa_ref)
        assert np.all(np.isfinite(fc)), e.name
        np.testing.assert_allclose(fc, fn, rtol=1e-12, atol=1e-11, err_msg=e.name)       # tolerance of tests/test_oracle_model.py


@pytest.mark.parametrize("name,model,fnp", MODELS)
def test_jacobian_matches_complex_step_at_edge_states(track, entries, name, model, fnp):
    for e in entries:
        _, J = orc.jac(model, e.x, e.u, track.s_ref, track.kappa_ref)
        _, Jcs = orc.jac(model, e.x, e.u, track.s_ref, track.kappa_ref, complex_step=True)
        assert np.all(np.isfinite(J)) and np.all(np.isfinite(Jcs)), e.name
        assert np.max(np.abs(J - Jcs) / (1.0 + np.abs(Jcs))) < 1e-11, e.name             # tolerance of tests/test_oracle_properties.py


def one_ulp_sensitivity(model, integ, M, x, u, s_ref, kappa_ref):
    """How far one ulp of any state component moves the oracle's records of one shooting interval: (A and B relative to the column
    scale, the increment x+ - x absolute).  A move of x+ within its own rounding grid (spacing(x+), which
    at psi = 1e5 is 1.5e-11) is the number format's and not the map's: it is taken off.  An ulp of s that takes the START of the interval
    into another segment of the table is not applied: d kappa / d s jumps at a knot by definition, both sides are handed the same bits of
    s, and which segment a knot belongs to (the one to its right) is exactly what the on-knot entries are there to check."""
    xn, A, Bm = orc.rk4_sens(model, x, u, s_ref, kappa_ref, DT, M, integrator=integ)
    assert np.all(np.isfinite(xn)) and np.all(np.isfinite(A)) and np.all(np.isfinite(Bm))
    ca = np.maximum(np.abs(A).max(axis=0, keepdims=True), 1e-30)
    cb = np.maximum(np.abs(Bm).max(axis=0, keepdims=True), 1e-30)
    s_ab = s_b = 0.0
    for i in range(8):
        for up in (np.inf, -np.inf):
            xp = x.copy()
            xp[i] = np.nextafter(x[i], up)
            if i == 0 and np.searchsorted(s_ref, xp[0], side="right") != np.searchsorted(s_ref, x[0], side="right"):
                continue
            xq, Aq, Bq = orc.rk4_sens(model, xp, u, s_ref, kappa_ref, DT, M, integrator=integ)
            s_ab = max(s_ab, np.max(np.abs(Aq - A) / ca), np.max(np.abs(Bq - Bm) / cb))
            d = np.maximum(np.abs((xq - xp) - (xn - x)) - np.spacing(np.abs(xn)), 0.0)
            s_b = max(s_b, d.max())
    return s_ab, s_b


def one_ulp_plant_sensitivity(model, integ, M, dt, x, u, s_ref, kappa_ref):
    """The same for a plant step (no sensitivities): the move of the increment relative to 1 + |x+|."""
    xn = orc.rk4(model, x, u, s_ref, kappa_ref, dt, M, integrator=integ)
    assert np.all(np.isfinite(xn))
    s_x = 0.0
    for i in range(8):
        for up in (np.inf, -np.inf):
            xp = x.copy()
            xp[i] = np.nextafter(x[i], up)
            if i == 0 and np.searchsorted(s_ref, xp[0], side="right") != np.searchsorted(s_ref, x[0], side="right"):
                continue
            xq = orc.rk4(model, xp, u, s_ref, kappa_ref, dt, M, integrator=integ)
            d = np.maximum(np.abs((xq - xp) - (xn - x)) - np.spacing(np.abs(xn)), 0.0)
            s_x = max(s_x, np.max(d / (1.0 + np.abs(xn))))
    return s_x


def _all_sensitivities(track, entries):
    """name -> model -> configuration -> (s_AB, s_b) for the integrators of a shooting interval, s_plant for the plant steps."""
    out = {}
    for e in entries:
        out[e.name] = {}
        for m, mc, _ in MODELS:
            d = {i: one_ulp_sensitivity(mc, ic, M, e.x, e.u, track.s_ref, track.kappa_ref) for i, ic, M in INTEGRATORS}
            d.update({"plant_" + p: one_ulp_plant_sensitivity(mc, ic, M, dt, e.x, e.u, track.s_ref, track.kappa_ref) for p, ic, M, dt in PLANTS})
            out[e.name][m] = d
    return out


@pytest.fixture(scope="module")
def sensitivities(track, entries):
    return _all_sensitivities(track, entries)


def _cases(sens_of_model):
    """(quantity, configuration, sensitivity) of every configuration of one model."""
    for i, _, _ in INTEGRATORS:
        yield "AB", i, sens_of_model[i][0]
        yield "b", i, sens_of_model[i][1]
    for p, _, _, _ in PLANTS:
        yield "plant", p, sens_of_model["plant_" + p]


def test_reference_is_well_conditioned(entries, sensitivities):
    """The conditioning cap: the oracle's one-ulp sensitivity stays below a tenth of the tolerance the entry carries for that model and
    integrator.  An entry that fails is a bad test input (or needs 16 x its sensitivity in edge_states.RAISED, for that configuration
    alone): the tolerance of the others is not loosened."""
    bad = []
    for e in entries:
        for m, _, _ in MODELS:
            for q, cfg, s in _cases(sensitivities[e.name][m]):
                if not s < 0.1 * e.tolerance(q, m, cfg):
                    bad.append((e.name, m, cfg, q, s, e.tolerance(q, m, cfg)))
    assert not bad, bad


def test_raised_tolerances_are_sixteen_times_the_sensitivity(entries, sensitivities):
    """A raised tolerance is not a free choice: it lies within [16, 18] x the measured sensitivity of the model and integrator it is
    for (the table stores it rounded up to two digits), and that sensitivity does exceed a tenth of the project's tolerance."""
    for e in entries:
        for (q, m, cfg), tol in E.RAISED.get(e.name, {}).items():
            s = dict(((qq, c), v) for qq, c, v in _cases(sensitivities[e.name][m]))[(q, cfg)]
            base = E.TOL[q][0 if (m == "fkin6" and cfg in E.RK4_CONFIGS) else 1]
            assert s >= 0.1 * base, (e.name, q, m, cfg, s)
            assert 16.0 * s <= tol <= 18.0 * s, (e.name, q, m, cfg, s, tol)
            assert e.tolerance(q, m, cfg) == tol


def _family_rows(entries, sens):
    """family -> [(s_AB, s_b) per integrator], worst over the family's entries and the three models: the rows of the docstring's table."""
    rows = {}
    for e in entries:
        rows.setdefault(e.family, None)
    for fam in rows:
        rows[fam] = [tuple(max(sens[e.name][m][i][q] for e in entries if e.family == fam for m, _, _ in MODELS) for q in (0, 1))
                     for i, _, _ in INTEGRATORS]
    return rows


def test_sensitivity_table_of_the_docstring_is_current(entries, sensitivities):
    """The table at the top of tests/edge_states.py is what this module measures (to a factor of 4: the smallest figures are a few
    roundings and move with the last bit of libm).  ``pytest tests/test_oracle_edge_states.py -s -k docstring`` prints the fresh rows."""
    import re

    rows = _family_rows(entries, sensitivities)
    for fam, vals in rows.items():
        print(f"{fam:<11s}" + "".join(f"{a:>12.1e} |{b:>9.1e} " for a, b in vals))
    for fam, vals in rows.items():
        m = re.search(r"^%s +(.*)$" % fam, E.__doc__[E.__doc__.index("Measured one-ulp sensitivities"):], flags=re.M)
        assert m, f"no row for family {fam} in the docstring of edge_states.py"
        doc = [float(v) for v in re.findall(r"[0-9.]+e[-+][0-9]+", m.group(1))]
        fresh = [v for pair in vals for v in pair]
        assert len(doc) == len(fresh), fam
        for d, f in zip(doc, fresh):
            assert d / 4.0 <= f <= 4.0 * d, (fam, doc, fresh)
