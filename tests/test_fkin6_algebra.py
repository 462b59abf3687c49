"""fkin6's arithmetic without a GPU (tools/probes/check_fkin6_algebra.cpp, built with the address and undefined-behaviour sanitizers).

(a) The steering block of ``fkin6_eval`` (csrc/model.hpp) takes cos(beta), sin(beta), beta' and beta'' of beta = atan(c tan(delta)) from
sin(delta), cos(delta) and one reciprocal, with no tangent.  On 200 001 angles over [-1.55, 1.55] plus every steering angle and steering
input of tests/edge_states.py, against the tan / atan formulas in long double: the worst relative error of each quantity may not exceed
twice that of the form it replaces (td = sd / cd, den = 1 + c^2 td^2), measured in the same run.  Both are printed.

(b) Rows 2 and 5 of the Jacobian in factored form (csrc/device_steps.hpp: ``fkin6_factored_row``) against the dense row products of
``sens_col_stage``: 10 000 random draws of (state, input, curvature, its slope, dX) and all ten column masks, agreement to 8 ulp of the
sum of the terms' absolute values; the rows that stay dense, xdot and every other Jacobian entry are equal bit for bit, and the factored
form writes 25 entries, none of them where the dense form writes one of rows 2 and 5 (both arrays start as NaN).

The probe's formulas are copies of the headers' (device code); the statements are compared with the headers' text here."""
import os
import re

import numpy as np
import pytest

import edge_states as E
import host_probe as HP
from host_probe import CSRC

PROBE = os.path.join(HP.ROOT, "tools", "probes", "check_fkin6_algebra.cpp")


def _steering_values(track):
    x, u = E.arrays(E.table(track.s_ref, track.kappa_ref))
    return sorted(set(x[:, 7].tolist()) | set(u[:, 1].tolist()))


@pytest.fixture(scope="module")
def probe(tmp_path_factory, track):
    exe = HP.build("check_fkin6_algebra", tmp_path_factory.mktemp("fkin6_algebra"), extra=("-ffp-contract=off",))
    values = _steering_values(track)
    out = HP.run(exe, *[repr(v) for v in values])
    return out, values


def test_edge_state_steering_values_are_in_the_grid(track):
    values = _steering_values(track)
    assert {1.5, -1.5, 0.78, -0.79, 1.2, -1.2, 0.1, 0.15} <= set(values)
    assert max(abs(v) for v in values) <= 1.55


def test_probe_passes(probe):
    out, _ = probe
    print(out.stdout[-3000:])
    assert HP.passed(out), HP.tail(out)


def test_steering_block_is_no_worse_than_twice_the_earlier_form(probe):
    out, values = probe
    rows = re.findall(r"steering (\S+)\s+worst relative error on (\d+) angles: new (\S+)\s+earlier (\S+)", out.stdout)
    assert [r[0] for r in rows] == ["cos(beta)", "sin(beta)", "beta'", "beta''"]
    for name, n, new, old in rows:
        assert int(n) == 200001 + 1 + len(values)
        assert 0.0 < float(old) < 1e-14          # the bound is a rounding-level one
        assert float(new) <= 2.0 * float(old), (name, new, old)


def test_factored_rows_agree_with_the_dense_products(probe):
    out, _ = probe
    m = re.search(r"factored rows: (\d+) draws x 10 columns, worst difference (\S+) ulp of the terms' sum in row 2, (\S+) in row 5", out.stdout)
    assert m and int(m.group(1)) == 10000
    assert float(m.group(2)) <= 8.0 and float(m.group(3)) <= 8.0


def _norm(text):
    return [" ".join(l.split()) for l in text.strip().splitlines() if l.strip()]


def _between(text, first, last):
    """The lines of ``text`` from the one that starts with ``first`` to the next one that starts with ``last``, both included."""
    lines = _norm(text)
    a = next(i for i, l in enumerate(lines) if l.startswith(first))
    b = next(i for i in range(a, len(lines)) if lines[i].startswith(last))
    return lines[a:b + 1]


def _marked(name):
    lines = _norm(open(PROBE).read())
    out, start = [], 0
    while f"// [{name}]" in lines[start:]:
        a = lines.index(f"// [{name}]", start)
        b = lines.index("// [end]", a)
        out.append(lines[a + 1:b])
        start = b
    return out


def test_probe_formulas_are_the_headers_text():
    model = open(os.path.join(CSRC, "model.hpp")).read()
    steps = open(os.path.join(CSRC, "device_steps.hpp")).read()
    fkin6 = model[model.index("void fkin6_eval("):model.index("// ---- lateral acceleration of the kinematic model")]
    steer = _marked("steering block")
    assert len(steer) == 1 and steer[0] == _between(fkin6, "const double hyp2 =", "const double bp =")
    jac = _marked("jacobian block")
    assert len(jac) == 1 and jac[0] == _between(fkin6, "if (WITH_JAC) {", "J[7][9] = ") + ["}"]
    row = _marked("factored row")
    body = steps[steps.index("double fkin6_factored_row("):]
    assert len(row) == 1 and row[0] == _between(body, "{", "return acc;") + ["}"]
    # the probe's fkin6 outside the marked block: the same statements as the header's, but for the trigonometric functions and the curvature
    probe_text = open(PROBE).read()
    host = _norm(probe_text[probe_text.index("void fkin6_host("):probe_text.index("// [jacobian block]")])
    for line in _between(fkin6, "const double c = k_rwd;", "f[7] = delta_dot;"):
        if line.startswith("//") or any(w in line for w in ("fast_sincos", "double sd, cd;", "double sp, cp;", "double dk;", "trk.kappa")):
            continue
        assert line in host, line
    for name in ("JX_MASK", "JU_MASK", "S_COL_MASK"):
        row0 = re.search(name + r"\[2\]\[\d+\] = \{(\{[^}]*\})", model).group(1)
        assert row0 in probe_text, name
    for c in ("FKIN6_F_ROW2 = 2, FKIN6_F_KAP = 6, FKIN6_F_DKS = 7, FKIN6_F_ROW5 = 5, FKIN6_F_DBD_DD = 0, FKIN6_F_DBD_DU = 1",
              "FKIN6_JAC_NONE = 0, FKIN6_JAC_DENSE = 1, FKIN6_JAC_FACTORED = 2"):
        assert c in model and c in probe_text
    from ihm2_amd import constants as K

    for name, v in (("k_m", K.m), ("k_lR", K.l_R), ("k_wheelbase", K.wheelbase), ("k_Cm0", K.C_m0), ("k_Cr0", K.C_r0), ("k_Cr1", K.C_r1),
                    ("k_Cr2", K.C_r2), ("k_tT", K.t_T), ("k_tdelta", K.t_delta)):
        for text in (model, probe_text):
            assert float(re.search(r"\b" + name + r" = ([0-9.e+-]+)", text).group(1)) == v, name
    assert np.isclose(K.l_R / K.wheelbase, 0.5)
