"""Per-instance slack penalties, the parts that need no GPU: the header declares the two entries, the ctypes table lists them, the
handle keeps their device copies as state, and controller.instance_penalties expands (B,) penalties into exactly the tables the scalar
path builds, instance by instance."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ihm2mpc_set_instance_soft", "ihm2mpc_set_instance_alat_soft")
LIMITS = dict(n_max=2.0, v_x_max=31.0, T_max=500.0, delta_max=0.5, T_dot_max=1e6, delta_dot_max=1.0)
NK, N, B = 50, 12, 6


def test_header_declares_both_entries():
    text = open(os.path.join(ROOT, "include", "ihm2mpc.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(ihm2mpc_handle \*h, const double \*soft_z, const double \*soft_Z\);" % name, text, re.M), name
    # the sentence of the per-instance bounds stays; the new paragraph says what stays shared
    assert "C, D, soft penalties, track rows and the a_lat row stay shared" in text
    assert "NULL, NULL = batch-shared penalties again" in text


def test_symbol_table_lists_both_entries_with_three_arguments():
    from ihm2_amd import _lib

    for name in ENTRIES:
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is _lib.C.c_int and len(argtypes) == 3
        assert argtypes[1:] == [_lib.c_double_p] * 2


def test_device_copies_are_state_buffers_of_the_handle():
    """The handle holds the block by value; every member of the block is a StateBuf (tests/test_buffer_classes.py reads the handle's
    direct members, this reads the block)."""
    text = open(os.path.join(ROOT, "ihm2_amd", "csrc", "ihm2mpc_internal.h")).read()
    m = re.search(r"^struct ihm2_inst_penalties \{\n(.*?)^\};", text, re.S | re.M)
    assert m
    code = re.sub(r"//[^\n]*", "", m.group(1))
    decl = re.findall(r"\b(DevBuf|StateBuf|WorkBuf)<(\w+)> ([\w, ]+);", code)
    assert decl and all(c == "StateBuf" and t == "double" for c, t, _ in decl)
    names = {n.strip() for _, _, ns in decl for n in ns.split(",")}
    assert names == {"alat_sz", "alat_sZ"}
    import test_buffer_classes as TB

    assert re.search(r"^\s*ihm2_inst_penalties ip;", TB.handle_body(text), re.M)


@pytest.mark.parametrize("kw", [
    dict(terminal_bounds="stage", soft_state_bounds=True),
    dict(track_rows=True, track_rows_penalty=True),
    dict(track_rows=True, track_rows_penalty=True, lateral_acceleration_row=True),
    dict(terminal_bounds="stage", soft_state_bounds=True, track_rows=True, track_rows_penalty=True, lateral_acceleration_row=True),
])
def test_instance_penalties_are_the_scalar_paths_tables(kw):
    from ihm2_amd.controller import controller_ocp, instance_penalties

    rng = np.random.default_rng(3)
    arrays = {}
    for name in ("soft_state_bounds", "track_rows_penalty"):
        if kw.get(name):
            # (B,) z and Z; two instances share a set, one has z = 0
            z, Z = rng.uniform(1.0, 500.0, B), rng.uniform(1.0, 500.0, B)
            z[1], Z[1] = z[0], Z[0]
            z[2] = 0.0
            arrays[name] = (z, Z)
    base = {k: v for k, v in kw.items() if k not in arrays}
    soft, alat = instance_penalties(B, LIMITS, NK, N, **{**base, **arrays})
    assert soft is not None and soft[0].shape == (B, N + 1, 28) and soft[1].shape == (B, N + 1, 28)
    for b in range(B):
        scal = {name: (float(z[b]), float(Z[b])) for name, (z, Z) in arrays.items()}
        d = controller_ocp(NK, N, LIMITS, **{**base, **scal})[1].flatten()
        np.testing.assert_array_equal(soft[0][b], d.soft_z)
        np.testing.assert_array_equal(soft[1][b], d.soft_Z)
        if kw.get("lateral_acceleration_row"):
            np.testing.assert_array_equal(alat[0][b], d.alat_soft_z)
            np.testing.assert_array_equal(alat[1][b], d.alat_soft_Z)
    if not kw.get("lateral_acceleration_row"):
        assert alat is None
    # a scalar beside an array broadcasts
    if "track_rows_penalty" in arrays:
        z, Z = arrays["track_rows_penalty"]
        soft2, _ = instance_penalties(B, LIMITS, NK, N, **{**base, **arrays, "track_rows_penalty": (z, 100.0)})
        d = controller_ocp(NK, N, LIMITS, **{**base, **{n: (float(a[0][3]), float(a[1][3])) for n, a in arrays.items()},
                                             "track_rows_penalty": (float(z[3]), 100.0)})[1].flatten()
        np.testing.assert_array_equal(soft2[1][3], d.soft_Z)


def test_scalars_expand_to_nothing_and_bad_shapes_are_refused():
    from ihm2_amd.controller import instance_penalties, instance_tuning

    assert instance_penalties(B, LIMITS, NK, N, terminal_bounds="stage", soft_state_bounds=(1000.0, 1000.0)) == (None, None)
    assert instance_penalties(B, LIMITS, NK, N, track_rows=True, track_rows_penalty=(100.0, 100.0), lateral_acceleration_row=True) == (None, None)
    assert instance_penalties(B, LIMITS, NK, N) == (None, None)
    assert instance_penalties(B, LIMITS, NK, N, track_rows=True, track_rows_penalty=None) == (None, None)
    # penalties of rows the OCP does not have
    assert instance_penalties(B, LIMITS, NK, N, track_rows=False, track_rows_penalty=(np.full(B, 3.0), 4.0)) == (None, None)
    with pytest.raises(ValueError, match="track_rows_penalty z"):
        instance_penalties(B, LIMITS, NK, N, track_rows=True, track_rows_penalty=(np.ones(B + 1), 1.0))
    # instance_tuning keeps its two return values
    assert instance_tuning(B, {}, LIMITS, NK, N) == (None, None)
