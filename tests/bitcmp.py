"""Bit comparisons that say what differs: the array's name, how many entries differ, and the first few indices with both values and
both bit patterns (NOTES.md R29: a failing bit comparison that names neither the array nor the entries cannot be read afterwards).
Nothing here reads a result."""
from __future__ import annotations

import numpy as np


def _bits(a):
    a = np.ascontiguousarray(np.atleast_1d(a))
    if a.dtype.kind in "iu":        # integers compare by value, whatever their width
        a = a.astype(np.int64)
    return a, (a.view(np.uint64) if a.dtype == np.float64 else a)


def report(name, got, want, first=6, nan_equal=False):
    """None if ``got`` and ``want`` have the same shape, type and bits (the sign of zero counts, and so do NaN payloads unless
    ``nan_equal``: then a NaN equals a NaN); else one line."""
    got, gb = _bits(got)
    want, wb = _bits(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{name}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    differ = gb != wb
    if nan_equal and got.dtype == np.float64:
        differ &= ~(np.isnan(got) & np.isnan(want))
    idx = np.argwhere(differ)
    if len(idx) == 0:
        return None

    def one(i):
        i = tuple(int(v) for v in i)
        if got.dtype == np.float64:
            return f"{list(i)}: {got[i]!r} ({int(gb[i]):#018x}) against {want[i]!r} ({int(wb[i]):#018x})"
        return f"{list(i)}: {got[i]!r} against {want[i]!r}"

    return (f"{name}: {len(idx)} of {gb.size} entries differ in their bits; the first {min(first, len(idx))}: "
            + "; ".join(one(i) for i in idx[:first]))


def assert_same_bits(name, got, want, rows=None, nan_equal=False):
    """``rows``: a mask or an index array on the first axis (the solved instances, say); the indices reported are then those of the
    selection."""
    if rows is not None:
        got, want = np.asarray(got)[rows], np.asarray(want)[rows]
    msg = report(name, got, want, nan_equal=nan_equal)
    assert msg is None, msg


def assert_all_same_bits(what, got: dict, want: dict, keys=None, nan_equal=False):
    """Every array of ``keys`` (default: those of ``want``); all the differing arrays are named, not the first one alone."""
    msgs = [m for m in (report(f"{what}: {k}", got[k], want[k], nan_equal=nan_equal) for k in (want if keys is None else keys)) if m is not None]
    assert not msgs, "\n".join(msgs)
