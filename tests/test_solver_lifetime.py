"""BatchedOcpSolver's finaliser and the torch layer's lifetime rule, without a GPU: a solver whose stream the layer has used is not
freed from __del__, whatever its weak references say -- in a garbage collection they are cleared before the finaliser runs, while the
tensors' memory is still held (NOTES.md R30: a segmentation fault after a failed test, whose traceback held the solver and a view of a
layer output in one cycle).  free() itself keeps its guard.  The library is a recorder here."""
import ctypes
import gc
import weakref

import pytest

from ihm2_amd.solver import BatchedOcpSolver


class _Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append(name)


class _Storage:
    pass


def _solver(users=None):
    s = BatchedOcpSolver.__new__(BatchedOcpSolver)
    s.lib, s._h, s._pinned = _Lib(), ctypes.c_void_p(1), []
    if users is not None:
        s._stream_users = users
    return s


def test_free_refuses_while_a_marked_storage_is_alive_and_frees_after():
    st = _Storage()
    s = _solver([weakref.ref(st)])
    with pytest.raises(RuntimeError, match="still alive"):
        s.free()
    assert s.lib.calls == []
    del st
    s.free()
    assert s.lib.calls == ["ihm2mpc_synchronize", "ihm2mpc_free"] and not s._h.value
    s.free()                                    # a second call does nothing
    assert s.lib.calls == ["ihm2mpc_synchronize", "ihm2mpc_free"]


def test_finaliser_frees_a_solver_the_layer_never_used():
    s = _solver()
    lib = s.lib
    del s
    gc.collect()
    assert lib.calls == ["ihm2mpc_synchronize", "ihm2mpc_free"]


@pytest.mark.parametrize("dead", [False, True])
def test_finaliser_leaves_a_solver_the_layer_used(dead):
    """dead: the weak reference already says the storage has gone -- which is what the collector makes every one of them say before it
    calls the finaliser of a solver that dies in the same collection as the storage."""
    st = _Storage()
    s = _solver([weakref.ref(st)])
    lib = s.lib
    if dead:
        del st
    del s
    gc.collect()
    assert lib.calls == []


def test_solver_and_storage_in_one_cycle():
    """The case itself: both unreachable at once.  The collector clears the weak reference first; the finaliser must not take that for
    the storage's memory being released."""
    st = _Storage()
    s = _solver([weakref.ref(st)])
    lib = s.lib
    st.solver, s.held = s, st                   # one cycle
    del st, s
    gc.collect()
    assert lib.calls == []
